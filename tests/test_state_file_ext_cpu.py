"""The extension block of the state file (every octave, SAD windows) through stereo_vo_amd/state_file.py, without a GPU.

The first test builds its bytes with struct.pack from the layout documented in state_file.py and beside svo_save_state in
include/svo_hip.h -- not with write_state -- so that reader and writer cannot agree on a private reading of it."""
import struct

import numpy as np
import pytest

from stereo_vo_amd.abi import keypoint_dtype, dmatch_dtype
from stereo_vo_amd.state_file import read_state, write_state


def keypoints(n, seed):
    rng = np.random.default_rng(seed)
    k = np.zeros(n, keypoint_dtype)
    k["x"], k["y"] = rng.uniform(0, 250, n).astype(np.float32), np.sort(rng.uniform(0, 186, n).astype(np.float32))
    k["response"], k["size"], k["angle"], k["octave"], k["class_id"] = rng.uniform(0, 99, n).astype(np.float32), 0.0, -1.0, 0, -1
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def group(nl, nr, nm, seed, with_ids=True):
    rng = np.random.default_rng(seed + 1000)
    m = np.zeros(nm, dmatch_dtype)
    if nm:
        m["queryIdx"], m["trainIdx"], m["distance"] = rng.integers(0, nl, nm), rng.integers(0, nr, nm), rng.integers(0, 400, nm)
    ids = rng.integers(0, 10 ** 6, nm).astype(np.int64) if with_ids else np.zeros(0, np.int64)
    return {"left": keypoints(nl, seed), "right": keypoints(nr, seed + 1), "matches": m, "ids": ids}


def windows(n, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (n, 8, 8), dtype=np.uint8), (rng.integers(0, 4, n) == 0).astype(np.uint8)


def pack_keypoints(k, d):
    out = [struct.pack("<Q", len(k))]
    for r in k:
        out.append(struct.pack("<fffffii", r["x"], r["y"], r["response"], r["size"], r["angle"], r["octave"], r["class_id"]))
    out.append(struct.pack("<iii", len(k), 32 if len(k) else 0, 0))
    return b"".join(out) + d.tobytes()


def pack_group(g):
    m, ids = g["matches"], g["ids"]
    out = [pack_keypoints(*g["left"]), pack_keypoints(*g["right"]), struct.pack("<QQ", len(m), len(ids))]
    for i in range(len(m)):
        if len(ids) == len(m):
            out.append(struct.pack("<Q", int(ids[i])))
        out.append(struct.pack("<iifi", m["queryIdx"][i], m["trainIdx"][i], m["distance"][i], m["imgIdx"][i]))
    return b"".join(out)


def assert_same_group(a, b, tag):
    for side in ("left", "right"):
        assert a[side][0].tobytes() == b[side][0].tobytes() and np.asarray(a[side][1]).tobytes() == np.asarray(b[side][1]).tobytes(), (tag, side)
    assert a["matches"].tobytes() == b["matches"].tobytes() and list(a["ids"]) == list(b["ids"]), tag


def test_read_state_parses_the_documented_bytes(tmp_path):
    """two octaves, windows on the CURRENT frame only, bytes put together by hand"""
    pre = [group(7, 5, 4, 1), group(3, 0, 0, 2, with_ids=False)]
    cur = [group(6, 6, 5, 3), group(2, 4, 1, 4)]
    cw = [{"left": windows(6, 10), "right": windows(6, 11)}, {"left": windows(2, 12), "right": windows(4, 13)}]
    b = struct.pack("<Q", 2) + pack_group(pre[0]) + pack_group(cur[0]) + struct.pack("<BQQQQQ", 1, 0, 11, 12, 13, 14)
    legacy_len = len(b)
    b += struct.pack("<IIIII", 0x58455653, 1, 2, 251, 187) + bytes([0, 1])
    b += pack_group(pre[1]) + pack_group(cur[1])
    for o in range(2):
        for side in ("left", "right"):
            win, flag = cw[o][side]
            b += struct.pack("<Q", len(flag)) + flag.tobytes() + win.tobytes()
    path = str(tmp_path / "ext.bin")
    open(path, "wb").write(b)
    s = read_state(path)
    assert s["npyr"] == 2 and s["size"] == (251, 187) and len(s["octaves"]) == 1
    assert (s["reset"], s["num_tracked_last_kf"], s["num_tracked_last_frame"], s["last_match_id"], s["kf_max_match_id"]) == (True, 11, 12, 13, 14)
    assert_same_group(pre[0], s["pre"], "pre 0"); assert_same_group(cur[0], s["cur"], "cur 0")
    assert_same_group(pre[1], s["octaves"][0]["pre"], "pre 1"); assert_same_group(cur[1], s["octaves"][0]["cur"], "cur 1")
    assert s["windows"]["pre"] is None and len(s["windows"]["cur"]) == 2
    for o in range(2):
        for side in ("left", "right"):
            win, flag = s["windows"]["cur"][o][side]
            assert win.shape == (len(flag), 8, 8) and (win == cw[o][side][0]).all() and (flag == cw[o][side][1]).all(), (o, side)
    # the bytes up to the tail are a file of the reference's layout on their own
    open(path, "wb").write(b[:legacy_len])
    s1 = read_state(path)
    assert s1["size"] is None and s1["octaves"] == [] and s1["windows"] is None
    assert_same_group(pre[0], s1["pre"], "legacy prefix")
    # a block cut short, a wrong magic, a windows count that is not its list's: assertions, as for trailing bytes before
    for bad in (b[:-1], b[:legacy_len + 10], b[:legacy_len] + b"\0" + b[legacy_len + 1:], b + b"\0"):
        open(path, "wb").write(bad)
        with pytest.raises((AssertionError, struct.error, ValueError)):
            read_state(path)
    off = legacy_len + 22 + len(pack_group(pre[1])) + len(pack_group(cur[1]))
    assert struct.unpack_from("<Q", b, off) == (6,)
    open(path, "wb").write(b[:off] + struct.pack("<Q", 5) + b[off + 8:])
    with pytest.raises(AssertionError):
        read_state(path)


def test_write_state_read_state_round_trip(tmp_path):
    """three octaves, windows on both frames"""
    pre = [group(9 - 2 * o, 8 - o, 4, 20 + o) for o in range(3)]
    cur = [group(8 - 2 * o, 9 - o, 3, 30 + o) for o in range(3)]
    wn = {name: [{side: windows(len(g[side][0]), 40 + 7 * o + i) for i, side in enumerate(("left", "right"))} for o, g in enumerate(gs)]
          for name, gs in (("pre", pre), ("cur", cur))}
    path = str(tmp_path / "rt.bin")
    write_state(path, pre[0], cur[0], reset=False, num_tracked_last_kf=5, num_tracked_last_frame=6, last_match_id=77, kf_max_match_id=70, npyr=3,
                octaves=[{"pre": pre[o], "cur": cur[o]} for o in (1, 2)], windows=wn, size=(760, 560))
    s = read_state(path)
    assert s["npyr"] == 3 and s["size"] == (760, 560) and len(s["octaves"]) == 2 and s["last_match_id"] == 77
    for o in range(3):
        assert_same_group(pre[o], s["pre"] if o == 0 else s["octaves"][o - 1]["pre"], ("pre", o))
        assert_same_group(cur[o], s["cur"] if o == 0 else s["octaves"][o - 1]["cur"], ("cur", o))
        for name in ("pre", "cur"):
            for side in ("left", "right"):
                assert (s["windows"][name][o][side][0] == wn[name][o][side][0]).all() and (s["windows"][name][o][side][1] == wn[name][o][side][1]).all()
    # lists of several octaves without windows: a block with has_windows = (0, 0)
    write_state(path, pre[0], cur[0], npyr=2, octaves=[{"pre": pre[1], "cur": cur[1]}], size=(251, 187))
    s = read_state(path)
    assert s["windows"] == {"pre": None, "cur": None} and len(s["octaves"]) == 1 and s["size"] == (251, 187)
    # a windows list that is not its keypoint list's length is not written
    bad = {"pre": None, "cur": [{"left": windows(3, 1), "right": wn["cur"][0]["right"]}]}
    with pytest.raises(AssertionError):
        write_state(path, pre[0], cur[0], windows=bad, size=(251, 187))


def test_a_legacy_file_reads_and_writes_as_before(tmp_path):
    pre, cur = group(5, 4, 3, 50), group(6, 5, 2, 51)
    path = str(tmp_path / "legacy.bin")
    write_state(path, pre, cur, reset=True, num_tracked_last_kf=1, num_tracked_last_frame=2, last_match_id=3, kf_max_match_id=4)
    want = struct.pack("<Q", 1) + pack_group(pre) + pack_group(cur) + struct.pack("<BQQQQQ", 1, 0, 1, 2, 3, 4)
    assert open(path, "rb").read() == want                      # no block unless it is asked for
    s = read_state(path)
    assert s["npyr"] == 1 and (s["size"], s["octaves"], s["windows"]) == (None, [], None)
    assert_same_group(pre, s["pre"], "pre"); assert_same_group(cur, s["cur"], "cur")
    open(path, "wb").write(want + b"\x01\x02\x03")
    with pytest.raises(AssertionError, match="trailing bytes"):
        read_state(path)
