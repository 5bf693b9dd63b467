"""Reader / writer of the estimator state file, the on-disk format either side of the hot path.

Layout = what CStereoOdometryEstimator::saveStateToFile writes (libstereo-odometry/src/common.cpp:475-543 with the
helpers m_dump_keypoints_to_stream :88-133 and m_dump_matches_to_stream :138-163), little-endian, size_t = 8 bytes:

    npyr                                                         u64
    PRE left, PRE right, PRE pairings, CUR left, CUR right, CUR pairings, where
      keypoints = count u64, then per keypoint  x y response size angle (f32)  octave class_id (i32),
                  then rows cols type (i32) and rows*cols descriptor bytes
      pairings  = count u64, id_count u64, then per pairing  [id u64 if count == id_count]
                  queryIdx trainIdx (i32) distance (f32) imgIdx (i32)
    m_reset u8, m_lastID, m_num_tracked_pairs_from_last_kf, m_num_tracked_pairs_from_last_frame,
    m_last_match_ID, m_kf_max_match_ID                            u64 each

The reference's loadStateFromFile (common.cpp:261-350) expects one more u64 ("v_s", :342-343) before m_last_match_ID
that its own saver never writes; this module, like svo_load_state, reads what the saver writes.

THE EXTENSION BLOCK.  svo_save_state appends it, directly behind the tail, when the context works on more than one octave or at
least one of the two frames has the SAD matchers' 8 x 8 windows; the bytes above stay first and unchanged (octave 0; npyr is then
the octave count), so a reader of the reference's layout still gets octave 0.  Little-endian, no padding:

    magic u32 = 0x58455653 ("SVEX"), version u32 = 1, n_oct u32 (1 .. 4), w u32, h u32      the octave-0 image size
    has_windows u8 x 2                                                                      PRE, CUR
    for octave 1 .. n_oct - 1:  PRE left, PRE right, PRE pairings, CUR left, CUR right, CUR pairings   (sub-layouts as above)
    for frame in (PRE, CUR) with has_windows, for octave 0 .. n_oct - 1, for side in (left, right):
        count u64 (= the list's keypoint count), count flag bytes (1: no window, too close to the border),
        count * 64 window bytes (8 rows of 8 pixels, top to bottom; zero where the flag is set)

read_state reports it under three more keys: `size` = (w, h), `octaves` = [{"pre": group, "cur": group}] for octaves 1 .. n_oct - 1
and `windows` = {"pre": w, "cur": w} with w = None or, per octave from 0, {"left": (windows [n, 8, 8], flags [n]), "right": ...}.
Without a block they are None, [] and None.  An independent reading of the layout: nothing here calls the library.
"""
import struct

import numpy as np

from .abi import keypoint_dtype, dmatch_dtype

_KP_FILE = np.dtype([("x", "<f4"), ("y", "<f4"), ("response", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _dump_keypoints(kps, desc):
    kps = np.asarray(kps, keypoint_dtype)
    n = len(kps)
    rec = np.zeros(n, _KP_FILE)
    for f in _KP_FILE.names:
        rec[f] = kps[f]
    desc = np.ascontiguousarray(desc, np.uint8).reshape(n, 32) if n else np.zeros((0, 32), np.uint8)
    return struct.pack("<Q", n) + rec.tobytes() + struct.pack("<iii", n, 32 if n else 0, 0) + desc.tobytes()


def _load_keypoints(buf, off):
    (n,) = struct.unpack_from("<Q", buf, off); off += 8
    rec = np.frombuffer(buf, _KP_FILE, n, off); off += n * _KP_FILE.itemsize
    rows, cols, _typ = struct.unpack_from("<iii", buf, off); off += 12
    kps = np.zeros(n, keypoint_dtype)
    for f in _KP_FILE.names:
        kps[f] = rec[f]
    desc = np.frombuffer(buf, np.uint8, rows * cols, off).reshape(rows, cols).copy(); off += rows * cols
    return kps, desc, off


def _dump_matches(m, ids):
    m = np.asarray(m, dmatch_dtype)
    ids = np.asarray(ids, np.int64)
    out = [struct.pack("<QQ", len(m), len(ids))]
    for i in range(len(m)):
        if len(m) == len(ids):
            out.append(struct.pack("<Q", int(ids[i])))
        out.append(struct.pack("<iifi", int(m["queryIdx"][i]), int(m["trainIdx"][i]), float(m["distance"][i]), int(m["imgIdx"][i])))
    return b"".join(out)


def _load_matches(buf, off):
    n, ni = struct.unpack_from("<QQ", buf, off); off += 16
    m = np.zeros(n, dmatch_dtype); ids = np.zeros(ni, np.int64)
    for i in range(n):
        if n == ni:
            (ids[i],) = struct.unpack_from("<Q", buf, off); off += 8
        q, t, d, im = struct.unpack_from("<iifi", buf, off); off += 16
        m[i] = (q, t, im, d)
    return m, ids, off


EXT_MAGIC, EXT_VERSION = 0x58455653, 1


def _dump_group(d):
    return [_dump_keypoints(*d["left"]), _dump_keypoints(*d["right"]), _dump_matches(d["matches"], d["ids"])]


def _load_group(buf, off):
    lk, ld, off = _load_keypoints(buf, off)
    rk, rd, off = _load_keypoints(buf, off)
    m, ids, off = _load_matches(buf, off)
    return {"left": (lk, ld), "right": (rk, rd), "matches": m, "ids": ids}, off


def write_state(path, pre, cur, reset=False, num_tracked_last_kf=0, num_tracked_last_frame=0, last_match_id=0, kf_max_match_id=0, npyr=1,
                octaves=None, windows=None, size=None):
    """pre / cur: dicts with left=(kps, desc), right=(kps, desc), matches, ids.  octaves / windows / size as read_state returns them:
    the extension block is written when any of them is given (size is then required)."""
    blob = [struct.pack("<Q", npyr)]
    for d in (pre, cur):
        blob += _dump_group(d)
    blob.append(struct.pack("<BQQQQQ", 1 if reset else 0, 0, num_tracked_last_kf, num_tracked_last_frame, last_match_id, kf_max_match_id))
    if octaves or windows is not None or size is not None:
        octaves = list(octaves or [])
        windows = windows or {"pre": None, "cur": None}
        n_oct = 1 + len(octaves)
        groups = [{"pre": pre, "cur": cur}] + octaves
        blob.append(struct.pack("<IIIIIBB", EXT_MAGIC, EXT_VERSION, n_oct, int(size[0]), int(size[1]),
                                1 if windows.get("pre") is not None else 0, 1 if windows.get("cur") is not None else 0))
        for o in octaves:
            blob += _dump_group(o["pre"]) + _dump_group(o["cur"])
        for name in ("pre", "cur"):
            wn = windows.get(name)
            if wn is None:
                continue
            assert len(wn) == n_oct, "windows of a frame: one entry per octave"
            for o in range(n_oct):
                for side in ("left", "right"):
                    win, flag = wn[o][side]
                    flag = np.ascontiguousarray(flag, np.uint8).reshape(-1)
                    win = np.ascontiguousarray(win, np.uint8).reshape(len(flag), 64)
                    assert len(flag) == len(groups[o][name][side][0]), "a windows count must equal its list's count"
                    blob += [struct.pack("<Q", len(flag)), flag.tobytes(), win.tobytes()]
    with open(path, "wb") as f:
        f.write(b"".join(blob))


def read_state(path):
    buf = open(path, "rb").read()
    (npyr,) = struct.unpack_from("<Q", buf, 0); off = 8
    out = {"npyr": npyr}
    for name in ("pre", "cur"):
        lk, ld, off = _load_keypoints(buf, off)
        rk, rd, off = _load_keypoints(buf, off)
        m, ids, off = _load_matches(buf, off)
        out[name] = {"left": (lk, ld), "right": (rk, rd), "matches": m, "ids": ids}
    r, last_id, nkf, nfr, lm, kfm = struct.unpack_from("<BQQQQQ", buf, off); off += 41
    out.update(reset=bool(r), last_id=last_id, num_tracked_last_kf=nkf, num_tracked_last_frame=nfr, last_match_id=lm, kf_max_match_id=kfm)
    out.update(size=None, octaves=[], windows=None)
    if off == len(buf):
        return out
    assert len(buf) - off >= 22, "trailing bytes in the state file"
    magic, version, n_oct, w, h, hw_pre, hw_cur = struct.unpack_from("<IIIIIBB", buf, off); off += 22
    assert magic == EXT_MAGIC, "trailing bytes in the state file"
    assert version == EXT_VERSION and 1 <= n_oct <= 4 and hw_pre in (0, 1) and hw_cur in (0, 1), "unknown extension block"
    out["size"] = (w, h)
    for _ in range(1, n_oct):
        o = {}
        o["pre"], off = _load_group(buf, off)
        o["cur"], off = _load_group(buf, off)
        out["octaves"].append(o)
    groups = [{"pre": out["pre"], "cur": out["cur"]}] + out["octaves"]
    out["windows"] = {"pre": None, "cur": None}
    for name, has in (("pre", hw_pre), ("cur", hw_cur)):
        if not has:
            continue
        wn = []
        for o in range(n_oct):
            e = {}
            for side in ("left", "right"):
                (n,) = struct.unpack_from("<Q", buf, off); off += 8
                assert n == len(groups[o][name][side][0]), "a windows count differs from its list's count"
                flag = np.frombuffer(buf, np.uint8, n, off).copy(); off += n
                win = np.frombuffer(buf, np.uint8, n * 64, off).reshape(n, 8, 8).copy(); off += n * 64
                e[side] = (win, flag)
            wn.append(e)
        out["windows"][name] = wn
    assert off == len(buf), "trailing bytes behind the extension block"
    return out
