"""Preconditions of tests/test_gpu_ham_scenes.py, on the oracle alone (no GPU): on every list of tests/ham_scenes.py the oracle's stage 3
and stage 4 return exactly what popcount and numpy's argmin predict -- one pairing per left keypoint, so no filter hides a word of the
matcher --, and the scenes do reach the edges k_hamming_f4 is built around (counted from the scenes themselves).  The float32 arithmetic
of the kernel's accumulator key is held as a test too: exact and strictly ordered over every (distance, index)."""
import os
import sys

import numpy as np

from stereo_vo_amd.abi import north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ham_scenes as HS                                                              # noqa: E402


def O():
    from oracle import oracle
    return oracle


def params():
    return north_star_params(O().default_params(), orb_nfeats=600)


def all_stereo():
    return HS.stereo_names() + HS.wide_names()


def test_generators_are_deterministic_and_in_row_order():
    for nm, gen, args in HS.STEREO + HS.WIDE[:2] + HS.TRACK:
        a, b = HS.scene(nm), gen(*args)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), (nm, k)
    for nm in all_stereo():
        s = HS.scene(nm)
        assert (s["kl"]["y"] == HS.ROW).all() and (s["kr"]["y"] == HS.ROW).all(), nm
        if len(s["kl"]) and len(s["kr"]):
            assert s["kl"]["x"].min() - s["kr"]["x"].max() >= 2 and s["kl"]["x"].max() - s["kr"]["x"].min() < 267, nm
        assert len(np.unique(s["kr"]["x"])) == len(s["kr"]) and len(np.unique(s["kl"]["x"])) == len(s["kl"]), nm      # 1 / 64 steps: exact
    for nm in HS.track_names() + [HS.TRACK_WIDE[0][0]]:
        s = HS.scene(nm)
        for kl, kr, m in ((s["pkl"], s["pkr"], s["pm"]), (s["ckl"], s["ckr"], s["cm"])):
            assert (np.diff(kl["y"]) >= 0).all() and (np.diff(kr["y"]) >= 0).all(), nm                        # both lists in row order
            assert (np.diff(m["queryIdx"]) > 0).all() and len(set(m["trainIdx"])) == len(m), nm              # queryIdx ascending, trainIdx a permutation
            assert len(kl) > len(m) and (m["queryIdx"] != np.arange(len(m))).any() and (m["trainIdx"] != m["queryIdx"]).any(), nm     # no identity
            assert (kl["x"][m["queryIdx"]] - kr["x"][m["trainIdx"]] == 20).all() and (kl["y"][m["queryIdx"]] == kr["y"][m["trainIdx"]]).all(), nm


def test_oracle_stage3_is_popcount_and_argmin_on_every_scene():
    """oracle.match_lr byte for byte the numpy array, one pairing per left keypoint (none for an empty side), and its row table"""
    p = HS.stereo_params(params())
    total = 0
    for nm in all_stereo():
        s = HS.scene(nm)
        m, ri = HS.oracle_match(p, s)
        assert len(m) == (len(s["kl"]) if len(s["kr"]) else 0), (nm, len(m))
        assert m.tobytes() == s["want"].tobytes(), nm
        assert list(ri) == list(s["want_ri"]), nm
        idx, dist = O().hamming_bf(s["dl"], s["dr"])
        if len(s["kr"]) and len(s["kl"]):
            assert (idx == s["D"].argmin(1)).all() and (dist == s["D"].min(1)).all(), nm
        total += 1
    assert total == sum(HS.FAMILY_COUNTS.values())
    # the octave-1 list of the two-octave lane, under the half-size image it is matched in
    s = HS.scene(HS.OCTAVES[1])
    m, ri = HS.oracle_match(p, s, (s["W"] // 2, s["H"] // 2))
    assert m.tobytes() == s["want"].tobytes() and list(ri) == list(s["want_ri"][:s["H"] // 2 + 1])


def test_oracle_stage4_is_popcount_and_argmin_through_the_pairing_lists():
    """oracle.track returns exactly the numpy pairs; every previous pairing finds its planted current pairing on both sides (the first of
    the copies), and each is tracked unless an earlier previous pairing took its target"""
    p = HS.track_params(params())
    for nm in HS.track_names() + [HS.TRACK_WIDE[0][0]]:
        s = HS.scene(nm)
        trk, ts = HS.oracle_track(p, s, key=("ham-scenes", nm))
        assert trk.tobytes() == s["want"].tobytes(), (nm, len(trk), len(s["want"]))
        t = s["plan_t"]
        assert (s["tL"] == t).all() and (s["tR"] == t).all(), nm
        first = [k for k in range(len(t)) if t[k] not in set(t[:k])]
        assert [(int(a), int(b)) for a, b in zip(s["want"]["first"], s["want"]["second"])] == [(k, int(t[k])) for k in first], nm
        assert [int(v) for v in ts[:2]] == [len(t), len(first)] and int(ts[7]) == len(first), (nm, list(ts))
    # sizes: every nprev and every ncur of the list, collisions where there are more previous pairings than current ones
    assert sorted(set(a for a, _ in HS.TRACK_SIZES)) == [32, 33, 255, 256, 257] and sorted(set(b for _, b in HS.TRACK_SIZES)) == [33, 64, 65, 97, 257]
    assert len(HS.scene("track-257-97")["want"]) < 97 and len(HS.scene("track-wide-300-8200")["want"]) == 300


def test_stage4_plants():
    for nm in HS.track_names() + [HS.TRACK_WIDE[0][0]]:
        s = HS.scene(nm)
        cm, ncur = s["cm"], len(s["cm"])
        kinds = [k for k, _, _ in s["plants"]]
        assert kinds.count("both") == 1 and kinds.count("left") == 1 and kinds.count("tile") >= 1, nm
        for kind, a, b in s["plants"]:
            assert a < b and (s["cdl"][cm["queryIdx"][a]] == s["cdl"][cm["queryIdx"][b]]).all(), (nm, kind)
            assert (s["cdr"][cm["trainIdx"][a]] == s["cdr"][cm["trainIdx"][b]]).all() == (kind != "left"), (nm, kind)
            k = int(np.flatnonzero(s["plan_t"] == a)[0])                          # the previous pairing that wants it: a tie on the left, on the right unless `left`
            assert list(np.flatnonzero(s["DL"][k] == s["dL"][k])) == [a, b] and (a in s["want"]["second"]) and (b not in s["want"]["second"]), (nm, kind)
            assert list(np.flatnonzero(s["DR"][k] == s["dR"][k])) == ([a] if kind == "left" else [a, b]), (nm, kind)
            if kind == "tile":
                assert a % 32 == 31 and b == a + 1 or nm.startswith("track-wide"), (nm, a, b)     # across a tile boundary of the PAIRING order ...
                assert cm["queryIdx"][b] > b, nm                                        # ... which is not the keypoint order
        if not nm.startswith("track-wide"):
            assert sum(k == "tile" for k in kinds) == (ncur - 1) // 32, nm           # every tile boundary of the current pairing list
        # decoys: unpaired current keypoints, index below ncur, that hold a query exactly -- nearer than anything paired, never matched
        for k, ul, ur in s["decoys"]:
            assert ul < ncur and ur < ncur and ul not in cm["queryIdx"] and ur not in cm["trainIdx"], nm
            assert (s["cdl"][ul] == s["pdl"][s["pm"]["queryIdx"][k]]).all() and (s["cdr"][ur] == s["pdr"][s["pm"]["trainIdx"][k]]).all() and s["dL"][k] > 0 and s["dR"][k] > 0, nm
    s = HS.scene("track-wide-300-8200")
    assert {0, 4095, 8191, 8193, 8199} <= set(int(v) for v in s["want"]["second"]) and 8192 not in s["want"]["second"]


def test_stage3_scenes_reach_the_edges():
    """counted from the scenes: every tile row wins a tie, against every class of partner; every tile boundary of the 289-row list
    carries a tie, won by the last row of a tile and by the first; every planted distance is a realised minimum at every planted place;
    the wide lists have winners on both sides of 8191 / 8192"""
    fam = {f: [nm for nm in all_stereo() if HS.scene(nm)["family"] == f] for f in HS.FAMILY_COUNTS}
    assert {f: len(v) for f, v in fam.items()} == HS.FAMILY_COUNTS
    assert sorted((len(HS.scene(nm)["kl"]), len(HS.scene(nm)["kr"])) for nm in fam["lengths"]) == sorted(HS.LENGTHS)
    nqs, nts = [a for a, _ in HS.LENGTHS], [b for _, b in HS.LENGTHS]
    assert all(len(set(b for a, b in HS.LENGTHS if a == nq)) >= 2 for nq in (1, 31, 32, 33, 64, 65, 255, 256, 257, 513)) and set(nqs) == {1, 31, 32, 33, 64, 65, 255, 256, 257, 513}
    assert set(nts) == {1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129, 255, 256, 257, 289}
    # ties: (winning row in its tile, class) over the tie scene
    s = HS.scene("ties-positions")
    won = set()
    for q, cls, a, b in s["plan"]:
        assert list(HS.minima(s["D"])[q]) == [a, b] and s["want"]["trainIdx"][q] == a
        won.add((a % 32, cls))
        assert {"next": b - a in (1, 5), "half": (a ^ b) & 4 == 4 and b - a == 4, "tile": b - a == 32, "last": b == len(s["kr"]) - 1}[cls], (a, b, cls)
    assert won == {(r, c) for r in range(32) for c in ("next", "half", "tile", "last")} and len(s["kr"]) == 128
    regs = {(a % 32, b % 32) for _, cls, a, b in s["plan"] if cls == "next" and a % 4 < 3}
    assert all(a // 4 == b // 4 for a, b in regs) and len(regs) == 24            # same lane half, same group of four registers
    last, first = HS.scene("ties-289-last"), HS.scene("ties-289-first")
    assert len(last["kr"]) == 289 and [(a, b) for _, _, a, b in last["plan"]] == [(32 * k - 1, 32 * k) for k in range(1, 10)]
    assert [a for _, _, a, _ in first["plan"]] == [32 * k for k in range(1, 9)] and all(b // 32 > a // 32 for _, _, a, b in first["plan"])
    for s in (last, first):
        for q, _, a, b in s["plan"]:
            assert list(HS.minima(s["D"])[q]) == [a, b] and s["want"]["trainIdx"][q] == a
    # random lists tie on their own as well (nobody planted these)
    natural = sum(sum(len(m) > 1 for m in HS.minima(HS.scene(nm)["D"])) for nm in fam["lengths"] if len(HS.scene(nm)["kr"])) - sum(sum(k == "tie" for _, k, _, _ in HS.scene(nm)["plan"]) for nm in fam["lengths"])
    assert natural >= 20, natural
    # distances
    seen = set()
    for nm in fam["distances"]:
        s = HS.scene(nm)
        for q, _, w, d in s["plan"]:
            assert s["want"]["trainIdx"][q] == w and s["want"]["distance"][q] == d
            seen.add((d, w))
    assert seen == {(d, w) for d in HS.DIST[:-1] for w in HS.DIST_WINNERS} | {(256, 0)}
    assert (HS.scene("dist-256")["D"] == 256).all() and (HS.scene("dist-255-32")["D"] >= 255).all()
    # wide lists
    seen, ties, lens = set(), set(), set()
    for nm in fam["wide"]:
        s = HS.scene(nm)
        lens.add(len(s["kr"]))
        for q, kind, a, b in s["plan"]:
            assert s["want"]["trainIdx"][q] == a
            if kind == "tie":
                ties.add((a, b, len(s["kr"])))
            else:
                assert s["want"]["distance"][q] == b
                seen.add((b, a if a in (0, 8191, 8192, 8193) else "last" if a == len(s["kr"]) - 1 else a))
    assert lens == set(HS.WIDE_NT) | {8225}
    assert {(d, w) for d in (0, 1) for w in (0, 8191, 8192, 8193, "last")} | {(d, w) for d in (127, 128) for w in (8191, 8192)} | {(256, 0)} <= seen
    assert {(8191, 8192, nt) for nt in (8193, 8225, 16383, 16384)} | {(8192, nt - 1, nt) for nt in (8225, 16383, 16384)} == ties
    won = np.concatenate([HS.scene(nm)["want"]["trainIdx"] for nm in fam["wide"]])
    assert (won < 8191).sum() >= 20 and (won > 8192).sum() >= 20 and (won >= 16383).any() and ((won & 8191) > 8000).any()
    # lanes: five lists of five lengths, an empty train list, an empty query list; two octaves with lists of their own
    shapes = [(len(HS.scene(nm)["kl"]), len(HS.scene(nm)["kr"])) for nm in HS.LANES]
    assert len(set(shapes)) == 5 and (40, 0) in shapes and (0, 40) in shapes and len(HS.scene("lane-40-0")["want"]) == 0
    assert HS.OCTAVES[0] != HS.OCTAVES[1]


def test_accumulator_key_is_exact_and_ordered():
    """k_hamming_f4's key row / 8192 + (2 ham - 256) + j0 / 8192 in binary32: exact for every ham 0 .. 256 and every index 0 .. 16383,
    strictly increasing in (ham, index), and both unpack forms give (ham, index) back -- the plain one (index = key - floor(key)) up to
    index 8191 only, which is why the wide lists need the other"""
    ham, idx = np.meshgrid(np.arange(257), np.arange(16384), indexing="ij")
    key = HS.f4_key(ham, idx % 32, idx - idx % 32)
    assert key.dtype == np.float32
    assert (key.astype(np.float64) == (2 * ham - 256) + idx / 8192.0).all()
    flat = key.reshape(-1)
    assert (np.diff(flat) > 0).all()                                               # ordered by distance first, index second
    h, i = HS.f4_unpack(key, wide=True)
    assert (h == ham).all() and (i == idx).all()
    h, i = HS.f4_unpack(key[:, :8192], wide=False)
    assert (h == ham[:, :8192]).all() and (i == idx[:, :8192]).all()
    h, i = HS.f4_unpack(key[:, 8192:], wide=False)
    assert (i != idx[:, 8192:]).all()                                              # floor(key) is odd there: the plain form loses index bit 13
    # the masked rows of a ragged tile (1e9) and the running minimum's start (3e38) lose against every key; a key never reaches the "nothing found" bound
    assert flat.max() < np.float32(1.0e8) < np.float32(1.0e9) < np.float32(3.0e38)
