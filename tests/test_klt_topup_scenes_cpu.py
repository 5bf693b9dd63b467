"""Every scene of tests/klt_topup_scenes.py does what it claims, on the numpy walk of tests/klt_topup_ref.py (tests/gftt_ref.py,
tests/lk_ref.py and the gate of tests/klt_ref.py).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402
import klt_topup_scenes as TS                                                          # noqa: E402

F = np.float32
NAMES = [s.name for s in TS.scenes()]


@pytest.mark.parametrize("name", NAMES)
def test_scene_reaches_what_it_claims(name):
    s = TS.scene(name)
    e = s.expect
    t0, t1, info, det = TS.walk(name)
    assert info[0] == e["corners"] and info[2] == e["appended"] and info[3] == e["reason"], (name, info)
    assert len(t1) == e.get("n_after", len(t0) + e["appended"])
    if e["reason"] != TR.OK:
        assert t1 is t0
        return
    n0 = len(t0)
    # what was there stays; what is new has fresh IDs, age 0 and no indices
    assert t1.left[:n0].tobytes() == t0.left.tobytes() and np.array_equal(t1.ids[:n0], t0.ids)
    assert np.array_equal(t1.ids[n0:], np.arange(t0.next_id, t0.next_id + info[2])) and not t1.age[n0:].any()
    assert (t1.idx[n0:] == -1).all() and (t1.pidx[n0:] == -1).all() and t1.next_id == t0.next_id + info[2]
    if det is None or not len(det["corners"]):
        return
    c, o, st = det["corners"], det["partners"], det["status"]
    if "status_ones" in e:
        assert int((st == 1).sum()) == e["status_ones"]
    if "status_zero" in e:
        # corner k of a scene without tracks is blob k: the grid is walked in raster order
        assert sorted(np.flatnonzero(st == 0).tolist()) == sorted(e["status_zero"])
    if "disparity" in e:
        d = (c[:, 0] - o[:, 0])[det["keep"]]
        assert len(d) and np.abs(d - e["disparity"]).max() < 0.01
    if "dy" in e:
        found = st == 1
        assert found.sum() >= len(c) // 2 and (np.abs(np.abs(c[found, 1] - o[found, 1]) - e["dy"]) < 0.05).all()
        assert (np.abs(c[found, 0] - o[found, 0] - 1.0) < 0.05).all()          # only max_dy stands between these pairs and the table
    if e.get("first_corner"):
        assert tuple(c[0]) == e["first_corner"]
    if e.get("absent"):
        assert e["absent"] not in [tuple(p) for p in c.tolist()]


def test_the_two_seed_scenes_differ_only_in_the_seed():
    a, b = TS.scene("seed_inside"), TS.scene("seed_just_outside")
    assert a.left.tobytes() == b.left.tobytes() and a.gftt == b.gftt
    cx, cy = b.expect["first_corner"]
    md = a.gftt["min_distance"]
    for s, closer in ((a, True), (b, False)):
        fx, fy = F(cx) - s.tracks[0][0, 0], F(cy) - s.tracks[0][0, 1]
        assert bool(F(fx * fx) + F(fy * fy) < F(md * md)) == closer
    # ... and for the second one double precision would have said "closer": the float32 rule in the direction gftt_ref.py documents
    sx, sy = (float(v) for v in b.tracks[0][0])
    assert (cx - sx) ** 2 + (cy - sy) ** 2 < md * md


def test_seam_interleaves_across_wave_and_chunk_seams():
    s = TS.seam()
    t0, t1, info, det = TS.walk("seam")
    assert info == (559, 567, s.expect["appended"], TR.OK) and info[0] > 512 and s.cap >= 600
    keep = det["keep"]
    assert np.array_equal(keep, s.expect["keep"])
    for a in (63, 127, 255, 511):                        # the last slot of a wave / a chunk and the first of the next
        assert keep[a] != keep[a + 1], a
    for a in range(63, len(keep) - 2, 64):               # ... and every wave seam has both kinds within two slots of it
        assert keep[a - 1:a + 3].any() and not keep[a - 1:a + 3].all(), a
    assert len(t0) == TS.SEAM_TRACKS > 0 and len(t1) == s.expect["n_after"] <= s.cap
    # the rejects are the erased blobs: status 1 at disparity 0, dropped by min_disp
    rej = ~keep
    assert (det["status"] == 1).all() and (det["corners"][rej, 0] == det["partners"][rej, 0]).all()


def test_overflow_image_overflows():
    import gftt_ref as GR
    im = TS.overflow_image()
    _, _, info, _ = GR.detect(im, None, TS.CAP, GR.GfttParams(**TS.GFTT), cand_cap=max(1024, TS.MAX_CAND))
    assert info[2] == 1 and info[1] > max(1024, TS.MAX_CAND) and info[0] == 0


def test_append_arrays_against_the_gate():
    left, right, status, ok = TS.append_arrays()
    g = KR.Gate(win=TS.WIN, **TS.GATE)
    assert np.array_equal(TR.gate_pass(left, right, status, g), ok)
    assert ok.any() and (~ok).any() and not np.isfinite(left).all() and not np.isfinite(right).all() and set(status) >= {0, 1, 2, 255}
    # into an empty table, into a full one, and one past cap
    t, m, _ = TR.append(KR.Table(), left, right, status, g, TS.CAP)
    assert m == int(ok.sum()) and np.array_equal(t.ids, np.arange(m))
    full, _ = KR.add_points(KR.Table(), *TS.tracks_on([(10 + k, 10) for k in range(TS.CAP)]), TS.CAP)
    t, m, _ = TR.append(full, left, right, status, g, TS.CAP)
    assert m == 0 and t.next_id == full.next_id
    almost, _ = KR.add_points(KR.Table(), *TS.tracks_on([(10 + k, 10) for k in range(TS.CAP - int(ok.sum()) + 1)]), TS.CAP)
    t, m, _ = TR.append(almost, left, right, status, g, TS.CAP)
    assert m == int(ok.sum()) - 1 and len(t) == TS.CAP


def test_want_of():
    tp = TR.TopupParams(64)
    assert (tp.below, tp.target, float(tp.init_disp)) == (32, 64, 0.0)
    assert TR.want_of(32, 64, tp) is None and TR.want_of(31, 64, tp) == 33 and TR.want_of(0, 64, tp) == 64
    assert TR.want_of(5, 64, TR.TopupParams(64, below=10, target=4)) == 0
