"""The inputs of the 16384-entry GPU tests (test_gpu_big_lists.py) have the properties those tests rely on -- from the oracle alone, no GPU:
the named lists hold more than 8192 and at most 16384 entries, frames 1 and 2 are valid, more than 1000 pairs are tracked."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_lists as B                                           # noqa: E402
import sad_ref as S                                             # noqa: E402
from oracle import oracle as O                                  # noqa: E402


def in_range(n):
    return B.LO < n <= B.HI


def test_case_a_orb_lists_exceed_8192():
    """orb_nfeats 10900: 16350 keypoints asked of the detector, 2 x 3551 corners ranked at level 0, more than 8192 kept after the NMS"""
    p = B.params_a()
    assert int(1.5 * p.orb_nfeats) == 16350 and 2 * O.level_quota(16350, 8)[0] == 7102
    assert int(1.5 * 11000) > B.HI                              # the request the GPU test expects to be refused
    recs = B.oracle_run(O, "A", p)
    for t, r in enumerate(recs):
        assert in_range(len(r["kl"][0])) and in_range(len(r["kr"][0])), (t, len(r["kl"][0]), len(r["kr"][0]))
        assert len(r["m"]) > 4096, (t, len(r["m"]))
        if t:
            assert r["valid"] and len(r["tracked"]) > 1000, (t, r["valid"], r["error_code"], len(r["tracked"]))


@pytest.mark.parametrize("ifm", [0, 1])
def test_case_b_every_corner_and_pairings_exceed_8192(ifm):
    """FAST+ORB without the NMS at threshold 5: keypoints AND pairings between 8192 and 16384 per frame, both trackers"""
    recs = B.oracle_run(O, "B%d" % ifm, B.params_b(ifm))
    for t, r in enumerate(recs):
        assert in_range(len(r["kl"][0])) and in_range(len(r["kr"][0])) and in_range(len(r["m"])), (t, len(r["kl"][0]), len(r["kr"][0]), len(r["m"]))
        if t:
            assert r["valid"] and len(r["tracked"]) > 1000, (t, r["valid"], r["error_code"], len(r["tracked"]))
            if ifm == 0:
                assert r["stats"][0] > B.LO, r["stats"]          # candidates of the brute-force tracker: the joint filter walks more than 8192


@pytest.mark.parametrize("one", [0, 1])
def test_case_b_prime_brute_force_matcher(one):
    """the same frames through the brute-force matcher: 14.5 k x 14.5 k descriptors, thousands of pairings, every frame >= 1 valid"""
    recs = B.oracle_run(O, "B'%d" % one, B.params_b(0, match_method=0, one_to_one=one))
    for t, r in enumerate(recs):
        assert in_range(len(r["kl"][0])) and in_range(len(r["kr"][0])), (t, len(r["kl"][0]), len(r["kr"][0]))
        assert len(r["m"]) > 4096, (t, len(r["m"]))
        if t:
            assert r["valid"], (t, r["error_code"])


def test_case_c_sad_walk_has_candidates():
    """case A's keypoints under smSAD / ifmSAD (window 40 x 40): the second frame is valid with at least 50 candidates"""
    p, cam = B.params_c(), B.camera()
    st = S.SadStream(O, p, cam)
    for t, (L, R) in enumerate(B.frames()[:2]):
        f = S.oracle_features(O, p, L, R, cam)
        assert in_range(len(f[0])) and in_range(len(f[2])), (t, len(f[0]), len(f[2]))
        o = st.step((L, R), f[0], f[2], f[4], f[5], f[1], f[3])
        assert len(o["matches"]) > 1000, (t, len(o["matches"]))
    assert o["valid"] and len(o["candidates"]) >= 50, (o["valid"], len(o["candidates"]))


def test_case_d_full_lists_are_exactly_full():
    """the blown-up lists of case D: exactly 16384 keypoints per side and pairings, indices in range, pairings in ascending left row,
    keypoint 16383 of both sides paired, and the oracle's stage 4 on them tracks something with repeated claims in play"""
    recs = B.oracle_run(O, "B0", B.params_b(0))
    prev, cur = B.full_lists(recs[0]), B.full_lists(recs[1])
    for kl, dl, kr, dr, m, ri in (prev, cur):
        assert len(kl) == len(kr) == len(m) == B.HI and dl.shape == dr.shape == (B.HI, 32)
        assert m["queryIdx"].max() == B.HI - 1 and m["trainIdx"].max() == B.HI - 1 and m["queryIdx"].min() >= 0 and m["trainIdx"].min() >= 0
        assert (np.diff(kl["y"][m["queryIdx"]]) >= 0).all() and ri[-1] == B.HI and (np.diff(ri) >= 0).all()
    p = B.params_b(0)
    zeros = np.zeros(B.H + 1, np.int64)
    tracked, ts = O.track(p, p.orb_max_distance, prev[0], prev[1], prev[2], prev[3], prev[4], zeros, cur[0], cur[1], cur[2], cur[3], cur[4], zeros, B.W, B.H, stats=True)
    assert ts[0] > B.LO and ts[0] > ts[1] > 1000 and len(tracked) > 100, (list(ts), len(tracked))     # collisions rejected candidates
