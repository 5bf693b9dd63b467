"""Preconditions of tests/test_gpu_ransac_forms.py, on the oracle alone (no GPU): the hand-built scenes of tests/ransac_scenes.py do put
pairs where the many-lane RANSAC kernels have their edges -- otherwise the GPU tests would pass without having reached them.

The error of every (model, pair) test is recomputed here in float64 numpy with the operation order of the oracle's fm_error
(ransac_scenes.fm_error_terms), for the models the oracle's own 7-point solve (O.seven_point) gives on the oracle's own samples
(O.ransac_samples); the counters are those of O.track(..., stats=True)."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd.abi import north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_scenes as RS                                                          # noqa: E402


def O():
    from oracle import oracle
    return oracle


@pytest.fixture(scope="module")
def facts(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    p = north_star_params(O().default_params(), orb_nfeats=int(g["orb_nfeats"]))
    return {nm: RS.scene_facts(p, RS.scene(nm)) for nm in RS.scene_names()}


def test_generators_give_exact_lists():
    """integer coordinates (the hair and near-epipole pairs: exact binary fractions), inside the image they are put with except for far_scene, right = left
    shifted by the integer disparity, every pairing continued by its own copy, the same lists from the same seed"""
    for nm in RS.scene_names():
        s = RS.scene(nm)
        p1, p2 = s["p1"].astype(np.float64), s["p2"].astype(np.float64)
        frac1, frac2 = p1 != np.round(p1), p2 != np.round(p2)
        assert (p2[frac2] == RS.HAIR).all() and set(p1[frac1] - 320.0) <= {v[0] for v in RS.NEAR}, nm
        assert (s["p1"].astype(np.float64) == p1).all() and np.float32(320.0 + 2.0 ** -14) != np.float32(320.0), nm
        inside = (p1 >= 0).all() and (p2 >= 0).all() and max(p1[:, 0].max(), p2[:, 0].max()) < s["W"] and max(p1[:, 1].max(), p2[:, 1].max()) < s["H"]
        assert inside == (not nm.startswith("far")), nm
        if nm.startswith("far"):
            assert p1.min() < 0 and p2[:, 0].max() > 3 * s["W"] and p2[:, 1].max() > 3 * s["H"], nm
        for a, b in (("pkl", "pkr"), ("ckl", "ckr")):
            assert (s[a]["x"] - s[b]["x"] == 20).all() and (s[a]["y"] == s[b]["y"]).all(), nm
        assert (s["pkl"]["x"] == p1[:, 0]).all() and (s["pkl"]["y"] == p1[:, 1]).all(), nm
        for prev, cur in ((s["pdl"], s["cdl"]), (s["pdr"], s["cdr"])):               # pairing k's descriptor sits once in the current list, where its point went
            for k in (0, len(prev) // 2, len(prev) - 1):
                at = np.flatnonzero((cur == prev[k]).all(1))
                assert len(at) == 1 and s["ckl"][at[0]]["x"] == p2[k, 0] and s["ckl"][at[0]]["y"] == p2[k, 1], (nm, k)
    for nm, gen, args in RS.SCENES[:3] + RS.SCENES[-1:]:
        a, b = gen(*args), gen(*args)
        assert all(np.array_equal(a[k], b[k]) for k in a), nm
    # a constant shift or zoom would be a homography (a degenerate 7-point problem): the motion varies from point to point
    for nm in RS.scene_names():
        s = RS.scene(nm)
        moved = s["p2"].astype(np.float64) - s["p1"]
        if len(moved) >= 8:
            assert len(np.unique(moved[:, 0])) >= 4, nm


def test_candidate_counts_cover_the_kernel_edges(facts):
    """every pairing of a hand-built scene reaches the RANSAC (track_stats[1]); together: 6, 7, 8, 14, 15, 16, 17, 31, 32, 33, 255, 256, 257,
    272 and one above 512"""
    for nm, f in facts.items():
        assert f["ts"][0] == f["ts"][1] == len(RS.scene(nm)["p1"]), (nm, f["ts"])
    seen = {f["ts"][1] for f in facts.values()}
    assert set(RS.CANDIDATE_COUNTS) <= seen and max(seen) > 512, sorted(seen)


def test_border_pairs_sit_inside_the_band(facts):
    """every sideways / forward / far scene in which a sampler runs (8 candidates or more: below that there is no model): at least 8 (model,
    pair) tests within 2^-22 of 1 over the models of the first 160 samples; at least two scenes with such a pair on the winning model"""
    for nm, f in facts.items():
        if f["ts"][1] >= 8:
            assert f["near"] >= 8, (nm, f)
    assert sum(f["win_near"] >= 1 for f in facts.values()) >= 2, {nm: f["win_near"] for nm, f in facts.items()}


def test_hair_pairs_are_outliers_just_past_the_band(facts):
    """the sideways / far scenes from 15 candidates on: tests with 1 + 2^-24 < error <= 1 + 2^-20, i.e. outliers (the float error is above
    1.0f) that a screen with a misplaced lower edge would count"""
    for nm, f in facts.items():
        if not nm.startswith("forward") and f["ts"][1] >= 15:
            assert f["hair"] >= 1, (nm, f)
    assert np.float32(RS.HAIR) == RS.HAIR and np.float32(RS.HAIR * RS.HAIR) > np.float32(1.0)


def test_epipole_pairs_fail_the_guards_and_give_nan(facts):
    """every forward scene (all have pairs on the epipole): a model under which such a pair's error is NaN (|l|^2 == 0 and d == 0: the
    oracle's 0 * inf), and a model under which its |l|^2 is positive but below the guard (2^28 E)^2 of store_model.  For the 8..14-candidate
    scenes the NaN is among the errors whose median LMedS takes (fm_error_key's ordering decides where it sorts)."""
    fw = [nm for nm in facts if nm.startswith("forward")]
    assert len(fw) >= 5 and sum(8 <= facts[nm]["ts"][1] <= 14 for nm in fw) >= 2
    for nm in fw:
        assert facts[nm]["nan"] >= 1 and facts[nm]["small"] >= 1, (nm, facts[nm])
        if 8 <= facts[nm]["ts"][1] <= 14:
            assert facts[nm]["ts"][4:6] == [300, 300], (nm, facts[nm])               # LMedS: its fixed budget (all 300 samples' models were looked at above)


def test_near_epipole_pairs_are_the_guards_alone_to_catch(facts):
    """the forward scenes with border pairs a few 2^-14 px beside the epipole: at least 8 tests with the error within 2^-20 of 1 on a line
    whose |l|^2 is positive but below the guard -- the matrix cores' d is good to ~1e-7 of such a line at best, far coarser than the
    band, so a screen without guards would give verdicts of its own"""
    for nm in ("forward-24", "forward-48", "forward-64", "forward-120"):
        assert facts[nm]["guarded"] >= 8, (nm, facts[nm])


def test_samples_visited_reach_every_chunk(facts):
    """by the oracle's samples-visited counters: a scene that ends within the many-lane schedule's first chunk (<= 32), one within the second
    (<= 160) and one beyond (the `rs_floor` early exit of chunks 1 and 2 then has contaminated lists to work on)"""
    visited = sorted(max(f["ts"][4], f["ts"][5]) for f in facts.values() if f["ts"][1] >= 15)
    assert any(0 < v <= 32 for v in visited) and any(32 < v <= 160 for v in visited) and any(v > 160 for v in visited), visited


def test_error_replica_agrees_with_the_oracle(golden_dir):
    """fm_error_terms is the oracle's expression: thresholding it reproduces the oracle's own inlier mask and count on the winning model"""
    for nm in ("sideways-255", "forward-150", "forward-272", "far-257"):
        s = RS.scene(nm)
        cnt, mask, F, best, visited = O().ransac_fundamental(s["p1"], s["p2"])
        e, _, _ = RS.fm_error_terms(F, s["p1"], s["p2"])
        with np.errstate(invalid="ignore"):
            mine = e <= np.float32(1.0)
        assert best >= 0 and (mine == mask.astype(bool)).all() and int(mine.sum()) == cnt, nm
