"""The hand-built SAD scenes of tests/sad_scenes.py without a GPU: tests/sad_ref.py's walks give what each construction predicts, every
label is there and every planned pairing is kept, stage 4's composed filter keeps every candidate -- and every rule the scenes are
named for, broken on purpose in the walk (sad_ref's `mutant`), changes the outcome of its scene.  A scene that no mutant changes proves
nothing; the last test refuses it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sad_ref as S                                             # noqa: E402
import sad_scenes as SS                                         # noqa: E402
from oracle import oracle as O                                  # noqa: E402

OUTSIDE = "window outside the image"


def walk3(s, variant, robust, mutant=None):
    """smSAD's walk on a scene: [(left, right, SAD)], or OUTSIDE where the walk asks for a window the image does not hold"""
    v = dict(SS.STEREO_DEFAULTS, **variant)
    try:
        m = S.match_lr_sad(s["imgs"][0], s["imgs"][1], s["kl"], s["kr"], SS.features_row_index(s["kl"], s["H"]), SS.features_row_index(s["kr"], s["H"]),
                           v["sad_max_distance"], v["max_y_diff"], robust, v["minimum_ORB_response"], mutant=mutant)
    except AssertionError as e:
        assert OUTSIDE in str(e)
        return OUTSIDE
    assert (m["imgIdx"] == -1).all() and (m["distance"] == np.floor(m["distance"])).all()
    return [(int(q), int(t), int(d)) for q, t, _, d in m.tolist()]


def walk4(s, variant, mutant=None, skip_flagged=True):
    """ifmSAD's walk (with the library's flag rule unless told otherwise): [(previous, current)] or OUTSIDE"""
    v = dict(SS.TRACK_DEFAULTS, **variant)
    pf, cf = SS.frames(s)
    try:
        pot = S.track_sad(pf, cf, v["ifm_win_w"], v["ifm_win_h"], v["ifm_sad_max_distance"], skip_flagged=skip_flagged, mutant=mutant)
    except AssertionError as e:
        assert OUTSIDE in str(e)
        return OUTSIDE
    return [(int(a), int(b)) for a, b in pot.tolist()]


# the number of pairings / candidate pairs per variant, counted by hand from each scene's docstring
STEREO_COUNTS = {"sad_threshold": [5, 2, 5, 10, 10], "sad_ties": [5], "sad_one_to_one": [5], "sad_border": [7, 7], "sad_disparity": [5],
                 "sad_rows": [0, 2, 4, 6], "sad_response": [4, 2]}
STEREO_LABELS = {"sad_threshold": 10, "sad_ties": 5, "sad_one_to_one": 10, "sad_border": 13, "sad_disparity": 11, "sad_rows": 7, "sad_response": 4}
TRACK_COUNTS = {"trk_gates": [3, 6, 9, 9], "trk_sums": [7, 7], "trk_window": [7], "trk_rows": [4, 2], "trk_flags": [1]}
TRACK_LABELS = {"trk_gates": 9, "trk_sums": 11, "trk_window": 14, "trk_rows": 9, "trk_flags": 7}


@pytest.mark.parametrize("name", SS.stereo_names())
def test_stage3_walk_gives_what_the_construction_predicts(name):
    s = SS.scene(name)
    assert len(s["label"]) == STEREO_LABELS[name] + 1 and s["label"][-1] == "last row" and len(set(s["label"])) == len(s["label"])
    assert len(s["variants"]) == len(STEREO_COUNTS[name])
    reached = set()
    for v, n in zip(s["variants"], STEREO_COUNTS[name]):
        for robust in (0, 1):
            want = s["want"](v, robust)
            assert walk3(s, v, robust) == want, (name, v, robust)
            assert len(want) == n, (name, v, robust, len(want))
            reached |= {i for i, _, _ in want}
    # every left keypoint with a plan is paired under some variant, and none without one ever is
    # (but for a claimant that is beaten under either rule)
    planned = {i for i, plan in enumerate(s["plan"]) if any(c is None or c(dict(SS.STEREO_DEFAULTS, **v)) for _, _, c in plan for v in s["variants"])}
    assert len(planned) == sum(1 for plan in s["plan"] if plan) - (name == "sad_rows")     # (off=3 is in no range: row r meets r - d .. r + d - 1)
    assert reached <= planned and all(s["label"][i].startswith("claim") for i in planned - reached), (name, [s["label"][i] for i in planned - reached])
    if name == "sad_one_to_one":                                                  # the two rules do differ, and the second choice stays free
        assert s["want"](s["variants"][0], 0) != s["want"](s["variants"][0], 1)
        assert all(j != s["right_at"]["alt"] for r in (0, 1) for _, j, _ in s["want"](s["variants"][0], r))
    if name == "sad_threshold":                                                   # DMatch.distance is the planted SAD, 14 bits of it
        assert [d for _, _, d in s["want"](dict(sad_max_distance=-1), 1)] == SS.THRESHOLD_DS


@pytest.mark.parametrize("name", SS.track_names())
def test_stage4_walk_gives_what_the_construction_predicts(name):
    s = SS.scene(name)
    assert len(s["label"]) == TRACK_LABELS[name] and len(set(s["label"])) == len(s["label"])
    assert len(s["variants"]) == len(TRACK_COUNTS[name])
    pf, cf = SS.frames(s)
    reached = set()
    for v, n in zip(s["variants"], TRACK_COUNTS[name]):
        want = s["want"](v)
        assert walk4(s, v) == want, (name, v)
        assert len(want) == n, (name, v, len(want))
        reached |= {pi for pi, _ in want}
        pot = np.array(want, S.index_pair_dtype)
        tracked, stats = S.filter_candidates(O, pf, cf, pot)                      # the RANSAC must not hide a wrong candidate list
        assert tracked.tobytes() == pot.tobytes() and stats[0] == stats[1] == stats[6] == stats[7] == n, (name, v, stats)
    claimed = {ci for plan in s["plan"] for ci, _, _, _ in plan}
    losers = {pi for pi, plan in enumerate(s["plan"]) if plan and pi not in reached}
    assert all("claim" in s["label"][pi] for pi in losers), (name, [s["label"][pi] for pi in losers])     # only a beaten claimant is never kept
    assert claimed, name
    if name != "trk_flags":                                                       # without flagged pairings the reference's own walk is the same
        for v in s["variants"]:
            assert walk4(s, v, skip_flagged=False) == s["want"](v), (name, v)


def test_two_octaves_and_large_indices():
    s0, s1, imgs0 = SS.scene("trk_octaves")
    assert imgs0[0].shape == (SS.H, SS.W) and s1["pimgs"][0].shape == (SS.H // 2, SS.W // 2)
    for v, n in zip(s1["variants"], [3, 6, 6]):                                   # 191: (192, *) and (*, 192) dropped; (128, 256) and x = W/2 - 4.99 never
        assert walk4(s1, v) == s1["want"](v) and len(s1["want"](v)) == n, (v, n)
        assert walk4(s1, v, skip_flagged=False) == s1["want"](v)
    assert len(walk4(s0, dict(ifm_sad_max_distance=192))) == 2 and walk4(s0, dict(ifm_sad_max_distance=191)) == []
    s3, s4 = SS.scene("big_index")
    v = s3["variants"][0]
    for robust in (0, 1):
        want = s3["want"](v, robust)
        assert walk3(s3, v, robust) == want and len(want) == 2 and min(j for _, j, _ in want) >= 8192 and max(d for _, _, d in want) == 16320
    want = s4["want"](s4["variants"][0])
    assert walk4(s4, s4["variants"][0]) == want and len(want) == 2 and all(pi >= 8192 for pi, _ in want) and len(s4["pm"]) == SS.N_FILL + 3


# ---------------------------------------------------------------------------------------------------------------------------------------
# mutants: one rule of the walk broken at a time -> the scenes that must notice
# ---------------------------------------------------------------------------------------------------------------------------------------
MUTANTS_S3 = {
    "ge_threshold": ["sad_threshold", "sad_disparity", "sad_border"], "and_ff": ["sad_threshold", "sad_one_to_one", "big_index"],
    "le_min": ["sad_ties"], "le_claim": ["sad_one_to_one"], "round_pt": ["sad_border"], "py_round": ["sad_rows"], "no_flag": ["sad_border"],
    "round_disparity": ["sad_disparity"], "le_response": ["sad_response"],
}
MUTANTS_S4 = {
    "ge_left": ["trk_gates", "trk_window", "trk_octaves"], "ge_right": ["trk_gates", "trk_window", "trk_octaves"], "and_ff": ["trk_sums", "big_index"],
    "le_min": ["trk_sums"], "le_claim": ["trk_sums"], "sum_gate": ["trk_gates"], "round_pt": ["trk_window"], "no_flag": ["trk_flags"],
    "oct0_size": ["trk_octaves"],
    # the two clamps keep the reference's walk inside the image; under the library's flag rule every keypoint they exclude is flagged
    # anyway, so they are tried on the walk without it (which equals the other on these scenes: asserted above)
    "lo0": ["trk_window", "trk_rows"], "awx": ["trk_window"],
}


def _stage3(name):
    return SS.scene(name)[0] if name == "big_index" else SS.scene(name)


def _stage4(name):
    return SS.scene(name)[1] if name in ("big_index", "trk_octaves") else SS.scene(name)


def red3(name, mutant):
    s = _stage3(name)
    return [(v, r) for v in s["variants"] for r in (0, 1) if walk3(s, v, r, mutant) != s["want"](v, r)]


def red4(name, mutant):
    s = _stage4(name)
    raw = mutant in ("lo0", "awx")
    return [v for v in s["variants"] if walk4(s, v, mutant, skip_flagged=not raw) != s["want"](v)]


@pytest.mark.parametrize("mutant", sorted(MUTANTS_S3))
def test_stage3_mutants_turn_their_scenes_red(mutant):
    for name in MUTANTS_S3[mutant]:
        assert red3(name, mutant), (mutant, name, "not noticed")


@pytest.mark.parametrize("mutant", sorted(MUTANTS_S4))
def test_stage4_mutants_turn_their_scenes_red(mutant):
    for name in MUTANTS_S4[mutant]:
        assert red4(name, mutant), (mutant, name, "not noticed")


def test_every_mutant_is_tried_and_every_scene_is_turned_red():
    assert set(MUTANTS_S3) == set(S.MUTANTS_S3) and set(MUTANTS_S4) == set(S.MUTANTS_S4)
    named3, named4 = {n for v in MUTANTS_S3.values() for n in v}, {n for v in MUTANTS_S4.values() for n in v}
    assert named3 == set(SS.stereo_names()) | {"big_index"} and named4 == set(SS.track_names()) | {"big_index", "trk_octaves"}
    # the walks with no mutant selected are the ones tests/test_sad_cpu.py pins on the photograph: nothing is red
    assert not any(red3(n, None) for n in named3) and not any(red4(n, None) for n in named4)
