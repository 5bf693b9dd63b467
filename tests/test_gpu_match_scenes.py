"""The pairing filters of stage 3 (k_match_lr_filter, k_match_lr_rbr<false>, lr_row_index) and the front end of stage 4
(k_track_filter<16|32|64>, k_track_win<false>), with k_hamming_f4 underneath, on the hand-built lists of tests/match_scenes.py: distances on
the threshold, disparities and row differences on their (int) truncations, 1-to-1 ties, the 8-bit accumulator's wrap, conflict chains that
need thousands of rounds, the three storage forms of the joint filter, negative and border rows, empty and one-entry lists.
tests/test_match_scenes_cpu.py asserts on the oracle alone that the scenes do reach those edges and that the oracle agrees with the
independent Python walks there.

Stage 3 / stage 4 alone on caller-supplied lists, byte for byte against the oracle.  Every test needs a real MI355X: `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_scenes as MS                                                            # noqa: E402
import ransac_scenes as RS                                                           # noqa: E402

pytestmark = pytest.mark.gpu


def params():
    return north_star_params(hip.default_params(), orb_nfeats=600)      # (the detector is not run: its quota only has to fit the smallest context)


def context(n_lanes=1, max_kps=1024, p=None):
    ctx = hip.Context(n_lanes=n_lanes, max_w=640, max_h=480, max_kps=max_kps, max_cand=1 << 15)
    ctx.set_params(params() if p is None else p)
    return ctx


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------------------------------
def put_stereo(ctx, lane, s):
    """the current frame's two lists; the row tables the library builds for them are the documented ones (what the oracle is handed)"""
    for side, (k, d) in enumerate(((s["kl"], s["dl"]), (s["kr"], s["dr"]))):
        ctx.put_features(lane, 0, side, k, d, s["W"], s["H"])
        got = ctx.row_index(lane, 0, side)
        assert list(got[:s["H"]]) == list(MS.features_row_index(k, s["H"])), ("row table of a put list", lane, side)


def check_stereo(tag, ctx, lane, s, want):
    m, ri = want
    got, got_ri = ctx.matches(lane, 0), ctx.matches_row_index(lane, 0)
    assert got.tobytes() == m.tobytes(), (tag, "pairings", len(got), len(m))
    assert list(got_ri[:s["H"] + 1]) == list(ri), (tag, "pairings' row table")
    assert int(ctx.result(lane).stereo_matches[0]) == len(m), (tag, "stereo_matches")
    assert not (ctx.status_word(lane) & 8), (tag, "SVO_ST_INTERNAL")


@pytest.mark.parametrize("robust", [0, 1])
@pytest.mark.parametrize("match_method", [0, 1])
def test_stage3_scenes(match_method, robust):
    """every stage-3 scene under every one of its parameter variants: ctx.matches byte for byte, ctx.matches_row_index and
    result.stereo_matches against oracle.match_lr"""
    ctx = context()
    failed, total = [], 0
    for nm in MS.stereo_names():
        s = MS.scene(nm)
        for v, variant in enumerate(s["variants"]):
            p = MS.stereo_params(params(), variant, match_method, robust)
            ctx.set_params(p)
            put_stereo(ctx, 0, s)
            ctx.run_stages(hip.RUN_MATCH)
            total += 1
            try:
                check_stereo((nm, v), ctx, 0, s, MS.oracle_match(p, s))
            except AssertionError as e:
                failed.append(str(e.args[0]).split("\n")[0])
    ctx.close()
    assert total == 20 and not failed, (match_method, robust, len(failed), failed[:12])


STEREO_LANES = ["bf-one-to-one", "rbr-wrap", "stereo-0-40", "bf-rows", "bf-epipolar"]                 # (one image size per context: the 320 x 240 scenes)


@pytest.mark.parametrize("match_method", [0, 1])
def test_stage3_lanes_side_by_side(match_method):
    """five lanes, five scenes (one of them with an empty left list) in one call: every lane equals its own oracle result.  Then lane 1 gets
    other lists and stays idle through active=: its pairings stay what they were, the other lanes are matched again."""
    p = MS.stereo_params(params(), {}, match_method, 1)
    ctx = context(n_lanes=5, p=p)
    scenes = [MS.scene(nm) for nm in STEREO_LANES]
    want = [MS.oracle_match(p, s) for s in scenes]
    for lane, s in enumerate(scenes):
        put_stereo(ctx, lane, s)
    ctx.run_stages(hip.RUN_MATCH)
    for lane, s in enumerate(scenes):
        check_stereo(("all lanes", STEREO_LANES[lane]), ctx, lane, s, want[lane])
    assert sum(len(w[0]) > 0 for w in want) == 4 and len(want[2][0]) == 0
    put_stereo(ctx, 1, MS.scene("bf-threshold"))
    for lane in (0, 3):                                                          # two active lanes swap their scenes
        put_stereo(ctx, lane, scenes[3 - lane])
    ctx.run_stages(hip.RUN_MATCH, active=[0, 2, 3, 4])
    check_stereo(("idle", "lane 1"), ctx, 1, scenes[1], want[1])
    for lane, k in ((0, 3), (3, 0), (2, 2), (4, 4)):
        check_stereo(("one idle", lane), ctx, lane, scenes[k], want[k])
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------------------------------------------------------------------
def put_track(ctx, lane, s):
    """both frames of a scene; the pairings' row tables the library builds are the documented ones"""
    RS.put_scene(ctx, lane, s)
    for which, key in ((1, "pri"), (0, "cri")):
        assert list(ctx.matches_row_index(lane, which)[:s["H"] + 1]) == list(s[key]), ("row table of put pairings", lane, which)


def lane_result(ctx, lane):
    return ctx.tracked(lane), [int(v) for v in ctx.result(lane).track_stats[:8]], ctx.status_word(lane)


def test_stage4_scenes():
    """every stage-4 scene that fits 1024 keypoints, under the tracker and the windows it asks for: tracked pairs byte for byte, all eight
    counters, SVO_ST_INTERNAL down"""
    ctx = context()
    failed, names = [], [nm for nm in MS.track_names() if nm not in MS.CHAIN_MAX_KPS or MS.CHAIN_MAX_KPS[nm] <= 1024]
    for nm in names:
        s = MS.scene(nm)
        p = MS.track_params(params(), s)
        ctx.set_params(p)
        put_track(ctx, 0, s)
        ctx.run_stages(hip.RUN_TRACK)
        try:
            RS.check_case(nm, lane_result(ctx, 0), RS.oracle_track(p, s, key=("match-scenes", nm)))
        except AssertionError as e:
            failed.append(str(e.args[0]).split("\n")[0])
    ctx.close()
    assert len(names) == 22 and not failed, (len(failed), failed[:12])


@pytest.mark.parametrize("name", ["track-chain-2100", "track-chain-4600"])
def test_conflict_chains_in_the_larger_storage_forms(name):
    """k_track_filter<32> (candidate state in LDS, items up to j = 16) on a chain of 2100 rounds and k_track_filter<64> (states in LDS, train
    indices re-read from global memory, items j >= 32) on one of 4600: exactly the even pairings survive"""
    s = MS.scene(name)
    p = MS.track_params(params(), s)
    ctx = context(max_kps=MS.CHAIN_MAX_KPS[name], p=p)
    put_track(ctx, 0, s)
    ctx.run_stages(hip.RUN_TRACK)
    got = lane_result(ctx, 0)
    ctx.close()
    RS.check_case(name, got, RS.oracle_track(p, s, key=("match-scenes", name)))
    J = len(s["cm"]) - 1
    assert (got[0]["first"] == 2 * np.arange(J)).all() and got[1][:2] == [2 * J, J]


def put_current_only(ctx, lane, s):
    for side, (k, d) in enumerate(((s["ckl"], s["cdl"]), (s["ckr"], s["cdr"]))):
        ctx.put_features(lane, 0, side, k, d, s["W"], s["H"])
    ctx.put_matches(lane, 0, s["cm"])


def _track_lanes(names, overrides, idle_swap):
    """the named scenes side by side (None: a lane with a current frame and no previous one), all under one parameter record; then lane 1
    gets the lists of `idle_swap` and stays idle"""
    p = params()
    for k, v in overrides.items():
        setattr(p, k, v)
    ctx = context(n_lanes=len(names), p=p)
    scenes = [None if nm is None else MS.scene(nm) for nm in names]
    want = [None if s is None else RS.oracle_track(p, s, key=("match-scenes lanes", nm, tuple(sorted(overrides.items())))) for nm, s in zip(names, scenes)]
    for lane, s in enumerate(scenes):
        if s is None:
            put_current_only(ctx, lane, MS.scene("track-chain-40"))
        else:
            put_track(ctx, lane, s)
    ctx.run_stages(hip.RUN_TRACK)

    def check(tag, lanes):
        for lane in lanes:
            got = lane_result(ctx, lane)
            if scenes[lane] is None:                                             # no previous frame: nothing tracked, every counter zero
                assert len(got[0]) == 0 and got[1] == [0] * 8 and not (got[2] & 8), (tag, lane, got)
            else:
                RS.check_case((tag, lane, names[lane]), got, want[lane])
    check("all lanes", range(len(names)))
    if idle_swap is not None:
        before = lane_result(ctx, 1)
        RS.put_scene(ctx, 1, MS.scene(idle_swap))
        ctx.run_stages(hip.RUN_TRACK, active=[l for l in range(len(names)) if l != 1])
        after = lane_result(ctx, 1)
        assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1], ("idle lane", before[1], after[1])
        check("one idle", [l for l in range(len(names)) if l != 1])
    ctx.close()
    return want


def test_stage4_lanes_side_by_side_brute_force():
    """five lanes: a 300-round chain, the threshold scene, a lane without previous pairings, the inconsistent survivors, a lane without a
    previous frame -- every lane equals its own oracle result; then once more with lane 1 idle"""
    want = _track_lanes(["track-chain-300", "track-threshold", "track-tiny-0-8-bf-640", "track-inconsistent", None], {}, "track-chain-40")
    assert len(want[2][0]) == 0 and len(want[0][0]) == 300


def test_stage4_lanes_side_by_side_windowed():
    """the same with ifmDescWin, windows 20 / 45 in every lane: the negative-row scenes, win-edges, an empty lane, a lane without a previous frame"""
    want = _track_lanes(["win-negative-rows-0", "win-edges-640", "track-tiny-8-0-win-640", "win-negative-rows-1", None], dict(ifm_method=1, ifm_win_w=20, ifm_win_h=45), "win-negative-rows-1")
    assert len(want[0][0]) == 200 and len(want[1][0]) > 8


def test_twelve_lanes_hand_the_chains_to_the_matrix_core_count():
    """more than 8 lane-octaves: stage 4's inlier count runs on the matrix cores; the chain and threshold scenes over twelve lanes"""
    names = ["track-chain-300", "track-threshold", "track-chain-40", "track-inconsistent"] * 3
    want = _track_lanes(names, {}, None)
    assert [len(w[0]) for w in want[:4]] == [300, 52, 40, 60]


def test_unsorted_lists():
    """Lists that are not in ascending row order (include/svo_hip.h, at svo_put_features / svo_put_matches).  The row-by-row stereo matcher
    states ascending rows as a precondition: outside it, it promises no particular pairing -- only that the call ends, with lists of legal
    length and indices, every keypoint paired at most once, and SVO_ST_INTERNAL down.  The windowed tracker takes every pairing's row
    iteration from the pairings' row table (the binary search k_track_win falls back on) and follows the oracle's walk for any order."""
    s = MS.unsorted_stereo()
    p = MS.stereo_params(params(), {}, 1, 1)
    ctx = context(p=p)
    for side, (k, d) in enumerate(((s["kl"], s["dl"]), (s["kr"], s["dr"]))):
        ctx.put_features(0, 0, side, k, d, s["W"], s["H"])
    ctx.run_stages(hip.RUN_MATCH)
    m = ctx.matches(0, 0)
    assert len(m) <= len(s["kl"]) and int(ctx.result(0).stereo_matches[0]) == len(m) and not (ctx.status_word(0) & 8)
    assert ((m["queryIdx"] >= 0) & (m["queryIdx"] < len(s["kl"])) & (m["trainIdx"] >= 0) & (m["trainIdx"] < len(s["kr"]))).all()
    assert len(set(m["queryIdx"])) == len(m) and len(set(m["trainIdx"])) == len(m)
    t = MS.unsorted_track()
    q = MS.track_params(params(), t)
    ctx.set_params(q)
    put_track(ctx, 0, t)
    ctx.run_stages(hip.RUN_TRACK)
    got = lane_result(ctx, 0)
    ctx.close()
    rows = t["pkl"]["y"][t["pm"]["queryIdx"]]
    assert (np.diff(rows) < 0).any() and (np.diff(t["pri"]) >= 0).all()
    RS.check_case("win-edges, pairings shuffled", got, RS.oracle_track(q, t))
