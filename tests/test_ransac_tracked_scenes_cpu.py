"""What the cases of tests/ransac_tracked_scenes.py reach on the oracle (no GPU): which path cv::findFundamentalMat takes, whether both
sides find a model, what is rejected.  tests/test_gpu_ransac_tracked.py puts the same cases into contexts and compares with the same walk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_tracked_ref as RR                                                        # noqa: E402
import ransac_tracked_scenes as RS                                                     # noqa: E402

# candidates -> (path, use_f) of the clean cases
# (8 clean pairs: the LMedS path keeps 8 on the left and 7 on the right, so there is no use_f: every pair stays)
CLEAN = {0: ("none", False), 6: ("none", False), 7: ("direct7", False), 8: ("lmeds", False), 14: ("lmeds", True), 15: ("ransac", True),
         64: ("ransac", True), 65: ("ransac", True), 256: ("ransac", True), 257: ("ransac", True), 1024: ("ransac", True)}


def test_the_counts_cover_every_path_and_seam():
    assert RS.COUNTS == tuple(sorted(CLEAN)) and RS.COUNTS[-1] == RS.MAX_KPS
    assert [RR.path_of(n) for n in (6, 7, 8, 14, 15)] == ["none", "direct7", "lmeds", "lmeds", "ransac"]


@pytest.mark.parametrize("n", RS.COUNTS)
def test_clean_case_takes_its_path(n):
    c, w = RS.case("clean_%d" % n), RS.walk("clean_%d" % n)
    assert len(c.tracked) == n and len(w.cand) == n
    assert (w.path, bool(w.use_f)) == CLEAN[n], (n, w.path, w.use_f, w.inliers)
    if n < 7:
        assert w.inliers == (0, 0) and w.stats[RR.TS_HYP_L] == 0
    if n == 7:
        assert w.inliers == (7, 7) and w.stats[RR.TS_HYP_L] == 0 and w.stats[RR.TS_HYP_R] == 0
    if not w.use_f:
        assert w.tracked.tobytes() == c.tracked.tobytes()
    if n >= 15:                                            # the RANSAC proper rejects nothing of a clean list
        assert w.keep.all() and w.tracked.tobytes() == c.tracked.tobytes(), (n, int((~w.keep).sum()))
        assert w.inliers == (n, n) and w.stats[RR.TS_HYP_L] >= 1
    assert list(w.stats[:2]) == [n, n] and w.stats[RR.TS_BOTH_MASKS] == w.stats[RR.TS_TRACKED] == len(w.tracked)
    # every level of indirection is a real permutation from 8 pairs on
    if n >= 8:
        assert (c.tracked["first"] != c.tracked["second"]).any() and (c.prev.matches["queryIdx"] != c.prev.matches["trainIdx"]).any()


@pytest.mark.parametrize("n,k", RS.PLANTED)
def test_planted_case_rejects_planted_pairs(n, k):
    name = "planted_%d_%d" % (n, k)
    c, w = RS.case(name), RS.walk(name)
    assert len(c.planted) == k and len(w.cand) == n and w.use_f
    rejected = np.flatnonzero(~w.keep)
    hit = np.intersect1d(rejected, c.planted)
    assert len(hit) >= 1, (name, rejected)
    if n >= 40:                                            # the RANSAC proper: most of the planted pairs go, few of the others
        good_lost = len(rejected) - len(hit)
        assert len(hit) >= 0.85 * k and good_lost <= 0.02 * (n - k), (name, len(hit), good_lost)
    # survivors keep their order
    assert w.tracked.tobytes() == c.tracked[w.keep].tobytes()


def test_hard_cases_visit_many_hypotheses():
    """the cases that take the sample schedule past its first chunks (32 and 160 samples)"""
    hyp = {nm: int(RS.walk(nm).stats[RR.TS_HYP_L]) for nm, _, _, _ in RS.HARD}
    assert hyp["heavy_64_30"] > 160 and hyp["heavy_300_150"] > 160 and hyp["noisy_65"] > 1 and hyp["noisy_257_45"] > 1, hyp
    for nm, n, k, _ in RS.HARD:
        w = RS.walk(nm)
        assert w.use_f and len(w.cand) == n and (k == 0 or len(np.intersect1d(np.flatnonzero(~w.keep), RS.case(nm).planted)) >= 1), nm


def test_lmeds_rejects_good_pairs_of_a_small_list():
    """the behaviour svo_hip.h documents: between 8 and 14 pairs the LMedS path can reject good pairs"""
    c, w = RS.case("planted_14_2"), RS.walk("planted_14_2")
    assert w.path == "lmeds"
    print("planted_14_2: rejected %d of 14, %d of them planted" % (int((~w.keep).sum()), len(np.intersect1d(np.flatnonzero(~w.keep), c.planted))))


def test_a_side_without_a_model_keeps_everything():
    c, w = RS.case("no_model_right"), RS.walk("no_model_right")
    assert w.path == "ransac" and w.inliers[0] >= 8 and w.inliers[1] == 0 and not w.use_f
    assert w.stats[RR.TS_HYP_R] == 0 and w.stats[RR.TS_HYP_L] >= 1
    assert w.tracked.tobytes() == c.tracked.tobytes() and w.stats[RR.TS_TRACKED] == 20


def test_bad_indices_are_no_candidates():
    c, w = RS.case("bad_indices"), RS.walk("bad_indices")
    assert len(c.bad) == 10 and len(c.tracked) == 34
    assert (c.tracked["first"][c.bad] < 0).sum() == 2 and (c.tracked["second"][c.bad] < 0).sum() == 1
    assert (c.tracked["first"] == len(c.prev.matches)).sum() == 1 and (c.tracked["second"] == len(c.cur.matches)).sum() == 1
    assert len(w.cand) == 24 and not np.intersect1d(w.cand, c.bad).size
    assert list(w.stats[:2]) == [34, 24] and w.use_f and w.keep.all()
    assert w.tracked.tobytes() == np.delete(c.tracked, c.bad).tobytes()


def test_lane_stats_sum_over_the_octaves():
    ws, stats = RR.walk_lane([RS.case("planted_40_8").octave(), RS.case("clean_15").octave()])
    assert (stats == ws[0].stats + ws[1].stats).all() and stats[RR.TS_THRESHOLD] == 55


def test_prune_removes_the_lost_slots_only():
    import klt_ref as KR
    t, _ = KR.add_points(KR.Table(), np.zeros((6, 2), np.float32), np.ones((6, 2), np.float32), 8)
    t.idx = np.arange(6, dtype=np.int32); t.pidx = np.array([0, 1, -1, 2, 3, -1], np.int32)
    before = np.array([(0, 0), (1, 1), (2, 3), (3, 4)], KR.index_pair_dtype)
    after = np.array([(0, 0), (3, 4)], KR.index_pair_dtype)
    t2, lost = RR.prune(t, before, after)
    assert list(lost) == [1, 3] and list(t2.ids) == [0, 2, 4, 5] and list(t2.idx) == [0, 2, 4, 5] and t2.next_id == 6


def test_the_gate_sequence_has_tracks_to_reject():
    """frames 0 and 1 of the resident gate's sequence through tests/lk_ref.py, the selection walk and the RANSAC walk: the tracks on the
    moving patch are followed, pass the stereo gate, and the RANSAC rejects at least one of them (what the GPU test asserts on the recipe)"""
    import klt_ref as KR
    import klt_scenes as KS
    import lk_ref as LR
    frames, (l0, r0) = RS.gate_sequence_frames(), RS.gate_sequence_points()
    P, g = LR.LkParams(**KS.SEQ_LK), KR.Gate(win=KS.WIN, **KS.SEQ_GATE)
    t, _ = KR.add_points(KR.Table(), l0, r0, KS.SEQ_CAP)
    assert len(t) == 52
    lists0, t, _ = KR.select(t, t.left, t.right, np.ones(52, np.uint8), np.ones(52, np.uint8), g, False, KS.H)
    assert len(lists0.tracked) == 0
    res = [LR.track(frames[0][sd], frames[1][sd], t.left if sd == 0 else t.right, params=P) for sd in (0, 1)]
    lists1, t1, reasons = KR.select(t, res[0][0], res[1][0], res[0][1], res[1][1], g, True, KS.H)
    patch_ids = {48, 49, 50, 51}
    on_patch = np.flatnonzero(np.isin(lists1.ids, list(patch_ids)))
    assert len(on_patch) >= 2, reasons[48:]
    w = RR.walk_octave(RS.lists_of(lists0), RS.lists_of(lists1), lists1.tracked)
    lost = np.setdiff1d(lists1.tracked["second"], w.tracked["second"])
    print("gate sequence, frame 1: %d candidates, path %s, use_f %s, rejected list indices %s, patch tracks at %s" % (len(w.cand), w.path, w.use_f, list(lost), list(on_patch)))
    assert w.use_f and len(np.intersect1d(lost, on_patch)) >= 1
    t2, _ = RR.prune(t1, lists1.tracked, w.tracked)
    assert len(t2) == len(t1) - len(lost)


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_built_steps_reject_the_slid_tracks_at_the_seams(mode):
    """the three selections of the resident gate's hand-built scene through the walks: step 1 has nothing to verify, steps 2 and 3 reject
    the tracks that slid (all but two at the most, and at most 2 % of the others); in mode 2 step 3's pairs no longer have first == second"""
    import klt_ref as KR
    import klt_scenes as KS
    world = RS.StepWorld(KS.CAP)
    t, _ = KR.add_points(KR.Table(), *world.arrays(0, np.arange(KS.CAP))[:2], KS.CAP)
    prev, stepped = None, False
    for k in range(3):
        l, r, slid = world.arrays(k, t.ids, RS.SEAMS if k else ())
        lists, t, _ = KR.select(t, l, r, KS.ones(len(t)), KS.ones(len(t)), KS.gate(), stepped, KS.H)
        stepped = True
        if k == 0:
            assert len(lists.tracked) == 0
        else:
            w = RR.walk_octave(RS.lists_of(prev), RS.lists_of(lists), lists.tracked)
            lost = np.setdiff1d(lists.tracked["second"], w.tracked["second"])
            hit = np.intersect1d(lost, slid)
            assert w.use_f and len(slid) >= 14 and len(hit) >= len(slid) - 2 and len(lost) - len(hit) <= 0.02 * len(lists.tracked), (k, list(lost))
            got = set(int(v) for v in hit)                 # (a track that slid along its epipolar line stays: each seam is hit on one side at least)
            assert got & {63, 64} and got & {127, 128} and got & {255, 256}, (k, list(hit))
            if k == 2 and mode == 2:
                assert (lists.tracked["first"] != lists.tracked["second"]).any()
            if mode == 2:
                t, _ = RR.prune(t, lists.tracked, w.tracked)
        prev = lists
