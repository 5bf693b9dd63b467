"""svo_ransac_tracked on the GPU, held to the walk of tests/ransac_tracked_ref.py: the lists arrive through the public puts, the call
runs, and the tracked pairs, their count, the eight track_stats and the status word must equal the walk's.  Three context shapes: one
lane of one octave (the few-lane RANSAC kernels), ten lanes of one octave (the many-lane kernels), five lanes of two octaves.

The refusal inside a captured graph is held by tools/klt_ransac_check.cpp (make hostcheck) only: no test here captures a stream."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import DM_FAST_ORB, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_tracked_ref as RR                                                        # noqa: E402
import ransac_tracked_scenes as RS                                                     # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6
CASE_NAMES = list(RS.cases())


def params(n_oct=1):
    p = north_star_params(hip.default_params(), orb_nfeats=300)
    p.orb_nlevels = 2
    if n_oct > 1:
        p.detect_method, p.nOctaves = DM_FAST_ORB, n_oct
    return p


def make_ctx(n_lanes, n_oct=1, set_params=True):
    c = hip.Context(n_lanes=n_lanes, max_w=RS.W, max_h=RS.H, max_kps=RS.MAX_KPS, max_cand=1 << 14, max_octaves=n_oct)
    if set_params:
        c.set_params(params(n_oct))
    return c


def lane_lists(c, lane, n_oct=1):
    """everything the call must leave alone in a lane outside the mask"""
    out = [bytes(c.result(lane)), c.status_word(lane)]
    for o in range(n_oct):
        out.append(c.tracked(lane, o).tobytes())
        for which in (0, 1):
            out.append(c.matches(lane, which, o).tobytes())
            for side in (0, 1):
                out.append(c.keypoints(lane, which, side, o)[0].tobytes())
    return out


def check_lane(c, lane, walks, tag):
    """the lane's tracked pairs per octave and its counters against the walks of its octaves"""
    for o, w in enumerate(walks):
        got = c.tracked(lane, o)
        assert len(got) == len(w.tracked), (tag, o, len(got), len(w.tracked))
        assert got.tobytes() == w.tracked.tobytes(), (tag, o)
    want = np.sum([w.stats for w in walks], axis=0)
    assert list(c.result(lane).track_stats) == [int(v) for v in want], (tag, list(c.result(lane).track_stats), list(want))
    assert c.status_word(lane) == 0, (tag, c.status_word(lane))


# ---- 1. one lane, one octave ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one():
    c = make_ctx(1)
    yield c
    c.close()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_equals_the_walk_one_lane(one, name):
    c = one
    c.reset()
    case = RS.case(name)
    RS.put_case(c, 0, case)
    before = lane_lists(c, 0)
    c.ransac_tracked()
    check_lane(c, 0, [RS.walk(name)], name)
    # nothing but the tracked pairs and the record's counters moved
    after = lane_lists(c, 0)
    assert before[3:] == after[3:] and c.result(0).error_code == 0, name


def test_a_second_call_reports_itself(one):
    c = one
    c.reset()
    case = RS.case("planted_257_45")
    RS.put_case(c, 0, case)
    c.ransac_tracked()
    w1 = RS.walk("planted_257_45")
    check_lane(c, 0, [w1], "first call")
    c.ransac_tracked()                                     # on the filtered list: its counters are this call's, not a sum
    w2 = RR.walk_octave(case.prev, case.cur, w1.tracked)
    assert w2.stats[RR.TS_THRESHOLD] == len(w1.tracked) < len(case.tracked)
    check_lane(c, 0, [w2], "second call")


def test_a_lane_without_a_previous_frame_gets_empty_lists(one):
    c = one
    c.reset()
    RS.put_case(c, 0, RS.case("planted_40_8"), with_prev=False)
    assert len(c.tracked(0)) == 40
    c.ransac_tracked()
    assert len(c.tracked(0)) == 0 and list(c.result(0).track_stats) == [0] * 8
    assert c.result(0).error_code == 0 and c.status_word(0) == 0


# ---- 2. ten lanes, one octave ---------------------------------------------------------------------------------------------------
TEN = ("planted_64_10", "clean_0", "heavy_64_30", "clean_7", "planted_1024_160", "planted_40_8", "bad_indices", "planted_14_2", "noisy_257_45", "no_model_right")
TEN_IDLE, TEN_NO_PREV = (3, 8), 5


def test_ten_lanes_with_idle_lanes_and_one_without_a_previous_frame():
    c = make_ctx(10)
    try:
        for lane, name in enumerate(TEN):
            RS.put_case(c, lane, RS.case(name), with_prev=lane != TEN_NO_PREV)
        idle_before = {l: lane_lists(c, l) for l in TEN_IDLE}
        active = [l for l in range(10) if l not in TEN_IDLE]
        c.ransac_tracked(active)
        for lane in active:
            if lane == TEN_NO_PREV:
                assert len(c.tracked(lane)) == 0 and list(c.result(lane).track_stats) == [0] * 8 and c.status_word(lane) == 0
            else:
                check_lane(c, lane, [RS.walk(TEN[lane])], (lane, TEN[lane]))
        for l in TEN_IDLE:
            assert lane_lists(c, l) == idle_before[l], l
        # the lanes that sat out, alone: the others keep what the first call left
        c.ransac_tracked(TEN_IDLE)
        for lane in range(10):
            if lane != TEN_NO_PREV:
                check_lane(c, lane, [RS.walk(TEN[lane])], ("second call", lane))
    finally:
        c.close()


# ---- 3. five lanes of two octaves -----------------------------------------------------------------------------------------------
TWO_OCT = (("planted_64_10", "clean_15"), ("clean_8", "planted_257_45"), ("heavy_300_150", "clean_0"), ("clean_6", "clean_6"), ("bad_indices", "noisy_65"))


def test_five_lanes_of_two_octaves():
    c = make_ctx(5, n_oct=2)
    try:
        for lane, names in enumerate(TWO_OCT):
            for o, name in enumerate(names):
                RS.put_case(c, lane, RS.case(name), octave=o)
        idle_before = lane_lists(c, 3, 2)
        c.ransac_tracked([0, 1, 2, 4])
        for lane in (0, 1, 2, 4):
            check_lane(c, lane, [RS.walk(n) for n in TWO_OCT[lane]], (lane, TWO_OCT[lane]))
        assert lane_lists(c, 3, 2) == idle_before
        c.ransac_tracked()                                 # every lane; the counters of lanes 0, 1, 2, 4 start over
        check_lane(c, 3, [RS.walk(n) for n in TWO_OCT[3]], "lane 3")
        case = RS.case("planted_257_45")
        w2 = RR.walk_octave(case.prev, case.cur, RS.walk("planted_257_45").tracked)
        check_lane(c, 1, [RS.walk("clean_8"), w2], "lane 1, second call")
    finally:
        c.close()


# ---- 4. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = hip.lib()
    c = make_ctx(2, set_params=False)
    try:
        assert L.svo_ransac_tracked(c.h, None) == SVO_ERR_STATE and b"svo_set_params" in L.svo_last_error(c.h)
        c.set_params(params())
        assert L.svo_ransac_tracked(c.h, None) == SVO_ERR_STATE and b"geometry" in L.svo_last_error(c.h)
        RS.put_case(c, 0, RS.case("planted_40_8"))
        before = lane_lists(c, 0)
        assert L.svo_ransac_tracked(c.h, (C.c_uint64 * 2)(1 << 2, 0)) == SVO_ERR_ARG and L.svo_last_error(c.h)
        assert L.svo_ransac_tracked(c.h, (C.c_uint64 * 2)(1, 1)) == SVO_ERR_ARG
        assert lane_lists(c, 0) == before
        assert L.svo_ransac_tracked(c.h, (C.c_uint64 * 2)(0, 0)) == 0 and lane_lists(c, 0) == before      # nobody takes part
        assert L.svo_ransac_tracked(None, None) == SVO_ERR_ARG
        # svo_klt_set_ransac before svo_klt_enable, and a mode out of range after it
        assert L.svo_klt_set_ransac(c.h, 1) == SVO_ERR_STATE and b"svo_klt_enable" in L.svo_last_error(c.h)
        assert c.klt_ransac() == 0
        c.klt_enable()
        assert L.svo_klt_set_ransac(c.h, 3) == SVO_ERR_ARG and L.svo_klt_set_ransac(c.h, -1) == SVO_ERR_ARG and c.klt_ransac() == 0
        c.klt_set_ransac(2)
        assert c.klt_ransac() == 2
        c.klt_set_ransac(0)
        assert c.klt_ransac() == 0
        # the call itself needs no front end, and "ransac_feed" is listed once it has run
        assert "ransac_feed" not in c.kernel_times(appended=True)
        c.ransac_tracked([0])
        check_lane(c, 0, [RS.walk("planted_40_8")], "after the refusals")
        assert "ransac_feed" in c.kernel_times(appended=True) and "klt_prune" not in c.kernel_times(appended=True)
    finally:
        c.close()
