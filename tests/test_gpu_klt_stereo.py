"""The stereo re-association of the resident KLT front end (svo_klt_set_stereo) on the GPU.

A step in mode 1 is held to its recipe: two contexts, A stepping with the row pass resident, B driven by KltStereoHostFrontEnd (the
recipe of svo_klt_step with the right job replaced by a svo_lk_track_rows job on the new pair); after every step all getters
(`snapshot` of tests/test_gpu_klt.py, re-stated in tests/test_gpu_klt_predict.py) and svo_klt_get_tracks must be equal as bytes."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import abi, hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_predict_scenes as PS                                                        # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import klt_stereo_ref as SR                                                            # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402
from test_gpu_klt import klt_params, params                                            # noqa: E402
from test_gpu_klt_predict import (SEQ_GFTT, assert_runs_equal, assert_same, assert_tracks, drive, host_topup, recipe_run, same, same_tracks,      # noqa: E402
                                  seq_klt_params, snapshot)

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6


def make_ctx(n_lanes=1, **kw):
    cfg = dict(n_lanes=n_lanes, max_w=PS.W, max_h=PS.H, max_kps=PS.MAX_KPS, max_cand=1 << 15)
    cfg.update(kw)
    c = hip.Context(**cfg)
    c.set_params(params())
    c.set_camera(PS.camera())
    return c


@pytest.fixture(scope="module")
def seq_pair():
    A, B = make_ctx(), make_ctx()
    A.klt_enable(seq_klt_params())
    assert A.klt_get_stereo() == 0
    A.klt_set_stereo(abi.KLT_STEREO_ROW)
    assert A.klt_get_stereo() == 1 and B.klt_get_stereo() == 0
    yield A, B
    A.close(); B.close()


@pytest.fixture(scope="module")
def seq_run(seq_pair):
    A, _ = seq_pair
    return drive(A, KS.sequence_frames(), KS.sequence_points())


@pytest.mark.parametrize("flags", [hip.RUN_OPTIMIZE, 0])
def test_sequence_in_mode_1_equals_the_recipe(seq_pair, seq_run, flags):
    A, B = seq_pair
    fe = SR.KltStereoHostFrontEnd(B, seq_klt_params(), KS.H)
    ref = recipe_run(B, fe, KS.sequence_frames(), KS.sequence_points(), flags=flags)
    got = seq_run if flags else drive(A, KS.sequence_frames(), KS.sequence_points(), flags=0)
    assert_runs_equal(got, ref, "mode 1, flags %d" % flags)
    # asserted on the RECIPE: every pair lies on one row, tracks survive to the last frame, and the first frame already ran the row pass
    for snap, table, _ in ref:
        assert len(table) > 0 and table.left[:, 1].tobytes() == table.right[:, 1].tobytes()
    first = ref[0][1]
    assert first.left.tobytes() == KS.sequence_points()[0][first.ids].tobytes() and first.right.tobytes() != KS.sequence_points()[1][first.ids].tobytes()


def test_the_sequence_is_the_cpu_walks(seq_run):
    import klt_ref as KR
    walk = SR.walk_sequence(KS.sequence_frames(), KS.sequence_points(), KS.SEQ_LK, KR.Gate(win=KS.WIN, **KS.SEQ_GATE), KS.SEQ_CAP, KS.H, 1)
    for f, ((snap, tracks), (lists, table, _, _)) in enumerate(zip(seq_run, walk)):
        assert tracks[0].tobytes() == table.left.tobytes() and tracks[1].tobytes() == table.right.tobytes(), f
        assert np.array_equal(tracks[2], table.ids), f


def test_device_and_pinned_images_equal_host_images(seq_pair, seq_run):
    import torch
    A, _ = seq_pair
    frames = KS.sequence_frames()
    stride = 192                                          # rows wider than the image: the copy honours the stride
    dev, pin = [], []
    for l, r in frames:
        for im in (l, r):
            host = np.zeros((KS.H, stride), np.uint8); host[:, :KS.W] = im
            dev.append(torch.from_numpy(host).cuda()); pin.append(torch.from_numpy(host).pin_memory())
    torch.cuda.synchronize()
    rec = lambda ts, f: tuple((ts[2 * f + s].data_ptr(), KS.W, KS.H, stride) for s in (0, 1))
    for name, ts, kw in (("device", dev, dict(device=True)), ("pinned", pin, dict(pinned=True))):
        got = drive(A, [rec(ts, f) for f in range(KS.SEQ_FRAMES)], KS.sequence_points(), **kw)
        for f in range(KS.SEQ_FRAMES):
            assert_same(got[f][0], seq_run[f][0], "%s images, frame %d" % (name, f))
            assert same_tracks(got[f][1], seq_run[f][1]), (name, f)


def test_five_lanes_with_an_idle_frame_an_unfed_lane_and_a_failing_lane():
    kp = seq_klt_params()
    frames, points = KS.sequence_frames(), KS.sequence_points()
    few = tuple(p[:3] for p in points)                    # three tracks: too few for stage 5, the lane's record stays invalid
    A, B = make_ctx(5), make_ctx(5)
    try:
        A.klt_enable(kp); A.klt_set_stereo(1)
        fe = SR.KltStereoHostFrontEnd(B, kp, KS.H)
        for lane, pts in ((0, points), (1, few), (2, points), (3, points)):
            assert A.klt_add_points(lane, *pts) == fe.add_points(lane, *pts) == len(pts[0])
        for f in range(KS.SEQ_FRAMES):
            active = [0, 1, 2] if f == 2 else [0, 1, 2, 3]          # lane 3 sits frame 2 out and resumes from frame 1; lane 4 is never fed
            k = lambda l: frames[f if l != 3 or f < 2 else f - 1] if l in active else None
            before3 = (snapshot(A, 3), A.klt_tracks(3)) if f == 2 else None
            A.klt_step([k(l) for l in range(5)], active=active)
            fe.step([k(l) for l in range(5)], active=active)
            for lane in active:
                same(A, B, fe, lane, "lane %d frame %d" % (lane, f))
            if f == 2:
                assert_same(snapshot(A, 3), before3[0], "the idle lane")
                assert same_tracks(A.klt_tracks(3), before3[1])
            assert B.result(1).valid == 0 and len(A.klt_tracks(4)[2]) == 0
            assert_same(snapshot(A, 2), snapshot(A, 0), "lanes 0 and 2 see the same frames")
        assert all(len(fe.tables[l]) > 0 for l in (0, 2, 3))          # asserted on the RECIPE
    finally:
        A.close(); B.close()


@pytest.mark.parametrize("fb_max,ransac,topup,predict", [(0.5, 0, False, False), (0.0, 1, False, True), (0.5, 2, True, False), (0.5, 2, False, True)])
def test_mode_1_composes_with_fb_max_the_ransac_gate_the_topup_and_the_prediction(fb_max, ransac, topup, predict):
    kp = seq_klt_params(fb_max=fb_max)
    frames, points = KS.sequence_frames(), KS.sequence_points()
    A, B = make_ctx(), make_ctx()
    try:
        A.klt_enable(kp); A.klt_set_stereo(1); A.klt_set_ransac(ransac); A.klt_set_prediction(1 if predict else 0)
        fe = SR.KltStereoRansacHostFrontEnd(B, kp, KS.H, ransac, PS.camera() if predict else None)
        tp = gp = None
        if topup:
            A.klt_topup_enable(None, below=KS.SEQ_CAP, init_disp=4.0, **SEQ_GFTT)
            tp, gp = TR.TopupParams(kp.cap, KS.SEQ_CAP, KS.SEQ_CAP, 4.0), abi.GfttParams(SEQ_GFTT["max_corners"], SEQ_GFTT["block"], SEQ_GFTT["min_distance"], SEQ_GFTT["quality"])
        assert A.klt_add_points(0, *points) == fe.add_points(0, *points) == 48
        predicted = appended = 0
        for f in range(KS.SEQ_FRAMES):
            A.klt_step([frames[f]]); fe.step([frames[f]])
            same(A, B, fe, 0, "fb %g ransac %d frame %d" % (fb_max, ransac, f))
            predicted += int(fe.guesses[0][2].sum()) if 0 in fe.guesses else 0
            if topup:
                A.klt_topup()
                appended += host_topup(B, fe, 0, frames[f], kp, tp, gp)
                assert_tracks(A, 0, fe.tables[0], "frame %d after the top-up" % f)
        print("fb %g ransac %d topup %d predict %d: predicted slots %d, appended %d, alive %d" % (fb_max, ransac, topup, predict, predicted, appended, len(fe.tables[0])))
        assert (predicted > 0) == predict and (appended > 0 or not topup), (predicted, appended)       # asserted on the RECIPE
        assert len(fe.tables[0]) > 0
    finally:
        A.close(); B.close()


def test_refusals_in_their_order_leave_everything_untouched(seq_pair):
    A, _ = seq_pair
    L = hip.lib()
    drive(A, KS.sequence_frames()[:3], KS.sequence_points())
    before, tracks = snapshot(A), A.klt_tracks(0)
    for mode in (2, -1, 7):
        assert L.svo_klt_set_stereo(A.h, mode) == SVO_ERR_ARG and ("mode %d" % mode).encode() in L.svo_last_error(A.h)
    assert A.klt_get_stereo() == 1
    assert_same(before, snapshot(A), "after the refusals")
    assert same_tracks(tracks, A.klt_tracks(0))
    c = hip.Context(n_lanes=1, max_w=PS.W, max_h=PS.H, max_kps=PS.MAX_KPS, max_cand=1 << 15)
    try:
        assert L.svo_klt_set_stereo(c.h, 1) == SVO_ERR_STATE and b"not enabled" in L.svo_last_error(c.h)
        assert L.svo_klt_set_stereo(c.h, 5) == SVO_ERR_STATE                      # the state before the mode
        assert L.svo_klt_get_stereo(c.h) == 0
        c.klt_enable(seq_klt_params())
        c.klt_set_stereo(1)                                   # the setter needs no svo_set_params
        assert c.klt_get_stereo() == 1
        # a svo_klt_enable that re-makes the buffers returns to mode 0; one with the parameters in force changes nothing
        c.klt_enable(seq_klt_params(win=9))
        assert c.klt_get_stereo() == 0
        c.klt_set_stereo(1)
        c.klt_enable(seq_klt_params(win=9))
        assert c.klt_get_stereo() == 1
    finally:
        c.close()


def test_mode_0_after_the_setter_equals_a_context_that_never_called_it():
    kp = seq_klt_params()
    A, B = make_ctx(kernel_times=True), make_ctx(kernel_times=True)
    try:
        for c in (A, B):
            c.klt_enable(kp)
        A.klt_set_stereo(1); A.klt_set_stereo(0)
        assert A.klt_get_stereo() == 0 and B.klt_get_stereo() == 0
        a = drive(A, KS.sequence_frames()[:4], KS.sequence_points())
        b = drive(B, KS.sequence_frames()[:4], KS.sequence_points())
        for f in range(4):
            assert_same(a[f][0], b[f][0], "frame %d" % f)
            assert same_tracks(a[f][1], b[f][1])
        ka, kb = A.kernel_times(appended=True), B.kernel_times(appended=True)
        assert list(ka) == list(kb) and "lk_track_row" not in ka
        assert [v[1] for v in ka.values()] == [v[1] for v in kb.values()]             # the same launches were counted
    finally:
        A.close(); B.close()


def test_the_kernel_time_name_appears_once_the_kernel_has_run():
    c = make_ctx(kernel_times=True)
    try:
        c.klt_enable(seq_klt_params())
        c.klt_add_points(0, *KS.sequence_points())
        frames = KS.sequence_frames()
        c.klt_step([frames[0]])
        names0 = list(c.kernel_times(appended=True))
        assert names0[-3:] == ["lk_pyrdown", "lk_track", "klt_select"]
        c.klt_set_stereo(1)
        assert list(c.kernel_times(appended=True)) == names0                     # the setter alone lists nothing
        c.klt_step([frames[1]]); c.klt_step([frames[2]])
        kt = c.kernel_times(appended=True)
        assert list(kt) == names0 + ["lk_track_row"] and kt["lk_track_row"][1] == 2 and kt["klt_select"][1] == 3
        assert list(c.kernel_times()) == names0[:c.FRAME_KERNEL_NAMES]
    finally:
        c.close()
