"""The pose prediction of the resident KLT front end (svo_klt_set_prediction) on the GPU.

svo_debug_klt_predict is held byte for byte to the walk of tests/klt_predict_ref.py on the hand-built scenes of
tests/klt_predict_scenes.py; svo_klt_predicted to the same walk fed with svo_get_result.  A step in mode 1 is held to its recipe: two
contexts, A stepping with the prediction resident, B driven by KltPredictHostFrontEnd (the recipe of svo_klt_step with the record and
the table read before the shift, the guesses of the walk, and `init` of both svo_lk_track jobs); after every step all getters
(`snapshot` of tests/test_gpu_klt.py, re-stated here) and svo_klt_get_tracks must be equal as bytes."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import abi, hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_predict_ref as PR                                                           # noqa: E402
import klt_predict_scenes as PS                                                        # noqa: E402
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402
from test_gpu_klt import klt_params, params                                            # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6
SCENE_NAMES = [s.name for s in PS.scenes()]
SEQ_GFTT = dict(max_corners=0, block=3, min_distance=8, quality=0.02)


def make_ctx(n_lanes=1, **kw):
    cfg = dict(n_lanes=n_lanes, max_w=PS.W, max_h=PS.H, max_kps=PS.MAX_KPS, max_cand=1 << 15)
    cfg.update(kw)
    c = hip.Context(**cfg)
    c.set_params(params())
    c.set_camera(PS.camera())
    return c


def snapshot(c, lane=0):
    """every public getter of a lane, as bytes (tests/test_gpu_klt.py)"""
    out = {}
    for which in (0, 1):
        for side in (0, 1):
            k, d = c.keypoints(lane, which, side)
            out["kps%d%d" % (which, side)] = k.tobytes() + d.tobytes()
            out["row%d%d" % (which, side)] = c.row_index(lane, which, side).tobytes() if which == 0 or len(k) else b""
        out["matches%d" % which] = c.matches(lane, which).tobytes()
        out["ids%d" % which] = c.match_ids(lane, which).tobytes()
        out["mrow%d" % which] = c.matches_row_index(lane, which).tobytes() if which == 0 or len(k) else b""
        out["values%d" % which] = b"|".join(a.tobytes() for a in c.values(lane, which))
    out["tracked"] = c.tracked(lane).tobytes()
    out["result"] = bytes(c.result(lane))
    out["residuals"] = c.residuals(lane).tobytes()
    out["outliers"] = c.outliers(lane).tobytes()
    return out


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s: getter '%s' differs (%d vs %d bytes)" % (tag, k, len(a[k]), len(b[k]))


def assert_tracks(c, lane, table, tag):
    l, r, ids, age = c.klt_tracks(lane)
    assert len(ids) == len(table), (tag, len(ids), len(table))
    assert l.tobytes() == table.left.tobytes() and r.tobytes() == table.right.tobytes(), tag
    assert np.array_equal(ids, table.ids) and np.array_equal(age, table.age), tag


def same(A, B, fe, lane, tag):
    assert_same(snapshot(A, lane), snapshot(B, lane), tag)
    assert_tracks(A, lane, fe.tables[lane], tag)


def same_tracks(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def blank():
    return np.zeros((PS.H, PS.W), np.uint8)


def seq_klt_params(**lk):
    d = dict(KS.SEQ_LK); d.update(lk)
    return klt_params(KS.SEQ_CAP, d, KS.SEQ_GATE)


def fast_klt_params():
    return klt_params(PS.FAST_CAP, PS.FAST_LK, PS.FAST_GATE)


def test_the_scenes_camera_is_the_sequence_worlds():
    assert bytes(PS.camera()) == bytes(KS.sequence_world().camera()) == bytes(PS.fast_world().camera())


# ---- 1. the rule on hand-built tables and increments --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_ctx():
    A = make_ctx()
    A.klt_enable(klt_params(PS.CAP, dict(win=PS.WIN), KS.GATE))
    A.klt_set_prediction(abi.KLT_PREDICT_POSE)
    yield A
    A.close()


def load_scene(A, sc):
    """the scene's table into lane 0 of a context whose lane has a last pair of the scenes' image size"""
    A.klt_reset()
    A.klt_step([(blank(), blank())], flags=0)          # the reset forgot the last pair: an empty table steps over a blank one
    assert A.klt_add_points(0, sc.left, sc.right) == len(sc.left)


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_debug_predict_equals_the_walk(scene_ctx, name):
    A, sc = scene_ctx, PS.scene(name)
    load_scene(A, sc)
    before, tracks = snapshot(A), A.klt_tracks(0)
    gl, gr, used = A.debug_klt_predict(0, sc.delta, sc.valid)
    o = PS.walk(sc)
    assert len(used) == len(sc.left)
    assert used.tobytes() == o.used.tobytes(), (name, used, o.used)
    assert gl.tobytes() == o.gl.tobytes() and gr.tobytes() == o.gr.tobytes(), name
    # nothing of the lane moved: its lists, its record, its table
    assert_same(before, snapshot(A), name)
    assert same_tracks(tracks, A.klt_tracks(0))
    # a smaller cap: the live count comes back, min(count, cap) entries are written, NULL arrays are left alone
    n = len(sc.left)
    if n >= 2:
        part = np.full((n, 2), -7.0, np.float32)
        assert hip.lib().svo_debug_klt_predict(A.h, 0, hip._vp(sc.delta), sc.valid, hip._vp(part), None, None, n // 2) == n
        assert part[:n // 2].tobytes() == o.gl[:n // 2].tobytes() and (part[n // 2:] == -7.0).all()


def test_a_lane_without_a_last_pair_does_not_predict(scene_ctx):
    A, sc = scene_ctx, PS.scene("delta_zero")
    A.klt_reset()
    assert A.klt_add_points(0, sc.left, sc.right) == len(sc.left)
    for gl, gr, used in (A.debug_klt_predict(0, PS.MOTION, 1), A.klt_predicted(0)):
        assert not used.any() and gl.tobytes() == sc.left.tobytes() and gr.tobytes() == sc.right.tobytes()


# ---- 2. the sequence of tests/klt_scenes.py ------------------------------------------------------------------------------------------
def drive(A, frames, points, flags=hip.RUN_OPTIMIZE, each=None, **kw):
    """a one-lane device context through a sequence from its starting points: [(snapshot, tracks)] per frame"""
    A.reset(); A.klt_reset()
    assert A.klt_add_points(0, *points) == len(points[0])
    out = []
    for f, fr in enumerate(frames):
        A.klt_step([fr], flags=flags, **kw)
        out.append((snapshot(A), A.klt_tracks(0)))
        if each:
            each(f)
    return out


def recipe_run(B, fe, frames, points, flags=hip.RUN_OPTIMIZE):
    """the recipe on its context: [(snapshot, table, used)] per frame"""
    B.reset()
    fe.add_points(0, *points)
    out = []
    for fr in frames:
        fe.step([fr], flags=flags)
        used = fe.guesses[0][2].copy() if getattr(fe, "guesses", None) and 0 in fe.guesses else np.zeros(0, np.uint8)
        out.append((snapshot(B), fe.tables[0].copy(), used))
    return out


def assert_runs_equal(got, ref, tag):
    for f, ((snap, tracks), (rsnap, table, _)) in enumerate(zip(got, ref)):
        assert_same(snap, rsnap, "%s frame %d" % (tag, f))
        assert tracks[0].tobytes() == table.left.tobytes() and tracks[1].tobytes() == table.right.tobytes(), (tag, f)
        assert np.array_equal(tracks[2], table.ids) and np.array_equal(tracks[3], table.age), (tag, f)


@pytest.fixture(scope="module")
def seq_pair():
    A, B = make_ctx(), make_ctx()
    A.klt_enable(seq_klt_params())
    A.klt_set_prediction(1)
    assert A.klt_prediction() == 1 and B.klt_prediction() == 0
    yield A, B
    A.close(); B.close()


@pytest.fixture(scope="module")
def seq_run(seq_pair):
    """A in mode 1 alone on the five frames, with svo_klt_predicted read after every step"""
    A, _ = seq_pair
    told = []

    def each(f):
        r, t = A.result(0), A.klt_tracks(0)
        told.append((A.klt_predicted(0), PR.predict(t[0], t[1], PS.camera(), np.array(r.delta), r.valid, PS.W, PS.H)[:3], r.valid))
    return drive(A, KS.sequence_frames(), KS.sequence_points(), each=each), told


def test_sequence_in_mode_1_equals_the_recipe(seq_pair, seq_run):
    _, B = seq_pair
    fe = PR.KltPredictHostFrontEnd(B, seq_klt_params(), KS.H, PS.camera())
    ref = recipe_run(B, fe, KS.sequence_frames(), KS.sequence_points())
    assert_runs_equal(seq_run[0], ref, "mode 1")
    # asserted on the RECIPE: the guesses were predicted ones from the third frame on, and none before stage 5 had run on tracked pairs
    assert not ref[0][2].any() and all(ref[f][2].any() for f in (3, 4)), [int(r[2].sum()) for r in ref]


def test_predicted_after_every_step_equals_the_walk_on_the_record(seq_run):
    _, told = seq_run
    for f, (got, want, valid) in enumerate(told):
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes(), f
    assert any(valid and got[2].any() for got, _, valid in told) and not told[0][0][2].any()


def test_without_optimize_no_lane_predicts_and_the_run_is_mode_0s(seq_pair):
    A, B = seq_pair
    frames, points = KS.sequence_frames(), KS.sequence_points()
    got = drive(A, frames, points, flags=0)
    fe = PR.KltPredictHostFrontEnd(B, seq_klt_params(), KS.H, PS.camera())
    ref = recipe_run(B, fe, frames, points, flags=0)
    assert_runs_equal(got, ref, "no stage 5")
    assert not any(r[2].any() for r in ref)
    A.klt_set_prediction(0)
    try:
        plain = drive(A, frames, points, flags=0)
    finally:
        A.klt_set_prediction(1)
    for f in range(len(frames)):
        assert_same(got[f][0], plain[f][0], "frame %d against mode 0" % f)
        assert same_tracks(got[f][1], plain[f][1])


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
            assert_same(got[f][0], seq_run[0][f][0], "%s images, frame %d" % (name, f))
            assert same_tracks(got[f][1], seq_run[0][f][1]), (name, f)


# ---- 3. many lanes: an idle frame, an unfed lane, a lane whose stage 5 fails --------------------------------------------------------------
def test_five_lanes_with_an_idle_frame_an_unfed_lane_and_a_failing_lane():
    kp = seq_klt_params()
    frames, points = KS.sequence_frames(), KS.sequence_points()
    few = tuple(p[:3] for p in points)                    # three tracks: too few for stage 5, the lane's record stays invalid
    A, B = make_ctx(5), make_ctx(5)
    try:
        A.klt_enable(kp); A.klt_set_prediction(1)
        fe = PR.KltPredictHostFrontEnd(B, kp, KS.H, PS.camera())
        for lane, pts in ((0, points), (1, few), (2, points), (3, points)):
            assert A.klt_add_points(lane, *pts) == fe.add_points(lane, *pts) == len(pts[0])
        predicted = {l: 0 for l in range(5)}
        for f in range(KS.SEQ_FRAMES):
            active = [0, 1, 2] if f == 2 else [0, 1, 2, 3]          # lane 3 sits frame 2 out and resumes from frame 1; lane 4 is never fed
            k = lambda l: frames[f if l != 3 or f < 2 else f - 1] if l in active else None
            before3 = (snapshot(A, 3), A.klt_tracks(3)) if f == 2 else None
            A.klt_step([k(l) for l in range(5)], active=active)
            fe.step([k(l) for l in range(5)], active=active)
            for lane in active:
                same(A, B, fe, lane, "lane %d frame %d" % (lane, f))
                if lane in fe.guesses:
                    predicted[lane] += int(fe.guesses[lane][2].sum())
            if f == 2:
                assert_same(snapshot(A, 3), before3[0], "the idle lane")
                assert same_tracks(A.klt_tracks(3), before3[1])
            assert B.result(1).valid == 0 and len(A.klt_tracks(4)[2]) == 0
            for lane in (0, 2):
                assert_same(snapshot(A, lane), snapshot(A, 0), "lanes 0 and 2 see the same frames")
        # asserted on the RECIPE: the failing lane never predicted while its neighbours did
        assert predicted[1] == 0 and predicted[0] > 0 and predicted[2] > 0 and predicted[3] > 0, predicted
    finally:
        A.close(); B.close()


# ---- 4. with the forward-backward pass, the RANSAC gate and a top-up between steps --------------------------------------------------------
def host_topup(B, fe, lane, pair, kp, tp, gp):
    """the recipe of svo_klt_topup on the HOST's table (tests/klt_topup_ref.py): detect, track left to right, gate, append"""
    t = fe.tables[lane]
    want = TR.want_of(len(t), kp.cap, tp)
    if want is None:
        return 0
    (corners, _, _, status), = B.gftt_detect([(pair[0], t.left, want)], gp)
    assert status == 0
    (out, st, _), = B.lk_track([(pair[0], pair[1], corners, TR.first_guess(corners, tp.init_disp))], kp.lk)
    fe.tables[lane], m, _ = TR.append(t, corners, out, st, fe.gate, kp.cap)
    return m


@pytest.mark.parametrize("fb_max,ransac,topup", [(0.5, 0, False), (0.0, 1, False), (0.5, 2, True)])
def test_mode_1_composes_with_fb_max_the_ransac_gate_and_the_topup(fb_max, ransac, topup):
    kp = seq_klt_params(fb_max=fb_max)
    frames, points = KS.sequence_frames(), KS.sequence_points()
    A, B = make_ctx(), make_ctx()
    try:
        A.klt_enable(kp); A.klt_set_prediction(1); A.klt_set_ransac(ransac)
        fe = PR.KltPredictRansacHostFrontEnd(B, kp, KS.H, PS.camera(), ransac)
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
        assert predicted > 0 and (appended > 0 or not topup), (predicted, appended)       # asserted on the RECIPE
    finally:
        A.close(); B.close()


# ---- 5. the fast-motion sequence: byte equality in both modes (what the prediction buys is asserted on the CPU) --------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_fast_motion_sequence_equals_its_recipe(mode):
    kp = fast_klt_params()
    A, B = make_ctx(), make_ctx()
    try:
        A.klt_enable(kp); A.klt_set_prediction(mode)
        fe = PR.KltPredictHostFrontEnd(B, kp, PS.H, PS.camera()) if mode else KR.KltHostFrontEnd(B, kp, PS.H)
        got = drive(A, PS.fast_frames(), PS.fast_points())
        ref = recipe_run(B, fe, PS.fast_frames(), PS.fast_points())
        assert_runs_equal(got, ref, "fast motion, mode %d" % mode)
        print("fast motion, mode %d: live tracks per frame %s, predicted slots per frame %s, valid %s" % (
            mode, [len(r[1]) for r in ref], [int(r[2].sum()) for r in ref], [abi.Result.from_buffer_copy(r[0]["result"]).valid for r in ref]))
    finally:
        A.close(); B.close()


# ---- 6. refusals, mode 0, the kernel-time name ---------------------------------------------------------------------------------------------
def test_refusals_in_their_order_leave_everything_untouched(seq_pair):
    A, _ = seq_pair
    L = hip.lib()
    drive(A, KS.sequence_frames()[:3], KS.sequence_points())
    before, tracks, guesses = snapshot(A), A.klt_tracks(0), A.klt_predicted(0)
    d = np.array(PS.MOTION)
    buf = np.zeros((KS.SEQ_CAP, 2), np.float32)
    cases = [
        (L.svo_klt_set_prediction(A.h, 2), SVO_ERR_ARG), (L.svo_klt_set_prediction(A.h, -1), SVO_ERR_ARG),
        (L.svo_klt_predicted(A.h, 1, None, None, None, 0), SVO_ERR_ARG), (L.svo_klt_predicted(A.h, -1, None, None, None, 0), SVO_ERR_ARG),
        (L.svo_klt_predicted(A.h, 0, hip._vp(buf), None, None, -1), SVO_ERR_ARG),
        (L.svo_debug_klt_predict(A.h, 0, None, 1, None, None, None, 0), SVO_ERR_ARG),
        (L.svo_debug_klt_predict(A.h, 3, None, 1, None, None, None, -1), SVO_ERR_ARG),
        (L.svo_debug_klt_predict(A.h, 0, hip._vp(d), 1, None, None, None, -1), SVO_ERR_ARG),
    ]
    for i, (rc, want) in enumerate(cases):
        assert rc == want, (i, rc, want)
    assert b"lane 3 of 1" in (L.svo_debug_klt_predict(A.h, 3, None, 1, None, None, None, -1), L.svo_last_error(A.h))[1]      # the lane before the count and delta6
    assert A.klt_prediction() == 1 and not buf.any()
    A.klt_set_prediction(0)
    try:                                                    # the mode before the arguments
        assert L.svo_klt_predicted(A.h, 9, None, None, None, -1) == SVO_ERR_STATE and b"svo_klt_set_prediction" in L.svo_last_error(A.h)
        assert L.svo_debug_klt_predict(A.h, 0, hip._vp(d), 1, None, None, None, 0) == SVO_ERR_STATE
    finally:
        A.klt_set_prediction(1)
    assert_same(before, snapshot(A), "after the refusals")
    assert same_tracks(tracks, A.klt_tracks(0)) and same_tracks(guesses, A.klt_predicted(0))
    # a context that has not enabled the front end, and one without parameters
    c = hip.Context(n_lanes=1, max_w=PS.W, max_h=PS.H, max_kps=PS.MAX_KPS, max_cand=1 << 15)
    try:
        assert L.svo_klt_set_prediction(c.h, 1) == SVO_ERR_STATE and b"not enabled" in L.svo_last_error(c.h)
        assert L.svo_klt_set_prediction(c.h, 5) == SVO_ERR_STATE                  # the state before the mode
        assert L.svo_klt_predicted(c.h, 0, None, None, None, 0) == SVO_ERR_STATE and L.svo_klt_get_prediction(c.h) == 0
        c.klt_enable(seq_klt_params())
        c.klt_set_prediction(1)                               # the setter needs no svo_set_params ...
        assert L.svo_klt_predicted(c.h, 0, None, None, None, 0) == SVO_ERR_STATE and b"svo_set_params" in L.svo_last_error(c.h)      # ... the reader does
        # a svo_klt_enable that re-makes the buffers drops the guess buffer and returns to mode 0
        c.klt_enable(seq_klt_params(win=9))
        assert c.klt_prediction() == 0
        c.klt_enable(seq_klt_params(win=9))                   # the parameters in force: nothing happens
        c.klt_set_prediction(1)
        c.klt_enable(seq_klt_params(win=9))
        assert c.klt_prediction() == 1
    finally:
        c.close()


def test_mode_0_after_the_setter_equals_a_context_that_never_called_it():
    kp = seq_klt_params()
    A, B = make_ctx(kernel_times=True), make_ctx(kernel_times=True)
    try:
        for c in (A, B):
            c.klt_enable(kp)
        A.klt_set_prediction(1); A.klt_set_prediction(0)
        assert A.klt_prediction() == 0 and B.klt_prediction() == 0
        a = drive(A, KS.sequence_frames()[:4], KS.sequence_points())
        b = drive(B, KS.sequence_frames()[:4], KS.sequence_points())
        for f in range(4):
            assert_same(a[f][0], b[f][0], "frame %d" % f)
            assert same_tracks(a[f][1], b[f][1])
        ka, kb = A.kernel_times(appended=True), B.kernel_times(appended=True)
        assert list(ka) == list(kb) and "klt_predict" not in ka
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
        c.klt_set_prediction(1)
        assert list(c.kernel_times(appended=True)) == names0                     # the setter alone lists nothing
        c.klt_step([frames[1]]); c.klt_step([frames[2]])
        kt = c.kernel_times(appended=True)
        assert list(kt) == names0 + ["klt_predict"] and kt["klt_predict"][1] == 2 and kt["klt_select"][1] == 3
        c.klt_predicted(0)                                     # (the binding calls twice: for the count, then for the entries)
        assert c.kernel_times(appended=True)["klt_predict"][1] == 4
        assert list(c.kernel_times()) == names0[:c.FRAME_KERNEL_NAMES]
    finally:
        c.close()
