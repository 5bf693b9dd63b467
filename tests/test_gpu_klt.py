"""The resident KLT front end on the GPU (svo_klt_step and its companions), held byte for byte to the host recipe it replaces.

Every comparison is between two contexts: one driven by the device front end, one by tests/klt_ref.KltHostFrontEnd (a shift-only call,
Context.lk_track, the selection walk in numpy, the svo_put_* calls, stage 5).  `snapshot` reads every public getter of a lane -- both
keypoint lists with descriptors, both row tables, pairings, pairing IDs, the pairings' row table and the values record of the current
AND the previous slot, the tracked pairs, the result record, residuals and outliers -- and the two snapshots must be equal as bytes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import VOEC_BAD_TRACKING, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_CAPACITY, SVO_ERR_STATE = -2, -5, -6
SCENE_NAMES = [s.name for s in KS.scenes()]


def params():
    p = north_star_params(hip.default_params())
    p.orb_nlevels, p.orb_nfeats = 2, 300  # the detector's pyramid fits the 160 x 120 images (only the plain context of the last test detects)
    p.bad_tracking_th = 1 << 20          # a stage 4 run on put lists always ends in voecBadTracking: how a test makes a lane hold its previous frame
    return p


def klt_params(cap, lk=None, gate=None):
    p = hip.default_klt_params()
    p.cap = cap
    for k, v in (lk or {}).items():
        setattr(p.lk, k, v)
    for k, v in (gate or {}).items():
        setattr(p, k, v)
    return p


def make_ctx(n_lanes=1, **kw):
    cfg = dict(n_lanes=n_lanes, max_w=KS.W, max_h=KS.H, max_kps=KS.MAX_KPS, max_cand=1 << 15)
    cfg.update(kw)
    c = hip.Context(**cfg)
    c.set_params(params())
    c.set_camera(KS.sequence_world().camera())
    return c


def snapshot(c, lane=0):
    out = {}
    for which in (0, 1):
        for side in (0, 1):
            k, d = c.keypoints(lane, which, side)
            out["kps%d%d" % (which, side)] = k.tobytes() + d.tobytes()
            # (the row tables of a slot no frame was written to yet hold whatever the context's history left there)
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


def blank():
    return np.zeros((KS.H, KS.W), np.uint8)


# ---- 1. the selection on hand-built inputs ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_pair():
    """(the device context, the recipe's context, the recipe): one lane each, the gates and the cap of klt_scenes"""
    kp = klt_params(KS.CAP, dict(win=KS.WIN), KS.GATE)
    A, B = make_ctx(), make_ctx()
    A.klt_enable(kp)
    A.klt_step([(blank(), blank())], flags=0)        # a step gives the context the geometry of the scenes' image size
    fe = KR.KltHostFrontEnd(B, kp, KS.H)
    yield A, B, fe
    A.close(); B.close()


def run_ops(A, B, fe, ops):
    """a scene's operations on both sides; the lists the walk made of the last selection"""
    A.reset(); B.reset(); A.klt_reset(); fe.reset(); fe.stepped = [False] * B.n_lanes
    lists = None
    for op in ops:
        if op[0] == "add":
            assert A.klt_add_points(0, op[1], op[2]) == fe.add_points(0, op[1], op[2])
        elif op[0] == "bad_tracking":
            for c in (A, B):
                c.run_stages(hip.RUN_TRACK)
                assert c.result(0).error_code == VOEC_BAD_TRACKING
        else:
            A.klt_debug_select(0, *op[1:])
            lists, _ = fe.debug_select(0, op[1], op[2], op[3], op[4], KS.W, KS.H)
    return lists


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_selection_scene_equals_the_walk_and_the_recipe(scene_pair, name):
    A, B, fe = scene_pair
    sc = KS.scene(name)
    lists = run_ops(A, B, fe, sc.ops)
    # the device against the walk, list by list ...
    for side in (0, 1):
        assert A.keypoints(0, 0, side)[0].tobytes() == lists.kps[side].tobytes(), (name, side)
        assert A.row_index(0, 0, side).tobytes() == lists.row_index[side].tobytes(), (name, side)
    assert A.matches(0, 0).tobytes() == lists.matches.tobytes() and A.match_ids(0, 0).tobytes() == lists.ids.tobytes(), name
    assert A.tracked(0).tobytes() == lists.tracked.tobytes(), name
    assert A.matches_row_index(0, 0).tobytes() == lists.mrow_index.tobytes(), name
    r = A.result(0)
    assert (r.detected_left[0], r.detected_right[0], r.stereo_matches[0]) == (len(lists.ids),) * 3
    # ... every getter against the recipe's context, and the new table against the walk's
    assert_same(snapshot(A), snapshot(B), name)
    assert_tracks(A, 0, fe.tables[0], name)


def test_debug_select_wants_the_live_count(scene_pair):
    A, B, fe = scene_pair
    run_ops(A, B, fe, KS.scene("count_65").ops)
    before, tracks = snapshot(A), A.klt_tracks(0)
    n = len(tracks[2])
    l, r = KS.good(n + 1)
    rc = hip.lib().svo_debug_klt_select(A.h, 0, hip._vp(l), hip._vp(r), hip._vp(KS.ones(n + 1)), hip._vp(KS.ones(n + 1)), n + 1)
    assert rc == SVO_ERR_ARG and b"holds" in hip.lib().svo_last_error(A.h)
    assert_same(before, snapshot(A), "refused debug select")
    assert all(np.array_equal(a, b) for a, b in zip(tracks, A.klt_tracks(0)))


# ---- 2. the sequence ------------------------------------------------------------------------------------------------------------
def seq_klt_params(**lk):
    d = dict(KS.SEQ_LK); d.update(lk)
    return klt_params(KS.SEQ_CAP, d, KS.SEQ_GATE)


def drive(A, frames_of, n_frames, flags=hip.RUN_OPTIMIZE, **kw):
    """a one-lane device context through the sequence from the grid points: [(snapshot, tracks)] per frame"""
    A.reset(); A.klt_reset()
    assert A.klt_add_points(0, *KS.sequence_points()) == 48
    out = []
    for f in range(n_frames):
        A.klt_step([frames_of(f)], flags=flags, **kw)
        out.append((snapshot(A), A.klt_tracks(0)))
    return out


@pytest.fixture(scope="module")
def seq_pair():
    kp = seq_klt_params()
    A, B = make_ctx(), make_ctx()
    A.klt_enable(kp)
    yield A, B, kp
    A.close(); B.close()


@pytest.fixture(scope="module")
def single_run(seq_pair):
    """the device front end alone on the five frames: what the other layouts and the many-lane run must reproduce"""
    A, _, _ = seq_pair
    frames = KS.sequence_frames()
    return drive(A, lambda f: frames[f], KS.SEQ_FRAMES)


def recipe_run(B, kp, frame_ids, between=None):
    B.reset()
    fe = KR.KltHostFrontEnd(B, kp, KS.H)
    fe.add_points(0, *KS.sequence_points())
    frames = KS.sequence_frames()
    out = []
    for k, f in enumerate(frame_ids):
        fe.step([frames[f]])
        out.append((snapshot(B), fe.tables[0].copy(), B.result(0).valid))
        if between:
            between(k, fe)
    return out


def test_sequence_equals_the_recipe_frame_by_frame(seq_pair, single_run):
    A, B, kp = seq_pair
    ref = recipe_run(B, kp, range(KS.SEQ_FRAMES))
    walk = KS.sequence_walk()
    for f, ((snap, tracks), (rsnap, table, valid)) in enumerate(zip(single_run, ref)):
        assert_same(snap, rsnap, "frame %d" % f)
        assert tracks[0].tobytes() == table.left.tobytes() and tracks[1].tobytes() == table.right.tobytes(), f
        assert np.array_equal(tracks[2], table.ids) and np.array_equal(tracks[3], table.age), f
        # the recipe on the device tracker is the walk on tests/lk_ref.py
        assert table.left.tobytes() == walk[f][1].left.tobytes() and np.array_equal(table.ids, walk[f][1].ids), f
        # stage 5 really ran on these lists: asserted on the RECIPE's context
        if f >= 2:
            assert valid == 1, (f, valid)


# ---- 3. many lanes, an idle one, one never fed ----------------------------------------------------------------------------------
def test_five_lanes_with_an_idle_frame_and_an_unfed_lane(seq_pair, single_run):
    _, B, kp = seq_pair
    frames = KS.sequence_frames()
    A5 = make_ctx(n_lanes=5)
    try:
        A5.klt_enable(kp)
        for lane in (0, 2, 3):
            assert A5.klt_add_points(lane, *KS.sequence_points()) == 48
        unfed = snapshot_lists(A5, 4)
        skip = recipe_run(B, kp, [0, 1, 3, 4])               # lane 3 sits frame 2 out and resumes from frame 1
        k3 = 0
        for f in range(KS.SEQ_FRAMES):
            active = [0, 2] if f == 2 else [0, 2, 3]
            before3 = (snapshot(A5, 3), A5.klt_tracks(3)) if f == 2 else None
            A5.klt_step([frames[f] if l in active else None for l in range(5)], active=active)
            for lane in (0, 2):
                assert_same(snapshot(A5, lane), single_run[f][0], "lane %d frame %d" % (lane, f))
                assert all(np.array_equal(a, b) for a, b in zip(A5.klt_tracks(lane), single_run[f][1])), (lane, f)
            if f == 2:
                assert_same(snapshot(A5, 3), before3[0], "the idle lane")
                assert all(np.array_equal(a, b) for a, b in zip(A5.klt_tracks(3), before3[1]))
            else:
                assert_same(snapshot(A5, 3), skip[k3][0], "lane 3 frame %d" % f)
                assert_tracks(A5, 3, skip[k3][1], "lane 3 frame %d" % f)
                k3 += 1
            assert snapshot_lists(A5, 4) == unfed and len(A5.klt_tracks(4)[2]) == 0 and len(A5.klt_tracks(1)[2]) == 0
        # svo_klt_reset on one lane leaves the others alone
        keep = A5.klt_tracks(0)
        A5.klt_reset([2])
        assert len(A5.klt_tracks(2)[2]) == 0 and all(np.array_equal(a, b) for a, b in zip(A5.klt_tracks(0), keep))
    finally:
        A5.close()


def snapshot_lists(c, lane):
    """the getters that need no geometry: for a lane nothing was ever put into"""
    return (c.keypoints(lane, 0, 0)[0].tobytes(), c.matches(lane, 0).tobytes(), c.tracked(lane).tobytes(), bytes(c.result(lane)))


# ---- 4. variants ---------------------------------------------------------------------------------------------------------------
def test_device_and_pinned_images_equal_host_images(seq_pair, single_run):
    import torch
    A, _, _ = seq_pair
    frames = KS.sequence_frames()
    stride = 192                                          # rows wider than the image: the copy honours the stride
    dev, pin = [], []
    for l, r in frames:
        for im, dst in ((l, 0), (r, 1)):
            host = np.zeros((KS.H, stride), np.uint8); host[:, :KS.W] = im
            t = torch.from_numpy(host).cuda()
            p = torch.from_numpy(host).pin_memory()
            dev.append(t); pin.append(p)
    torch.cuda.synchronize()
    rec = lambda ts, f: tuple((ts[2 * f + s].data_ptr(), KS.W, KS.H, stride) for s in (0, 1))
    for name, ts, kw in (("device", dev, dict(device=True)), ("pinned", pin, dict(pinned=True))):
        got = drive(A, lambda f: rec(ts, f), KS.SEQ_FRAMES, **kw)
        for f in range(KS.SEQ_FRAMES):
            assert_same(got[f][0], single_run[f][0], "%s images, frame %d" % (name, f))
            assert all(np.array_equal(a, b) for a, b in zip(got[f][1], single_run[f][1])), (name, f)


def test_forward_backward_add_points_and_reset_equal_the_recipe(seq_pair):
    """fb_max = 0.5 (the backward launch), a top-up of 10 points after the second frame, a call that overflows cap, and a reset of the
    lane after the fourth frame followed by fresh points: the device and the recipe agree after every frame"""
    A, B, kp0 = seq_pair
    kp = seq_klt_params(fb_max=0.5)
    A.reset(); A.klt_reset()
    A.klt_enable(kp)                                      # other parameters: accepted because the table is empty
    frames, world = KS.sequence_frames(), KS.sequence_world()
    B.reset()
    fe = KR.KltHostFrontEnd(B, kp, KS.H)
    for side in (A.klt_add_points, fe.add_points):
        assert side(0, *KS.sequence_points()) == 48
    try:
        for f in range(KS.SEQ_FRAMES):
            A.klt_step([frames[f]]); fe.step([frames[f]])
            assert_same(snapshot(A), snapshot(B), "fb frame %d" % f)
            assert_tracks(A, 0, fe.tables[0], "fb frame %d" % f)
            if f == 1:                                    # a top-up between the grid points, then more than the table can take
                left = np.array([(20.0 + 13 * i, 30.0 + 6 * i) for i in range(10)], np.float32)
                right = left.copy(); right[:, 0] -= (world.f * world.B / KS.gt_depth(world, 1, left)).astype(np.float32)
                assert A.klt_add_points(0, left, right) == fe.add_points(0, left, right) == 10
                live = len(fe.tables[0])
                many = KS.good(KS.SEQ_CAP)
                assert A.klt_add_points(0, *many) == fe.add_points(0, *many) == KS.SEQ_CAP - live
                assert_tracks(A, 0, fe.tables[0], "after the overflow")
            if f == 3:
                A.klt_reset([0]); fe.reset([0])
                assert len(A.klt_tracks(0)[2]) == 0
                for side in (A.klt_add_points, fe.add_points):
                    assert side(0, *KS.sequence_points()) == 48
                assert A.klt_tracks(0)[2][0] == fe.tables[0].ids[0] == 0          # a reset lane numbers its tracks afresh
    finally:
        A.reset(); A.klt_reset(); A.klt_enable(kp0)


# ---- 5. refusals, kernel-time names, contexts that never enable the front end ------------------------------------------------------
def _frames(n, pairs, flags_device=False):
    fr = (hip.Frame * n)()
    for i, (l, r) in enumerate(pairs):
        if l is not None:
            fr[i].left = hip.Image(l.ctypes.data, l.shape[1], l.shape[0], l.strides[0])
        if r is not None:
            fr[i].right = hip.Image(r.ctypes.data, r.shape[1], r.shape[0], r.strides[0])
    return fr


def test_refusals_leave_everything_untouched(seq_pair):
    A, _, kp = seq_pair
    L = hip.lib()
    frames = KS.sequence_frames()
    drive(A, lambda f: frames[f], 2)
    before, tracks = snapshot(A), A.klt_tracks(0)
    good = _frames(1, [frames[2]])
    small = np.zeros((60, 60), np.uint8)
    big = np.zeros((KS.H + 1, KS.W), np.uint8)
    words = (C.c_uint64 * 2)(2, 0)
    cases = [
        (L.svo_klt_step(A.h, good, hip.FLAG_BGR_IMAGES, None), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, good, hip.RUN_OPTIMIZE | hip.RUN_MATCH, None), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, good, hip.FLAG_DEVICE_IMAGES | hip.FLAG_PINNED_IMAGES, None), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, None, hip.RUN_OPTIMIZE, None), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, good, hip.RUN_OPTIMIZE, words), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, _frames(1, [(frames[2][0], None)]), hip.RUN_OPTIMIZE, None), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, _frames(1, [(frames[2][0], small)]), hip.RUN_OPTIMIZE, None), SVO_ERR_ARG),
        (L.svo_klt_step(A.h, _frames(1, [(small, small)]), hip.RUN_OPTIMIZE, None), SVO_ERR_CAPACITY),
        (L.svo_klt_step(A.h, _frames(1, [(big, big)]), hip.RUN_OPTIMIZE, None), SVO_ERR_CAPACITY),
        (L.svo_klt_add_points(A.h, 1, None, None, 0), SVO_ERR_ARG),
        (L.svo_klt_add_points(A.h, 0, None, None, 3), SVO_ERR_ARG),
        (L.svo_klt_get_tracks(A.h, -1, None, None, None, None, 0), SVO_ERR_ARG),
    ]
    for i, (rc, want) in enumerate(cases):
        assert rc == want, (i, rc, want)
    assert L.svo_last_error(A.h)
    # the parameters: ranges, the capacity, and other parameters while the table holds tracks
    for change, want in ((dict(cap=0), SVO_ERR_ARG), (dict(cap=KS.MAX_KPS + 1), SVO_ERR_CAPACITY), (dict(max_dy=-1.0), SVO_ERR_ARG),
                         (dict(min_disp=2.0, max_disp=1.0), SVO_ERR_ARG), (dict(cap=32), SVO_ERR_STATE)):
        p = seq_klt_params()
        for k, v in change.items():
            setattr(p, k, v)
        assert L.svo_klt_enable(A.h, C.byref(p)) == want, change
    p = seq_klt_params(win=4)
    assert L.svo_klt_enable(A.h, C.byref(p)) == SVO_ERR_ARG
    assert L.svo_klt_enable(A.h, C.byref(kp)) == 0           # the parameters in force again: nothing happens
    assert_same(before, snapshot(A), "after the refusals")
    assert all(np.array_equal(a, b) for a, b in zip(tracks, A.klt_tracks(0)))
    # the next frame is what it would have been
    A.klt_step([frames[2]])
    cfg = dict(n_lanes=1, max_w=KS.W, max_h=KS.H, max_kps=KS.MAX_KPS, max_cand=1 << 15)
    # a context that has not enabled the front end, and one without parameters
    c = hip.Context(**cfg)
    try:
        assert L.svo_klt_step(c.h, good, hip.RUN_OPTIMIZE, None) == SVO_ERR_STATE and b"not enabled" in L.svo_last_error(c.h)
        assert L.svo_klt_add_points(c.h, 0, None, None, 0) == SVO_ERR_STATE
        c.klt_enable(kp)
        assert L.svo_klt_step(c.h, good, hip.RUN_OPTIMIZE, None) == SVO_ERR_STATE and b"svo_set_params" in L.svo_last_error(c.h)
    finally:
        c.close()


def test_a_member_of_a_frame_parallel_stream_is_refused():
    from stereo_vo_amd.pipeline import FrameParallelStream
    fp = FrameParallelStream(params(), KS.sequence_world().camera(), KS.W, KS.H, lanes=1, contexts=2, max_kps=KS.MAX_KPS, max_cand=1 << 15)
    try:
        kp = seq_klt_params()
        for c in fp.ctxs:
            assert hip.lib().svo_klt_enable(c.h, C.byref(kp)) == SVO_ERR_STATE and b"frame-parallel" in hip.lib().svo_last_error(c.h)
    finally:
        fp.close()


def test_kernel_time_names_are_appended_as_documented():
    c = make_ctx(kernel_times=True)
    try:
        names0 = list(c.kernel_times(appended=True))
        assert "klt_select" not in names0 and "lk_track" not in names0
        c.klt_enable(seq_klt_params())
        assert list(c.kernel_times(appended=True)) == names0          # enabling alone lists nothing
        c.klt_add_points(0, *KS.sequence_points())
        frames = KS.sequence_frames()
        c.klt_step([frames[0]]); c.klt_step([frames[1]])
        kt = c.kernel_times(appended=True)
        assert list(kt)[:len(names0)] == names0 and list(kt)[len(names0):] == ["lk_pyrdown", "lk_track", "klt_select"]
        assert kt["klt_select"][1] == 2 and kt["lk_track"][1] == 1 and kt["lk_pyrdown"][1] == 2 and kt["gauss_newton"][1] == 2
        assert list(c.kernel_times()) == names0[:c.FRAME_KERNEL_NAMES]
    finally:
        c.close()


def test_a_context_that_never_enables_it_is_unaffected(seq_pair):
    A, _, _ = seq_pair
    frames = KS.sequence_frames()
    plain = make_ctx(kernel_times=True)
    try:
        def run():
            plain.reset()
            plain.process_host([frames[0]]); plain.process_host([frames[1]])
            return snapshot(plain)
        first = run()
        names = list(plain.kernel_times(appended=True))
        drive(A, lambda f: frames[f], 2)
        assert_same(first, run(), "a plain context around another context's steps")
        assert list(plain.kernel_times(appended=True)) == names and "klt_select" not in names
    finally:
        plain.close()
