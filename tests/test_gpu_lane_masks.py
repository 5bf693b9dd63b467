"""svo_process_lanes: a step in which some lanes take no part.  For an idle lane the call is as if it had not been made, for an
active one it is svo_process -- every lane is held against an oracle of its own that sees a frame only on the lane's active steps.

Integers and lists are compared bit for bit; the pose and residual tolerances are those of test_gpu_parity.assert_same_frame."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import DM_FAST_ORB, StereoCamera, north_star_params
from stereo_vo_amd.synth import SyntheticStereoWorld

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
from test_gpu_parity import O, assert_same_frame, load_small    # noqa: E402
from test_gpu_frame_layouts import assert_same_octaves          # noqa: E402
from test_gpu_faster import assert_same_lists, assert_same_pairings, snapshot as octave_snapshot       # noqa: E402
from test_gpu_sad import assert_same_snapshot                   # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6
W, H, STEPS = 320, 240, 8
# lane 0 every step; lane 1 starts late (still unstarted while the others run); lane 2 alternates; lane 3 ends early
SCHEDULE = ([1] * 8, [0, 0, 1, 1, 1, 1, 1, 1], [1, 0, 1, 0, 1, 0, 1, 0], [1, 1, 1, 0, 0, 0, 0, 0])


def active_at(step):
    return [l for l in range(len(SCHEDULE)) if SCHEDULE[l][step]]


_FRAMES = []


def lane_frames():
    """frames[lane][k]: the k-th frame the lane's camera delivers -- a world of its own per lane, as many frames as the schedule has
    active steps for it; rendered once and shared by the three staggered tests (read only)"""
    if not _FRAMES:
        out = []
        for l, sched in enumerate(SCHEDULE):
            world = SyntheticStereoWorld(W, H, 400.0 * W / 640.0, 0.12, seed=300 + l, n_frames=STEPS)
            out.append([tuple(np.ascontiguousarray(x.numpy()) for x in world.render(t)) for t in range(sum(sched))])
        _FRAMES.extend([out, world.camera()])
    return _FRAMES


def assert_fresh(ctx, lane, n_oct, tag):
    """a lane nothing has touched: the zeroed record and the empty lists of a context just created"""
    r = ctx.result(lane)
    assert (r.valid, r.error_code, r.num_it, r.num_it_final, r.n_residual, r.n_outliers, r.status) == (0, 0, 0, 0, 0, 0, 0), tag
    assert r.tracked_feats_from_last_frame == 0 and r.tracked_feats_from_last_KF == 0 and list(r.track_stats) == [0] * 8, tag
    assert list(r.outPose) == [0.0] * 6 and ctx.status_word(lane) == 0, tag
    for o in range(n_oct):
        assert (r.detected_left[o], r.detected_right[o], r.stereo_matches[o]) == (0, 0, 0), (tag, o)
        for which in (0, 1):
            for side in (0, 1):
                assert len(ctx.keypoints(lane, which, side, o)[0]) == 0, (tag, which, side, o)
            assert len(ctx.matches(lane, which, o)) == 0 and len(ctx.match_ids(lane, which, o)) == 0, (tag, which, o)
        assert len(ctx.tracked(lane, o)) == 0, (tag, o)


def assert_lane(ctx, lane, orc, ro, n_oct, ids, tag):
    """the lane against its oracle's CURRENT state (ro: the record of the oracle's last frame), previous frame included"""
    r = ctx.result(lane)
    if n_oct == 1:
        assert_same_frame(ctx, lane, orc, r, ro, tag)
    else:
        assert_same_octaves(ctx, lane, orc, r, ro, n_oct, tag)
    assert list(r.track_stats) == list(ro.track_stats) and r.tracked_feats_from_last_frame == ro.tracked_feats_from_last_frame, tag
    has_prev = len(ctx.keypoints(lane, 1, 0, 0)[0]) > 0
    assert has_prev == (len(orc.keypoints(1, 0, 0)[0]) > 0), (tag, "previous frame present")
    for o in range(n_oct):
        if ids:
            assert (ctx.match_ids(lane, 0, o) == orc.match_ids(0, o)).all() and len(ctx.match_ids(lane, 0, o)) == ro.stereo_matches[o], (tag, "match IDs", o)
        if not has_prev:
            continue
        for side in (0, 1):
            assert ctx.keypoints(lane, 1, side, o)[0].tobytes() == orc.keypoints(1, side, o)[0].tobytes(), (tag, "previous frame", o, side)
        assert ctx.matches(lane, 1, o).tobytes() == orc.matches(1, o).tobytes(), (tag, "previous pairings", o)
        if ids:
            assert (ctx.match_ids(lane, 1, o) == orc.match_ids(1, o)).all(), (tag, "previous match IDs", o)
    if ids:
        assert r.tracked_feats_from_last_KF == ro.tracked_feats_from_last_KF, tag
    assert ctx.status_word(lane) == 0, tag


def oracle_params(kind):
    if kind == "orb":
        return north_star_params(hip.default_params(), orb_nfeats=400), 1, False
    p = north_star_params(hip.default_params(), orb_nfeats=300)
    p.detect_method = DM_FAST_ORB; p.nOctaves = 2; p.nmsMethod = 1
    p.match_method = 1; p.ifm_method = 1; p.max_y_diff = 2.0; p.ifm_win_w = 20; p.ifm_win_h = 30
    p.vo_use_matches_ids = 1
    return p, 2, True


@pytest.mark.parametrize("kind", ["orb", "fastorb_anms_rbr_win_ids"])
def test_staggered_lanes_against_their_own_oracles(kind):
    """four lanes on the fixed schedule above, the idle lanes' frames[] entries NULL: after every step every lane equals its own
    oracle, which processed a frame only on the lane's active steps.  With match IDs: an idle step consumes none."""
    p, n_oct, ids = oracle_params(kind)
    frames, cam = lane_frames()
    ctx = hip.Context(n_lanes=4, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, max_octaves=n_oct)
    ctx.set_params(p); ctx.set_camera(cam)
    orcs = [O().Oracle(p) for _ in range(4)]
    last, k = [None] * 4, [0] * 4
    for step in range(STEPS):
        act = active_at(step)
        ctx.process_host([frames[l][k[l]] if l in act else None for l in range(4)], active=act)
        for l in act:
            last[l] = orcs[l].process(frames[l][k[l]][0], frames[l][k[l]][1], cam)
            k[l] += 1
        for l in range(4):
            tag = "%s step %d lane %d (%s)" % (kind, step, l, "active" if l in act else "idle")
            if last[l] is None:
                assert_fresh(ctx, l, n_oct, tag)
            else:
                assert_lane(ctx, l, orcs[l], last[l], n_oct, ids, tag)
    assert k == [8, 6, 4, 3]
    assert last[0].valid and last[1].valid and last[0].tracked_feats_from_last_frame > 20, (last[0].valid, last[1].valid)
    if ids:
        assert orcs[2].match_ids(0, 0).max() > orcs[2].match_ids(1, 0).max() > 0      # the alternating lane's IDs did advance, by its own frames only
    ctx.close()


def test_staggered_lanes_dmfaster_sad():
    """dmFASTER + smSAD + ifmSAD on two octaves, the same schedule: the lists and pairings of every active frame are those of the
    walks in tests/faster_ref.py / tests/sad_ref.py, and every lane's whole state -- tracked pairs, counters, pose, residuals -- equals
    a one-lane context that was handed the lane's frames alone (as test_gpu_faster compares lanes)"""
    NO = 2
    p = F.faster_params(hip.default_params(), t=20, orb_nfeats=400, n_oct=NO, sad=800, ifm_sad=800)
    p.ifm_win_w = p.ifm_win_h = 24
    frames, cam = lane_frames()
    kw = dict(max_w=W, max_h=H, max_kps=1024, max_cand=1 << 16, max_octaves=NO)
    ctx = hip.Context(n_lanes=4, **kw)
    ctx.set_params(p); ctx.set_camera(cam)
    single = [hip.Context(n_lanes=1, **kw) for _ in range(4)]
    for c in single:
        c.set_params(p); c.set_camera(cam)
    k, tracked = [0] * 4, 0
    for step in range(STEPS):
        act = active_at(step)
        ctx.process_host([frames[l][k[l]] if l in act else None for l in range(4)], active=act)
        for l in act:
            single[l].process_host([frames[l][k[l]]])
        res = ctx.results()
        for l in range(4):
            tag = "faster step %d lane %d" % (step, l)
            if k[l] == 0 and l not in act:
                assert_fresh(ctx, l, NO, tag)
                continue
            if l in act:                          # the walks: numpy FAST-12 + KLT response, the oracle's NMS and row sort, the SAD matcher
                feats = F.faster_features(frames[l][k[l]][0], frames[l][k[l]][1], p, 4)
                assert min(len(f[0]) for f in feats) >= 30, [len(f[0]) for f in feats]
                assert_same_lists(ctx, l, feats, tag, res[l])
                assert_same_pairings(ctx, l, feats, p, tag, res[l])
            assert_same_snapshot(octave_snapshot(ctx, l, res[l], NO), octave_snapshot(single[l], 0, single[l].result(0), NO), tag)
            for o in range(NO):
                assert ctx.keypoints(l, 1, 0, o)[0].tobytes() == single[l].keypoints(0, 1, 0, o)[0].tobytes(), (tag, "previous frame", o)
            tracked = max(tracked, res[l].tracked_feats_from_last_frame)
        for l in act:
            k[l] += 1
    assert tracked >= 20, tracked
    ctx.close()
    for c in single:
        c.close()


def test_mask_words_at_the_64_lane_boundary(golden_dir):
    """70 lanes, active {0, 63, 64, 69} for two steps: both words of the mask reach the kernels, the neighbours 62 and 65 stay fresh"""
    g, cam, p = load_small(golden_dir)
    Wg, Hg = int(g["W"]), int(g["H"])
    ctx = hip.Context(n_lanes=70, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    act = [0, 63, 64, 69]
    orcs = {63: O().Oracle(p), 64: O().Oracle(p)}
    for t in range(2):
        # lane 63 runs one frame behind lane 64: a lane that read its neighbour's bit would show the neighbour's frame
        pick = {0: t, 63: t, 64: t + 1, 69: t + 2}
        ctx.process_host([(g["L%d" % pick[l]], g["R%d" % pick[l]]) if l in act else None for l in range(70)], active=act)
        for l in (63, 64):
            ro = orcs[l].process(g["L%d" % pick[l]], g["R%d" % pick[l]], cam)
            assert_lane(ctx, l, orcs[l], ro, 1, False, "t=%d lane %d" % (t, l))
        for l in (62, 65):
            assert_fresh(ctx, l, 1, "t=%d lane %d" % (t, l))
    assert ctx.result(64).valid
    ctx.close()


def test_recovery_across_an_idle_step(golden_dir):
    """valid frames, a blank frame (voecBadTracking), an idle step, a valid frame: the shift rule of P:86-100 applies once -- the
    lane equals an oracle that never saw the idle step, keeps its previous frame across the bad one and is valid again afterwards"""
    g, cam, p = load_small(golden_dir)
    Wg, Hg = int(g["W"]), int(g["H"])
    ctx = hip.Context(n_lanes=2, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    blank = np.full_like(g["L0"], 128)
    fr = lambda t: (g["L%d" % t], g["R%d" % t])
    lane0 = [fr(0), fr(1), (blank, blank), None, fr(2), fr(3)]          # None: the lane sits the step out
    lane1 = [fr(3), fr(2), fr(1), fr(0), fr(1), fr(2)]
    orcs, last = [O().Oracle(p), O().Oracle(p)], [None, None]
    codes = []
    for step, pairs in enumerate(zip(lane0, lane1)):
        act = [l for l in (0, 1) if pairs[l] is not None]
        ctx.process_host(list(pairs), active=act)
        for l in act:
            last[l] = orcs[l].process(pairs[l][0], pairs[l][1], cam)
        for l in (0, 1):
            assert_lane(ctx, l, orcs[l], last[l], 1, False, "step %d lane %d" % (step, l))
        codes.append((ctx.result(0).valid, ctx.result(0).error_code))
    assert codes[1][0] == 1 and codes[2] == (0, 5) and codes[3] == (0, 5) and codes[4][0] == 1 and codes[5][0] == 1, codes     # 5: voecBadTracking
    ctx.close()


def lane_bytes(ctx, lane):
    r = ctx.result(lane)
    return (bytes(r), ctx.keypoints(lane, 0, 0)[0].tobytes(), ctx.keypoints(lane, 0, 1)[0].tobytes(), ctx.keypoints(lane, 0, 0)[1].tobytes(),
            ctx.keypoints(lane, 1, 0)[0].tobytes(), ctx.matches(lane).tobytes(), ctx.matches(lane, 1).tobytes(), ctx.tracked(lane).tobytes(),
            ctx.residuals(lane).tobytes(), ctx.outliers(lane).tobytes(), ctx.status_word(lane))


def test_split_and_pipelined_call_shapes(golden_dir):
    """detect-no-post / post / stages 3-5 as three calls, and the SVO_FLAG_DETECT_AHEAD pair, each with a partial mask: the results are
    those of the one-call masked step.  A different mask on a later call of the frame is SVO_ERR_STATE and changes nothing."""
    g, cam, p = load_small(golden_dir)
    Wg, Hg = int(g["W"]), int(g["H"])
    AHEAD = 4096
    kw = dict(n_lanes=3, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15)
    one, three, ahead = hip.Context(**kw), hip.Context(**kw), hip.Context(**kw)
    for c in (one, three, ahead):
        c.set_params(p); c.set_camera(cam)
    masks = [[0, 1, 2], [0, 2], [1, 2], [0, 1, 2]]
    REST = hip.RUN_MATCH | hip.RUN_TRACK | hip.RUN_OPTIMIZE
    for t, act in enumerate(masks):
        pairs = [(g["L%d" % ((t + l) % 4)], g["R%d" % ((t + l) % 4)]) if l in act else None for l in range(3)]
        one.process_host(pairs, active=act)
        three.process_host(pairs, hip.RUN_DETECT | hip.FLAG_DETECT_NO_POST, active=act)
        if t == 1:
            before = [lane_bytes(three, l) for l in range(3)]
            for wrong in ([0, 1, 2], [0], [1]):
                w = hip.lane_mask_words(wrong, 3) + [0]
                rc = three.L.svo_process_lanes(three.h, None, C.c_uint32(hip.RUN_DETECT_POST | hip.FLAG_NO_SHIFT), (C.c_uint64 * 2)(*w))
                assert rc == SVO_ERR_STATE and b"same mask" in three.L.svo_last_error(three.h), (wrong, rc)
            rc = three.L.svo_process(three.h, None, C.c_uint32(REST | hip.FLAG_NO_SHIFT))          # svo_process counts as every lane
            assert rc == SVO_ERR_STATE
            assert [lane_bytes(three, l) for l in range(3)] == before
        three.run_stages(hip.RUN_DETECT_POST, active=act)
        three.run_stages(REST, active=act)
        ahead.process_host(pairs, hip.RUN_DETECT | hip.FLAG_DETECT_NO_POST | hip.FLAG_NO_SHIFT | AHEAD, active=act)
        if t == 2:
            w = hip.lane_mask_words([0, 1, 2], 3) + [0]
            rc = ahead.L.svo_process_lanes(ahead.h, None, C.c_uint32(hip.RUN_DETECT_POST | REST | AHEAD), (C.c_uint64 * 2)(*w))
            assert rc == SVO_ERR_STATE and ahead.L.svo_last_error(ahead.h)
        ahead._process(None, hip.RUN_DETECT_POST | REST | AHEAD, hip.lane_mask_words(act, 3))
        ref = [lane_bytes(one, l) for l in range(3)]
        assert [lane_bytes(three, l) for l in range(3)] == ref, ("three calls", t)
        assert [lane_bytes(ahead, l) for l in range(3)] == ref, ("detect ahead", t)
    assert one.result(2).valid and one.result(0).valid
    for c in (one, three, ahead):
        c.close()


def test_refusals_and_no_ops(golden_dir):
    g, cam, p = load_small(golden_dir)
    Wg, Hg = int(g["W"]), int(g["H"])
    ctx = hip.Context(n_lanes=3, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15, kernel_times=True)
    ctx.set_params(p); ctx.set_camera(cam)
    L = ctx.L
    imgs = [np.ascontiguousarray(g[k]) for k in ("L0", "R0", "L1", "R1")]

    def table(t, lanes):
        fr = (hip.Frame * 3)()
        for l in lanes:
            fr[l].left = hip.Image(imgs[2 * t].ctypes.data, Wg, Hg, Wg)
            fr[l].right = hip.Image(imgs[2 * t + 1].ctypes.data, Wg, Hg, Wg)
        return fr

    def counts():
        ctx.wait()
        return {k: v[1] for k, v in ctx.kernel_times().items() if v[1]}

    mask = lambda *w: (C.c_uint64 * 2)(*w)
    # a bit at or above n_lanes, in either word
    for w in ((0b1000, 0), (1, 1), (0, 1 << 63)):
        assert L.svo_process_lanes(ctx.h, table(0, (0, 1, 2)), C.c_uint32(hip.RUN_ALL), mask(*w)) == SVO_ERR_ARG, w
        assert b"n_lanes" in L.svo_last_error(ctx.h)
    assert L.svo_process_lanes(ctx.h, table(0, (0, 1, 2)), C.c_uint32(hip.RUN_ALL), None) == SVO_ERR_ARG
    # NULL data in an active lane; NULL in an idle one is fine
    assert L.svo_process_lanes(ctx.h, table(0, (0,)), C.c_uint32(hip.RUN_ALL), mask(0b011, 0)) == SVO_ERR_ARG
    assert counts() == {}
    # nobody active: SVO_OK, nothing enqueued, no text
    assert L.svo_process_lanes(ctx.h, table(0, ()), C.c_uint32(hip.RUN_ALL), mask(0, 0)) == 0
    assert L.svo_last_error(ctx.h) == b"" and counts() == {}
    for l in range(3):
        assert_fresh(ctx, l, 1, "after the refusals, lane %d" % l)
    # every lane active: the launches of svo_process, name for name and count for count
    per_frame = []
    for t, masked in enumerate((False, True)):
        ctx.kernel_times_reset()
        if masked:
            assert L.svo_process_lanes(ctx.h, table(t, (0, 1, 2)), C.c_uint32(hip.RUN_ALL), mask(0b111, 0)) == 0
        else:
            assert L.svo_process(ctx.h, table(t, (0, 1, 2)), C.c_uint32(hip.RUN_ALL)) == 0
        per_frame.append(counts())
    assert per_frame[0] == per_frame[1] and per_frame[0]["fast"] == 1 and per_frame[0]["gauss_newton"] == 1, per_frame
    # ... and an all-clear mask in mid-stream leaves the counts and the lanes alone
    before = [lane_bytes(ctx, l) for l in range(3)]
    ctx.kernel_times_reset()
    assert L.svo_process_lanes(ctx.h, table(0, ()), C.c_uint32(hip.RUN_ALL), mask(0, 0)) == 0
    assert counts() == {} and [lane_bytes(ctx, l) for l in range(3)] == before
    ctx.close()


def test_graphs_replay_all_active_steps_and_step_aside_for_a_partial_mask(golden_dir):
    """svo_use_graphs: masked steps with every lane active are captured and replayed, a partial mask in between runs as plain
    launches, and the next all-active step replays again -- each lane equal to its oracle throughout"""
    g, cam, p = load_small(golden_dir)
    Wg, Hg = int(g["W"]), int(g["H"])
    ctx = hip.Context(n_lanes=2, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam); ctx.use_graphs(True)
    orcs, last = [O().Oracle(p), O().Oracle(p)], [None, None]
    # (frame of lane 0, frame of lane 1) per step; steps 0-3 capture both ring slots and replay them, step 4 is partial
    seq = [((0, 1), [0, 1]), ((1, 2), [0, 1]), ((2, 3), [0, 1]), ((3, 0), [0, 1]), ((0, None), [0]), ((1, 1), [0, 1]), ((None, 2), [1]), ((2, 3), [0, 1]), ((3, 0), [0, 1])]
    for i, (ts, act) in enumerate(seq):
        pairs = [(g["L%d" % t], g["R%d" % t]) if t is not None else None for t in ts]
        before = ctx.graph_count()
        ctx.process_host(pairs, active=act)
        cap, rep = ctx.graph_count()
        if len(act) == 2:       # captured (a ring slot seen for the first time) or replayed: never plain
            assert (cap - before[0], rep - before[1]) in ((1, 0), (0, 1)), ("all-active step %d" % i, before, (cap, rep))
        else:                   # plain launches: nothing captured, nothing replayed
            assert (cap, rep) == before, ("partial step %d" % i, before, (cap, rep))
        for l in act:
            last[l] = orcs[l].process(pairs[l][0], pairs[l][1], cam)
        for l in (0, 1):
            assert_lane(ctx, l, orcs[l], last[l], 1, False, "graphs step %d lane %d" % (i, l))
    assert ctx.graph_count() == (2, 5)          # seven all-active steps: one capture per ring slot, the rest replays
    ctx.close()


@pytest.mark.parametrize("path", ["device", "pinned", "bgr", "rectify"])
def test_partial_masks_on_every_frame_path(golden_dir, path):
    """the other ways a frame comes in, each with idle lanes whose entries are None: device frames read in place, page-locked
    frames on the copy stream, and stage 1 on the device (k_prepare: BGR frames with three equal channels, an identity
    rectification map -- both reproduce the grey image exactly, so the oracle sees the plain frames)"""
    import torch
    g, cam, p = load_small(golden_dir)
    Wg, Hg = int(g["W"]), int(g["H"])
    ctx = hip.Context(n_lanes=3, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    if path == "rectify":
        mx, my = np.meshgrid(np.arange(Wg, dtype=np.float32), np.arange(Hg, dtype=np.float32))
        for side in (0, 1):
            ctx.set_rectify_map(-1, side, mx, my)
    orcs, last, keep = [O().Oracle(p) for _ in range(3)], [None] * 3, []
    for step, act in enumerate(([0, 1, 2], [0, 2], [1], [0, 1, 2])):
        pick = {l: (step + l) % 4 for l in act}
        imgs = {l: (g["L%d" % t], g["R%d" % t]) for l, t in pick.items()}
        if path in ("device", "pinned"):
            tens = {l: tuple(torch.from_numpy(x).cuda() if path == "device" else torch.from_numpy(np.ascontiguousarray(x)).pin_memory() for x in imgs[l]) for l in act}
            keep.append(tens)
            torch.cuda.synchronize()
            ptrs = [(tens[l][0].data_ptr(), tens[l][1].data_ptr()) if l in act else None for l in range(3)]
            (ctx.process_device if path == "device" else ctx.process_pinned)(ptrs, Wg, Hg, Wg, active=(l for l in act))      # (a generator: consumed once)
            if path == "pinned":
                ctx.wait_upload()
        elif path == "bgr":
            ctx.process_host([tuple(np.repeat(x[:, :, None], 3, axis=2) for x in imgs[l]) if l in act else None for l in range(3)], active=act)
        else:
            ctx.process_host([imgs[l] if l in act else None for l in range(3)], active=act)
        for l in act:
            last[l] = orcs[l].process(imgs[l][0], imgs[l][1], cam)
        for l in range(3):
            assert_lane(ctx, l, orcs[l], last[l], 1, False, "%s step %d lane %d" % (path, step, l))
    assert all(ctx.result(l).valid for l in range(3))
    ctx.close()
