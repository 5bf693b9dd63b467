"""dmFASTER on the HIP path against tests/faster_ref.py (FAST-12 + KLT response in numpy, the oracle's NMS and row sort) and, downstream
of the lists, the SAD walks of tests/sad_ref.py.

Integers and lists are compared bit for bit; pose and residual tolerances are those of test_gpu_sad.assert_same_as_reference.
tests/test_faster_cpu.py asserts, from the reference alone, that every input used here has something to compare."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, DM_FAST_ORB, DM_FASTER, DM_KLT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
import image_content as IC                                      # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_faster_cpu import BIG_T, CHECKER_SEED, big_list_frame, geometry_crops, photograph      # noqa: E402
from test_gpu_parity import O                                   # noqa: E402
from test_gpu_frame_layouts import lay_out, make_frames         # noqa: E402
from test_gpu_sad import assert_same_as_reference, assert_same_snapshot     # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_UNSUPPORTED, SVO_ERR_STATE = -2, -3, -6
NEW_KERNELS = ("faster", "faster_nms")
ST_CAND_OVERFLOW, ST_KPS_OVERFLOW = 1, 2


def params(t=20, orb_nfeats=500, n_oct=3, nms=1, **kw):
    return F.faster_params(hip.default_params(), t=t, orb_nfeats=orb_nfeats, n_oct=n_oct, nms=nms, **kw)


def assert_same_lists(ctx, lane, feats, tag, r=None):
    """per octave: the keypoint records (all seven fields), the row tables and the all-zero descriptor rows"""
    for o, f in enumerate(feats):
        for side in (0, 1):
            k, d = ctx.keypoints(lane, 0, side, o)
            assert len(k) == len(f[side]) and k.tobytes() == f[side].tobytes(), (tag, "keypoints", o, side, len(k), len(f[side]))
            assert d.shape == (len(k), 32) and not d.any(), (tag, "descriptors", o, side)
            assert (ctx.row_index(lane, 0, side, o) == f[2 + side]).all(), (tag, "row table", o, side)
        if r is not None:
            assert (r.detected_left[o], r.detected_right[o]) == (len(f[0]), len(f[1])), (tag, o)


def assert_same_pairings(ctx, lane, feats, p, tag, r, floor=None):
    for o, (kl, kr, il, ir, l, rr, _, _) in enumerate(feats):
        m = S.match_lr_sad(l, rr, kl, kr, il, ir, p.sad_max_distance, p.max_y_diff, p.enable_robust_1to1_match, 0.0)
        if floor:
            assert len(m) >= floor[o], (tag, o, len(m))
        assert ctx.matches(lane, 0, o).tobytes() == m.tobytes(), (tag, "pairings", o, len(ctx.matches(lane, 0, o)), len(m))
        assert (ctx.matches_row_index(lane, 0, o) == S.matches_row_index(m, kl, l.shape[0])).all(), (tag, "row table of the pairings", o)
        assert r.stereo_matches[o] == len(m), (tag, o)


def test_reference_defaults_on_the_photograph(golden_dir):
    """the reference's out-of-the-box configuration: dmFASTER + smSAD, three octaves, grid NMS"""
    L, R = photograph(golden_dir)
    cam = StereoCamera.simple(500.0, 400.0, 300.0, 0.12, 800, 600)
    p = params(20, 500, 3)
    feats = F.faster_features(L, R, p, 4)
    ctx = hip.Context(n_lanes=1, max_w=800, max_h=600, max_kps=4096, max_cand=1 << 17, max_octaves=3)
    ctx.set_params(p); ctx.set_camera(cam)
    assert ctx.klt_win() == 4                                   # S2:47
    ctx.process_host([(L, R)])
    r = ctx.result(0)
    assert r.n_octaves == 3 and ctx.status_word(0) == 0 and r.status == 0
    assert_same_lists(ctx, 0, feats, "photograph", r)
    assert_same_pairings(ctx, 0, feats, p, "photograph", r, floor=(70, 70, 20))
    for o in (1, 2):
        for side in (0, 1):
            assert (ctx.level(0, side, o) == feats[o][4 + side]).all(), ("octave image", o, side)
    assert not r.valid and r.error_code == 4                    # voecFirstIteration
    ctx.close()


def test_no_nms_keeps_every_corner_in_raster_order(golden_dir):
    L, R = photograph(golden_dir)
    p = params(10, 500, 3, nms=0)
    feats = F.faster_features(L, R, p, 4)
    for o, f in enumerate(feats):
        assert len(f[0]) == f[6] and len(f[1]) == f[7] and max(f[6], f[7]) <= 4096 >> o, (o, f[6], f[7])       # every corner, and they fit the octave's slots
        yx = list(zip(f[0]["y"].tolist(), f[0]["x"].tolist()))
        assert yx == sorted(yx) and len(yx) >= (1800, 400, 100)[o]
    ctx = hip.Context(n_lanes=1, max_w=800, max_h=600, max_kps=4096, max_cand=1 << 17, max_octaves=3)
    ctx.set_params(p)
    ctx.process_host([(L, R)], hip.RUN_DETECT)
    assert ctx.status_word(0) == 0
    assert_same_lists(ctx, 0, feats, "no NMS", ctx.result(0))
    ctx.close()


def test_crop_sequence_in_place(golden_dir):
    """four 760 x 560 crops of the photograph read in place at stride 800: dmFASTER + smSAD + ifmSAD with match IDs"""
    L, R = photograph(golden_dir)
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = params(10, 1200, 1)
    p.vo_use_matches_ids = 1
    [(pl, pr)], buf, host = lay_out([(L, R)], "rows", 800, [(0, 0)], seed=5)
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=4096, max_cand=1 << 17)
    ctx.set_params(p); ctx.set_camera(cam)
    st = S.SadStream(O(), p, cam)
    for t, (x, y) in enumerate(S.CROPS):
        l, r = np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])
        feats = F.faster_features(l, r, p, 4)
        o = st.step((l, r), feats[0][0], feats[0][1], feats[0][2], feats[0][3])
        assert len(o["matches"]) >= 400 and (not t or (o["valid"] and len(o["tracked"]) >= 400)), (t, len(o["matches"]), len(o["tracked"]))
        ctx.process_device([(pl + y * 800 + x, pr + y * 800 + x)], w, h, 800)
        res = ctx.result(0)
        assert_same_lists(ctx, 0, feats, "crops t=%d" % t, res)
        assert_same_as_reference(ctx, 0, res, o, "crops t=%d" % t, ids=True)
    ctx.close()
    IC.assert_untouched(buf, host)


@pytest.mark.parametrize("win", [4, 1, 7, 15])
def test_partial_tiles_at_an_odd_stride(golden_dir, win):
    """251 x 187 at stride 259 and odd byte offsets, three octaves: partial tiles, the last valid column w-4 and row h-4, every
    halo width the response window can ask for"""
    (l, r), _ = geometry_crops(golden_dir)
    p = params(20, 500, 3)
    feats = F.faster_features(l, r, p, win)
    [(pl, pr)], buf, host = lay_out([(l, r)], "rows", 259, [(3, 7)], seed=11)
    ctx = hip.Context(n_lanes=1, max_w=251, max_h=187, max_kps=1024, max_cand=1 << 15, max_octaves=3)
    ctx.set_params(p); ctx.set_klt_win(win)
    ctx.process_device([(pl, pr)], 251, 187, 259, hip.RUN_DETECT | hip.RUN_MATCH)
    res = ctx.result(0)
    assert ctx.status_word(0) == 0 and res.n_octaves == 3
    assert_same_lists(ctx, 0, feats, "251x187 win %d" % win, res)
    assert_same_pairings(ctx, 0, feats, p, "251x187 win %d" % win, res)
    ctx.close()
    IC.assert_untouched(buf, host)


@pytest.mark.parametrize("nms", [1, 0])
def test_four_octaves_down_to_12x9(golden_dir, nms):
    """100 x 76 on four octaves: octave 3 is 12 x 9, its corners all fail the border rule of the response (nothing outside the image
    is read: the frame sits in poison)"""
    _, (l, r) = geometry_crops(golden_dir)
    p = params(10, 500, 4, nms=nms)
    feats = F.faster_features(l, r, p, 4)
    assert feats[3][4].shape == (9, 12) and feats[3][6] > 0 and (feats[3][0]["response"] == 0).all()
    [(pl, pr)], buf, host = lay_out([(l, r)], "rows", 100, [(1, 2)], seed=12)
    ctx = hip.Context(n_lanes=1, max_w=100, max_h=76, max_kps=1024, max_cand=1 << 14, max_octaves=4)
    ctx.set_params(p)
    ctx.process_device([(pl, pr)], 100, 76, 100, hip.RUN_DETECT | hip.RUN_MATCH)
    res = ctx.result(0)
    assert ctx.status_word(0) == 0 and res.n_octaves == 4
    assert_same_lists(ctx, 0, feats, "100x76 nms %d" % nms, res)
    assert_same_pairings(ctx, 0, feats, p, "100x76 nms %d" % nms, res)
    ctx.close()
    IC.assert_untouched(buf, host)


def test_tied_responses_through_the_nms():
    """`periodic`: 18470 corners, every response shared with another one -- the (response desc, raster position asc) order decides
    what the NMS keeps over nine chunks of the radix select.  (Detection only: the right image is an exact shift of a 64-periodic
    texture, whose SADs of zero tests/sad_ref.py cannot divide.)"""
    L = IC.periodic(320, 240, seed=1)
    R = IC.right_of(L, 6)
    p = params(20, 1000, 1)
    feats = F.faster_features(L, R, p, 4)
    assert feats[0][6] == 18470 and len(feats[0][0]) >= 1500
    ctx = hip.Context(n_lanes=1, max_w=320, max_h=240, max_kps=2048, max_cand=1 << 15)
    ctx.set_params(p)
    ctx.process_host([(L, R)], hip.RUN_DETECT)
    assert ctx.status_word(0) == 0
    assert_same_lists(ctx, 0, feats, "periodic", ctx.result(0))
    ctx.close()
    # the same frame with a candidate list too short for it: status bit 1, no fault; nothing else is promised about the lists
    ctx = hip.Context(n_lanes=1, max_w=320, max_h=240, max_kps=2048, max_cand=1 << 13)
    ctx.set_params(p)
    ctx.process_host([(L, R)], hip.RUN_DETECT)
    assert ctx.status_word(0) & ST_CAND_OVERFLOW and ctx.result(0).status & ST_CAND_OVERFLOW
    ctx.close()


def test_tied_responses_without_nms_fill_the_list():
    """NMS off on the same frame: 18470 corners against the 16384 slots of the largest context.  What stays is the head of the
    (response desc, raster position asc) order -- the ties at the cut decided by position --, in raster order, with status bit 2"""
    L = IC.periodic(320, 240, seed=1)
    R = IC.right_of(L, 6)
    p = params(20, 1000, 1, nms=0)
    ctx = hip.Context(n_lanes=1, max_w=320, max_h=240, max_kps=16384, max_cand=1 << 15)
    ctx.set_params(p)
    ctx.process_host([(L, R)], hip.RUN_DETECT)
    assert ctx.status_word(0) == ST_KPS_OVERFLOW
    for side, img in enumerate((L, R)):
        raw = F.corners(img, 20, 4)
        key = (raw["response"].view(np.uint32).astype(np.uint64) | np.uint64(0x80000000)) << np.uint64(32) | (np.uint64(0xFFFFFFFF) - np.arange(len(raw), dtype=np.uint64))
        assert (raw["response"] >= 0).all() and len(raw) > 16384
        head = np.sort(np.argsort(key)[::-1][:16384])           # the 16384 largest keys, back in raster order
        k, d = ctx.keypoints(0, 0, side)
        assert len(k) == 16384 and k.tobytes() == raw[head].tobytes() and not d.any(), side
    ctx.close()


@pytest.mark.parametrize("t", [19, 20, 21])
def test_scores_on_the_threshold(t):
    """`threshold_edge`: circle pixels exactly 20 and 21 away from the centre -- the comparisons are strict.  At 21 nothing is a
    corner and the frames complete with voecFirstIteration, then with the bad-tracking code, as the composed reference says.  (At
    19 and 20 detection only: the blocks repeat, and tests/sad_ref.py cannot divide their SADs of zero.)"""
    te = IC.threshold_edge(320, 240, seed=1, th=20)
    frames = [(te, IC.right_of(te, 6)), (IC.moved(te, 3, 2), IC.right_of(IC.moved(te, 3, 2), 6))]
    cam = StereoCamera.simple(300.0, 160.0, 120.0, 0.12, 320, 240)
    p = params(t, 500, 1)
    ctx = hip.Context(n_lanes=1, max_w=320, max_h=240, max_kps=1024, max_cand=1 << 14)
    ctx.set_params(p); ctx.set_camera(cam)
    st = S.SadStream(O(), p, cam)
    for i, (l, r) in enumerate(frames):
        feats = F.faster_features(l, r, p, 4)
        assert (feats[0][6] == 0) == (t == 21) and (t == 21 or len(feats[0][0]) >= 100)
        ctx.process_host([(l, r)], hip.RUN_ALL if t == 21 else hip.RUN_DETECT)
        res = ctx.result(0)
        assert ctx.status_word(0) == 0
        assert_same_lists(ctx, 0, feats, "threshold_edge %d frame %d" % (t, i), res)
        if t == 21:
            o = st.step((l, r), feats[0][0], feats[0][1], feats[0][2], feats[0][3])
            assert not o["valid"] and len(o["tracked"]) < p.bad_tracking_th
            assert_same_as_reference(ctx, 0, res, o, "threshold_edge 21 frame %d" % i)
            assert res.error_code == (4 if i == 0 else 5), (i, res.error_code)       # voecFirstIteration, then voecBadTracking (P:326-341)
    ctx.close()


def test_checker_has_no_corners_on_any_octave():
    L = IC.checker(320, 240, seed=CHECKER_SEED)
    p = params(20, 500, 3)
    ctx = hip.Context(n_lanes=1, max_w=320, max_h=240, max_kps=1024, max_cand=1 << 14, max_octaves=3)
    ctx.set_params(p)
    ctx.process_host([(L, IC.right_of(L, 6))], hip.RUN_DETECT | hip.RUN_MATCH)
    r = ctx.result(0)
    assert ctx.status_word(0) == 0 and r.n_octaves == 3
    for o in range(3):
        for side in (0, 1):
            assert len(ctx.keypoints(0, 0, side, o)[0]) == 0 and not ctx.row_index(0, 0, side, o).any()
        assert len(ctx.matches(0, 0, o)) == 0 and (r.detected_left[o], r.detected_right[o], r.stereo_matches[o]) == (0, 0, 0)
    ctx.close()


def snapshot(ctx, lane, r, n_oct):
    """everything a frame leaves behind for one lane, every octave: (the lists and integers, the pose, the residuals)"""
    exact = []
    for o in range(n_oct):
        exact += [ctx.keypoints(lane, 0, 0, o)[0].tobytes(), ctx.keypoints(lane, 0, 1, o)[0].tobytes(), ctx.matches(lane, 0, o).tobytes(),
                  ctx.matches_row_index(lane, 0, o).tobytes(), ctx.tracked(lane, o).tobytes()]
    exact += [tuple(r.track_stats), r.valid, r.error_code, r.n_residual, r.n_outliers, ctx.outliers(lane).tobytes(), ctx.status_word(lane)]
    return tuple(exact), np.array(r.outPose), ctx.residuals(lane)


def test_several_lanes_batch_and_graphs():
    """four lanes on four moving synthetic streams, two octaves, KLT_win 5: every lane equals a one-lane context, lane 0's lists the
    reference; StreamBatch (two contexts, detect-ahead) and a graph-replaying context give the same snapshots"""
    import torch
    from stereo_vo_amd.pipeline import StreamBatch
    w, h, B, T, NO, WIN = 640, 480, 4, 3, 2, 5
    streams = [make_frames("world", w, h, T, seed=40 + g) for g in range(B)]
    cam = StereoCamera.simple(400.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = params(20, 800, NO, sad=800, ifm_sad=800)
    p.ifm_win_w = p.ifm_win_h = 24
    kw = dict(max_w=w, max_h=h, max_kps=2048, max_cand=1 << 16, max_octaves=NO)
    single = []
    for g in range(B):
        ctx = hip.Context(n_lanes=1, **kw)
        ctx.set_params(p); ctx.set_camera(cam); ctx.set_klt_win(WIN)
        snaps = []
        for t in range(T):
            ctx.process_host([streams[g][t]])
            r = ctx.result(0)
            if g == 0:
                feats = F.faster_features(streams[g][t][0], streams[g][t][1], p, WIN)
                assert min(len(f[0]) for f in feats) >= 100, [len(f[0]) for f in feats]
                assert_same_lists(ctx, 0, feats, "world lane 0 t=%d" % t, r)
                assert_same_pairings(ctx, 0, feats, p, "world lane 0 t=%d" % t, r, floor=(50, 20))
                if t:
                    assert r.tracked_feats_from_last_frame >= 30, (t, r.tracked_feats_from_last_frame)
            snaps.append(snapshot(ctx, 0, r, NO))
        ctx.close()
        single.append(snaps)
    ctx = hip.Context(n_lanes=B, **kw)
    ctx.set_params(p); ctx.set_camera(cam); ctx.set_klt_win(WIN)
    for t in range(T):
        ctx.process_host([streams[g][t] for g in range(B)])
        res = ctx.results()
        for g in range(B):
            assert_same_snapshot(snapshot(ctx, g, res[g], NO), single[g][t], ("four lanes", g, t))
    ctx.close()
    batch = StreamBatch(p, cam, w, h, B, 2, max_kps=2048, max_cand=1 << 16, max_octaves=NO)
    batch.set_klt_win(WIN)
    assert [c.klt_win() for c in batch.ctxs] == [WIN, WIN]
    steps = [lay_out([s[t] for s in streams], "rows", w, [(0, 0)] * B, seed=t) for t in range(T)]
    for t, (ptrs, buf, host) in enumerate(steps):
        batch.step(ptrs)
        batch.synchronize()
        res = batch.results()
        for g in range(B):
            c, lane = batch.lane(g)
            assert_same_snapshot(snapshot(c, lane, res[g], NO), single[g][t], ("batch", g, t))
    batch.close()
    ctx = hip.Context(n_lanes=1, **kw)
    ctx.set_params(p); ctx.set_camera(cam); ctx.set_klt_win(WIN)
    ctx.use_graphs(True)
    for rep in range(2):                                       # the second pass replays the graphs the first one captured
        ctx.reset()
        for t in range(T):
            ctx.process_host([streams[1][t]])
            assert_same_snapshot(snapshot(ctx, 0, ctx.result(0), NO), single[1][t], ("graphs", rep, t))
    ctx.close()
    torch.cuda.synchronize()


def test_more_than_8192_corners_in_a_16384_entry_context():
    L, R = big_list_frame()
    p = params(BIG_T, 1000, 1, nms=0)
    feats = F.faster_features(L, R, p, 4)
    assert all(8192 < n <= 16384 for n in (feats[0][6], feats[0][7])) and len(feats[0][0]) == feats[0][6]
    ctx = hip.Context(n_lanes=1, max_w=640, max_h=480, max_kps=16384, max_cand=1 << 15)
    ctx.set_params(p)
    ctx.process_host([(L, R)], hip.RUN_DETECT)
    assert ctx.status_word(0) == 0
    assert_same_lists(ctx, 0, feats, "16384-entry lists", ctx.result(0))
    ctx.close()


def small_seq(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    return g, W, H, StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)


def test_refusals_and_the_context_value(golden_dir):
    g, W, H, cam = small_seq(golden_dir)
    base = params(20, 300, 1)
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(base); ctx.set_camera(cam)
    # KLT_win: default 4; 0, 16 and negatives are refused and the value in force stays
    assert ctx.klt_win() == 4
    ctx.set_klt_win(7)
    for bad in (0, 16, -1):
        assert ctx.L.svo_set_klt_win(ctx.h, bad) == SVO_ERR_ARG and b"KLT_win" in ctx.L.svo_last_error(ctx.h)
        assert ctx.klt_win() == 7
    ctx.set_klt_win(4)
    ctx.process_host([(g["L0"], g["R0"])])
    feats = F.faster_features(g["L0"], g["R0"], base, 4)
    assert len(feats[0][0]) >= 100
    assert_same_lists(ctx, 0, feats, "before the refusals", ctx.result(0))
    before = (ctx.keypoints(0, 0, 0)[0].tobytes(), ctx.keypoints(0, 0, 1)[0].tobytes(), ctx.matches(0).tobytes())
    assert len(ctx.matches(0)) >= 20
    fr = (hip.Frame * 1)()
    fr[0].left = hip.Image(g["L1"].ctypes.data, W, H, W); fr[0].right = hip.Image(g["R1"].ctypes.data, W, H, W)

    def refused(change, rc_want, text):
        q = base.copy()
        for k, v in change.items():
            setattr(q, k, v)
        ctx.set_params(q)
        rc = ctx.L.svo_process(ctx.h, fr, hip.RUN_ALL)
        assert rc == rc_want and text in ctx.L.svo_last_error(ctx.h), (change, rc, ctx.L.svo_last_error(ctx.h))
        assert (ctx.keypoints(0, 0, 0)[0].tobytes(), ctx.keypoints(0, 0, 1)[0].tobytes(), ctx.matches(0).tobytes()) == before, change

    refused({"match_method": 0}, SVO_ERR_STATE, b"dmFASTER computes no descriptors")
    refused({"match_method": 1}, SVO_ERR_STATE, b"dmFASTER computes no descriptors")
    refused({"ifm_method": 0}, SVO_ERR_STATE, b"dmFASTER computes no descriptors")
    refused({"ifm_method": 1}, SVO_ERR_STATE, b"dmFASTER computes no descriptors")
    refused({"nmsMethod": 1}, SVO_ERR_UNSUPPORTED, b"adaptive NMS")
    refused({"initial_FAST_threshold": 256}, SVO_ERR_ARG, b"initial_FAST_threshold")
    refused({"initial_FAST_threshold": -1}, SVO_ERR_ARG, b"initial_FAST_threshold")
    refused({"detect_method": DM_KLT}, SVO_ERR_UNSUPPORTED, b"")
    refused({"ifm_method": 3}, SVO_ERR_UNSUPPORTED, b"")
    # the dynamic FAST threshold of the ORB paths has no part in dmFASTER: m_threshold stays initial_FAST_threshold
    ctx.set_params(base)
    ctx.set_fast_threshold(5)
    assert ctx.fast_threshold() == 5
    ctx.reset()
    ctx.process_host([(g["L0"], g["R0"])])
    assert (ctx.keypoints(0, 0, 0)[0].tobytes(), ctx.keypoints(0, 0, 1)[0].tobytes(), ctx.matches(0).tobytes()) == before
    ctx.close()


def test_no_cost_without_dmfaster(golden_dir):
    """a context on ORB or FAST+ORB launches none of the new kernels and exactly the detector kernels it launched before; a dmFASTER
    context launches neither fast, select nor describe, and each new kernel once per frame"""
    g, W, H, cam = small_seq(golden_dir)
    for method in (0, DM_FAST_ORB, DM_FASTER):
        p = params(20, 300, 1) if method == DM_FASTER else hip.default_params()
        p.detect_method, p.nOctaves = method, 1
        ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam)
        for t in range(3):
            ctx.process_host([(g["L%d" % t], g["R%d" % t])])
        kt = ctx.kernel_times()
        new = [kt[k][1] for k in NEW_KERNELS]
        old = [kt[k][1] for k in ("fast", "select", "describe")]
        if method == DM_FASTER:
            assert new == [3, 3] and old == [0, 0, 0], (new, old)
            assert kt["sad_patch"][1] == kt["match_lr_sad"][1] == kt["track_sad"][1] == 3
        else:
            assert new == [0, 0] and old == [3, 3, 3], (method, new, old)
        assert list(kt)[-2:] == list(NEW_KERNELS)                # appended: the earlier names keep their places
        ctx.close()
