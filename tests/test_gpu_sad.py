"""smSAD and ifmSAD on the HIP path against the reference walks of tests/sad_ref.py (the CPU oracle refuses these selectors).

Integers and lists are compared exactly; pose and residual tolerances are those of test_gpu_parity.assert_same_frame.  Every case
first asserts, from the reference alone, that there is something to compare."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, DM_FAST_ORB

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_content as IC                                      # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_gpu_parity import O, POSE_TOL_M, POSE_TOL_RAD         # noqa: E402
from test_gpu_frame_layouts import lay_out, make_frames         # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_UNSUPPORTED, SVO_ERR_STATE = -3, -6
NEW_KERNELS = ("sad_patch", "match_lr_sad", "track_sad")


def photograph(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_pair_800x600.npz"))
    return g["left"], g["right"]


def assert_same_features(ctx, lane, feats, tag, octave=0):
    """keypoints, descriptors and row tables equal the oracle's: detection does not depend on the selectors"""
    kl, dl, kr, dr, il, ir = feats
    for side, (ko, do, io) in enumerate(((kl, dl, il), (kr, dr, ir))):
        k, d = ctx.keypoints(lane, 0, side, octave)
        assert len(k) == len(ko) and k.tobytes() == ko.tobytes(), (tag, "keypoints", side, len(k), len(ko))
        assert (d == do).all(), (tag, "descriptors", side)
        assert (ctx.row_index(lane, 0, side, octave) == io).all(), (tag, "row table", side)


def assert_same_as_reference(ctx, lane, r, o, tag, ids=False):
    """one frame of one lane against SadStream.step's record"""
    assert ctx.matches(lane).tobytes() == o["matches"].tobytes(), (tag, "pairings", len(ctx.matches(lane)), len(o["matches"]))
    assert (ctx.matches_row_index(lane, 0) == o["mri"]).all(), (tag, "row table of the pairings")
    assert r.stereo_matches[0] == len(o["matches"]), tag
    assert ctx.tracked(lane).tobytes() == o["tracked"].tobytes(), (tag, "tracked pairs", len(ctx.tracked(lane)), len(o["tracked"]))
    assert list(r.track_stats) == list(o["stats"]), (tag, "stage-4 counters", list(r.track_stats), list(o["stats"]))
    assert r.tracked_feats_from_last_frame == len(o["tracked"]), tag
    assert bool(r.valid) == bool(o["valid"]), (tag, r.valid, r.error_code)
    if ids:
        assert (ctx.match_ids(lane, 0) == o["ids"]).all(), (tag, "match IDs")
    if o["valid"]:
        ro = o["result"]
        assert (r.error_code, r.n_residual, r.n_outliers) == (ro.error_code, ro.n_residual, ro.n_outliers), tag
        dp = np.abs(np.array(r.outPose) - np.array(ro.outPose))
        assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (tag, dp)
        assert (ctx.outliers(lane) == o["inliers"]).all(), (tag, "inlier list")
        a, b = ctx.residuals(lane), o["residuals"]
        fin = b < 1e300
        assert ((a < 1e300) == fin).all() and np.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-9), (tag, "residuals")
    assert ctx.status_word(lane) == 0, (tag, ctx.status_word(lane))


@pytest.mark.parametrize("sad,one,floor", [(400, 1, 200), (400, 0, 200), (0, 1, 40)])
def test_photograph_full_frame_smsad(golden_dir, sad, one, floor):
    """match_method = 2 on the reference's own stereo pair: at threshold 400 with both assignment rules, and with the field left at 0
    (the reference's default 200)"""
    L, R = photograph(golden_dir)
    cam = StereoCamera.simple(500.0, 400.0, 300.0, 0.12, 800, 600)
    p = S.photo_params(hip.default_params(), sad_max_distance=sad, one_to_one=one)
    feats = S.oracle_features(O(), p, L, R, cam)
    o = S.SadStream(O(), p, cam).step((L, R), feats[0], feats[2], feats[4], feats[5], feats[1], feats[3])
    assert len(o["matches"]) >= floor, len(o["matches"])
    ctx = hip.Context(n_lanes=1, max_w=800, max_h=600, max_kps=4096, max_cand=1 << 17)
    ctx.set_params(p); ctx.set_camera(cam)
    ctx.process_host([(L, R)])
    r = ctx.result(0)
    tag = "photograph smSAD %d 1to1 %d" % (sad, one)
    assert_same_features(ctx, 0, feats, tag)
    assert_same_as_reference(ctx, 0, r, o, tag)
    assert (ctx.matches(0)["imgIdx"] == -1).all()
    ctx.close()


@pytest.mark.parametrize("mm,ifm,th,ids", [(2, 2, 200, 0), (2, 2, 400, 1), (1, 2, 400, 0), (2, 0, 0, 0)])
def test_crop_sequence_in_place(golden_dir, mm, ifm, th, ids):
    """four 760x560 crops of the photograph read in place at stride 800 as a moving sequence: smSAD + ifmSAD at both tracker
    thresholds (once with match IDs), the row-by-row Hamming matcher under ifmSAD, and smSAD under the brute-force tracker"""
    L, R = photograph(golden_dir)
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = S.photo_params(hip.default_params(), ifm_sad_max_distance=th, match_method=mm, ifm_method=ifm)
    p.vo_use_matches_ids = ids
    [(pl, pr)], buf, host = lay_out([(L, R)], "rows", 800, [(0, 0)], seed=5)
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=4096, max_cand=1 << 17)
    ctx.set_params(p); ctx.set_camera(cam)
    st = S.SadStream(O(), p, cam)
    for t, (x, y) in enumerate(S.CROPS):
        l, r = np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])
        feats = S.oracle_features(O(), p, l, r, cam)
        o = st.step((l, r), feats[0], feats[2], feats[4], feats[5], feats[1], feats[3], ctx.orb_threshold())
        if t and ifm == 2:
            assert len(o["candidates"]) >= 50, (t, len(o["candidates"]))
        if t:
            assert o["valid"] and len(o["tracked"]) >= 50, (t, o["valid"], len(o["tracked"]))
        ctx.process_device([(pl + y * 800 + x, pr + y * 800 + x)], w, h, 800)
        tag = "crops match %d ifm %d th %d t=%d" % (mm, ifm, th, t)
        assert_same_features(ctx, 0, feats, tag)
        assert_same_as_reference(ctx, 0, ctx.result(0), o, tag, ids=bool(ids))
    ctx.close()
    IC.assert_untouched(buf, host)


def test_fast_orb_two_octaves_smsad(golden_dir):
    """FAST+ORB keeps one list per x1/2 octave: the windows come from each octave's own image"""
    L, R = photograph(golden_dir)
    cam = StereoCamera.simple(500.0, 400.0, 300.0, 0.12, 800, 600)
    p = S.photo_params(hip.default_params(), orb_nfeats=600, ifm_method=1)
    p.detect_method = DM_FAST_ORB; p.nOctaves = 2
    q = p.copy(); q.match_method = 1
    orc = O().Oracle(q)
    orc.process(L, R, cam)
    ctx = hip.Context(n_lanes=1, max_w=800, max_h=600, max_kps=4096, max_cand=1 << 17, max_octaves=2)
    ctx.set_params(p); ctx.set_camera(cam)
    ctx.process_host([(L, R)])
    r = ctx.result(0)
    assert r.n_octaves == 2 and ctx.status_word(0) == 0
    for oc in range(2):
        feats = orc.keypoints(0, 0, oc) + orc.keypoints(0, 1, oc) + (orc.row_index(0, 0, oc), orc.row_index(0, 1, oc))
        assert_same_features(ctx, 0, feats, "fast+orb octave %d" % oc, octave=oc)
        imgs = ctx.level(0, 0, oc), ctx.level(0, 1, oc)
        assert imgs[0].shape == (600 >> oc, 800 >> oc)
        if oc == 0:
            assert (imgs[0] == L).all() and (imgs[1] == R).all()
        m = S.match_lr_sad(imgs[0], imgs[1], feats[0], feats[2], feats[4], feats[5], p.sad_max_distance, p.max_y_diff, p.enable_robust_1to1_match, 0.0)
        assert len(m) >= 30, (oc, len(m))
        assert ctx.matches(0, 0, oc).tobytes() == m.tobytes(), ("fast+orb pairings", oc, len(ctx.matches(0, 0, oc)), len(m))
        assert (ctx.matches_row_index(0, 0, oc) == S.matches_row_index(m, feats[0], 600 >> oc)).all(), oc
        assert r.stereo_matches[oc] == len(m)
    ctx.close()


def snapshot(ctx, lane, r):
    """everything a frame leaves behind for one lane: (the lists and integers, the pose, the residuals)"""
    exact = (ctx.keypoints(lane, 0, 0)[0].tobytes(), ctx.keypoints(lane, 0, 1)[0].tobytes(), ctx.matches(lane).tobytes(),
             ctx.matches_row_index(lane, 0).tobytes(), ctx.tracked(lane).tobytes(), tuple(r.track_stats), r.valid, r.error_code,
             r.n_residual, r.n_outliers, ctx.outliers(lane).tobytes(), ctx.status_word(lane))
    return exact, np.array(r.outPose), ctx.residuals(lane)


def assert_same_snapshot(a, b, tag):
    assert a[0] == b[0], (tag, [i for i, (x, y) in enumerate(zip(a[0], b[0])) if x != y])
    dp = np.abs(a[1] - b[1])
    assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (tag, dp)
    fin = b[2] < 1e300
    assert ((a[2] < 1e300) == fin).all() and np.allclose(a[2][fin], b[2][fin], rtol=1e-6, atol=1e-9), (tag, "residuals")


def test_several_lanes_batch_and_graphs():
    """four lanes of one context on four moving synthetic streams: every lane equals a one-lane context fed the same frames, lane 0
    equals the composed reference; the same streams through StreamBatch (two contexts, the detect-ahead schedule) and one of
    them through a graph-replaying context give the same lists"""
    import torch
    from stereo_vo_amd.pipeline import StreamBatch
    w, h, B, T = 640, 480, 4, 3
    streams = [make_frames("world", w, h, T, seed=40 + g) for g in range(B)]
    cam = StereoCamera.simple(400.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = S.photo_params(hip.default_params(), orb_nfeats=800, sad_max_distance=800, ifm_sad_max_distance=800)       # (SADs above 255 in play)
    p.ifm_win_w = p.ifm_win_h = 24
    # one-lane contexts: the record every other schedule must reproduce; lane 0 against the composed reference
    single = []
    for g in range(B):
        ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 16)
        ctx.set_params(p); ctx.set_camera(cam)
        st = S.SadStream(O(), p, cam) if g == 0 else None
        snaps = []
        for t in range(T):
            ctx.process_host([streams[g][t]])
            r = ctx.result(0)
            if st:
                l, rr = streams[g][t]
                feats = S.oracle_features(O(), p, l, rr, cam)
                o = st.step((l, rr), feats[0], feats[2], feats[4], feats[5], feats[1], feats[3], ctx.orb_threshold())
                assert len(o["matches"]) >= 100, (t, len(o["matches"]))
                if t:
                    assert len(o["candidates"]) >= 50 and o["valid"], (t, len(o["candidates"]), o["valid"])
                assert_same_features(ctx, 0, feats, "world lane 0 t=%d" % t)
                assert_same_as_reference(ctx, 0, r, o, "world lane 0 t=%d" % t)
            snaps.append(snapshot(ctx, 0, r))
        ctx.close()
        single.append(snaps)
    ctx = hip.Context(n_lanes=B, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 16)
    ctx.set_params(p); ctx.set_camera(cam)
    for t in range(T):
        ctx.process_host([streams[g][t] for g in range(B)])
        res = ctx.results()
        for g in range(B):
            assert_same_snapshot(snapshot(ctx, g, res[g]), single[g][t], ("four lanes", g, t))
    ctx.close()
    # the batched schedule: two contexts of two lanes, detect ahead of the stages 3-5 of the frame before
    batch = StreamBatch(p, cam, w, h, B, 2, max_kps=2048, max_cand=1 << 16)
    steps = [lay_out([s[t] for s in streams], "rows", w, [(0, 0)] * B, seed=t) for t in range(T)]
    for t, (ptrs, buf, host) in enumerate(steps):
        batch.step(ptrs)
        batch.synchronize()
        res = batch.results()
        for g in range(B):
            c, lane = batch.lane(g)
            assert_same_snapshot(snapshot(c, lane, res[g]), single[g][t], ("batch", g, t))
    batch.close()
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 16)
    ctx.set_params(p); ctx.set_camera(cam)
    ctx.use_graphs(True)
    for rep in range(2):                                       # the second pass replays the graphs the first one captured
        ctx.reset()
        for t in range(T):
            ctx.process_host([streams[1][t]])
            assert_same_snapshot(snapshot(ctx, 0, ctx.result(0)), single[1][t], ("graphs", rep, t))
    ctx.close()
    torch.cuda.synchronize()


def test_refusals(golden_dir):
    """a SAD stage on a frame whose windows were never gathered is SVO_ERR_STATE with a text, before anything is enqueued; optical
    flow stays unsupported"""
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)
    base = S.photo_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]), match_method=1, ifm_method=1)
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(base); ctx.set_camera(cam)
    ctx.process_host([(g["L0"], g["R0"])])
    kl, dl = ctx.keypoints(0, 0, 0); kr, dr = ctx.keypoints(0, 0, 1)
    # caller features carry no image: smSAD on them is refused
    sad = base.copy(); sad.match_method = 2
    ctx.reset(); ctx.set_params(sad)
    ctx.put_features(0, 0, 0, kl, dl, W, H); ctx.put_features(0, 0, 1, kr, dr, W, H)
    rc = ctx.L.svo_process(ctx.h, None, hip.RUN_MATCH | hip.FLAG_NO_SHIFT)
    assert rc == SVO_ERR_STATE and b"never gathered" in ctx.L.svo_last_error(ctx.h), (rc, ctx.L.svo_last_error(ctx.h))
    # a stream that switches to ifmSAD: the frame after a non-SAD one is refused, nothing is enqueued, the next one goes through
    ctx.reset(); ctx.set_params(base)
    ctx.process_host([(g["L0"], g["R0"])])
    before = ctx.matches(0).tobytes()
    trk = base.copy(); trk.ifm_method = 2; trk.ifm_sad_max_distance = -1          # (negative: no threshold)
    st = S.SadStream(O(), trk, cam)
    ctx.set_params(trk)
    fr = (hip.Frame * 1)()
    fr[0].left = hip.Image(g["L1"].ctypes.data, W, H, W); fr[0].right = hip.Image(g["R1"].ctypes.data, W, H, W)
    rc = ctx.L.svo_process(ctx.h, fr, hip.RUN_ALL)
    assert rc == SVO_ERR_STATE and b"previous frame" in ctx.L.svo_last_error(ctx.h), (rc, ctx.L.svo_last_error(ctx.h))
    assert ctx.matches(0).tobytes() == before                   # the refused call left the lists alone
    for t in (1, 2):                                            # frame 1 starts the lane's track afresh, frame 2 is tracked with ifmSAD
        ctx.process_host([(g["L%d" % t], g["R%d" % t])])
        r = ctx.result(0)
        feats = S.oracle_features(O(), trk, g["L%d" % t], g["R%d" % t], cam)
        o = st.step((g["L%d" % t], g["R%d" % t]), feats[0], feats[2], feats[4], feats[5], feats[1], feats[3], ctx.orb_threshold())
        assert_same_as_reference(ctx, 0, r, o, "after the refusal, t=%d" % t)
        if t == 1:
            assert not r.valid and r.error_code == 4 and len(o["matches"]) > 50          # voecFirstIteration
        else:
            assert len(o["candidates"]) >= 50 and o["valid"], (len(o["candidates"]), o["valid"])
    # optical flow: still outside the hot path
    flow = base.copy(); flow.ifm_method = 3
    ctx.set_params(flow)
    assert ctx.L.svo_process(ctx.h, fr, hip.RUN_ALL) == SVO_ERR_UNSUPPORTED
    ctx.close()


def test_no_cost_without_sad(golden_dir):
    """a context that never selects SAD launches none of the new kernels; one that does launches each once per frame"""
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)
    for sad in (False, True):
        p = hip.default_params()
        if sad:
            p.match_method, p.ifm_method, p.max_y_diff = 2, 2, 2.0
        ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam)
        for t in range(3):
            ctx.process_host([(g["L%d" % t], g["R%d" % t])])
        kt = ctx.kernel_times()
        assert [kt[k][1] for k in NEW_KERNELS] == ([3, 3, 3] if sad else [0, 0, 0]), {k: kt[k] for k in NEW_KERNELS}
        assert kt["fast"][1] == 3
        ctx.close()
