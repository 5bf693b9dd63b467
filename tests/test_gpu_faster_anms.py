"""The adaptive NMS under dmFASTER on the HIP path (svo_set_faster_adaptive_nms, svo_adaptive_nms), lists bit for bit.

Scenes: every hand-built list of tests/anms_scenes.py through Context.adaptive_nms against oracle.anms_copy.  Images and sequences:
dmFASTER + nmsmAdaptive against tests/faster_anms_ref.py (faster_ref with the oracle's adaptive NMS in place of the grid NMS), every
record field, row table and descriptor row through test_gpu_faster.assert_same_lists; pairings, tracks and poses downstream as every
dmFASTER test holds them (test_gpu_sad.assert_same_as_reference).  tests/test_anms_scenes_cpu.py and tests/test_faster_anms_cpu.py
pin, without a GPU, that each input reaches its case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, DM_FAST_ORB

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anms_scenes as A                                         # noqa: E402
import faster_anms_ref as R                                     # noqa: E402
import faster_dyn_ref as D                                      # noqa: E402
import faster_ref as F                                          # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_faster_anms_cpu import NOISE_T, PHOTO_NFEATS, PHOTO_OCT, PHOTO_T, TILED_T, noise_frame, tiled_frame      # noqa: E402
from test_faster_cpu import photograph                          # noqa: E402
from test_gpu_faster import assert_same_lists, assert_same_pairings, snapshot       # noqa: E402
from test_gpu_frame_layouts import lay_out, make_frames         # noqa: E402
from test_gpu_parity import O                                   # noqa: E402
from test_gpu_sad import assert_same_as_reference, assert_same_snapshot             # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_UNSUPPORTED = -2, -3
ST_CAND_OVERFLOW = 1
OLD_TEXT = b"the adaptive NMS is not built for dmFASTER: use nmsMethod = nmsmStandard"
W, H = 320, 240
CAM = StereoCamera.simple(300.0, W / 2.0, H / 2.0, 0.12, W, H)
KW = dict(max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15)
REST = hip.RUN_MATCH | hip.RUN_TRACK | hip.RUN_OPTIMIZE
AHEAD = 4096


def params(t=20, orb_nfeats=500, n_oct=1, **kw):
    return R.params(hip.default_params(), t, orb_nfeats, n_oct, **kw)


def context(p, n_lanes=1, cam=CAM, **kw):
    ctx = hip.Context(n_lanes=n_lanes, **dict(KW, **kw))
    ctx.set_params(p); ctx.set_camera(cam)
    ctx.set_faster_adaptive_nms(True)
    return ctx


# ---- the kernel on hand-built lists ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def list_ctx():
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=4096, max_cand=1 << 15)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("letter", sorted(A.SCENES))
def test_scene(list_ctx, letter):
    assert not list_ctx.faster_adaptive_nms()                   # the stand-in needs no opt-in
    for i, (name, k, num, w, h) in enumerate(A.cases(letter)):
        want = A.expected(letter, i)
        n, got = list_ctx.adaptive_nms(k, num, w, h)
        assert n == len(want) == min(num, len(k)), (name, n, len(want))
        assert np.array_equal(got, want), (name, int((got != want).argmax()), got[:8], want[:8])


def test_stand_in_capacity_and_refusals(list_ctx):
    ctx, L = list_ctx, list_ctx.L
    name, k, num, w, h = A.cases("f")[3]
    want = A.expected("f", 3)
    n, got = ctx.adaptive_nms(k, num, w, h, cap=10)             # more kept than the caller has room for: the count, and the first cap indices
    assert n == len(want) > 10 and np.array_equal(got, want[:10])
    assert ctx.adaptive_nms(k, num, w, h, cap=0)[0] == len(want)
    out = np.zeros(len(k), np.int32)

    def refused(kps, num_out, iw, ih, text, n=None):
        rc = L.svo_adaptive_nms(ctx.h, kps.ctypes.data if kps is not None else None, len(kps) if n is None else n, num_out, iw, ih, out.ctypes.data, len(out))
        assert rc == SVO_ERR_ARG and text in L.svo_last_error(ctx.h), (text, rc, L.svo_last_error(ctx.h))

    def changed(i, field, v):
        q = k.copy(); q[field][i] = v
        return q

    refused(changed(5, "x", k["x"][5] + 0.5), num, w, h, b"integer coordinates")
    refused(changed(5, "x", -1.0), num, w, h, b"integer coordinates")
    refused(changed(5, "y", float(h)), num, w, h, b"integer coordinates")
    refused(changed(5, "response", np.nan), num, w, h, b"NaN")
    refused(np.ascontiguousarray(k[::-1]), num, w, h, b"ascending raster order")
    refused(np.ascontiguousarray(k[[0, 1, 1, 2]]), num, w, h, b"ascending raster order")
    refused(k, num, 4096, 4096, b"2^24")
    refused(k, num, 0, h, b"2^24")
    refused(None, num, w, h, b"kps", n=3)
    refused(k, num, w, h, b"kps", n=-1)
    big = A.make(np.arange(40000) % 256, np.arange(40000) // 256, np.ones(40000))
    refused(big, 10, 256, 256, b"candidate capacity")           # n above max(1024, max_cand) = 32768
    name, kh, _, wh, hh = A.cases("h")[0]
    refused(kh, 5000, wh, hh, b"max_kps")                       # min(num_out_points, n) above the 4096 keys the selection sorts
    assert L.svo_adaptive_nms(ctx.h, k.ctypes.data, len(k), num, w, h, None, 5) == SVO_ERR_ARG and b"out_order" in L.svo_last_error(ctx.h)
    n, got = ctx.adaptive_nms(k, num, w, h)                     # ... and the context still works
    assert np.array_equal(got, want)


# ---- images ----------------------------------------------------------------------------------------------------------------

def test_photograph_three_octaves(golden_dir):
    """800 x 600, t = 10, 500 features over three octaves, smSAD pairings: level 0 has 2294 corners of which ~428 stay -- and the grid
    NMS would keep other ones (test_faster_anms_cpu)"""
    L, Rt = photograph(golden_dir)
    p = params(PHOTO_T, PHOTO_NFEATS, PHOTO_OCT)
    feats = R.features(L, Rt, p, 4)
    assert feats[0][6] >= 2000 and len(feats[0][0]) == F.kps_to_detect(PHOTO_NFEATS, PHOTO_OCT)[0]
    ctx = context(p, cam=StereoCamera.simple(500.0, 400.0, 300.0, 0.12, 800, 600), max_w=800, max_h=600, max_kps=4096, max_cand=1 << 17, max_octaves=3)
    ctx.process_host([(L, Rt)])
    r = ctx.result(0)
    assert r.n_octaves == 3 and ctx.status_word(0) == 0 and r.status == 0
    assert_same_lists(ctx, 0, feats, "photograph", r)
    assert_same_pairings(ctx, 0, feats, p, "photograph", r, floor=(50, 30, 10))
    grid = F.faster_features(L, Rt, F.faster_params(hip.default_params(), PHOTO_T, PHOTO_NFEATS, PHOTO_OCT), 4)
    assert ctx.keypoints(0, 0, 0, 0)[0].tobytes() != grid[0][0].tobytes()
    ctx.close()


@pytest.mark.parametrize("content", ["noise", "tiled"])
def test_dense_frames(content):
    """uniform noise (10 966 corners, the border ring at response 0) and a repeated tile (11 240 corners, nearly all tied, 48 at the
    maximum: the strongest corner is decided by position) at 320 x 240"""
    L, Rt = noise_frame() if content == "noise" else tiled_frame()
    p = params(NOISE_T if content == "noise" else TILED_T, 500, 1)
    feats = R.features(L, Rt, p, 4)
    assert min(feats[0][6], feats[0][7]) >= 10000 and len(feats[0][0]) == 1000
    ctx = context(p)
    ctx.process_host([(L, Rt)], hip.RUN_DETECT)
    assert ctx.status_word(0) == 0
    assert_same_lists(ctx, 0, feats, content, ctx.result(0))
    ctx.close()


def test_crop_sequence_in_place(golden_dir):
    """the four in-place crops of test_gpu_faster.test_crop_sequence_in_place under the adaptive NMS: smSAD + ifmSAD with match IDs"""
    L, Rt = photograph(golden_dir)
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = params(10, 1200, 1)
    p.vo_use_matches_ids = 1
    [(pl, pr)], buf, host = lay_out([(L, Rt)], "rows", 800, [(0, 0)], seed=5)
    ctx = context(p, cam=cam, max_w=w, max_h=h, max_kps=4096, max_cand=1 << 17)
    st = S.SadStream(O(), p, cam)
    for t, (x, y) in enumerate(S.CROPS):
        l, r = np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(Rt[y:y + h, x:x + w])
        feats = R.features(l, r, p, 4)
        o = st.step((l, r), feats[0][0], feats[0][1], feats[0][2], feats[0][3])
        assert len(o["matches"]) >= 300 and (not t or (o["valid"] and len(o["tracked"]) >= 200)), (t, len(o["matches"]), len(o["tracked"]))
        ctx.process_device([(pl + y * 800 + x, pr + y * 800 + x)], w, h, 800)
        res = ctx.result(0)
        assert_same_lists(ctx, 0, feats, "crops t=%d" % t, res)
        assert_same_as_reference(ctx, 0, res, o, "crops t=%d" % t, ids=True)
    ctx.close()


# ---- call shapes, all at 320 x 240 -------------------------------------------------------------------------------------------

def lane_streams(T=3):
    return [make_frames("world", W, H, T, seed=70 + g) for g in range(3)]


def shape_params():
    p = params(20, 400, 2, sad=800, ifm_sad=800)
    p.ifm_win_w = p.ifm_win_h = 24
    return p


def singles(streams, p):
    """every stream through a one-lane context of its own: the snapshots the other call shapes must reproduce; lane 0 held to the reference"""
    out = []
    for g, s in enumerate(streams):
        ctx = context(p, max_octaves=2)
        snaps = []
        for t in range(len(s)):
            ctx.process_host([s[t]])
            r = ctx.result(0)
            if g == 0:
                feats = R.features(s[t][0], s[t][1], p, 4)
                assert min(len(f[0]) for f in feats) >= 50
                assert_same_lists(ctx, 0, feats, "single t=%d" % t, r)
            snaps.append(snapshot(ctx, 0, r, 2))
        ctx.close()
        out.append(snaps)
    return out


def test_lanes_and_an_idle_lane():
    """three lanes with different content; lane 1 sits frame 1 out: its lists, records and state stay untouched, and every lane equals a
    one-lane context fed the frames that lane took part in"""
    streams, p = lane_streams(3), shape_params()
    took = [[0, 1, 2], [0, 2], [0, 1, 2]]
    base = singles([[s[t] for t in tk] for s, tk in zip(streams, took)], p)
    ctx = context(p, n_lanes=3, max_octaves=2)
    seen = [0, 0, 0]
    kept = None
    for t in range(3):
        act = [g for g in range(3) if t in took[g]]
        ctx.process_host([streams[g][t] if g in act else None for g in range(3)], active=act)
        res = ctx.results()
        for g in range(3):
            if g in act:
                assert_same_snapshot(snapshot(ctx, g, res[g], 2), base[g][seen[g]], ("lanes", g, t))
                seen[g] += 1
                if g == 1:
                    kept = snapshot(ctx, 1, res[1], 2)[0]
            else:
                assert snapshot(ctx, g, res[g], 2)[0] == kept, ("idle lane", g, t)
    assert seen == [3, 2, 3]
    ctx.close()


def test_graphs_and_split_calls():
    T = 3
    streams, p = lane_streams(T), shape_params()
    base = singles(streams[:2], p)
    ctx = context(p, max_octaves=2)
    ctx.use_graphs(True)
    for rep in range(2):                                       # the second pass replays the graphs the first one captured
        ctx.reset()
        for t in range(T):
            ctx.process_host([streams[0][t]])
            assert_same_snapshot(snapshot(ctx, 0, ctx.result(0), 2), base[0][t], ("graphs", rep, t))
    captured, replayed = ctx.graph_count()
    assert captured >= 1 and replayed >= T, (captured, replayed)
    ctx.close()
    three, ahead = context(p, max_octaves=2), context(p, max_octaves=2)
    for t in range(T):
        three.process_host([streams[1][t]], hip.RUN_DETECT | hip.FLAG_DETECT_NO_POST)
        three.run_stages(hip.RUN_DETECT_POST)
        three.run_stages(REST)
        assert_same_snapshot(snapshot(three, 0, three.result(0), 2), base[1][t], ("detect, post, rest", t))
        ahead.process_host([streams[1][t]], hip.RUN_DETECT | hip.FLAG_DETECT_NO_POST | hip.FLAG_NO_SHIFT | AHEAD)
        ahead._process(None, hip.RUN_DETECT_POST | REST | AHEAD, hip.lane_mask_words([0], 1))
        assert_same_snapshot(snapshot(ahead, 0, ahead.result(0), 2), base[1][t], ("detect ahead", t))
    three.close(); ahead.close()


def test_schedulers():
    """svo_batch with 2 contexts x 2 lanes and svo_fpstream with 2 contexts equal single contexts, list for list, over 3 frames"""
    import torch
    from stereo_vo_amd.pipeline import FrameParallelStream, StreamBatch
    T = 3
    streams = lane_streams(T) + [make_frames("world", W, H, T, seed=73)]
    p = shape_params()
    base = singles(streams, p)
    batch = StreamBatch(p, CAM, W, H, 4, 2, max_kps=1024, max_cand=1 << 15, max_octaves=2)
    with pytest.raises(hip.SvoError):                           # not opted in yet: the step is refused as ever
        batch.step(lay_out([s[0] for s in streams], "rows", W, [(0, 0)] * 4, seed=9)[0])
    batch.set_faster_adaptive_nms(True)
    assert [c.faster_adaptive_nms() for c in batch.ctxs] == [True, True]
    steps = [lay_out([s[t] for s in streams], "rows", W, [(0, 0)] * 4, seed=t) for t in range(T)]
    for t, (ptrs, buf, host) in enumerate(steps):
        batch.step(ptrs)
        batch.synchronize()
        res = batch.results()
        for g in range(4):
            c, lane = batch.lane(g)
            assert_same_snapshot(snapshot(c, lane, res[g], 2), base[g][t], ("batch", g, t))
    batch.close()
    fp = FrameParallelStream(p, CAM, W, H, lanes=1, contexts=2, max_kps=1024, max_cand=1 << 15, max_octaves=2)
    fp.set_faster_adaptive_nms(True)
    assert [c.faster_adaptive_nms() for c in fp.ctxs] == [True, True]
    for t in range(T):
        c = fp.push([steps[t][0][2]])
        fp.synchronize()
        assert_same_snapshot(snapshot(c, 0, c.result(0), 2), base[2][t], ("frame parallel", t))
    fp.close()
    torch.cuda.synchronize()


def test_dynamic_threshold():
    """svo_set_dyn_fast_threshold on top: thresholds and statistics equal the literal walk over 4 frames (they depend on the corner
    counts alone), and the lists equal the adaptive reference at the walked thresholds"""
    frames = make_frames("world", W, H, 4, seed=70)
    p = params(5, 400, 2)
    target = 0.001                                             # far too few: the thresholds rise by two a frame
    pg = p.copy(); pg.nmsMethod = 0
    walk = D.walk(frames, pg, target, 4)
    ctx = context(p, max_octaves=2)
    ctx.set_dyn_fast_threshold(True, target)
    for t, ((l, r), (_, stats)) in enumerate(zip(frames, walk)):
        assert stats["used_left"] == [5 + 2 * t] * 2 and stats["used_right"] == [6 + 2 * t] * 2
        ctx.process_host([(l, r)], hip.RUN_DETECT | hip.RUN_MATCH)
        assert ctx.faster_stats(0).as_dict(2) == dict(stats, frame=t + 1), (t, ctx.faster_stats(0).as_dict(2), stats)
        feats = R.features(l, r, p, 4, stats["used_left"], stats["used_right"])
        assert [f[6] for f in feats] == stats["corners_left"] and [f[7] for f in feats] == stats["corners_right"]
        assert_same_lists(ctx, 0, feats, "dynamic t=%d" % t, ctx.result(0))
    ctx.close()


# ---- the opt-in ---------------------------------------------------------------------------------------------------------------

def lists_of(ctx):
    """what a refused call must leave alone (the row tables cannot be read between a svo_set_params and the next detect call)"""
    return ctx.keypoints(0, 0, 0)[0].tobytes(), ctx.keypoints(0, 0, 1)[0].tobytes(), ctx.matches(0).tobytes()


def test_opt_in_semantics(golden_dir):
    frames = make_frames("world", W, H, 2, seed=70)
    pa = params(20, 400, 1)
    pg = pa.copy(); pg.nmsMethod = 0
    ctx = hip.Context(n_lanes=1, **KW)
    ctx.set_params(pg); ctx.set_camera(CAM)
    assert ctx.faster_adaptive_nms() is False and ctx.L.svo_get_faster_adaptive_nms(ctx.h) == 0
    ctx.process_host([frames[0]], hip.RUN_DETECT | hip.RUN_MATCH)
    grid = F.faster_features(frames[0][0], frames[0][1], pg, 4)
    assert_same_lists(ctx, 0, grid, "grid NMS, opt-in off")
    before = lists_of(ctx)
    fr = (hip.Frame * 1)()
    l1, r1 = np.ascontiguousarray(frames[1][0]), np.ascontiguousarray(frames[1][1])
    fr[0].left = hip.Image(l1.ctypes.data, W, H, W); fr[0].right = hip.Image(r1.ctypes.data, W, H, W)

    def refused():
        for flags in (hip.RUN_ALL, hip.RUN_DETECT, hip.RUN_DETECT_POST | hip.FLAG_NO_SHIFT):
            rc = ctx.L.svo_process(ctx.h, fr, C.c_uint32(flags))
            assert rc == SVO_ERR_UNSUPPORTED and ctx.L.svo_last_error(ctx.h) == OLD_TEXT, (flags, rc, ctx.L.svo_last_error(ctx.h))
        assert lists_of(ctx) == before

    ctx.set_params(pa)
    refused()                                                   # off: the old status, the old text, nothing moves
    ctx.set_faster_adaptive_nms(True)
    assert ctx.faster_adaptive_nms() is True and ctx.L.svo_get_faster_adaptive_nms(ctx.h) == 1
    ctx.process_host([frames[1]], hip.RUN_DETECT | hip.RUN_MATCH)
    adaptive = R.features(frames[1][0], frames[1][1], pa, 4)
    assert_same_lists(ctx, 0, adaptive, "adaptive NMS, opt-in on", ctx.result(0))
    ctx.set_params(pg)                                          # on, but nmsmStandard selected: the grid NMS, as without the opt-in
    ctx.process_host([frames[0]], hip.RUN_DETECT | hip.RUN_MATCH)
    assert lists_of(ctx) == before
    ctx.set_params(pa)
    ctx.set_faster_adaptive_nms(False)
    assert ctx.faster_adaptive_nms() is False
    refused()                                                   # off again: refused again
    for bad, rc_want in ((dict(detect_method=3), SVO_ERR_UNSUPPORTED), (dict(ifm_method=3), SVO_ERR_UNSUPPORTED)):       # dmKLT, optical flow: refused either way
        for on in (False, True):
            ctx.set_faster_adaptive_nms(on)
            q = pa.copy()
            for k, v in bad.items():
                setattr(q, k, v)
            ctx.set_params(q)
            assert ctx.L.svo_process(ctx.h, fr, C.c_uint32(hip.RUN_ALL)) == rc_want, (bad, on)
    ctx.close()
    # under FAST+ORB and ORB the setter is accepted and inert: identical bytes with it on and off, with either NMS method
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    Wg, Hg = int(g["W"]), int(g["H"])
    for method in (0, DM_FAST_ORB):
        for nms_method in (0, 1):
            got = []
            for on in (False, True):
                p = hip.default_params()
                p.detect_method, p.nOctaves, p.orb_nfeats, p.nmsMethod = method, 1, 300, nms_method
                c = hip.Context(n_lanes=1, max_w=Wg, max_h=Hg, max_kps=1024, max_cand=1 << 15)
                c.set_params(p)
                c.set_faster_adaptive_nms(on)
                c.process_host([(g["L0"], g["R0"])], hip.RUN_DETECT | hip.RUN_MATCH)
                k0, d0 = c.keypoints(0, 0, 0)
                assert len(k0) >= 50
                got.append((k0.tobytes(), d0.tobytes(), c.keypoints(0, 0, 1)[0].tobytes(), c.matches(0).tobytes()))
                c.close()
            assert got[0] == got[1], (method, nms_method)


def test_kernel_time_names_and_launch_counts():
    """the new selection counts under "faster_nms": one launch per frame where the grid NMS had one; the name list is unchanged"""
    frames = make_frames("world", W, H, 2, seed=70)
    names = []
    for adaptive in (False, True):
        p = params(20, 400, 1)
        p.nmsMethod = 1 if adaptive else 0
        ctx = hip.Context(n_lanes=1, kernel_times=True, **KW)
        ctx.set_params(p); ctx.set_camera(CAM)
        ctx.set_faster_adaptive_nms(adaptive)
        for f in frames:
            ctx.process_host([f])
        kt = ctx.kernel_times()
        assert kt["faster"][1] == 2 and kt["faster_nms"][1] == 2 and kt["select"][1] == 0, adaptive
        names.append(list(kt))
        ctx.close()
    assert names[0] == names[1] and names[0][-2:] == ["faster", "faster_nms"]


def test_candidate_overflow():
    """the noise frame against a candidate list of 4096: status bit 1, exactly min(cap, cand_cap) entries, nothing faults; which corners
    a cut list holds is undefined, as under the grid NMS"""
    L, Rt = noise_frame()
    p = params(NOISE_T, 500, 1)
    ctx = context(p, max_cand=4096)
    ctx.process_host([(L, Rt)], hip.RUN_DETECT)
    assert ctx.status_word(0) & ST_CAND_OVERFLOW and ctx.result(0).status & ST_CAND_OVERFLOW
    cap = F.kps_to_detect(500, 1)[0]
    for side in (0, 1):
        k, d = ctx.keypoints(0, 0, side)
        assert len(k) == min(cap, 4096) and not d.any()
        assert len(set(zip(k["x"].tolist(), k["y"].tolist()))) == len(k) and (np.diff(k["y"]) >= 0).all()
    ctx.close()
