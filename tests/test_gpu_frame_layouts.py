"""Device frames read IN PLACE from caller memory (SVO_FLAG_DEVICE_IMAGES without a rectify map, BGR or graphs: level 0 is never
copied) at the strides and byte alignments a caller's memory really has -- padded rows, odd widths held contiguously, crops of a
larger frame, side-by-side stereo frames -- against the CPU oracle fed contiguous copies of the same images.

What the layouts select in the kernels: k_resize stages its window by LDS-DMA when the pitch is a multiple of 16 (reading the row
padding when stride > w) and by a byte loop otherwise; k_harris takes the 12-byte-load form only when base and pitch are multiples
of 4 and the byte-wise harris_at otherwise; fast_stage (k_fast), k_describe's window fetch and k_half take any alignment through
one path; k_prepare reads caller memory when the frames are BGR or a rectify map is set.  Every frame sits in a buffer of random
poison bytes (tests/image_content.py: place), so a read outside the contract of svo_image.stride (include/svo_hip.h) gives a wrong
list, and the buffer is compared with its host copy afterwards: nothing writes caller memory."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, north_star_params, DM_FAST_ORB
from stereo_vo_amd.synth import SyntheticStereoWorld

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_content as IC                                      # noqa: E402
from test_gpu_parity import assert_same_frame, O, POSE_TOL_M, POSE_TOL_RAD, _distortion_maps    # noqa: E402

pytestmark = pytest.mark.gpu


def make_frames(content, w, h, n, seed, shift=0):
    """n (left, right) pairs of one moving stream: the synthetic world, or a structured image (rolled right by `shift` px first)
    whose right image is the left one rolled by -6 px and whose following frames are rolled by (3, 2) px each"""
    if content == "world":
        import torch
        world = SyntheticStereoWorld(w + (-w) % 8, h + (-h) % 8, 400.0 * w / 640.0, 0.12, seed=seed, n_frames=n, device=torch.device("cpu"))
        return [tuple(np.ascontiguousarray(x.numpy()[:h, :w]) for x in world.render(t)) for t in range(n)]
    base = IC.moved(IC.CONTENTS[content](w, h, seed=seed), shift, 0)
    out = []
    for t in range(n):
        L = IC.moved(base, 3 * t, 2 * t)
        out.append((L, IC.right_of(L, 6)))
    return out


def lay_out(pairs, kind, stride, offs, seed):
    """one time step of every lane in ONE poisoned device buffer: ([(left address, right address)] per lane, buffer, host copy)"""
    if kind == "sbs":               # one side-by-side frame per lane: stride = 2 w, the right image starts w bytes into the row
        w = pairs[0][0].shape[1]
        ptrs, buf, host = IC.place([np.hstack([L, R]) for L, R in pairs], stride, [o[0] for o in offs], seed)
        return [(a, a + w) for a in ptrs], buf, host
    ptrs, buf, host = IC.place([x for pr in pairs for x in pr], stride, [o for pr in offs for o in pr], seed)
    return [(ptrs[2 * i], ptrs[2 * i + 1]) for i in range(len(pairs))], buf, host


def assert_same_octaves(ctx, lane, orc, r, ro, noct, tag):
    """the per-octave lists of the FAST+ORB mode, as test_fast_orb_multi_octave_matches_oracle compares them"""
    assert r.n_octaves == ro.n_octaves == noct, tag
    for o in range(noct):
        for side in (0, 1):
            k, d = ctx.keypoints(lane, 0, side, o); ko, do = orc.keypoints(0, side, o)
            assert len(k) == len(ko) and k.tobytes() == ko.tobytes() and (d == do).all(), (tag, o, side, len(k), len(ko))
            assert (ctx.row_index(lane, 0, side, o) == orc.row_index(0, side, o)).all(), (tag, o, side)
        assert ctx.matches(lane, 0, o).tobytes() == orc.matches(0, o).tobytes(), (tag, o, "pairings")
        assert ctx.tracked(lane, o).tobytes() == orc.tracked(o).tobytes(), (tag, o, "tracked pairs")
        assert (r.detected_left[o], r.detected_right[o], r.stereo_matches[o]) == (ro.detected_left[o], ro.detected_right[o], ro.stereo_matches[o]), (tag, o)
    assert (r.valid, r.error_code, r.n_residual, r.n_outliers) == (ro.valid, ro.error_code, ro.n_residual, ro.n_outliers), tag
    if ro.valid:
        dp = np.abs(np.array(r.outPose) - np.array(ro.outPose))
        assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (tag, dp)
        assert (ctx.outliers(lane) == orc.outliers()).all(), tag


def check_pyramid_and_raw(monkeypatch, w, h, nfe, pairs, process, tag, max_kps=2048, max_cand=1 << 16, oracle_list=None):
    """debug mode 9 (the detector's own order): level 0 is the caller's image, levels 1..7 the oracle's resize chain, and the raw
    keypoint list -- positions, responses, angles, descriptors, order -- is O.orb_detect's.  process(ctx) hands the frame (one pair
    per lane) to the context with RUN_DETECT; oracle_list(lane, side, img) may supply the oracle's list (after asserting on it)"""
    monkeypatch.setenv("SVO_DEBUG_MODE", "9")
    ctx = hip.Context(n_lanes=len(pairs), max_w=w, max_h=h, max_kps=max_kps, max_cand=max_cand)
    monkeypatch.delenv("SVO_DEBUG_MODE")
    ctx.set_params(north_star_params(hip.default_params(), orb_nfeats=nfe))
    ctx.set_camera(StereoCamera.simple(400.0 * w / 640.0, w / 2.0, h / 2.0, 0.12, w, h))
    process(ctx)
    lw, lh, _ = O().pyramid_sizes(w, h, 8)
    for lane, pr in enumerate(pairs):
        for side, img in enumerate(pr):
            assert (ctx.level(lane, side, 0) == img).all(), (tag, lane, side, "level 0")
            prev = img
            for l in range(1, 8):
                ref = O().resize(prev, lw[l], lh[l])
                got = ctx.level(lane, side, l)
                assert (got == ref).all(), (tag, lane, side, "level %d: %d pixels differ" % (l, int((got != ref).sum())))
                prev = ref
            k, d = ctx.raw_keypoints(lane, side)
            ko, do = oracle_list(lane, side, img) if oracle_list else O().orb_detect(img, int(1.5 * nfe), 8, 20)
            assert len(k) == len(ko) and len(ko) > 50, (tag, lane, side, len(k), len(ko))
            assert k.tobytes() == ko.tobytes(), (tag, lane, side, "raw keypoints: %d positions / %d responses / %d angles differ" % (
                int(((k["x"] != ko["x"]) | (k["y"] != ko["y"]) | (k["octave"] != ko["octave"])).sum()), int((k["response"] != ko["response"]).sum()), int((k["angle"] != ko["angle"]).sum())))
            assert (d == do).all(), (tag, lane, side, "raw descriptors")
        assert ctx.status_word(lane) == 0, (tag, lane, ctx.status_word(lane))
    ctx.close()


# id, w, h, stride, kind, (left, right) base offsets per lane, content per lane, requested features
LAYOUTS = [
    ("control-640", 640, 480, 640, "rows", [(0, 0)], ["world"], 500),
    ("pad-656", 640, 480, 656, "rows", [(0, 0)], ["world"], 500),                    # k_resize DMA branch reading row padding
    ("pad-704", 640, 480, 704, "rows", [(0, 0)], ["world"], 500),
    ("odd-643", 640, 480, 643, "rows", [(0, 0)], ["binary_blocks"], 500),           # byte branch of k_resize, harris_at
    ("pitch-644-base-2-0", 640, 480, 644, "rows", [(2, 0)], ["world"], 500),        # pitch % 4 == 0, % 16 != 0; the pair differs in alignment
    ("base-1-3", 640, 480, 640, "rows", [(1, 3)], ["binary_blocks"], 500),          # aligned pitch, odd bases: DMA from odd addresses, harris_at
    ("base-5-11", 640, 480, 640, "rows", [(5, 11)], ["world"], 500),
    ("contiguous-417x311", 417, 311, 417, "rows", [(0, 0)], ["world"], 300),
    ("contiguous-1241x376", 1241, 376, 1241, "rows", [(0, 0)], ["world"], 900),
    ("side-by-side-640", 640, 480, 1280, "sbs", [(0, 0)], ["world"], 500),
    ("side-by-side-1241", 1241, 376, 2482, "sbs", [(0, 0)], ["world"], 900),
    ("three-lanes-672", 640, 480, 672, "rows", [(0, 5), (7, 2), (13, 9)], ["world", "binary_blocks", "world"], 500),
]


@pytest.mark.parametrize("name,w,h,stride,kind,offs,contents,nfe", LAYOUTS, ids=[c[0] for c in LAYOUTS])
def test_frames_read_in_place_match_oracle(monkeypatch, name, w, h, stride, kind, offs, contents, nfe):
    n_lanes, n_frames = len(offs), 3
    # (block images are rolled by 15 px first: a block edge then lies between the last two columns, so the clamp of the byte
    # branch of k_resize to column w - 1 decides pixels)
    streams = [make_frames(c, w, h, n_frames, seed=40 + 7 * lane, shift=15) for lane, c in enumerate(contents)]
    steps = [lay_out([s[t] for s in streams], kind, stride, offs, seed=t) for t in range(n_frames)]
    # (1) + (2): the pyramid and the detector's raw list of the first frame
    check_pyramid_and_raw(monkeypatch, w, h, nfe, [s[0] for s in streams], lambda c: c.process_device(steps[0][0], w, h, stride, hip.RUN_DETECT), name)
    # (3): three frames, every list
    cam = StereoCamera.simple(400.0 * w / 640.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    ctx = hip.Context(n_lanes=n_lanes, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 16)
    ctx.set_params(p); ctx.set_camera(cam)
    orcs = [O().Oracle(p) for _ in range(n_lanes)]
    for t, (ptrs, buf, host) in enumerate(steps):
        ctx.process_device(ptrs, w, h, stride)
        for lane in range(n_lanes):
            L, R = streams[lane][t]
            ro = orcs[lane].process(L, R, cam)
            assert_same_frame(ctx, lane, orcs[lane], ctx.result(lane), ro, "%s lane=%d t=%d" % (name, lane, t))
            assert ctx.status_word(lane) == 0, (name, lane, t)
            assert ro.detected_left[0] > 100, (name, lane, t, "the oracle's frame is all but empty")
    ctx.close()
    # (4): nothing wrote the caller's memory
    for ptrs, buf, host in steps:
        IC.assert_untouched(buf, host)


FAST_ORB_LAYOUTS = [c for c in LAYOUTS if c[0] in ("odd-643", "base-1-3", "side-by-side-1241")]


@pytest.mark.parametrize("name,w,h,stride,kind,offs,contents,nfe", FAST_ORB_LAYOUTS, ids=[c[0] for c in FAST_ORB_LAYOUTS])
def test_fast_orb_two_octaves_read_in_place(name, w, h, stride, kind, offs, contents, nfe):
    """FAST+ORB on a 2-octave x1/2 pyramid: k_half reads level 0 in place (besides k_fast and k_describe).  Where the ORB case runs
    0 / 255 blocks this one runs the periodic texture (saturated pixels too): perfect blocks are plateaus of equal FAST scores at
    every x1/2 octave, which the strict 3x3 NMS removes altogether, and an empty list compares equal to anything"""
    streams = [make_frames("periodic" if c == "binary_blocks" else c, w, h, 3, seed=61) for c in contents]
    cam = StereoCamera.simple(400.0 * w / 640.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.detect_method = DM_FAST_ORB; p.nOctaves = 2
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=4096, max_cand=1 << 17, max_octaves=2)
    ctx.set_params(p); ctx.set_camera(cam)
    orc = O().Oracle(p)
    keep = []
    for t in range(3):
        ptrs, buf, host = lay_out([streams[0][t]], kind, stride, offs, seed=10 + t)
        keep.append((buf, host))
        ctx.process_device(ptrs, w, h, stride)
        r, ro = ctx.result(0), orc.process(streams[0][t][0], streams[0][t][1], cam)
        assert ctx.status_word(0) == 0, (name, t)
        assert_same_octaves(ctx, 0, orc, r, ro, 2, "%s t=%d" % (name, t))
        assert ro.detected_left[0] > 100 and ro.detected_left[1] > 20, (name, t)
    ctx.close()
    for buf, host in keep:
        IC.assert_untouched(buf, host)


def test_graph_replay_copies_strided_device_frames():
    """svo_use_graphs: a captured frame reads fixed addresses, so device frames go to the ring slot first -- a strided
    device-to-device copy from an odd stride and odd bases; both slots captured, then replayed"""
    w, h, stride, offs = 640, 480, 643, [(1, 3)]
    frames = make_frames("world", w, h, 3, seed=71)
    cam = StereoCamera.simple(400.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = north_star_params(hip.default_params(), orb_nfeats=500)
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 16)
    ctx.set_params(p); ctx.set_camera(cam); ctx.use_graphs(True)
    orc = O().Oracle(p)
    steps = [lay_out([frames[t]], "rows", stride, offs, seed=t) for t in range(3)]
    for i, t in enumerate((0, 1, 2, 1, 0)):
        ctx.process_device(steps[t][0], w, h, stride)
        ro = orc.process(frames[t][0], frames[t][1], cam)
        assert_same_frame(ctx, 0, orc, ctx.result(0), ro, "graph i=%d" % i)
        assert ctx.status_word(0) == 0
    ctx.close()
    for ptrs, buf, host in steps:
        IC.assert_untouched(buf, host)


@pytest.mark.parametrize("rectify", [False, True])
def test_bgr_device_frames_at_an_odd_stride(rectify):
    """k_prepare reads caller memory: BGR device frames at stride 3 w + 7 from an odd base, with and without a rectify map; the
    prepared level-0 images and the whole frame against the oracle's, as test_stage1_grey_and_rectify_on_device compares them"""
    w, h = 640, 480
    stride = 3 * w + 7
    grey = make_frames("world", w, h, 2, seed=81)
    cam = StereoCamera.simple(400.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = north_star_params(hip.default_params(), orb_nfeats=300)
    ctx = hip.Context(n_lanes=2, max_w=w, max_h=h, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    maps = [_distortion_maps(w, h), _distortion_maps(w, h, k1=-0.05, shift=(-3.25, 0.5), rot=-0.004)]
    if rectify:
        ctx.set_rectify_map(0, 0, *maps[0]); ctx.set_rectify_map(0, 1, *maps[1])      # lane 0 rectifies, lane 1 does not
    orcs = [O().Oracle(p), O().Oracle(p)]
    keep = []
    for t in range(2):
        L, R = grey[t]
        L = np.ascontiguousarray(np.stack([L, np.roll(L, 3, 1), 255 - L // 2], -1)); R = np.ascontiguousarray(np.stack([R, np.roll(R, 2, 0), 255 - R // 2], -1))
        ptrs, buf, host = IC.place([L, R], stride, [1, 1], seed=t)
        keep.append((buf, host))
        ctx.process_device([(ptrs[0], ptrs[1])] * 2, w, h, stride, hip.RUN_ALL | hip.FLAG_BGR_IMAGES)
        want = [[O().prepare(L, *maps[0]), O().prepare(R, *maps[1])] if rectify else [O().prepare(L), O().prepare(R)], [O().prepare(L), O().prepare(R)]]
        for lane in range(2):
            for side in range(2):
                assert (ctx.level(lane, side, 0) == want[lane][side]).all(), (t, lane, side)
            ro = orcs[lane].process(want[lane][0], want[lane][1], cam)
            assert_same_frame(ctx, lane, orcs[lane], ctx.result(lane), ro, "bgr rectify=%s t=%d lane=%d" % (rectify, t, lane))
            assert ro.detected_left[0] > 100
    ctx.close()
    for buf, host in keep:
        IC.assert_untouched(buf, host)


def test_stream_batch_steps_over_strided_device_memory():
    """StreamBatch.step(ptrs, stride=...) with DEVICE memory at stride 643: two contexts of two lanes, every lane against its own
    oracle (page-locked host memory, as the padded-stride batch test uses, is uploaded into aligned buffers first and never
    reaches the in-place branches)"""
    from stereo_vo_amd.pipeline import StreamBatch
    w, h, stride, B, NC = 640, 480, 643, 4, 2
    contents = ["world", "binary_blocks", "world", "world"]
    streams = [make_frames(c, w, h, 3, seed=90 + lane, shift=15) for lane, c in enumerate(contents)]
    offs = [(0, 0), (1, 2), (3, 0), (6, 15)]
    cam = StereoCamera.simple(400.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = north_star_params(hip.default_params(), orb_nfeats=500)
    batch = StreamBatch(p, cam, w, h, B, NC, max_kps=2048, max_cand=1 << 16)
    orcs = [O().Oracle(p) for _ in range(B)]
    steps = [lay_out([s[t] for s in streams], "rows", stride, offs, seed=t) for t in range(3)]
    for t, (ptrs, buf, host) in enumerate(steps):
        batch.step(ptrs, stride=stride)
        batch.synchronize()
        res = batch.results()
        for g in range(B):
            ctx, lane = batch.lane(g)
            ro = orcs[g].process(streams[g][t][0], streams[g][t][1], cam)
            assert_same_frame(ctx, lane, orcs[g], res[g], ro, "batch lane %d t=%d" % (g, t))
            assert ctx.status_word(lane) == 0
    batch.close()
    for ptrs, buf, host in steps:
        IC.assert_untouched(buf, host)


def test_stride_contract_is_enforced_before_any_launch(golden_dir):
    """svo_process refuses, with SVO_ERR_ARG and a text in svo_last_error, a stride smaller than a row (grey and BGR, device and
    host frames) and a device frame whose h * stride exceeds the 32-bit offsets the kernels compute; nothing is enqueued, and the
    context processes a good frame afterwards as if the refused calls had never been made"""
    import torch
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    orc = O().Oracle(p)
    ptrs0, buf0, host0 = lay_out([(g["L0"], g["R0"])], "rows", W + 3, [(1, 2)], seed=0)
    ctx.process_device(ptrs0, W, H, W + 3)
    assert_same_frame(ctx, 0, orc, ctx.result(0), orc.process(g["L0"], g["R0"], cam), "before the refusals")
    ptrs1, buf1, host1 = lay_out([(g["L1"], g["R1"])], "rows", W + 3, [(1, 2)], seed=1)
    for stride, flags, text in ((W - 1, hip.RUN_ALL, "smaller than a row"), (0, hip.RUN_ALL, "smaller than a row"), (-(W + 3), hip.RUN_ALL, "smaller than a row"),
                                (3 * W - 1, hip.RUN_ALL | hip.FLAG_BGR_IMAGES, "smaller than a row"),
                                ((1 << 31) // H + 1, hip.RUN_ALL, "exceeds"), (1 << 33, hip.RUN_ALL, "exceeds"), ((1 << 32) + W + 3, hip.RUN_ALL, "exceeds")):
        with pytest.raises(hip.SvoError, match="invalid argument.*stride %d is.*" % stride + text if text != "exceeds" else "invalid argument.*x %d exceeds" % stride):
            ctx.process_device(ptrs1, W, H, stride, flags)
    # svo_last_error speaks of the call it follows: a refusal that has no text of its own does not inherit the stride message
    q = p.copy(); q.min_distance = 1
    ctx.set_params(q)
    with pytest.raises(hip.SvoError) as e:
        ctx.process_device(ptrs1, W, H, W + 3)
    assert "invalid argument" in str(e.value) and "stride" not in str(e.value) and "exceeds" not in str(e.value), str(e.value)
    ctx.set_params(p)
    fr = (hip.Frame * 1)()
    fr[0].left = hip.Image(g["L1"].ctypes.data, W, H, W - 1); fr[0].right = hip.Image(g["R1"].ctypes.data, W, H, W)
    assert ctx.L.svo_process(ctx.h, fr, hip.RUN_ALL) == -2 and b"smaller than a row" in ctx.L.svo_last_error(ctx.h)      # SVO_ERR_ARG, host frames too
    # the refused calls left no trace: the next good frame continues the stream
    ctx.process_device(ptrs1, W, H, W + 3)
    ro = orc.process(g["L1"], g["R1"], cam)
    assert_same_frame(ctx, 0, orc, ctx.result(0), ro, "after the refusals")
    assert ro.valid and ctx.status_word(0) == 0
    ctx.close()
    IC.assert_untouched(buf0, host0); IC.assert_untouched(buf1, host1)
    torch.cuda.synchronize()


def _ref_pair(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_pair_800x600.npz"))
    return g["left"], g["right"]


@pytest.mark.parametrize("nfe,match_method,ifm_method", [(500, 0, 0), (1200, 1, 1)])
def test_photograph_full_frame_and_in_place_crops(golden_dir, nfe, match_method, ifm_method):
    """The reference's only real stereo pair (800x600, 3 % of the pixels at 255 and 8 % at 0): the full pair through process_host,
    then, uploaded once, four 760x560 crops read in place at stride 800 from (20,20), (17,22), (13,23), (10,25) -- base addresses
    4, 1, 13, 10 mod 16 -- as a moving sequence; brute-force matcher / tracker at 500 features, row-by-row / windowed at 1200"""
    L, R = _ref_pair(golden_dir)
    assert L.shape == (600, 800)
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.match_method = match_method; p.ifm_method = ifm_method
    cam = StereoCamera.simple(500.0, 400.0, 300.0, 0.12, 800, 600)
    ctx = hip.Context(n_lanes=1, max_w=800, max_h=600, max_kps=4096, max_cand=1 << 17)
    ctx.set_params(p); ctx.set_camera(cam)
    orc = O().Oracle(p)
    ctx.process_host([(L, R)])
    ro = orc.process(L, R, cam)
    assert_same_frame(ctx, 0, orc, ctx.result(0), ro, "photograph, full frame")
    assert ro.detected_left[0] > 300 and ro.stereo_matches[0] > 150 and ctx.status_word(0) == 0
    ctx.close()
    w, h = 760, 560
    [(pl, pr)], buf, host = lay_out([(L, R)], "rows", 800, [(0, 0)], seed=5)
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=4096, max_cand=1 << 17)
    ctx.set_params(p); ctx.set_camera(cam)
    orc = O().Oracle(p)
    for t, (x, y) in enumerate(((20, 20), (17, 22), (13, 23), (10, 25))):
        o = y * 800 + x
        assert (pl + o) % 16 == (4, 1, 13, 10)[t]
        ctx.process_device([(pl + o, pr + o)], w, h, 800)
        ro = orc.process(np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w]), cam)
        assert_same_frame(ctx, 0, orc, ctx.result(0), ro, "photograph crop (%d,%d)" % (x, y))
        assert ctx.status_word(0) == 0
        if t > 0:                                   # from the oracle's own result: the test cannot pass on an empty frame
            assert ro.valid and ro.tracked_feats_from_last_frame > 50, (t, ro.valid, ro.tracked_feats_from_last_frame)
    ctx.close()
    IC.assert_untouched(buf, host)
