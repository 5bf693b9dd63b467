"""Rectification maps built on the device from a stereo calibration (svo_set_undistort_rectify, svo_set_stereo_calibration;
k_rectify_map) against the independent walk of tests/rectify_ref.py pushed through the existing float-map setter, and whole frames
rectified by those maps against the oracle's svo_oracle_prepare.  Every test here needs a real MI355X: run with `pytest -m gpu`."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import CameraModel, north_star_params
from stereo_vo_amd.synth import SyntheticStereoWorld

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_ref as RR                                           # noqa: E402
from test_gpu_parity import assert_same_frame, O, _distortion_maps    # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 320, 240
_shared = {}


def mild():
    """the mild calibration at 320 x 240 with its walk, and two rendered frames of the world test_stage1_grey_and_rectify_on_device uses"""
    if not _shared:
        import torch
        cal = RR.calibration_mild(0, W, H, 150.0)
        r, sides = RR.walk(cal)
        world = SyntheticStereoWorld(W, H, 150.0, 0.12, seed=3, n_frames=2, device=torch.device("cpu"))
        frames = [[np.ascontiguousarray(x.numpy()[:H, :W]) for x in world.render(t)] for t in range(2)]
        _shared.update(cal=cal, r=r, sides=sides, frames=frames, maps=[(s["mx"], s["my"]) for s in sides])
    return _shared


def context(n_lanes):
    ctx = hip.Context(n_lanes=n_lanes, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15)
    p = north_star_params(hip.default_params(), orb_nfeats=300)
    ctx.set_params(p)
    return ctx, p


def coloured(L, R):
    """a colour pair whose grey value is not just one of its channels"""
    return (np.ascontiguousarray(np.stack([L, np.roll(L, 3, 1), 255 - L // 2], -1)), np.ascontiguousarray(np.stack([R, np.roll(R, 2, 0), 255 - R // 2], -1)))


@pytest.mark.parametrize("name,fn,zd", [("A", RR.calibration_a, 0), ("A", RR.calibration_a, 1), ("B", RR.calibration_b, 0), ("B", RR.calibration_b, 1)],
                         ids=["A-zd0", "A-zd1", "B-zd0", "B-zd1"])
def test_kernel_table_is_the_float_maps_table_exactly(name, fn, zd):
    """k_rectify_map is, entry for entry, "compute the float maps of the model, then svo_set_rectify_map": lane 0 gets the calibration
    through the device path, lane 1 the walk's float32 maps through the host path; no entry may differ.  A (96 x 64) and B (333 x 127:
    odd rows start 8-byte aligned only, the row tail is one entry) reach sentinels and the -1 / last rows and columns on both sides
    (test_rectify_cpu.py pins how many)."""
    cal = fn(zd)
    w, h = cal["w"], cal["h"]
    _, sides = RR.walk(cal)
    ctx = hip.Context(n_lanes=2, max_w=w, max_h=h, max_kps=1024, max_cand=1 << 15)
    for side, s in enumerate(sides):
        ctx.set_undistort_rectify(0, side, CameraModel.make(*s["cam"]), s["R"], s["P"], w, h)
        ctx.set_rectify_map(1, side, s["mx"], s["my"])
    for side, s in enumerate(sides):
        dev, host = ctx.rectify_map_fixed(0, side), ctx.rectify_map_fixed(1, side)
        assert len(dev[0]) == w * h == len(host[0])
        bad = np.flatnonzero((dev[0] != host[0]) | (dev[1] != host[1]))
        assert bad.size == 0, (name, zd, side, bad.size, [(int(b % w), int(b // w), hex(dev[0][b]), hex(host[0][b]), hex(dev[1][b]), hex(host[1][b])) for b in bad[:5]])
        # the host setter's lines, written a third time in numpy (what the reach counts of test_rectify_cpu.py are taken from)
        assert (host[0] == s["fixed"][0].reshape(-1)).all() and (host[1] == s["fixed"][1].reshape(-1)).all()
    ctx.close()


@pytest.mark.parametrize("bgr,device", [(False, False), (False, True), (True, False)], ids=["host-grey", "device-grey", "host-bgr"])
def test_whole_call_rectifies_every_lane_like_the_oracle(bgr, device):
    """svo_set_stereo_calibration(lane = -1, set_camera = 1) on three lanes: the prepared level-0 images are svo_oracle_prepare's with
    the walk's float maps, bit for bit, and every list and the pose are the oracle's on those images with the returned camera."""
    import torch
    S = mild()
    ctx, p = context(3)
    out = ctx.set_stereo_calibration(RR.to_ctypes(S["cal"]), lane=-1, set_camera=True)
    cam = out.cam
    assert abs(cam.l_fx - S["r"]["P1"][0]) <= 1e-12 * cam.l_fx and cam.baseline == -out.tx and (cam.ncols, cam.nrows) == (W, H)
    for lane in range(3):
        for side in range(2):
            xy, frac = ctx.rectify_map_fixed(lane, side)
            assert (xy == S["sides"][side]["fixed"][0].reshape(-1)).all() and (frac == S["sides"][side]["fixed"][1].reshape(-1)).all(), (lane, side)
    orc = O().Oracle(p)
    for t in range(2):
        L, R = S["frames"][t]
        if bgr:
            L, R = coloured(L, R)
        if device:
            tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
            ctx.process_device([(tl.data_ptr(), tr.data_ptr())] * 3, W, H, L.strides[0], hip.RUN_ALL | (hip.FLAG_BGR_IMAGES if bgr else 0))
        else:
            ctx.process_host([(L, R)] * 3)
        want = [O().prepare(L, *S["maps"][0]), O().prepare(R, *S["maps"][1])]
        ro = orc.process(want[0], want[1], cam)
        for lane in range(3):
            for side in range(2):
                assert (ctx.level(lane, side, 0) == want[side]).all(), (t, lane, side)
            assert_same_frame(ctx, lane, orc, ctx.result(lane), ro, "t=%d lane=%d" % (t, lane))
    assert ro.valid and ro.tracked_feats_from_last_frame >= 8, "the synthetic world no longer tracks through this calibration"
    ctx.close()


def test_sharing_and_detaching():
    """After lane = -1 the lanes share one table per side.  A per-lane set by either setter, or a per-lane clear, detaches that lane
    only; a calibration of another size while maps exist is refused and changes nothing."""
    S = mild()
    ctx, p = context(3)
    ctx.set_stereo_calibration(RR.to_ctypes(S["cal"]), lane=-1, set_camera=True)
    shared = [S["sides"][s]["fixed"] for s in range(2)]

    def same(lane, side, fx):
        xy, frac = ctx.rectify_map_fixed(lane, side)
        return len(xy) == W * H and (xy == fx[0].reshape(-1)).all() and (frac == fx[1].reshape(-1)).all()

    # the new setter on one lane: the table of the zero-disparity variant for lane 1's left camera; lanes 0 and 2 keep the shared one
    cal1 = RR.calibration_mild(1, W, H, 150.0)
    _, sides1 = RR.walk(cal1)
    ctx.set_undistort_rectify(1, 0, CameraModel.make(*sides1[0]["cam"]), sides1[0]["R"], sides1[0]["P"], W, H)
    assert not (sides1[0]["fixed"][0] == shared[0][0]).all()
    assert same(1, 0, sides1[0]["fixed"]) and same(0, 0, shared[0]) and same(2, 0, shared[0]) and same(1, 1, shared[1])
    # the old setter on lane 1, both sides; lane 2 cleared
    own = [_distortion_maps(W, H), _distortion_maps(W, H, k1=-0.05, shift=(-3.25, 0.5), rot=-0.004)]
    for side in range(2):
        ctx.set_rectify_map(1, side, *own[side])
        ctx.set_rectify_map(2, side, None, None)
    for side in range(2):
        assert same(0, side, shared[side]) and same(1, side, RR.fixed(*own[side])) and len(ctx.rectify_map_fixed(2, side)[0]) == 0
    L, R = S["frames"][0]
    ctx.process_host([(L, R)] * 3)
    want = [[O().prepare(L, *S["maps"][0]), O().prepare(R, *S["maps"][1])], [O().prepare(L, *own[0]), O().prepare(R, *own[1])], [L, R]]
    for lane in range(3):
        for side in range(2):
            assert (ctx.level(lane, side, 0) == want[lane][side]).all(), (lane, side)
    # another size while maps exist: SVO_ERR_ARG with a text, and every table is what it was
    other = RR.to_ctypes(RR.calibration_mild(0, 160, 120, 75.0))
    assert ctx.L.svo_set_stereo_calibration(ctx.h, -1, C.byref(other), 1, None) == -2 and ctx.L.svo_last_error(ctx.h)
    assert ctx.L.svo_set_stereo_calibration(ctx.h, 0, C.byref(other), 1, None) == -2
    s0 = S["sides"][0]
    assert ctx.L.svo_set_undistort_rectify(ctx.h, 0, 0, C.byref(CameraModel.make(*s0["cam"])), s0["R"].ctypes.data_as(C.c_void_p), s0["P"].ctypes.data_as(C.c_void_p), 160, 120) == -2
    for side in range(2):
        assert same(0, side, shared[side]) and same(1, side, RR.fixed(*own[side])) and len(ctx.rectify_map_fixed(2, side)[0]) == 0
    # a refused calibration changes nothing either, and says why
    bad = RR.to_ctypes(dict(S["cal"], alpha=0.5))
    assert ctx.L.svo_set_stereo_calibration(ctx.h, -1, C.byref(bad), 1, None) == -3 and b"alpha" in ctx.L.svo_last_error(ctx.h)
    assert same(0, 0, shared[0]) and len(ctx.rectify_map_fixed(2, 0)[0]) == 0
    # lane = -1 again brings every lane back to one table
    ctx.set_stereo_calibration(RR.to_ctypes(S["cal"]), lane=-1, set_camera=False)
    for lane in range(3):
        for side in range(2):
            assert same(lane, side, shared[side])
    ctx.close()


def test_one_frame_with_an_idle_lane():
    """svo_process_lanes with lane 1 idle: the active lanes are rectified by the shared table, the idle one is as if not called"""
    S = mild()
    ctx, p = context(3)
    cam = ctx.set_stereo_calibration(RR.to_ctypes(S["cal"]), lane=-1, set_camera=True).cam
    L, R = S["frames"][0]
    ctx.process_host([(L, R), None, (L, R)], active=[0, 2])
    want = [O().prepare(L, *S["maps"][0]), O().prepare(R, *S["maps"][1])]
    orc = O().Oracle(p)
    ro = orc.process(want[0], want[1], cam)
    for lane in (0, 2):
        for side in range(2):
            assert (ctx.level(lane, side, 0) == want[side]).all(), (lane, side)
        assert_same_frame(ctx, lane, orc, ctx.result(lane), ro, "lane=%d" % lane)
    r1 = ctx.result(1)
    assert r1.detected_left[0] == 0 and r1.detected_right[0] == 0 and not r1.valid
    ctx.close()


def test_one_frame_with_graphs_on():
    """svo_use_graphs switched on after the calibration: the frame is rectified and computed as without it"""
    S = mild()
    ctx, p = context(3)
    cam = ctx.set_stereo_calibration(RR.to_ctypes(S["cal"]), lane=-1, set_camera=True).cam
    ctx.use_graphs(True)
    L, R = S["frames"][0]
    ctx.process_host([(L, R)] * 3)
    want = [O().prepare(L, *S["maps"][0]), O().prepare(R, *S["maps"][1])]
    orc = O().Oracle(p)
    ro = orc.process(want[0], want[1], cam)
    for lane in range(3):
        for side in range(2):
            assert (ctx.level(lane, side, 0) == want[side]).all(), (lane, side)
        assert_same_frame(ctx, lane, orc, ctx.result(lane), ro, "graphs lane=%d" % lane)
    ctx.close()
