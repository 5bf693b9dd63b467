"""svo_lk_track on the GPU, held bit for bit to its definition (tests/lk_ref.py) on the hand-built scenes of tests/lk_scenes.py: every
pyramid level byte for byte, next_pts as float32 bit patterns, status and err for every point -- nothing left out, no tolerance.
Then the layouts (device images in place, one call against many), every refusal, the absence of side effects on the frame pipeline,
the kernel-time names and the read contract of strided device images."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import LkImage, LkJob, LkParams, StereoCamera, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_scenes as LS                                                                 # noqa: E402

pytestmark = pytest.mark.gpu

SCENE_NAMES = [s.name for s in LS.scenes()]


def make_ctx(**kw):
    cfg = dict(n_lanes=2, max_w=321, max_h=243, max_kps=LS.MAX_KPS, max_cand=1 << 15)         # a call takes 4 * 2 * 1 = 8 jobs
    cfg.update(kw)
    return hip.Context(**cfg)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


def lk_params(scene):
    p = hip.default_lk_params()
    for k, v in scene.params.items():
        setattr(p, k, v)
    return p


def assert_equals_walk(name, got, what=""):
    ref = LS.reference(name)
    assert len(got) == len(ref)
    for j, ((o, s, e), (ro, rs, re_, traces, pre)) in enumerate(zip(got, ref)):
        tag = "%s job %d %s" % (name, j, what)
        assert o.shape == ro.shape and s.shape == rs.shape and e.shape == re_.shape, tag
        bad = np.flatnonzero((o.view(np.uint32) != ro.view(np.uint32)).any(axis=1) | (s != rs) | (e.view(np.uint32) != re_.view(np.uint32)))
        assert bad.size == 0, "%s: %d of %d points differ, first %d: device %s %d %r, walk %s %d %r, trace %s" % (
            tag, bad.size, len(s), bad[0], o[bad[0]], s[bad[0]], e[bad[0]], ro[bad[0]], rs[bad[0]], re_[bad[0]], traces[bad[0]])


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_equals_the_walk(ctx, name):
    scene = LS.scene(name)
    got = ctx.lk_track(scene.jobs, lk_params(scene))
    assert_equals_walk(name, got)
    # every level of both images, byte for byte; the level behind the last does not exist
    for j, (ro, rs, re_, traces, pre) in enumerate(LS.reference(name)):
        for which in (0, 1):
            for lvl, want in enumerate(pre.pyr[which]):
                have = ctx.lk_level(j, which, lvl)
                assert have is not None and have.shape == want.shape and have.tobytes() == want.tobytes(), (name, j, which, lvl)
            assert ctx.lk_level(j, which, len(pre.pyr[which])) is None
    assert ctx.lk_level(len(scene.jobs), 0, 0) is None


def _on_device(jobs):
    """every image in device memory with the row stride it has on the host: ([(prev, next, pts, init)] with (address, w, h, stride), keep)"""
    import torch
    keep, out = [], []
    for prev, nxt, pts, init in jobs:
        recs = []
        for im in (prev, nxt):
            h, w = im.shape
            stride = im.strides[0]
            host = np.zeros((h, stride), np.uint8)
            host[:, :w] = im
            t = torch.from_numpy(host).cuda()
            keep.append(t)
            recs.append((t.data_ptr(), w, h, stride))
        out.append((recs[0], recs[1], pts, init))
    torch.cuda.synchronize()
    return out, keep


def test_device_images_in_place_equal_host_images(ctx):
    scene = LS.scene("mixed_call")
    dev_jobs, keep = _on_device(scene.jobs)
    got = ctx.lk_track(dev_jobs, lk_params(scene), device=True)
    assert_equals_walk("mixed_call", got, "(device images)")
    lvl0 = ctx.lk_level(1, 1, 0)                                     # level 0 of a device image is read where the caller holds it
    assert lvl0.tobytes() == np.ascontiguousarray(scene.jobs[1][1]).tobytes()
    assert ctx.lk_level(1, 1, 1).tobytes() == LS.reference("mixed_call")[1][4].pyr[1][1].tobytes()
    host = ctx.lk_track(scene.jobs, lk_params(scene))
    for a, b in zip(got, host):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # page-locked host images
    import torch
    small = LS.scene("count_5")
    prev, nxt, pts, init = small.jobs[0]
    tp, tn = (torch.from_numpy(np.ascontiguousarray(im)).pin_memory() for im in (prev, nxt))
    assert_equals_walk("count_5", ctx.lk_track([(tp.numpy(), tn.numpy(), pts)], lk_params(small), pinned=True), "(pinned images)")


def test_one_call_of_five_jobs_equals_five_calls(ctx):
    scene = LS.scene("mixed_call")
    p = lk_params(scene)
    together = ctx.lk_track(scene.jobs, p)
    for j, job in enumerate(scene.jobs):
        (alone,) = ctx.lk_track([job], p)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(alone, together[j])), j
    assert ctx.lk_track([], p) == []


def _raw_job(prev, nxt, pts, out, status, err, init=None):
    j = LkJob()
    j.prev = LkImage(prev.ctypes.data, prev.shape[1], prev.shape[0], prev.strides[0])
    j.next = LkImage(nxt.ctypes.data, nxt.shape[1], nxt.shape[0], nxt.strides[0])
    j.pts, j.init, j.n = pts.ctypes.data, (init.ctypes.data if init is not None else None), len(pts)
    j.next_pts, j.status, j.err = out.ctypes.data, status.ctypes.data, err.ctypes.data
    return j


def test_refusals_leave_the_outputs_untouched(ctx):
    ARG, CAP = -2, -5
    prev, nxt = LS.texture(96, 80), LS.shifted(96, 80, 0.6, 0.4)
    pts = LS.grid_points(96, 80, 4, 20)
    out, status, err = np.full((4, 2), 7.5, np.float32), np.full(4, 9, np.uint8), np.full(4, -3.0, np.float32)
    keep = [prev, nxt, pts]
    L, h = ctx.L, ctx.h

    def call(job=None, params=None, flags=0, n_jobs=1, jobs=None):
        arr = jobs if jobs is not None else ((LkJob * 1)(job) if job is not None else None)
        rc = L.svo_lk_track(h, arr, n_jobs, C.byref(params) if params is not None else None, C.c_uint32(flags))
        return rc, L.svo_last_error(h).decode()

    def good():
        return _raw_job(prev, nxt, pts, out, status, err)

    def par(**kw):
        p = hip.default_lk_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = []
    for field in ("pts", "next_pts", "status"):
        j = good(); setattr(j, field, None); cases.append((field + " NULL", j, None, 0, ARG))
    j = good(); j.prev.data = None; cases.append(("prev.data NULL", j, None, 0, ARG))
    j = good(); j.next.data = None; cases.append(("next.data NULL", j, None, 0, ARG))
    for win in (3, 20, 33):
        cases.append(("win %d" % win, good(), par(win=win), 0, ARG))
    for ml in (-1, 6):
        cases.append(("max_level %d" % ml, good(), par(max_level=ml), 0, ARG))
    for it in (0, 101):
        cases.append(("max_iters %d" % it, good(), par(max_iters=it), 0, ARG))
    j = good(); j.n = -1; cases.append(("negative n", j, None, 0, ARG))
    j = good(); j.next.w = 95; cases.append(("sizes differ", j, None, 0, ARG))
    j = good(); j.next.h = 79; cases.append(("sizes differ", j, None, 0, ARG))
    j = good(); j.prev.stride = 95; cases.append(("stride below a row", j, None, 0, ARG))
    j = good(); j.next.stride = (1 << 31) // 80 + 1; cases.append(("device span", j, None, hip.FLAG_DEVICE_IMAGES, ARG))
    cases.append(("unknown flag", good(), None, hip.FLAG_BGR_IMAGES, ARG))
    cases.append(("unknown flag", good(), None, hip.RUN_DETECT, ARG))
    j = good(); j.n = LS.MAX_KPS + 1; cases.append(("n above max_kps", j, None, 0, CAP))
    j = good(); j.prev.w = j.next.w = 322; j.prev.stride = j.next.stride = 322; cases.append(("wider than max_w", j, None, 0, CAP))
    j = good(); j.prev.h = j.next.h = 244; cases.append(("taller than max_h", j, None, 0, CAP))
    for what, job, params, flags, want in cases:
        rc, text = call(job, params, flags)
        assert rc == want and text, (what, rc, text)
        assert (out == 7.5).all() and (status == 9).all() and (err == -3.0).all(), what
    many = (LkJob * 9)(*[good() for _ in range(9)])
    rc, text = call(jobs=many, n_jobs=9)
    assert rc == CAP and "9" in text and "8" in text, (rc, text)
    rc, text = call(n_jobs=1)                                         # jobs == NULL
    assert rc == ARG and text
    assert L.svo_lk_track(h, None, -1, None, 0) == ARG and L.svo_last_error(h)
    assert (out == 7.5).all() and (status == 9).all() and (err == -3.0).all()
    # n_jobs = 0 and n = 0 are fine; err may be NULL; and after all the refusals a good call gives the walk's answer
    assert L.svo_lk_track(h, None, 0, None, 0) == 0
    j = good(); j.n = 0; j.pts = j.next_pts = j.status = j.err = None
    assert call(j)[0] == 0 and (out == 7.5).all()
    j = good(); j.err = None
    assert call(j)[0] == 0 and (err == -3.0).all() and status.tolist() != [9] * 4
    (want,) = ctx.lk_track([(prev, nxt, pts)])
    assert out.tobytes() == want[0].tobytes() and status.tobytes() == want[1].tobytes()
    del keep


def test_an_lk_call_leaves_the_frame_pipeline_alone(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    scene = LS.scene("count_65")
    records = []
    for with_lk in (False, True):
        c = hip.Context(n_lanes=1, max_w=max(W, 96), max_h=max(H, 80), max_kps=1024, max_cand=1 << 15)
        c.set_params(p); c.set_camera(cam)
        rec = []
        for t in range(3):
            if with_lk and t > 0:
                assert_equals_walk("count_65", c.lk_track(scene.jobs, lk_params(scene)), "(between frames)")
            c.process_host([(g["L%d" % t], g["R%d" % t])])
            k, d = c.keypoints(0, 0, 0)
            rec.append((bytes(c.result(0)), k.tobytes(), d.tobytes(), c.matches(0).tobytes(), c.tracked(0).tobytes()))
        records.append(rec)
        c.close()
    assert records[0] == records[1]


def test_kernel_time_names(ctx):
    scene = LS.scene("count_65")
    never = make_ctx(kernel_times=True)
    before, before_all = never.kernel_times(), never.kernel_times(appended=True)
    assert "lk_track" not in before_all and "lk_pyrdown" not in before_all
    never.lk_track(scene.jobs, lk_params(scene))
    after, after_all = never.kernel_times(), never.kernel_times(appended=True)
    assert list(after) == list(before), "the frame's names are the ones they always were"
    assert list(after_all) == list(before_all) + ["lk_pyrdown", "lk_track"]
    assert after_all["lk_pyrdown"][1] == 1 and after_all["lk_track"][1] == 1 and after_all["lk_track"][0] > 0
    assert all(after_all[k][1] == 0 for k in before_all)
    never.kernel_times_select("lk_track")
    never.kernel_times_select(None)
    never.close()


def test_read_contract_of_strided_device_images(ctx):
    """rows with a stride larger than w hold a poison pattern behind the pixels, and guard rows of poison lie before and behind each
    image: the results equal those of the tight layout, and the buffers are as they were"""
    import torch
    scene = LS.scene("win_31")                                       # the widest tiles
    prev, nxt, pts, init = scene.jobs[0]
    h, w = prev.shape
    p = lk_params(scene)
    (tight,) = ctx.lk_track([(prev, nxt, pts)], p)
    assert_equals_walk("win_31", [tight])
    rng = np.random.default_rng(5)
    bufs, recs = [], []
    for im, stride in ((prev, w + 1), (nxt, w + 63)):
        host = rng.integers(0, 256, ((h + 2) * stride,), dtype=np.uint8)          # poison everywhere ...
        view = host.reshape(h + 2, stride)
        view[1:h + 1, :w] = im                                                      # ... except the pixels
        t = torch.from_numpy(host).cuda()
        bufs.append((t, host))
        recs.append((t.data_ptr() + stride, w, h, stride))
    torch.cuda.synchronize()
    (strided,) = ctx.lk_track([(recs[0], recs[1], pts)], p, device=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(strided, tight))
    for t, host in bufs:
        assert t.cpu().numpy().tobytes() == host.tobytes()
