"""svo_lk_track_rows on the GPU, held bit for bit to its definition (tests/lk_row_ref.py) on the hand-built scenes of
tests/lk_row_scenes.py: next_pts as float32 bit patterns, status and err for every point -- nothing left out, no tolerance.  Then the
layouts (host, pinned, device images in place), every refusal of svo_lk_track made again with the same status, svo_lk_track around a
rows call, the pyramid getter and the kernel-time name."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import LkImage, LkJob

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_row_scenes as RS                                                             # noqa: E402
import lk_scenes as LS                                                                 # noqa: E402

pytestmark = pytest.mark.gpu

SCENE_NAMES = [s.name for s in RS.scenes()]


def make_ctx(**kw):
    cfg = dict(n_lanes=2, max_w=321, max_h=243, max_kps=RS.MAX_KPS, max_cand=1 << 15)         # a call takes 4 * 2 * 1 = 8 jobs
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
    ref = RS.reference(name)
    assert len(got) == len(ref)
    for j, ((o, s, e), (ro, rs, re_, traces, pre)) in enumerate(zip(got, ref)):
        tag = "%s job %d %s" % (name, j, what)
        assert o.shape == ro.shape and s.shape == rs.shape and e.shape == re_.shape, tag
        bad = np.flatnonzero((o.view(np.uint32) != ro.view(np.uint32)).any(axis=1) | (s != rs) | (e.view(np.uint32) != re_.view(np.uint32)))
        assert bad.size == 0, "%s: %d of %d points differ, first %d: device %s %d %r, walk %s %d %r, trace %s" % (
            tag, bad.size, len(s), bad[0], o[bad[0]], s[bad[0]], e[bad[0]], ro[bad[0]], rs[bad[0]], re_[bad[0]], traces[bad[0]])


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_equals_the_walk(ctx, name):
    scene = RS.scene(name)
    got = ctx.lk_track_rows(scene.jobs, lk_params(scene))
    assert_equals_walk(name, got)
    # svo_debug_lk_get_level answers for the call as for svo_lk_track: the top level of both images, byte for byte
    for j, (ro, rs, re_, traces, pre) in enumerate(RS.reference(name)):
        for which in (0, 1):
            top = len(pre.pyr[which]) - 1
            have = ctx.lk_level(j, which, top)
            assert have is not None and have.tobytes() == pre.pyr[which][top].tobytes(), (name, j, which)
            assert ctx.lk_level(j, which, top + 1) is None


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


def test_host_pinned_and_device_images_give_the_same_bytes(ctx):
    import torch
    scene = RS.scene("mixed_call")
    dev_jobs, keep = _on_device(scene.jobs)
    got = ctx.lk_track_rows(dev_jobs, lk_params(scene), device=True)
    assert_equals_walk("mixed_call", got, "(device images)")
    assert ctx.lk_level(1, 1, 0).tobytes() == np.ascontiguousarray(scene.jobs[1][1]).tobytes()      # read where the caller holds it
    host = ctx.lk_track_rows(scene.jobs, lk_params(scene))
    for a, b in zip(got, host):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for name in ("count_5", "leaves_strip"):
        small = RS.scene(name)
        prev, nxt, pts, init = small.jobs[0]
        tp, tn = (torch.from_numpy(np.ascontiguousarray(im)).pin_memory() for im in (prev, nxt))
        assert_equals_walk(name, ctx.lk_track_rows([(tp.numpy(), tn.numpy(), pts, init)], lk_params(small), pinned=True), "(pinned images)")
    # a device image whose rows are wider than w, poison behind the pixels: the strip reads inside the rows only
    scene = RS.scene("leaves_strip")
    prev, nxt, pts, init = scene.jobs[0]
    h, w = prev.shape
    rng = np.random.default_rng(5)
    bufs, recs = [], []
    for im, stride in ((prev, w + 1), (nxt, w + 63)):
        hostbuf = rng.integers(0, 256, ((h + 2) * stride,), dtype=np.uint8)
        hostbuf.reshape(h + 2, stride)[1:h + 1, :w] = im
        t = torch.from_numpy(hostbuf).cuda()
        bufs.append(t)
        recs.append((t.data_ptr() + stride, w, h, stride))
    torch.cuda.synchronize()
    assert_equals_walk("leaves_strip", ctx.lk_track_rows([(recs[0], recs[1], pts, init)], lk_params(scene), device=True), "(strided device images)")


def _raw_job(prev, nxt, pts, out, status, err, init=None):
    j = LkJob()
    j.prev = LkImage(prev.ctypes.data, prev.shape[1], prev.shape[0], prev.strides[0])
    j.next = LkImage(nxt.ctypes.data, nxt.shape[1], nxt.shape[0], nxt.strides[0])
    j.pts, j.init, j.n = pts.ctypes.data, (init.ctypes.data if init is not None else None), len(pts)
    j.next_pts, j.status, j.err = out.ctypes.data, status.ctypes.data, err.ctypes.data
    return j


def test_every_refusal_of_lk_track_is_made_with_the_same_status(ctx):
    ARG, CAP = -2, -5
    prev, nxt = RS.texture(96, 80), RS.shifted(96, 80, 0.6, 0.0)
    pts = RS.grid_points(96, 80, 4, 20)
    out, status, err = np.full((4, 2), 7.5, np.float32), np.full(4, 9, np.uint8), np.full(4, -3.0, np.float32)
    L, h = ctx.L, ctx.h

    def call(entry, job=None, params=None, flags=0, n_jobs=1, jobs=None):
        arr = jobs if jobs is not None else ((LkJob * 1)(job) if job is not None else None)
        rc = getattr(L, entry)(h, arr, n_jobs, C.byref(params) if params is not None else None, C.c_uint32(flags))
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
    cases.append(("both image flags", good(), None, hip.FLAG_DEVICE_IMAGES | hip.FLAG_PINNED_IMAGES, ARG))
    j = good(); j.n = RS.MAX_KPS + 1; cases.append(("n above max_kps", j, None, 0, CAP))
    j = good(); j.prev.w = j.next.w = 322; j.prev.stride = j.next.stride = 322; cases.append(("wider than max_w", j, None, 0, CAP))
    j = good(); j.prev.h = j.next.h = 244; cases.append(("taller than max_h", j, None, 0, CAP))
    # the order: flags before parameters before the job count before the jobs
    j = good(); j.pts = None; cases.append(("flags first", j, par(win=4), 1 << 20, ARG))
    for what, job, params, flags, want in cases:
        rc, text = call("svo_lk_track_rows", job, params, flags)
        rc0, text0 = call("svo_lk_track", job, params, flags)
        assert rc == want and text, (what, rc, text)
        assert (rc0, text0) == (rc, text), (what, rc0, text0, text)              # the same decision, the same words
        assert (out == 7.5).all() and (status == 9).all() and (err == -3.0).all(), what
    assert "flags" in call("svo_lk_track_rows", cases[-1][1], cases[-1][2], cases[-1][3])[1]
    many = (LkJob * 9)(*[good() for _ in range(9)])
    rc, text = call("svo_lk_track_rows", jobs=many, n_jobs=9)
    assert rc == CAP and "9" in text and "8" in text, (rc, text)
    rc, text = call("svo_lk_track_rows", n_jobs=1)                      # jobs == NULL
    assert rc == ARG and text
    assert L.svo_lk_track_rows(h, None, -1, None, 0) == ARG and L.svo_last_error(h)
    assert L.svo_lk_track_rows(None, None, 0, None, 0) == ARG
    assert (out == 7.5).all() and (status == 9).all() and (err == -3.0).all()
    # n_jobs = 0 and n = 0 are fine; err may be NULL; and after all the refusals a good call gives the walk's answer
    assert L.svo_lk_track_rows(h, None, 0, None, 0) == 0
    j = good(); j.n = 0; j.pts = j.next_pts = j.status = j.err = None
    assert call("svo_lk_track_rows", j)[0] == 0 and (out == 7.5).all()
    j = good(); j.err = None
    assert call("svo_lk_track_rows", j)[0] == 0 and (err == -3.0).all() and status.tolist() != [9] * 4
    (want,) = ctx.lk_track_rows([(prev, nxt, pts)])
    assert out.tobytes() == want[0].tobytes() and status.tobytes() == want[1].tobytes()
    import lk_row_ref
    ro, rs, _, _ = lk_row_ref.track(prev, nxt, pts)
    assert out.tobytes() == ro.tobytes() and status.tobytes() == rs.tobytes()


def test_lk_track_around_a_rows_call_returns_what_it_returned_alone():
    c = make_ctx()
    two_d = LS.scene("count_65")
    alone = c.lk_track(two_d.jobs, lk_params(two_d))
    rows = RS.scene("fb_rows")
    assert_equals_walk("fb_rows", c.lk_track_rows(rows.jobs, lk_params(rows)))
    after = c.lk_track(two_d.jobs, lk_params(two_d))
    for a, b in zip(alone, after):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    ref = LS.reference("count_65")
    assert all(x.tobytes() == y.tobytes() for x, y in zip(after[0], ref[0][:3]))
    # the two trackers differ where they should: on the edge the rows call tracks, svo_lk_track does not
    edge = RS.scene("vertical_step_edge")
    (o2, s2, _), = c.lk_track(edge.jobs, lk_params(edge))
    (o1, s1, _), = c.lk_track_rows(edge.jobs, lk_params(edge))
    assert not s2.any() and s1.all()
    c.close()


def test_kernel_time_name():
    scene = RS.scene("count_65")
    c = make_ctx(kernel_times=True)
    before_all = c.kernel_times(appended=True)
    assert "lk_track_row" not in before_all
    c.lk_track(LS.scene("count_5").jobs, lk_params(LS.scene("count_5")))
    mid = c.kernel_times(appended=True)
    assert list(mid) == list(before_all) + ["lk_pyrdown", "lk_track"]
    c.lk_track_rows(scene.jobs, lk_params(scene))
    after = c.kernel_times(appended=True)
    assert list(after) == list(mid) + ["lk_track_row"]
    assert after["lk_track_row"][1] == 1 and after["lk_track_row"][0] > 0 and after["lk_track"][1] == 1 and after["lk_pyrdown"][1] == 2
    c.kernel_times_select("lk_track_row")
    c.kernel_times_select(None)
    c.close()
