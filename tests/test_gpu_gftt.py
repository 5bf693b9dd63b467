"""svo_gftt_detect on the GPU, held bit for bit to its definition (tests/gftt_ref.py) on the hand-built scenes of tests/gftt_scenes.py: the
response map as float32 bit patterns, pts, response and the three info words -- nothing left out, no tolerance.  Then the layouts
(one call against many, device images in place, page-locked images), every refusal, the absence of side effects on the frame
pipeline, the kernel-time names and the composition with svo_lk_track."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import GfttJob, LkImage, StereoCamera, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gftt_ref as G                                                                   # noqa: E402
import gftt_scenes as GS                                                               # noqa: E402
import lk_ref                                                                          # noqa: E402

pytestmark = pytest.mark.gpu

SCENE_NAMES = [s.name for s in GS.scenes()]


def make_ctx(**kw):
    cfg = dict(n_lanes=2, max_w=321, max_h=243, max_kps=GS.MAX_KPS, max_cand=GS.MAX_CAND)     # a call takes 4 * 2 * 1 = 8 jobs
    cfg.update(kw)
    return hip.Context(**cfg)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def small_ctx():
    c = make_ctx(max_cand=256)
    yield c
    c.close()


def gftt_params(scene):
    p = hip.default_gftt_params()
    for k, v in scene.params.items():
        setattr(p, k, v)
    return p


def assert_equals_walk(name, got, what="", jobs=None):
    ref = GS.reference(name)
    if jobs is not None:
        ref = [ref[j] for j in jobs]
    assert len(got) == len(ref)
    for j, ((pts, resp, n_cand, status), (rp, rr, rinfo, rmap)) in enumerate(zip(got, ref)):
        tag = "%s job %d %s" % (name, j, what)
        assert (len(pts), n_cand, status) == rinfo, "%s: info device %r, walk %r" % (tag, (len(pts), n_cand, status), rinfo)
        assert pts.shape == rp.shape and resp.shape == rr.shape, tag
        bad = np.flatnonzero((pts.view(np.uint32) != rp.view(np.uint32)).any(axis=1) | (resp.view(np.uint32) != rr.view(np.uint32)))
        assert bad.size == 0, "%s: %d of %d corners differ, first %d: device %s %r, walk %s %r" % (
            tag, bad.size, len(rp), bad[0], pts[bad[0]], resp[bad[0]], rp[bad[0]], rr[bad[0]])


def assert_maps_equal_walk(c, name):
    for j, (rp, rr, rinfo, rmap) in enumerate(GS.reference(name)):
        have = c.gftt_response(j)
        assert have is not None and have.shape == rmap.shape, (name, j)
        bad = np.argwhere(have.view(np.uint32) != rmap.view(np.uint32))
        assert len(bad) == 0, "%s job %d: %d response pixels differ, first (y, x) = %s: device %r, walk %r" % (
            name, j, len(bad), bad[0], have[tuple(bad[0])], rmap[tuple(bad[0])])
    assert c.gftt_response(len(GS.reference(name))) is None


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_equals_the_walk(ctx, small_ctx, name):
    scene = GS.scene(name)
    c = small_ctx if scene.max_cand == 256 else ctx
    assert scene.max_cand in (None, 256)
    got = c.gftt_detect(scene.jobs, gftt_params(scene))
    assert_equals_walk(name, got)
    assert_maps_equal_walk(c, name)


def test_one_call_of_five_jobs_equals_five_calls(ctx):
    scene = GS.scene("mixed_call")
    p = gftt_params(scene)
    together = ctx.gftt_detect(scene.jobs, p)
    assert_equals_walk("mixed_call", together)
    for j, job in enumerate(scene.jobs):
        (alone,) = ctx.gftt_detect([job], p)
        assert alone[0].tobytes() == together[j][0].tobytes() and alone[1].tobytes() == together[j][1].tobytes() and alone[2:] == together[j][2:], j
    assert ctx.gftt_detect([], p) == []


def test_overflow_leaves_the_other_jobs_alone(small_ctx):
    over, room = GS.scene("overflow_lattice"), GS.scene("threshold_one_level_stronger_kept")
    p = gftt_params(room)
    got = small_ctx.gftt_detect([room.jobs[0], over.jobs[0], room.jobs[0]], p)
    assert_equals_walk(room.name, [got[0]])
    assert_equals_walk(room.name, [got[2]])
    ref = G.detect(over.jobs[0][0], None, GS.MAX_KPS, room.ref_params(), cand_cap=1024)
    assert (len(got[1][0]), got[1][2], got[1][3]) == ref[2] and ref[2][2] == 1


def _on_device(img, stride, offset, rng):
    """the image inside a poisoned device buffer: `offset` bytes in, rows `stride` apart; -> ((address, w, h, stride), tensor, host copy)"""
    import torch
    h, w = img.shape
    host = rng.integers(0, 256, (offset + h * stride + 64,), dtype=np.uint8)
    view = host[offset:offset + h * stride].reshape(h, stride)
    view[:, :w] = img
    t = torch.from_numpy(host).cuda()
    return (t.data_ptr() + offset, w, h, stride), t, host


def test_device_images_in_place_and_pinned_images(ctx):
    import torch
    scene = GS.scene("mixed_call")
    p = gftt_params(scene)
    rng = np.random.default_rng(5)
    jobs, keep = [], []
    for k, (img, seeds, cap) in enumerate(scene.jobs):
        rec, t, host = _on_device(img, img.shape[1] + (0, 1, 63, 7, 3)[k], (0, 1, 3, 64, 5)[k], rng)     # odd strides and byte alignments
        jobs.append((rec, seeds, cap)); keep.append((t, host))
    torch.cuda.synchronize()
    got = ctx.gftt_detect(jobs, p, device=True)
    assert_equals_walk("mixed_call", got, "(device images)")
    assert_maps_equal_walk(ctx, "mixed_call")
    for t, host in keep:                                              # nothing of the caller's was written
        assert t.cpu().numpy().tobytes() == host.tobytes()
    # host images whose rows are not contiguous with each other, and page-locked ones
    wide = np.zeros((243, 400), np.uint8); wide[:, :321] = scene.jobs[0][0]
    assert_equals_walk("mixed_call", ctx.gftt_detect([(wide[:, :321], scene.jobs[0][1], scene.jobs[0][2])], p), "(strided host image)", jobs=[0])
    pinned = torch.from_numpy(np.ascontiguousarray(scene.jobs[3][0])).pin_memory()
    assert_equals_walk("mixed_call", ctx.gftt_detect([(pinned.numpy(), scene.jobs[3][1], scene.jobs[3][2])], p, pinned=True), "(pinned image)", jobs=[3])


def test_refusals_leave_the_outputs_untouched(ctx):
    ARG, CAP = -2, -5
    scene = GS.scene("distance_exact_kept")
    img = scene.jobs[0][0]
    seeds = np.array([[5, 5], [9, 9]], np.float32)
    pts, resp, info = np.full((8, 2), 7.5, np.float32), np.full(8, -3.0, np.float32), np.full(3, 99, np.int32)
    L, h = ctx.L, ctx.h

    def untouched():
        return (pts == 7.5).all() and (resp == -3.0).all() and (info == 99).all()

    def good():
        j = GfttJob()
        j.img = LkImage(img.ctypes.data, img.shape[1], img.shape[0], img.strides[0])
        j.seeds, j.n_seeds, j.cap = seeds.ctypes.data, 2, 8
        j.pts, j.response, j.info = pts.ctypes.data, resp.ctypes.data, info.ctypes.data
        return j

    def call(job=None, params=None, flags=0, n_jobs=1, jobs=None):
        arr = jobs if jobs is not None else ((GfttJob * 1)(job) if job is not None else None)
        rc = L.svo_gftt_detect(h, arr, n_jobs, C.byref(params) if params is not None else None, C.c_uint32(flags))
        return rc, L.svo_last_error(h).decode()

    def par(**kw):
        p = hip.default_gftt_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    cases = []
    for field in ("pts", "info", "seeds"):
        j = good(); setattr(j, field, None); cases.append((field + " NULL", j, None, 0, ARG))
    j = good(); j.img.data = None; cases.append(("img.data NULL", j, None, 0, ARG))
    for block in (1, 4, 9):
        cases.append(("block %d" % block, good(), par(block=block), 0, ARG))
    for md in (-1, 256):
        cases.append(("min_distance %d" % md, good(), par(min_distance=md), 0, ARG))
    for q in (0.0, -1.0, 1.5, float("nan"), float("inf")):
        cases.append(("quality %r" % q, good(), par(quality=q), 0, ARG))
    cases.append(("negative max_corners", good(), par(max_corners=-1), 0, ARG))
    j = good(); j.cap = -1; cases.append(("negative cap", j, None, 0, ARG))
    j = good(); j.n_seeds = -1; cases.append(("negative n_seeds", j, None, 0, ARG))
    j = good(); j.img.w = 7; cases.append(("side below 8", j, None, 0, ARG))
    j = good(); j.img.h = 7; cases.append(("side below 8", j, None, 0, ARG))
    j = good(); j.img.stride = img.shape[1] - 1; cases.append(("stride below a row", j, None, 0, ARG))
    j = good(); j.img.stride = (1 << 31) // img.shape[0] + 1; cases.append(("device span", j, None, hip.FLAG_DEVICE_IMAGES, ARG))
    cases.append(("unknown flag", good(), None, hip.FLAG_BGR_IMAGES, ARG))
    cases.append(("unknown flag", good(), None, hip.RUN_DETECT, ARG))
    cases.append(("both image flags", good(), None, hip.FLAG_DEVICE_IMAGES | hip.FLAG_PINNED_IMAGES, ARG))
    j = good(); j.cap = GS.MAX_KPS + 1; cases.append(("cap above max_kps", j, None, 0, CAP))
    j = good(); j.n_seeds = GS.MAX_KPS + 1; cases.append(("n_seeds above max_kps", j, None, 0, CAP))
    cases.append(("max_corners above max_kps", good(), par(max_corners=GS.MAX_KPS + 1), 0, CAP))
    j = good(); j.img.w = 322; j.img.stride = 322; cases.append(("wider than max_w", j, None, 0, CAP))
    j = good(); j.img.h = 244; cases.append(("taller than max_h", j, None, 0, CAP))
    for what, job, params, flags, want in cases:
        rc, text = call(job, params, flags)
        assert rc == want and text, (what, rc, text)
        assert untouched(), what
    many = (GfttJob * 9)(*[good() for _ in range(9)])
    rc, text = call(jobs=many, n_jobs=9)
    assert rc == CAP and "9" in text and "8" in text and untouched(), (rc, text)
    rc, text = call(n_jobs=1)                                         # jobs == NULL
    assert rc == ARG and text
    assert L.svo_gftt_detect(h, None, -1, None, 0) == ARG and L.svo_last_error(h)
    assert untouched()
    # n_jobs = 0 is fine; response may be NULL; cap = 0 needs no pts; after all the refusals a good call gives the walk's answer
    assert L.svo_gftt_detect(h, None, 0, None, 0) == 0 and untouched()
    j = good(); j.cap = 0; j.pts = None; j.response = None
    assert call(j)[0] == 0 and (pts == 7.5).all() and info.tolist() == [0, 4, 0]
    j = good(); j.response = None
    assert call(j)[0] == 0 and (resp == -3.0).all() and info.tolist() == [4, 4, 0]
    assert call(good())[0] == 0
    want = G.detect(img, seeds, 8, G.GfttParams())
    assert pts[:4].tobytes() == want[0].tobytes() and resp[:4].tobytes() == want[1].tobytes() and (pts[4:] == 7.5).all() and (resp[4:] == -3.0).all()


def test_a_gftt_call_leaves_the_frame_pipeline_alone(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    scene = GS.scene("seeds_exact_and_inside")
    records = []
    for with_gftt in (False, True):
        c = hip.Context(n_lanes=1, max_w=max(W, 321), max_h=max(H, 243), max_kps=1024, max_cand=GS.MAX_CAND)
        c.set_params(p); c.set_camera(cam)
        rec = []
        for t in range(3):
            if with_gftt and t > 0:
                assert_equals_walk(scene.name, c.gftt_detect(scene.jobs, gftt_params(scene)), "(between frames)")
            c.process_host([(g["L%d" % t], g["R%d" % t])])
            k, d = c.keypoints(0, 0, 0)
            rec.append((bytes(c.result(0)), k.tobytes(), d.tobytes(), c.matches(0).tobytes(), c.tracked(0).tobytes()))
        records.append(rec)
        c.close()
    assert records[0] == records[1]


def test_kernel_time_names():
    scene = GS.scene("distance_exact_kept")
    names = ["gftt_response", "gftt_candidates", "gftt_select"]
    c = make_ctx(kernel_times=True)
    before, before_all = c.kernel_times(), c.kernel_times(appended=True)
    assert not set(names) & set(before_all)
    c.gftt_detect(scene.jobs, gftt_params(scene))
    after, after_all = c.kernel_times(), c.kernel_times(appended=True)
    assert list(after) == list(before), "the frame's names are the ones they always were"
    assert list(after_all) == list(before_all) + names
    assert all(after_all[k][1] == 1 and after_all[k][0] > 0 for k in names) and all(after_all[k][1] == 0 for k in before_all)
    # beside an LK call: the LK names stay last
    img = scene.jobs[0][0]
    c.lk_track([(img, img, np.array([[40, 30]], np.float32))])
    assert list(c.kernel_times(appended=True)) == list(before_all) + names + ["lk_pyrdown", "lk_track"]
    c.kernel_times_select("gftt_select")
    c.kernel_times_select(None)
    c.close()
    only_lk = make_ctx(kernel_times=True)
    only_lk.lk_track([(img, img, np.array([[40, 30]], np.float32))])
    assert list(only_lk.kernel_times(appended=True)) == list(before_all) + ["lk_pyrdown", "lk_track"]
    only_lk.close()


def test_detected_corners_feed_the_tracker(ctx):
    """corners of an image, followed into its copy shifted by (2, 1) pixels: the device's chain equals the two walks chained"""
    prev = GS.blocks(200, 160, 9, 41)
    nxt = np.roll(prev, (1, 2), axis=(0, 1))
    p = hip.default_gftt_params(); p.max_corners = 40
    ((pts, resp, n_cand, status),) = ctx.gftt_detect([(prev, None, GS.MAX_KPS)], p)
    want = G.detect(prev, None, GS.MAX_KPS, G.GfttParams(max_corners=40))
    assert pts.tobytes() == want[0].tobytes() and resp.tobytes() == want[1].tobytes() and len(pts) == 40
    ((out, st, err),) = ctx.lk_track([(prev, nxt, pts)])
    ro, rs, re_ = lk_ref.track(prev, nxt, want[0], None, lk_ref.LkParams())[:3]
    assert out.tobytes() == np.asarray(ro, np.float32).tobytes() and st.tobytes() == np.asarray(rs, np.uint8).tobytes()
    assert err.tobytes() == np.asarray(re_, np.float32).tobytes() and st.sum() > 0
