"""svo_lk_track and svo_lk_track_rows under svo_lk_set_photometric(ctx, 1) on the GPU, held bit for bit to their definition
(tests/lk_photo_ref.py) on every scene of tests/lk_photo_scenes.py: next_pts as float32 bit patterns, status and err for every point of
every job -- nothing left out, no tolerance.  Then the layouts (host, pinned, device images with an odd stride), switching the mode
back, the pyramid getter, the refusals of the setter and the kernel-time names."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_photo_scenes as PS                                                           # noqa: E402
import lk_ref                                                                          # noqa: E402
import lk_row_ref                                                                      # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6
SCENE_NAMES = [s.name for s in PS.scenes()]


def make_ctx(**kw):
    cfg = dict(n_lanes=2, max_w=321, max_h=243, max_kps=PS.MAX_KPS, max_cand=1 << 15)         # a call takes 4 * 2 * 1 = 8 jobs
    cfg.update(kw)
    return hip.Context(**cfg)


@pytest.fixture(scope="module")
def ctx():
    c = make_ctx()
    assert c.lk_get_photometric() == 0
    c.lk_set_photometric(1)
    assert c.lk_get_photometric() == 1
    yield c
    c.close()


def lk_params(scene):
    p = hip.default_lk_params()
    for k, v in scene.params.items():
        setattr(p, k, v)
    return p


def track(c, rows, jobs, params, **kw):
    return (c.lk_track_rows if rows else c.lk_track)(jobs, params, **kw)


def assert_equals(got, ref, tag):
    assert len(got) == len(ref)
    for j, ((o, s, e), r) in enumerate(zip(got, ref)):
        ro, rs, re_ = r[0], r[1], r[2]
        traces = r[3] if len(r) > 3 else None
        assert o.shape == ro.shape and s.shape == rs.shape and e.shape == re_.shape, (tag, j)
        bad = np.flatnonzero((o.view(np.uint32) != ro.view(np.uint32)).any(axis=1) | (s != rs) | (e.view(np.uint32) != re_.view(np.uint32)))
        assert bad.size == 0, "%s job %d: %d of %d points differ, first %d: device %s %d %r, walk %s %d %r, trace %s" % (
            tag, j, bad.size, len(s), bad[0], o[bad[0]], s[bad[0]], e[bad[0]], ro[bad[0]], rs[bad[0]], re_[bad[0]], traces[bad[0]] if traces else None)


@pytest.mark.parametrize("rows", [False, True], ids=["2d", "rows"])
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_equals_the_walk(ctx, name, rows):
    scene = PS.scene(name)
    got = track(ctx, rows, scene.jobs, lk_params(scene))
    assert_equals(got, PS.reference(name, rows), "%s %s" % (name, "rows" if rows else "2d"))


@pytest.mark.parametrize("rows", [False, True], ids=["2d", "rows"])
def test_host_pinned_and_device_images_give_the_same_bytes(ctx, rows):
    import torch
    scene = PS.scene("mixed_call")
    ref = PS.reference("mixed_call", rows)
    # every image in device memory with an odd row stride and poison behind the pixels
    rng = np.random.default_rng(5)
    keep, dev_jobs = [], []
    for prev, nxt, pts, init in scene.jobs:
        recs = []
        for im, extra in ((prev, 1), (nxt, 63)):
            h, w = im.shape
            stride = w + extra + (w + extra + 1) % 2
            assert stride % 2 == 1
            buf = rng.integers(0, 256, ((h + 2) * stride,), dtype=np.uint8)
            buf.reshape(h + 2, stride)[1:h + 1, :w] = im
            t = torch.from_numpy(buf).cuda()
            keep.append(t)
            recs.append((t.data_ptr() + stride, w, h, stride))
        dev_jobs.append((recs[0], recs[1], pts, init))
    torch.cuda.synchronize()
    assert_equals(track(ctx, rows, dev_jobs, lk_params(scene), device=True), ref, "mixed_call (device images, odd strides)")
    pin_jobs = []
    for prev, nxt, pts, init in scene.jobs:
        tp, tn = (torch.from_numpy(np.ascontiguousarray(im)).pin_memory() for im in (prev, nxt))
        keep += [tp, tn]
        pin_jobs.append((tp.numpy(), tn.numpy(), pts, init))
    assert_equals(track(ctx, rows, pin_jobs, lk_params(scene), pinned=True), ref, "mixed_call (pinned images)")


def test_mode_0_after_mode_1_gives_the_plain_walks_bytes_and_the_pyramid_is_the_modes_alike():
    c = make_ctx()
    try:
        scene = PS.scene("gain_1.4_p20")
        prev, nxt, pts, _ = scene.jobs[0]
        P = scene.ref_params()
        pre = PS.prepared(scene.name)[0]
        plain = [lk_ref.track(prev, nxt, pts, None, P, prepared=pre)[:3]]
        plain_rows = [lk_row_ref.track(prev, nxt, pts, None, P, prepared=pre)[:3]]
        levels = {}
        for mode in (0, 1, 0):
            c.lk_set_photometric(mode)
            assert c.lk_get_photometric() == mode
            for rows, want in ((False, plain), (True, plain_rows)):
                got = track(c, rows, scene.jobs, lk_params(scene))
                assert_equals(got, PS.reference(scene.name, rows) if mode else want, "mode %d rows %d" % (mode, rows))
                # svo_debug_lk_get_level is the mode's alike: every level of both images, byte for byte
                for which in (0, 1):
                    for l in range(len(pre.pyr[which]) + 1):
                        have = c.lk_level(0, which, l)
                        if l == len(pre.pyr[which]):
                            assert have is None
                            continue
                        assert have.tobytes() == pre.pyr[which][l].tobytes(), (mode, rows, which, l)
                        assert levels.setdefault((which, l), have.tobytes()) == have.tobytes()
        # the scene needs the mode: the plain bytes are not the compensated ones
        assert plain[0][0].tobytes() != PS.reference(scene.name, False)[0][0].tobytes()
    finally:
        c.close()


def test_the_setter_refuses_other_modes_and_leaves_the_mode():
    c = make_ctx()
    L = hip.lib()
    try:
        assert c.lk_get_photometric() == 0                                  # no svo_set_params, no svo_klt_enable: accepted at once
        for keep in (0, 1):
            c.lk_set_photometric(keep)
            for mode in (2, -1):
                assert L.svo_lk_set_photometric(c.h, mode) == SVO_ERR_ARG
                assert ("mode %d" % mode).encode() in L.svo_last_error(c.h)
                assert L.svo_lk_get_photometric(c.h) == keep
        with pytest.raises(hip.SvoError):
            c.lk_set_photometric(2)
        assert c.lk_get_photometric() == 1
    finally:
        c.close()


def test_kernel_time_names_are_the_same_in_both_modes():
    scene = PS.scene("count_5")
    a, b = make_ctx(kernel_times=True), make_ctx(kernel_times=True)
    try:
        b.lk_set_photometric(1)
        assert list(a.kernel_times(appended=True)) == list(b.kernel_times(appended=True))      # the setter alone lists nothing
        for c in (a, b):
            c.lk_track(scene.jobs, lk_params(scene))
            c.lk_track_rows(scene.jobs, lk_params(scene))
        ka, kb = a.kernel_times(appended=True), b.kernel_times(appended=True)
        assert list(ka) == list(kb) and list(ka)[-3:] == ["lk_pyrdown", "lk_track", "lk_track_row"]
        assert [v[1] for v in ka.values()] == [v[1] for v in kb.values()]                      # the same launches were counted
        assert kb["lk_track"][1] == 1 and kb["lk_track_row"][1] == 1 and kb["lk_track"][0] > 0 and kb["lk_track_row"][0] > 0
    finally:
        a.close(); b.close()


def test_inside_a_captured_graph_the_setter_is_refused():
    import torch
    c = make_ctx()
    L = hip.lib()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    try:
        c.lk_set_photometric(1)
        c.set_stream(s.cuda_stream)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            g.capture_begin(capture_error_mode="thread_local")
            try:
                rc = L.svo_lk_set_photometric(c.h, 0)
                text = L.svo_last_error(c.h)
                inside = L.svo_lk_get_photometric(c.h)
            finally:
                g.capture_end()
        torch.cuda.synchronize()
        assert rc == SVO_ERR_STATE and b"capturing" in text and inside == 1
        c.set_stream(None)
        c.lk_set_photometric(0)                                             # outside the capture it is accepted again
        assert c.lk_get_photometric() == 0
    finally:
        c.close()
