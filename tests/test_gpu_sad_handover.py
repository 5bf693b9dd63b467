"""Hand-over records that carry the 8 x 8 windows of smSAD / ifmSAD (k_handover.hip, layout version 3): frame-parallel runs and
manual svo_export_frame / svo_import_frame hops under the SAD selectors.

The yardstick everywhere is ONE plain hip.Context fed the same frames sequentially (tests/test_gpu_sad.py and tests/test_gpu_faster.py
hold that run to the reference's walks): keypoints and descriptors of both sides and every octave, pairings, tracked pairs, match IDs
and the result record are compared as bytes, per lane and frame.  Inputs: the four 760 x 560 crops of the photograph (sad_ref.CROPS),
read in place at stride 800."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, keypoint_dtype, dmatch_dtype

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
import sad_ref as S                                             # noqa: E402

pytestmark = pytest.mark.gpu

W, H, STRIDE = S.CROP_W, S.CROP_H, 800
MAX_KPS, MAX_CAND = 1024, 1 << 15
SVO_ERR_ARG = -2
VOEC_FIRST_ITERATION, VOEC_BAD_TRACKING = 4, 5
ST_HANDOVER_MISMATCH = 4
TAIL = hip.RUN_TRACK | hip.RUN_OPTIMIZE                          # stages 4-5 (Context.run_stages adds SVO_FLAG_NO_SHIFT)


def camera():
    return StereoCamera.simple(500.0, W / 2.0, H / 2.0, 0.12, W, H)


def default_config(n_oct=3):
    """the reference's out-of-the-box configuration: dmFASTER + smSAD + ifmSAD, with match IDs"""
    p = F.faster_params(hip.default_params(), t=20, orb_nfeats=500, n_oct=n_oct)
    p.vo_use_matches_ids = 1
    return p


def orb_config(match_method=2, ifm_method=2):
    """ORB (1.5 x 600 = 900 keypoints asked of the detector: within the 1024-entry lists) under the given matcher and tracker"""
    p = S.photo_params(hip.default_params(), orb_nfeats=600, ifm_sad_max_distance=400, match_method=match_method, ifm_method=ifm_method)
    p.vo_use_matches_ids = 1
    return p


@pytest.fixture(scope="module")
def photo(golden_dir):
    """the photograph and a constant-grey frame on the device; frame(i) = the (left, right) addresses of crop i, stride 800"""
    import torch
    g = np.load(os.path.join(golden_dir, "ref_pair_800x600.npz"))
    L, R = torch.from_numpy(g["left"]).cuda(), torch.from_numpy(g["right"]).cuda()
    assert L.shape == (600, STRIDE) and L.is_contiguous() and R.is_contiguous()
    grey = torch.full((H, STRIDE), 128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    class Photo:
        keep = (L, R, grey)

        @staticmethod
        def frame(i):
            x, y = S.CROPS[i]
            return (L.data_ptr() + y * STRIDE + x, R.data_ptr() + y * STRIDE + x)

        @staticmethod
        def blank():
            return (grey.data_ptr(), grey.data_ptr())
    return Photo


def context(p, lanes=1, n_oct=1, **kw):
    ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=MAX_KPS, max_cand=MAX_CAND, max_octaves=n_oct, **kw)
    ctx.set_params(p); ctx.set_camera(camera())
    return ctx


def snapshot(ctx, lane, n_oct):
    """everything a frame leaves behind for one lane, as bytes"""
    out = []
    for o in range(n_oct):
        for side in (0, 1):
            k, d = ctx.keypoints(lane, 0, side, o)
            out += [k.tobytes(), d.tobytes()]
        out += [ctx.matches(lane, 0, o).tobytes(), ctx.tracked(lane, o).tobytes(), ctx.match_ids(lane, 0, o).tobytes()]
    out.append(bytes(ctx.result(lane)))
    return out


NAMES = ("left keypoints", "left descriptors", "right keypoints", "right descriptors", "pairings", "tracked pairs", "match IDs")


def assert_same(a, b, tag):
    bad = [(NAMES[i % 7] + " octave %d" % (i // 7)) if i < len(a) - 1 else "result record" for i, (x, y) in enumerate(zip(a, b)) if x != y]
    assert len(a) == len(b) and not bad, (tag, bad)


LANE_ORDER = ((0, 1, 2, 3, 0, 1, 2, 3), (3, 2, 1, 0, 3, 2, 1, 0))       # lane 1 sees the crops in reverse: the lanes differ


def sequential(photo, p, n_oct):
    """the yardstick: one context, two lanes, eight frames; per frame and lane (snapshot, result)"""
    ctx = context(p, lanes=2, n_oct=n_oct)
    ref = []
    for t in range(8):
        ctx.process_device([photo.frame(LANE_ORDER[lane][t]) for lane in (0, 1)], W, H, STRIDE)
        res = ctx.results()
        assert ctx.status_word(0) == 0 and ctx.status_word(1) == 0, (t, ctx.status_word(0), ctx.status_word(1))
        ref.append([(snapshot(ctx, lane, n_oct), res[lane]) for lane in (0, 1)])
    ctx.close()
    # not vacuous: on each lane at least three of the later frames are tracked from their previous frame and solved
    for lane in (0, 1):
        good = [t for t in range(1, 8) if ref[t][lane][1].valid and ref[t][lane][1].tracked_feats_from_last_frame >= p.bad_tracking_th]
        print("sequential lane %d: valid %s tracked %s (bad_tracking_th %d)" % (lane, [int(ref[t][lane][1].valid) for t in range(8)],
              [ref[t][lane][1].tracked_feats_from_last_frame for t in range(8)], p.bad_tracking_th))
        assert len(good) >= 3, (lane, good)
    return ref


def frame_parallel_equals_sequential(photo, p, n_oct, contexts):
    from stereo_vo_amd.pipeline import FrameParallelStream
    ref = sequential(photo, p, n_oct)
    for G in contexts:
        # frame by frame ...
        fp = FrameParallelStream(p, camera(), W, H, lanes=2, contexts=G, max_kps=MAX_KPS, max_cand=MAX_CAND, max_octaves=n_oct)
        for t in range(8):
            c = fp.push([photo.frame(LANE_ORDER[lane][t]) for lane in (0, 1)], STRIDE)
            fp.synchronize()
            for lane in (0, 1):
                assert_same(snapshot(c, lane, n_oct), ref[t][lane][0], ("contexts %d frame %d lane %d" % (G, t, lane)))
        fp.close()
        # ... and pushed back to back: the last G frames are still on their owners
        fp = FrameParallelStream(p, camera(), W, H, lanes=2, contexts=G, max_kps=MAX_KPS, max_cand=MAX_CAND, max_octaves=n_oct)
        owners = [fp.push([photo.frame(LANE_ORDER[lane][t]) for lane in (0, 1)], STRIDE) for t in range(8)]
        fp.synchronize()
        for t in range(8 - G, 8):
            for lane in (0, 1):
                assert_same(snapshot(owners[t], lane, n_oct), ref[t][lane][0], ("back to back, contexts %d frame %d lane %d" % (G, t, lane)))
        fp.close()


def test_frame_parallel_equals_sequential_default_configuration(photo):
    """dmFASTER + smSAD + ifmSAD on three octaves, match IDs on, two lanes, frames dealt to two and to three contexts: every context
    imports the windows of the frame before its own and exports those of its own.  (Without windows in the record the second push
    is SVO_ERR_STATE: "... windows of its previous frame were never gathered".)"""
    frame_parallel_equals_sequential(photo, default_config(3), 3, (2, 3))


def test_frame_parallel_equals_sequential_orb_smsad_ifmsad(photo):
    frame_parallel_equals_sequential(photo, orb_config(2, 2), 1, (2,))


def test_frame_parallel_equals_sequential_orb_smsad_descriptor_tracker(photo):
    """a stream whose records carry windows although its tracker (ifmDescBF) needs none"""
    frame_parallel_equals_sequential(photo, orb_config(2, 0), 1, (2,))


def device_blob(nbytes):
    import torch
    blob = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()              # torch fills the buffer on ITS stream: through before a context writes it on its own
    return blob


def test_manual_hop_through_the_older_slot(photo):
    """after a frame without corners (voecBadTracking) the OLDER frame stays the previous one: the export takes the lists AND the
    windows of that slot, and the importer tracks from them"""
    p, n_oct = default_config(3), 3
    seq = context(p, n_oct=n_oct)
    for fr in (photo.frame(0), photo.frame(1), photo.blank()):
        seq.process_device([fr], W, H, STRIDE)
    assert seq.result(0).error_code == VOEC_BAD_TRACKING and not seq.result(0).valid
    seq.process_device([photo.frame(2)], W, H, STRIDE)
    want = snapshot(seq, 0, n_oct)
    assert seq.result(0).valid and len(seq.tracked(0, 0)) >= p.bad_tracking_th, (seq.result(0).error_code, len(seq.tracked(0, 0)))
    a, b = context(p, n_oct=n_oct), context(p, n_oct=n_oct)
    for fr in (photo.frame(0), photo.frame(1), photo.blank()):
        a.process_device([fr], W, H, STRIDE)
    nb = a.handover_bytes()
    assert nb == b.handover_bytes()
    blob = device_blob(nb)
    a.export_frame(blob.data_ptr(), nb); a.wait()
    b.process_device([photo.frame(2)], W, H, STRIDE, hip.RUN_DETECT | hip.RUN_MATCH)
    b.import_frame(blob.data_ptr(), nb)
    b.run_stages(TAIL)
    got = snapshot(b, 0, n_oct)
    assert_same(got, want, "hop through the older slot")
    assert len(b.tracked(0, 0)) > 0 and b.status_word(0) == 0
    for c in (seq, a, b):
        c.close()


def record_bytes_v2(max_kps, max_h):
    """one lane-octave of the version 2 layout, from its description in k_handover.hip: a 256-byte header, then
    kps[2][max_kps] | desc[2][max_kps][32] | matches[max_kps] | ids[max_kps] | row_index[2][max_h] | mrow_index[max_h + 1],
    every section starting on a multiple of 16"""
    a16 = lambda v: (v + 15) & ~15                              # noqa: E731
    return (256 + a16(2 * max_kps * keypoint_dtype.itemsize) + a16(2 * max_kps * 32) + a16(max_kps * dmatch_dtype.itemsize) + a16(max_kps * 4) +
            a16(2 * max_h * 4) + a16((max_h + 1) * 4))


def window_bytes(max_kps):
    """what version 3 adds: wflag[2][align16(max_kps)] | win[2][max_kps][64]"""
    return 2 * ((max_kps + 15) & ~15) + 2 * max_kps * 64


def test_sizes_and_kinds(photo):
    lanes, n_oct = 2, 3
    plain = context(orb_config(0, 0), lanes=lanes, n_oct=n_oct)                  # Hamming matchers: never selects SAD
    v2 = lanes * n_oct * record_bytes_v2(MAX_KPS, H)
    assert plain.handover_bytes() == v2
    carrying = context(orb_config(2, 0), lanes=lanes, n_oct=n_oct)
    v3 = v2 + lanes * n_oct * window_bytes(MAX_KPS)
    assert carrying.handover_bytes() == v3
    carrying.set_params(orb_config(0, 0))                                         # sticky: once a SAD method was selected
    assert carrying.handover_bytes() == v3
    carrying.set_params(orb_config(2, 0))
    for c in (plain, carrying):
        for i in (0, 1):
            c.process_device([photo.frame(i), photo.frame(3 - i)], W, H, STRIDE)
    blob = device_blob(v3)
    L = carrying.L
    assert L.svo_export_frame(carrying.h, C.c_void_p(blob.data_ptr()), C.c_size_t(v2)) == SVO_ERR_ARG
    spare = device_blob(v3 + 16)                                                  # the windows are copied in 16-byte pieces
    assert L.svo_export_frame(carrying.h, C.c_void_p(spare.data_ptr() + 4), C.c_size_t(v3)) == SVO_ERR_ARG and b"16-byte aligned" in L.svo_last_error(carrying.h)
    carrying.export_frame(blob.data_ptr(), v3); carrying.wait()
    head = blob[:48].cpu().numpy().view(np.int32)
    assert head[1] == 3 and head[11] == 1, head                                  # version 3, windows gathered
    # a record with windows handed to a context that carries none: another layout -- flagged, nothing copied
    before = [plain.keypoints(lane, 1, side)[0].tobytes() for lane in (0, 1) for side in (0, 1)]
    assert all(len(x) for x in before)
    plain.import_frame(blob.data_ptr(), v3); plain.wait()
    for lane in (0, 1):
        assert plain.status_word(lane) & ST_HANDOVER_MISMATCH and plain.result(lane).status & ST_HANDOVER_MISMATCH
    assert [plain.keypoints(lane, 1, side)[0].tobytes() for lane in (0, 1) for side in (0, 1)] == before
    # the record of a context that carries none says version 2 and leaves the spare header word alone
    blob2 = device_blob(v2)
    plain.export_frame(blob2.data_ptr(), v2); plain.wait()
    head = blob2[:48].cpu().numpy().view(np.int32)
    assert head[1] == 2 and head[11] == 0, head
    plain.close(); carrying.close()


def test_record_without_windows_into_a_carrying_context(photo):
    """a context on the Hamming matchers (version 2 records) hands its frame to contexts that carry windows: under a descriptor
    tracker the lists are all that is needed; under ifmSAD the lane cannot track from a frame without windows and starts afresh --
    decided on the device at the import, by the parameters then in force"""
    pa, pb, pc = orb_config(0, 0), orb_config(2, 0), orb_config(2, 2)
    # the sequential counterpart of a -> b: two frames under pa, then the parameters of b
    seq = context(pa)
    for i in (0, 1):
        seq.process_device([photo.frame(i)], W, H, STRIDE)
    seq.set_params(pb)
    seq.process_device([photo.frame(2)], W, H, STRIDE)
    want = snapshot(seq, 0, 1)
    assert seq.result(0).valid and len(seq.tracked(0)) >= pb.bad_tracking_th
    seq.close()
    a = context(pa)
    for i in (0, 1):
        a.process_device([photo.frame(i)], W, H, STRIDE)
    b, c = context(pb), context(pc)
    nb = b.handover_bytes()
    assert a.handover_bytes() < nb == c.handover_bytes()
    blob = device_blob(nb)
    a.export_frame(blob.data_ptr(), a.handover_bytes()); a.wait()
    b.process_device([photo.frame(2)], W, H, STRIDE, hip.RUN_DETECT | hip.RUN_MATCH)
    b.import_frame(blob.data_ptr(), nb)
    b.run_stages(TAIL)
    assert_same(snapshot(b, 0, 1), want, "version 2 record under smSAD + ifmDescBF")
    assert b.status_word(0) == 0
    c.process_device([photo.frame(2)], W, H, STRIDE, hip.RUN_DETECT | hip.RUN_MATCH)
    c.import_frame(blob.data_ptr(), nb)
    c.run_stages(TAIL)
    r = c.result(0)
    assert not r.valid and r.error_code == VOEC_FIRST_ITERATION and r.status == 0 and c.status_word(0) == 0, (r.valid, r.error_code, r.status)
    assert len(c.tracked(0)) == 0
    c.process_device([photo.frame(3)], W, H, STRIDE)
    r = c.result(0)
    assert r.valid and r.tracked_feats_from_last_frame >= pc.bad_tracking_th, (r.error_code, r.tracked_feats_from_last_frame)
    for x in (a, b, c):
        x.close()


def test_stream_that_selects_sad_in_mid_stream(photo):
    """svo_fpstream_set_params re-reads the record size: a stream created and run on the Hamming matchers switches to smSAD after
    two frames -- the records grow, the last owner exports again, and the run stays the sequential one"""
    from stereo_vo_amd.pipeline import FrameParallelStream
    pa, pb = orb_config(0, 0), orb_config(2, 0)
    seq = context(pa)
    want = []
    for t in range(4):
        if t == 2:
            seq.set_params(pb)
        seq.process_device([photo.frame(t)], W, H, STRIDE)
        want.append(snapshot(seq, 0, 1))
    assert seq.result(0).valid
    seq.close()
    fp = FrameParallelStream(pa, camera(), W, H, lanes=1, contexts=2, max_kps=MAX_KPS, max_cand=MAX_CAND)
    small = fp.ctxs[0].handover_bytes()
    for t in range(4):
        if t == 2:
            fp.set_params(pb)
            assert fp.ctxs[0].handover_bytes() == fp.ctxs[1].handover_bytes() == small + window_bytes(MAX_KPS)
        c = fp.push([photo.frame(t)], STRIDE)
        fp.synchronize()
        assert_same(snapshot(c, 0, 1), want[t], "switch in mid-stream, frame %d" % t)
    fp.close()
