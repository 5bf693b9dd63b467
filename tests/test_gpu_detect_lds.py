"""The dynamic-LDS and scratch carve-ups of the detector kernels and of stage 5 at every context size, on the smallest input.

The kernels of k_detect.hip and k_gn.hip place their LDS and scratch arrays at offsets that depend on the context's sizes (max_kps, the
detector's quotas), not on the length of the lists: the four frames of tests/golden/oracle_small_seq.npz (256 x 192) go through
contexts whose sizes select every layout form.

  orb      ORB, 8 levels.  The detector is asked for nfe = int(1.5 orb_nfeats) keypoints, level_quota splits them over the levels, and
           ensure_geometry drops level 7 (53 rows: nothing inside the 31-pixel border), so k_nms_rowsort sorts n_slots = nfe - quota[7]
           keys in pmax = the next power of two:
             max_kps  4096, orb_nfeats  2700: nfe  4050, n_slots  3805, pmax  4096 -- k_nms_rowsort<4>, all in LDS (127152 B), sel_max 2048
             max_kps  8192, orb_nfeats  5400: nfe  8100, n_slots  7609, pmax  8192 -- k_nms_rowsort<8>, wide part in big_scratch, sel_max 4096
             max_kps 16384, orb_nfeats 10900: nfe 16350, n_slots 15359, pmax 16384 -- k_nms_rowsort<16>, sel_max 8192 (k_select_sort<8192>)
           Stage 5 (k_gauss_newton, pmax = max_kps) and svo_get_values (record strided by max_kps) run in all three.
  fo_grid  FAST+ORB, one octave, grid NMS: k_fastorb_nms with ACC_MAX = max_kps
  fo_anms  FAST+ORB, one octave, adaptive NMS: k_fastorb_anms with kmax from max_kps and its three-array scratch
  faster   dmFASTER, one octave, grid NMS: k_faster_nms (64-bit keys, three chunks: about 4250 corners at FAST threshold 10), smSAD / ifmSAD

The reference of the first three is the CPU oracle, that of dmFASTER tests/faster_ref.py + tests/sad_ref.py as in test_gpu_faster.py.
Every frame is compared as test_gpu_big_lists.same_as_record / test_gpu_faster.py do (lists exact, poses within their tolerances,
status words 0).  The references are computed once per process and never modified."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, north_star_params, DM_FAST_ORB

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_lists as B                                           # noqa: E402
import faster_ref as F                                          # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_gpu_parity import O                                   # noqa: E402
from test_gpu_big_lists import same_as_record                   # noqa: E402
from test_gpu_faster import assert_same_lists                   # noqa: E402
from test_gpu_sad import assert_same_as_reference               # noqa: E402

N_FRAMES = 4
SIZES = (4096, 8192, 16384)
ORB_NFEATS = {4096: 2700, 8192: 5400, 16384: 10900}
ORB_PMAX = {4096: 4096, 8192: 8192, 16384: 16384}               # what the docstring derives; checked against level_quota below
_cache = {}


def small(golden_dir):
    if "g" not in _cache:
        g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
        _cache["g"] = g, StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    return _cache["g"]


def params(g, mode, max_kps):
    if mode == "faster":
        p = F.faster_params(hip.default_params(), t=10, orb_nfeats=500, n_oct=1)       # (at the reference's threshold 20 frame 2 tracks 9 pairs)
        p.vo_use_matches_ids = 1
        return p
    p = north_star_params(hip.default_params(), orb_nfeats=ORB_NFEATS[max_kps] if mode == "orb" else int(g["orb_nfeats"]))
    p.vo_use_matches_ids = 1
    if mode != "orb":
        p.detect_method, p.nOctaves, p.nmsMethod = DM_FAST_ORB, 1, int(mode == "fo_anms")
    return p


def ref_key(mode, max_kps):
    return (mode, max_kps if mode == "orb" else 0)               # only ORB's parameters change with the context's size


def reference(golden_dir, mode, max_kps):
    """per frame: oracle modes -- the oracle's record (big_lists.record) with its match IDs; faster -- (faster_features, SadStream.step's record)"""
    key = ref_key(mode, max_kps)
    if key not in _cache:
        g, cam = small(golden_dir)
        p, out = params(g, mode, max_kps), []
        if mode == "faster":
            st = S.SadStream(O(), p, cam)
            for t in range(N_FRAMES):
                L, R = g["L%d" % t], g["R%d" % t]
                f = F.faster_features(L, R, p, 4)
                out.append((f, st.step((L, R), f[0][0], f[0][1], f[0][2], f[0][3])))
        else:
            orc = O().Oracle(p)
            for t in range(N_FRAMES):
                rec = B.record(orc, orc.process(g["L%d" % t], g["R%d" % t], cam))
                rec["ids"] = orc.match_ids(0).copy()
                out.append(rec)
        _cache[key] = out
    return _cache[key]


def orb_pmax(orb_nfeats, w, h, nlev=8):
    """nms_pmax of an ORB-mode context: level_quota and the live levels of ensure_geometry (svo_api.hip), in the same float operations"""
    f32 = np.float32
    factor = f32(1.0 / 1.2)
    nfe = int(1.5 * orb_nfeats)
    nd = f32(nfe) * (f32(1.0) - factor) / (f32(1.0) - f32(float(factor) ** nlev))
    quota = []
    for _ in range(nlev - 1):
        quota.append(int(np.rint(nd)))
        nd = f32(nd * factor)
    quota.append(max(nfe - sum(quota), 0))
    n_slots = 0
    for l in range(nlev):
        sf = f32(1.2 ** l)
        lw, lh = int(np.rint(f32(w) / sf)), int(np.rint(f32(h) / sf))
        if lw - 62 > 0 and lh - 62 > 0:
            n_slots += quota[l]
    p = 64
    while p < n_slots:
        p <<= 1
    return p, 2 * quota[0]


CASES = [(mode, mk) for mode in ("orb", "fo_grid", "fo_anms", "faster") for mk in SIZES]


def test_orb_requests_select_every_rowsort_form(golden_dir):
    g, _ = small(golden_dir)
    for mk in SIZES:
        pmax, ranked = orb_pmax(ORB_NFEATS[mk], int(g["W"]), int(g["H"]))
        assert pmax == ORB_PMAX[mk] and ranked <= mk // 2 and int(1.5 * ORB_NFEATS[mk]) <= mk, (mk, pmax, ranked)


@pytest.mark.parametrize("mode,max_kps", CASES)
def test_small_sequence_has_something_to_compare(golden_dir, mode, max_kps):
    """from the references alone: at least 60 keypoints per image on every frame, and every later frame valid with at least 20 tracked
    pairs -- no case below passes on an empty list"""
    for t, rec in enumerate(reference(golden_dir, mode, max_kps)):
        if mode == "faster":
            nl, nr, tracked, valid = len(rec[0][0][0]), len(rec[0][0][1]), rec[1]["tracked"], rec[1]["valid"]
        else:
            nl, nr, tracked, valid = len(rec["kl"][0]), len(rec["kr"][0]), rec["tracked"], rec["valid"]
        assert nl >= 60 and nr >= 60, (mode, t, nl, nr)
        if t:
            assert valid and len(tracked) >= 20, (mode, t, valid, len(tracked))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,max_kps", CASES)
def test_small_sequence_at_every_context_size(golden_dir, mode, max_kps):
    g, cam = small(golden_dir)
    ref = reference(golden_dir, mode, max_kps)
    ctx = hip.Context(n_lanes=1, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=max_kps, max_cand=1 << 15, kernel_times=True)
    ctx.set_params(params(g, mode, max_kps)); ctx.set_camera(cam)
    for t in range(N_FRAMES):
        ctx.process_host([(g["L%d" % t], g["R%d" % t])])
        tag = "%s max_kps %d t=%d" % (mode, max_kps, t)
        if mode == "faster":
            r = ctx.result(0)
            assert_same_lists(ctx, 0, ref[t][0], tag, r)
            assert_same_as_reference(ctx, 0, r, ref[t][1], tag, ids=True)
        else:
            r = same_as_record(ctx, 0, ref[t], tag)
            assert (ctx.match_ids(0, 0) == ref[t]["ids"]).all(), (tag, "match IDs")
        assert r.status == 0 and ctx.status_word(0) == 0, (tag, r.status, ctx.status_word(0))
    assert r.valid and r.tracked_feats_from_last_frame >= 20 and len(ctx.tracked(0)) == r.tracked_feats_from_last_frame, (tag, r.valid, r.tracked_feats_from_last_frame)
    if mode == "orb":
        # svo_get_values: the packed record (strided by max_kps) against the separate getters, all six lists and the four counts
        kl, dl, kr, dr, m, ids = ctx.values(0, 0, 0)
        assert (len(kl), len(kr), len(m), len(ids)) == (r.detected_left[0], r.detected_right[0], r.stereo_matches[0], len(ctx.match_ids(0, 0))), tag
        assert len(kl) >= 60 and len(m) >= 60 and len(ids) == len(m), (tag, len(kl), len(m), len(ids))
        for side, (k, d) in enumerate(((kl, dl), (kr, dr))):
            ks, ds = ctx.keypoints(0, 0, side)
            assert k.tobytes() == ks.tobytes() and d.shape == ds.shape and (d == ds).all(), (tag, "svo_get_values", side)
        assert m.tobytes() == ctx.matches(0).tobytes() and (ids == ctx.match_ids(0, 0)).all(), (tag, "svo_get_values")
    # the instantiations the case is about were launched every frame, under the names they have always had
    kt = ctx.kernel_times()
    count = {k: v[1] for k, v in kt.items() if v[1]}
    if mode == "orb":
        wide = max_kps == 16384
        assert kt["nms_rowsort_16"][1] == (N_FRAMES if wide else 0) and kt["nms_rowsort"][1] == (0 if wide else N_FRAMES), (tag, count)
        assert kt["select_8192"][1] == (N_FRAMES if wide else 0) and kt["select"][1] == (0 if wide else N_FRAMES), (tag, count)
    elif mode == "faster":
        assert kt["faster_nms"][1] == N_FRAMES and kt["faster"][1] == N_FRAMES and kt["select"][1] == 0, (tag, count)
    else:
        assert kt["fast"][1] == N_FRAMES and kt["faster_nms"][1] == 0 and kt["nms_rowsort"][1] + kt["nms_rowsort_16"][1] == N_FRAMES, (tag, count)
    assert kt["gauss_newton"][1] == N_FRAMES, (tag, count)
    ctx.close()
