"""The inputs of tests/test_gpu_faster_anms.py, pinned from the reference alone (no GPU), and the ABI of the new entry points.

Floors: each image must give the adaptive NMS what its GPU test is there for -- thousands of candidates, zero responses, ties at the
top -- and the adaptive NMS must keep something other than the grid NMS, or a kernel that silently ran the grid NMS would pass."""
import ctypes as C
import inspect
import os
import sys

import numpy as np

from stereo_vo_amd import hip
from stereo_vo_amd.abi import keypoint_dtype

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_anms_ref as R                                     # noqa: E402
import faster_ref as F                                          # noqa: E402
import image_content as IC                                      # noqa: E402
from test_faster_cpu import photograph                          # noqa: E402

SVO_ERR_ARG = -2
NOISE_T = TILED_T = 20
PHOTO_T, PHOTO_NFEATS, PHOTO_OCT = 10, 500, 3


def noise_frame():
    """uniform noise at 320 x 240: about a seventh of the pixels are corners, the border ring with response exactly 0"""
    L = np.random.default_rng(1).integers(0, 256, (240, 320), dtype=np.uint8)
    return L, IC.right_of(L, 6)


def tiled_frame():
    """a 40 x 40 random tile repeated 8 x 6: every interior response occurs once per repetition -- ties everywhere, the maximum included"""
    tile = np.random.default_rng(2).integers(0, 256, (40, 40), dtype=np.uint8)
    L = np.ascontiguousarray(np.tile(tile, (6, 8)))
    return L, IC.right_of(L, 6)


def test_guard_noise():
    raw = F.corners(noise_frame()[0], NOISE_T, 4)
    assert len(raw) >= 10000 and (raw["response"] == 0).sum() >= 250, (len(raw), (raw["response"] == 0).sum())


def test_guard_tiled():
    raw = F.corners(tiled_frame()[0], TILED_T, 4)
    r = raw["response"]
    assert len(raw) >= 10000 and (r == r.max()).sum() >= 40 and len(r) - len(np.unique(r)) >= 5000, (len(raw), (r == r.max()).sum(), len(np.unique(r)))


def test_guard_photograph_keeps_other_corners_than_the_grid_nms(golden_dir):
    from oracle import oracle as O
    L, _ = photograph(golden_dir)
    raw = F.corners(L, PHOTO_T, 4)
    keep = F.kps_to_detect(PHOTO_NFEATS, PHOTO_OCT)[0]
    assert len(raw) >= 2000 and 400 <= keep <= 500, (len(raw), keep)
    grid, adaptive = set(O.nms_copy(raw, 3, 800, 600, keep).tolist()), set(O.anms_copy(raw, keep).tolist())
    assert len(adaptive) == keep and len(grid & adaptive) <= keep // 2, (len(grid), len(adaptive), len(grid & adaptive))


def test_reference_is_faster_ref_with_the_other_nms():
    L, Rt = noise_frame()
    p = R.params(hip.default_params(), NOISE_T, 500, 1)
    assert p.nmsMethod == 1 and p.non_maximal_suppression == 1 and p.detect_method == 2
    f = R.features(L[:120, :160], Rt[:120, :160], p, 4)
    assert len(f) == 1 and len(f[0][0]) == min(f[0][6], F.kps_to_detect(500, 1)[0]) and (np.diff(f[0][0]["y"]) >= 0).all()


def test_python_mirror_signatures():
    assert list(inspect.signature(hip.Context.set_faster_adaptive_nms).parameters) == ["self", "enable"]
    assert list(inspect.signature(hip.Context.faster_adaptive_nms).parameters) == ["self"]
    assert list(inspect.signature(hip.Context.adaptive_nms).parameters) == ["self", "kps", "num_out_points", "img_w", "img_h", "cap"]
    from stereo_vo_amd import pipeline
    for cls in (pipeline.StreamBatch, pipeline.FrameParallelStream):
        assert list(inspect.signature(cls.set_faster_adaptive_nms).parameters) == ["self", "enable"]
    for name in ("svo_set_faster_adaptive_nms", "svo_get_faster_adaptive_nms", "svo_adaptive_nms"):
        assert name in hip.EXPORTS
    for name in ("svo_batch_set_faster_adaptive_nms", "svo_fpstream_set_faster_adaptive_nms"):
        assert name in hip.BATCH_EXPORTS
    L = hip.lib()
    assert L.svo_set_faster_adaptive_nms.argtypes == [C.c_void_p, C.c_int] and L.svo_get_faster_adaptive_nms.argtypes == [C.c_void_p]
    assert L.svo_adaptive_nms.argtypes == [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    assert L.svo_set_faster_adaptive_nms(None, 1) == SVO_ERR_ARG and L.svo_get_faster_adaptive_nms(None) == SVO_ERR_ARG
    assert L.svo_adaptive_nms(None, None, 0, 0, 64, 48, None, 0) == SVO_ERR_ARG
    assert L.svo_batch_set_faster_adaptive_nms(None, 1) == SVO_ERR_ARG and L.svo_fpstream_set_faster_adaptive_nms(None, 1) == SVO_ERR_ARG
    assert keypoint_dtype.itemsize == 28


def test_header_declares_what_the_mirror_binds():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "svo_hip.h")).read()
    assert "int svo_set_faster_adaptive_nms(svo_ctx* ctx, int enable);" in h and "int svo_get_faster_adaptive_nms(const svo_ctx* ctx);" in h
    assert "int svo_adaptive_nms(svo_ctx* ctx, const svo_keypoint* kps, int n, int num_out_points, int img_w, int img_h," in h
    b = open(os.path.join(root, "include", "svo_batch.h")).read()
    assert "svo_batch_set_faster_adaptive_nms(svo_batch* b, int enable);" in b and "svo_fpstream_set_faster_adaptive_nms(svo_fpstream* f, int enable);" in b
