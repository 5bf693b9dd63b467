"""svo_gftt_detect at the ABI: the library exports its three symbols, the Python records have the sizes and offsets of the C ones, the
defaults are the documented ones, and the kernel-time table kept its tail.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GFTT_SYMBOLS = ("svo_gftt_default_params", "svo_gftt_detect", "svo_debug_gftt_get_response")


def test_library_exports_the_gftt_symbols():
    L = hip.lib()
    for name in GFTT_SYMBOLS:
        assert name in hip.EXPORTS
        getattr(L, name)


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    for name in GFTT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "typedef struct svo_gftt_job" in text
    assert "typedef struct svo_gftt_params" in open(os.path.join(ROOT, "include", "svo_types.h")).read()


def test_record_sizes_and_offsets():
    """svo_gftt_params: four 4-byte fields.  svo_gftt_job on the LP64 ABI: a 24-byte svo_image, a pointer, two int32, three pointers =
    64 bytes (gftt_call.cpp asserts the same of the C structs, so a library that loads was compiled with these sizes)."""
    assert C.sizeof(abi.GfttParams) == 16
    assert [getattr(abi.GfttParams, f).offset for f in ("max_corners", "block", "min_distance", "quality")] == [0, 4, 8, 12]
    assert C.sizeof(abi.GfttJob) == 64
    J = abi.GfttJob
    assert (J.img.offset, J.seeds.offset, J.n_seeds.offset, J.cap.offset, J.pts.offset, J.response.offset, J.info.offset) == (0, 24, 32, 36, 40, 48, 56)
    src = open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "gftt_call.cpp")).read()
    assert "sizeof(svo_gftt_params) == 16" in src and "sizeof(svo_gftt_job) == 64" in src and "offsetof(svo_gftt_job, info) == 56" in src


def test_defaults():
    p = hip.default_gftt_params()
    assert (p.max_corners, p.block, p.min_distance) == (0, 3, 20)
    assert p.quality == C.c_float(0.01).value
    hip.lib().svo_gftt_default_params(None)             # NULL is ignored
