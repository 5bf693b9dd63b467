"""svo_lk_track at the ABI: the library exports its three symbols, the Python records have the sizes of the C ones, and the defaults
are the documented ones.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LK_SYMBOLS = ("svo_lk_default_params", "svo_lk_track", "svo_debug_lk_get_level")


def test_library_exports_the_lk_symbols():
    L = hip.lib()
    for name in LK_SYMBOLS:
        assert name in hip.EXPORTS
        getattr(L, name)


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    for name in LK_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "typedef struct svo_lk_job" in text
    assert "typedef struct svo_lk_params" in open(os.path.join(ROOT, "include", "svo_types.h")).read()


def test_record_sizes():
    """svo_lk_params: six 4-byte fields.  svo_lk_job as include/svo_hip.h declares it on the LP64 ABI: two 24-byte svo_image records, two
    pointers, an int32 padded to 8, three pointers = 48 + 16 + 8 + 24 = 96 bytes (lk_call.cpp asserts the same of the C structs, so a
    library that loads was compiled with these sizes)."""
    assert C.sizeof(abi.LkParams) == 24
    assert C.sizeof(abi.LkImage) == 24
    assert C.sizeof(abi.LkJob) == 96
    assert abi.LkJob.pts.offset == 48 and abi.LkJob.init.offset == 56 and abi.LkJob.n.offset == 64
    assert abi.LkJob.next_pts.offset == 72 and abi.LkJob.status.offset == 80 and abi.LkJob.err.offset == 88
    src = open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "lk_call.cpp")).read()
    assert "sizeof(svo_lk_params) == 24" in src and "sizeof(svo_lk_job) == 96" in src


def test_defaults():
    p = hip.default_lk_params()
    assert (p.win, p.max_level, p.max_iters) == (21, 3, 30)
    assert p.eps == C.c_float(0.01).value and p.min_eig == C.c_float(1e-4).value and p.fb_max == 0.0
    hip.lib().svo_lk_default_params(None)               # NULL is ignored
