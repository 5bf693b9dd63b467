"""The resident KLT front end at the ABI: the library exports its symbols, the Python record has the size of the C one, the defaults are
the documented ones, and every entry point answers a NULL context with SVO_ERR_ARG.  No GPU: nothing here creates a context."""
import ctypes as C
import math
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KLT_SYMBOLS = ("svo_klt_default_params", "svo_klt_enable", "svo_klt_reset", "svo_klt_add_points", "svo_klt_step", "svo_klt_get_tracks",
               "svo_debug_klt_select")
SVO_ERR_ARG = -2


def test_library_exports_the_klt_symbols():
    L = hip.lib()
    for name in KLT_SYMBOLS:
        assert name in hip.EXPORTS
        getattr(L, name)


def test_header_declares_them():
    text = open(os.path.join(ROOT, "include", "svo_hip.h")).read()
    for name in KLT_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, text), name
    assert "typedef struct svo_klt_params" in open(os.path.join(ROOT, "include", "svo_types.h")).read()


def test_record_size():
    """svo_klt_params: svo_lk_params (24 bytes), cap and three floats = 40 bytes; klt_call.cpp asserts the same of the C struct, so a
    library that loads was compiled with this size"""
    assert C.sizeof(abi.KltParams) == 40
    assert abi.KltParams.cap.offset == 24 and abi.KltParams.max_dy.offset == 28 and abi.KltParams.min_disp.offset == 32 and abi.KltParams.max_disp.offset == 36
    assert "sizeof(svo_klt_params) == 40" in open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "klt_call.cpp")).read()


def test_defaults():
    p, lk = hip.default_klt_params(), hip.default_lk_params()
    assert bytes(p.lk) == bytes(lk)
    assert p.cap == 1024 and p.max_dy == 1.5 and p.min_disp == 0.5 and math.isinf(p.max_disp) and p.max_disp > 0
    hip.lib().svo_klt_default_params(None)               # NULL is ignored


def test_null_context_is_an_argument_error():
    L = hip.lib()
    p = hip.default_klt_params()
    assert L.svo_klt_enable(None, C.byref(p)) == SVO_ERR_ARG
    assert L.svo_klt_reset(None, None) == SVO_ERR_ARG
    assert L.svo_klt_add_points(None, 0, None, None, 0) == SVO_ERR_ARG
    assert L.svo_klt_step(None, None, 0, None) == SVO_ERR_ARG
    assert L.svo_klt_get_tracks(None, 0, None, None, None, None, 0) == SVO_ERR_ARG
    assert L.svo_debug_klt_select(None, 0, None, None, None, None, 0) == SVO_ERR_ARG
