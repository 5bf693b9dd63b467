"""The resident top-up of the KLT front end at the ABI: the header, stereo_vo_amd/abi.py and the shared object agree on the entry
points, their arguments and the size of svo_klt_topup_params; every host-side refusal that needs no device is the documented one; the
host check program of the decisions is part of `make hostcheck`.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVO_ERR_ARG = -2
# name -> (return type, the parameter types as the header spells them)
SIGNATURES = {
    "svo_klt_topup_default_params": ("void", ["const svo_ctx*", "svo_klt_topup_params*"]),
    "svo_klt_topup_enable": ("int", ["svo_ctx*", "const svo_klt_topup_params*"]),
    "svo_klt_topup": ("int", ["svo_ctx*", "const uint64_t[2]"]),
    "svo_klt_topup_info": ("int", ["svo_ctx*", "int", "int32_t[4]"]),
    "svo_debug_klt_topup_append": ("int", ["svo_ctx*", "int", "const float*", "const float*", "const uint8_t*", "int"]),
}
CTYPES_OF = {"const svo_ctx*": C.c_void_p, "svo_ctx*": C.c_void_p, "svo_klt_topup_params*": C.c_void_p, "const svo_klt_topup_params*": C.c_void_p,
             "const uint64_t[2]": C.POINTER(C.c_uint64), "int": C.c_int, "int32_t[4]": C.c_void_p, "const float*": C.c_void_p, "const uint8_t*": C.c_void_p}


def header():
    return open(os.path.join(ROOT, "include", "svo_hip.h")).read()


def declared(name):
    """(return type, [parameter types]) of a prototype of svo_hip.h, names and comments dropped"""
    m = re.search(r"^(\w+)\s+%s\s*\((.*?)\);" % name, header(), re.S | re.M)
    assert m, name
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
        a = " ".join(a.split())
        arr = re.search(r"(\[\d+\])$", a)
        a = re.sub(r"\s*\w+(\[\d+\])?$", "", a) if not a.endswith("*") else a           # drop the parameter's name
        args.append(a + (arr.group(1) if arr else ""))
    return m.group(1), args


def test_header_abi_and_library_agree_on_the_entry_points():
    L = hip.lib()
    for name, (ret, args) in SIGNATURES.items():
        assert declared(name) == (ret, args), (name, declared(name))
        assert name in hip.EXPORTS
        f = getattr(L, name)
        assert list(f.argtypes) == [CTYPES_OF[a] for a in args], name
        assert (f.restype is None) == (ret == "void"), name


def test_record_size_and_layout():
    """svo_klt_topup_params: svo_gftt_params (16 bytes), below, target, init_disp = 28 bytes; klt_call.cpp asserts the same of the C
    struct, so a library that loads was compiled with this size"""
    assert C.sizeof(abi.KltTopupParams) == 28
    T = abi.KltTopupParams
    assert (T.gftt.offset, T.below.offset, T.target.offset, T.init_disp.offset) == (0, 16, 20, 24)
    assert "sizeof(svo_klt_topup_params) == 28" in open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "klt_call.cpp")).read()
    types = open(os.path.join(ROOT, "include", "svo_types.h")).read()
    body = re.search(r"typedef struct svo_klt_topup_params \{(.*?)\} svo_klt_topup_params;", types, re.S).group(1)
    fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert fields == [("svo_gftt_params", "gftt"), ("int32_t", "below"), ("int32_t", "target"), ("float", "init_disp")]
    assert [f[0] for f in T._fields_] == [f[1] for f in fields]


def test_defaults_without_a_context():
    """a NULL context: the defaults of a front end of 1024 tracks; a NULL record is ignored"""
    p = abi.KltTopupParams()
    hip.lib().svo_klt_topup_default_params(None, C.byref(p))
    assert bytes(p.gftt) == bytes(hip.default_gftt_params())
    assert (p.below, p.target, p.init_disp) == (512, 1024, 0.0)
    hip.lib().svo_klt_topup_default_params(None, None)


def test_null_context_is_an_argument_error():
    L = hip.lib()
    p = abi.KltTopupParams()
    info = (C.c_int32 * 4)()
    assert L.svo_klt_topup_enable(None, C.byref(p)) == SVO_ERR_ARG
    assert L.svo_klt_topup_enable(None, None) == SVO_ERR_ARG
    assert L.svo_klt_topup(None, None) == SVO_ERR_ARG
    assert L.svo_klt_topup_info(None, 0, info) == SVO_ERR_ARG
    assert L.svo_debug_klt_topup_append(None, 0, None, None, None, 0) == SVO_ERR_ARG


def test_reason_codes_match_the_kernels():
    src = open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "svo_kernels.h")).read()
    assert "enum { KLT_TOPUP_OK = 0, KLT_TOPUP_OVERFLOW, KLT_TOPUP_ENOUGH, KLT_TOPUP_NO_PAIR, KLT_TOPUP_NOT_ASKED };" in src
    assert (abi.TOPUP_OK, abi.TOPUP_OVERFLOW, abi.TOPUP_ENOUGH, abi.TOPUP_NO_PAIR, abi.TOPUP_NOT_ASKED) == (0, 1, 2, 3, 4)


def test_the_host_check_is_part_of_hostcheck():
    mk = open(os.path.join(ROOT, "stereo_vo_amd", "csrc", "Makefile")).read()
    assert re.search(r"^hostcheck:.*\$\(TOPUPCHECK\)", mk, re.M) and "TOPUPCHECK = ../../tools/klt_topup_check" in mk
    rule = re.search(r"^\$\(TOPUPCHECK\):.*\n\t(.*)$", mk, re.M).group(1)
    assert "-fsanitize=address,undefined" in rule and "klt_topup_check.cpp" in rule and "klt_call.cpp" in rule
    assert "int main()" in open(os.path.join(ROOT, "tools", "klt_topup_check.cpp")).read()
