"""The RANSAC gate at the ABI: the header, stereo_vo_amd/hip.py and the shared object agree on svo_ransac_tracked, svo_klt_set_ransac and
svo_klt_get_ransac; svo_klt_params is still 40 bytes (the gate's mode is a setter, not a field); the C++ face has its two methods; the
host check program of the decisions is part of `make hostcheck`.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVO_ERR_ARG = -2
# name -> (return type, the parameter types as the header spells them)
SIGNATURES = {
    "svo_ransac_tracked": ("int", ["svo_ctx*", "const uint64_t[2]"]),
    "svo_klt_set_ransac": ("int", ["svo_ctx*", "int"]),
    "svo_klt_get_ransac": ("int", ["const svo_ctx*"]),
}
CTYPES_OF = {"const svo_ctx*": C.c_void_p, "svo_ctx*": C.c_void_p, "const uint64_t[2]": C.POINTER(C.c_uint64), "int": C.c_int}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def declared(name):
    """(return type, [parameter types]) of a prototype of svo_hip.h, names and comments dropped"""
    m = re.search(r"^(\w+)\s+%s\s*\((.*?)\);" % name, read("include", "svo_hip.h"), re.S | re.M)
    assert m, name
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
        a = " ".join(a.split())
        arr = re.search(r"(\[\d+\])$", a)
        a = re.sub(r"\s*\w+(\[\d+\])?$", "", a) if not a.endswith("*") else a           # drop the parameter's name
        args.append(a + (arr.group(1) if arr else ""))
    return m.group(1), args


def test_header_binding_and_library_agree_on_the_entry_points():
    L = hip.lib()
    for name, (ret, args) in SIGNATURES.items():
        assert declared(name) == (ret, args), (name, declared(name))
        assert name in hip.EXPORTS
        f = getattr(L, name)
        assert list(f.argtypes) == [CTYPES_OF[a] for a in args], name
        assert f.restype is C.c_int, name


def test_klt_params_is_still_40_bytes():
    assert C.sizeof(abi.KltParams) == 40
    assert "sizeof(svo_klt_params) == 40" in read("stereo_vo_amd", "csrc", "klt_call.cpp")
    body = re.search(r"typedef struct svo_klt_params \{(.*?)\} svo_klt_params;", read("include", "svo_types.h"), re.S).group(1)
    assert "ransac" not in body


def test_a_null_context_is_refused_without_a_device():
    L = hip.lib()
    assert L.svo_ransac_tracked(None, None) == SVO_ERR_ARG
    assert L.svo_klt_set_ransac(None, 1) == SVO_ERR_ARG
    assert L.svo_klt_get_ransac(None) == SVO_ERR_ARG


def test_the_modes_and_the_faces():
    assert (abi.KLT_RANSAC_OFF, abi.KLT_RANSAC_FILTER, abi.KLT_RANSAC_PRUNE) == (0, 1, 2)
    call = read("stereo_vo_amd", "csrc", "klt_call.hpp")
    assert re.search(r"KLT_RANSAC_OFF = 0, KLT_RANSAC_FILTER = 1, KLT_RANSAC_PRUNE = 2", call)
    for m in ("ransac_tracked", "klt_set_ransac", "klt_ransac"):
        assert callable(getattr(hip.Context, m)), m
    est = read("stereo_vo_amd", "csrc", "rso_estimator.hpp")
    assert "void filterTrackedRANSAC()" in est and "void setKLTRansac(int mode)" in est


def test_the_host_check_is_part_of_make_hostcheck():
    mk = read("stereo_vo_amd", "csrc", "Makefile")
    assert re.search(r"^hostcheck:.*\$\(KLTRANSACCHECK\)", mk, re.M) and "tools/klt_ransac_check.cpp" in mk
    assert "tools/klt_ransac_check" in read(".gitignore").split()
    src = read("tools", "klt_ransac_check.cpp")
    assert "int main()" in src and "check_ransac_tracked" in src and "check_klt_set_ransac" in src
