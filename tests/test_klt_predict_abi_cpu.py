"""The pose prediction of the KLT front end at the ABI: the header, stereo_vo_amd/hip.py and the shared object agree on
svo_klt_set_prediction, svo_klt_get_prediction, svo_klt_predicted and svo_debug_klt_predict; svo_klt_params is still 40 bytes (the mode
is a setter, not a field); the C++ face has its pass-through; the host check program of the decisions is part of `make hostcheck`.
No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVO_ERR_ARG = -2
# name -> (return type, the parameter types as the header spells them)
SIGNATURES = {
    "svo_klt_set_prediction": ("int", ["svo_ctx*", "int"]),
    "svo_klt_get_prediction": ("int", ["const svo_ctx*"]),
    "svo_klt_predicted": ("int", ["svo_ctx*", "int", "float*", "float*", "uint8_t*", "int"]),
    "svo_debug_klt_predict": ("int", ["svo_ctx*", "int", "const double*", "int", "float*", "float*", "uint8_t*", "int"]),
}
CTYPES_OF = {"const svo_ctx*": C.c_void_p, "svo_ctx*": C.c_void_p, "int": C.c_int, "float*": C.c_void_p, "uint8_t*": C.c_void_p, "const double*": C.c_void_p}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def declared(name):
    """(return type, [parameter types]) of a prototype of svo_hip.h, names and comments dropped"""
    m = re.search(r"^(\w+)\s+%s\s*\((.*?)\);" % name, read("include", "svo_hip.h"), re.S | re.M)
    assert m, name
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
        a = " ".join(a.split())
        args.append(a if a.endswith("*") else re.sub(r"\s*\w+$", "", a))              # drop the parameter's name
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
    body = re.search(r"typedef struct svo_klt_params \{(.*?)\} svo_klt_params;", read("include", "svo_types.h"), re.S).group(1)
    assert "predict" not in body


def test_a_null_context_is_refused_without_a_device():
    L = hip.lib()
    assert L.svo_klt_set_prediction(None, 1) == SVO_ERR_ARG
    assert L.svo_klt_get_prediction(None) == SVO_ERR_ARG
    assert L.svo_klt_predicted(None, 0, None, None, None, 0) == SVO_ERR_ARG
    assert L.svo_debug_klt_predict(None, 0, None, 1, None, None, None, 0) == SVO_ERR_ARG


def test_the_modes_and_the_faces():
    assert (abi.KLT_PREDICT_OFF, abi.KLT_PREDICT_POSE) == (0, 1)
    assert re.search(r"KLT_PREDICT_OFF = 0, KLT_PREDICT_POSE = 1", read("stereo_vo_amd", "csrc", "klt_call.hpp"))
    for m in ("klt_set_prediction", "klt_prediction", "klt_predicted", "debug_klt_predict"):
        assert callable(getattr(hip.Context, m)), m
    assert "void setKltPrediction(int mode)" in read("stereo_vo_amd", "csrc", "rso_estimator.hpp")


def test_the_kernel_shares_its_expressions_with_k_project_points():
    src = read("stereo_vo_amd", "csrc", "k_gn.hip")
    body = lambda name: re.search(r"__global__[^\n]*\b%s\b.*?\n}\n" % name, src, re.S).group(0)
    assert "triangulate_move_project(" in body("k_project_points") and "triangulate_move_project(" in body("k_klt_predict")
    assert "rodrigues_with_derivs<false>" in body("k_klt_predict") and "__syncthreads()" in body("k_klt_predict")
    assert "const int has_init" in read("stereo_vo_amd", "csrc", "k_klt.hip")


def test_the_host_check_is_part_of_make_hostcheck():
    mk = read("stereo_vo_amd", "csrc", "Makefile")
    assert re.search(r"^hostcheck:.*\$\(KLTPREDICTCHECK\)", mk, re.M) and "tools/klt_predict_check.cpp" in mk
    assert "tools/klt_predict_check" in read(".gitignore").split()
    src = read("tools", "klt_predict_check.cpp")
    assert "int main()" in src and "check_klt_set_prediction" in src and "check_klt_predict_call" in src and "plan_predict" in src
