"""The stereo re-association of the KLT front end at the ABI: the header, stereo_vo_amd/hip.py and the shared object agree on
svo_klt_set_stereo and svo_klt_get_stereo; svo_klt_params is still 40 bytes (the mode is a setter, not a field); the C++ face has its
pass-through; the host check program of the decisions is part of `make hostcheck`.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVO_ERR_ARG = -2
SIGNATURES = {
    "svo_klt_set_stereo": ("int", ["svo_ctx*", "int"]),
    "svo_klt_get_stereo": ("int", ["const svo_ctx*"]),
}
CTYPES_OF = {"const svo_ctx*": C.c_void_p, "svo_ctx*": C.c_void_p, "int": C.c_int}


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def declared(name):
    """(return type, [parameter types]) of a prototype of svo_hip.h, names and comments dropped"""
    m = re.search(r"^(\w+)\s+%s\s*\((.*?)\);" % name, read("include", "svo_hip.h"), re.S | re.M)
    assert m, name
    args = []
    for a in re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S).split(","):
        a = " ".join(a.split())
        args.append(a if a.endswith("*") else re.sub(r"\s*\w+$", "", a))
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
    assert "stereo" not in body


def test_a_null_context_is_refused_without_a_device():
    L = hip.lib()
    assert L.svo_klt_set_stereo(None, 1) == SVO_ERR_ARG
    assert L.svo_klt_get_stereo(None) == SVO_ERR_ARG


def test_the_modes_and_the_faces():
    assert (abi.KLT_STEREO_TEMPORAL, abi.KLT_STEREO_ROW) == (0, 1)
    assert re.search(r"KLT_STEREO_TEMPORAL = 0, KLT_STEREO_ROW = 1", read("stereo_vo_amd", "csrc", "klt_call.hpp"))
    for m in ("klt_set_stereo", "klt_get_stereo", "lk_track_rows"):
        assert callable(getattr(hip.Context, m)), m
    est = read("stereo_vo_amd", "csrc", "rso_estimator.hpp")
    assert "void setKltStereo(int mode)" in est and "int getKltStereo() const" in est


def test_the_step_forms_its_guesses_on_the_device():
    src = read("stereo_vo_amd", "csrc", "k_klt.hip")
    body = re.search(r"__global__[^\n]*\bk_klt_row_guess\b.*?\n}\n", src, re.S).group(0)
    assert "nl.x - (pl.x - pr.x)" in body                                 # the rule as written
    klt, lk = read("stereo_vo_amd", "csrc", "svo_klt.hip"), read("stereo_vo_amd", "csrc", "svo_lk.hip")
    step = klt[klt.index('extern "C" int svo_klt_step('):klt.index('extern "C" int svo_debug_klt_select(')]
    assert "enqueue_lk_track(" in step                                    # the tracking launches are the helper's: it belongs to the step
    step += lk[lk.index("void enqueue_lk_track("):lk.index("// svo_lk_track and svo_lk_track_rows")]
    assert "launch_klt_row_guess(" in step and "launch_lk_track_row(" in step
    assert "hipStreamSynchronize" not in step and "hipMalloc" not in step and "lk_realloc" not in step


def test_the_host_check_is_part_of_make_hostcheck():
    mk = read("stereo_vo_amd", "csrc", "Makefile")
    assert re.search(r"^hostcheck:.*\$\(KLTSTEREOCHECK\)", mk, re.M) and "tools/klt_stereo_check.cpp" in mk
    assert "tools/klt_stereo_check" in read(".gitignore").split()
    src = read("tools", "klt_stereo_check.cpp")
    assert "int main()" in src and "check_klt_set_stereo" in src and "plan_stereo" in src and "check_lk_call" in src
