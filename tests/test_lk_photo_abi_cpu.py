"""The photometric mode of the LK trackers at the ABI: the header, stereo_vo_amd/hip.py and the shared object agree on
svo_lk_set_photometric and svo_lk_get_photometric; svo_lk_params is still 24 bytes and svo_lk_job 96 (the mode is a setter on the
context, not a field); the C++ face has its pass-through; the mode check is host-only and part of `make hostcheck`.  No GPU: nothing
here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVO_ERR_ARG = -2
SIGNATURES = {
    "svo_lk_set_photometric": ("int", ["svo_ctx*", "int"]),
    "svo_lk_get_photometric": ("int", ["const svo_ctx*"]),
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


def test_the_records_keep_their_sizes():
    assert C.sizeof(abi.LkParams) == 24 and C.sizeof(abi.LkJob) == 96
    body = re.search(r"typedef struct svo_lk_params \{(.*?)\} svo_lk_params;", read("include", "svo_types.h"), re.S).group(1)
    assert "photo" not in body
    assert "svo_lk_params p; int backward, photo;" in read("stereo_vo_amd", "csrc", "svo_kernels.h")      # the mode rides in the launch arguments


def test_a_null_context_is_refused_without_a_device():
    L = hip.lib()
    assert L.svo_lk_set_photometric(None, 1) == SVO_ERR_ARG
    assert L.svo_lk_get_photometric(None) == SVO_ERR_ARG


def test_the_faces():
    for m in ("lk_set_photometric", "lk_get_photometric"):
        assert callable(getattr(hip.Context, m)), m
    est = read("stereo_vo_amd", "csrc", "rso_estimator.hpp")
    assert "void setLkPhotometric(int mode)" in est and "int getLkPhotometric() const" in est
    assert 'hasattr(L, "svo_lk_set_photometric")' in read("stereo_vo_amd", "hip.py")


def test_every_tracker_launch_of_the_front_end_carries_the_mode():
    klt = read("stereo_vo_amd", "csrc", "svo_klt.hip")
    made = re.findall(r"const LkTrackArgs \w+\{[^;]*\};", klt)
    assert len(made) == 3 and all(m.rstrip("};").rstrip().endswith("ctx->lk_photo") for m in made), made
    assert "lk_photo" not in klt[klt.index("void klt_free("):klt.index("static svo_klt::Caps klt_caps(")]   # svo_klt_enable leaves it alone


def test_the_mode_check_is_host_only_and_part_of_make_hostcheck():
    assert "int check_lk_set_photometric(int mode, bool capturing, std::string& why);" in read("stereo_vo_amd", "csrc", "lk_call.hpp")
    assert "hip_runtime" not in read("stereo_vo_amd", "csrc", "lk_call.cpp") and "int check_lk_set_photometric(" in read("stereo_vo_amd", "csrc", "lk_call.cpp")
    mk = read("stereo_vo_amd", "csrc", "Makefile")
    assert re.search(r"^hostcheck:.*\$\(LKCHECK\)", mk, re.M)
    src = read("tools", "lk_check.cpp")
    assert "int main()" in src and "check_lk_set_photometric" in src
