"""svo_lk_track_rows at the ABI: the header, stereo_vo_amd/hip.py and the shared object agree on it; it takes svo_lk_track's records,
which keep their sizes; the kernel is one of its own beside k_lk_track.  No GPU: nothing here creates a context."""
import ctypes as C
import os
import re

from stereo_vo_amd import abi, hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SVO_ERR_ARG = -2


def read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def prototype(name):
    m = re.search(r"^int\s+%s\s*\((.*?)\);" % name, read("include", "svo_hip.h"), re.S | re.M)
    assert m, name
    return [" ".join(re.sub(r"\s*\w+$", "", " ".join(a.split())).split()) for a in m.group(1).split(",")]


def test_header_binding_and_library_agree():
    assert prototype("svo_lk_track_rows") == prototype("svo_lk_track") == ["svo_ctx*", "const svo_lk_job*", "int", "const svo_lk_params*", "uint32_t"]
    assert "svo_lk_track_rows" in hip.EXPORTS
    f = hip.lib().svo_lk_track_rows
    assert list(f.argtypes) == list(hip.lib().svo_lk_track.argtypes) == [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
    assert f.restype is C.c_int
    assert callable(hip.Context.lk_track_rows)


def test_the_records_are_lk_tracks():
    assert C.sizeof(abi.LkParams) == 24 and C.sizeof(abi.LkJob) == 96


def test_a_null_context_is_refused_without_a_device():
    assert hip.lib().svo_lk_track_rows(None, None, 0, None, 0) == SVO_ERR_ARG


def test_the_kernel_is_one_of_its_own():
    src = read("stereo_vo_amd", "csrc", "k_lk.hip")
    body = lambda name: re.search(r"__global__[^\n]*\b%s\b\(.*?\n}\n" % name, src, re.S).group(0)
    row, two_d = body("k_lk_track_row"), body("k_lk_track")
    assert "k_lk_track_row" not in two_d and "sqrt" in two_d and "sqrt" not in row
    assert row.count("lk_wave_sum(s1)") == 1 and "s2" not in row and "Iy" not in row
    assert "__syncthreads" not in row and "lk_stage_strip(" in row
    for np_, back in ((2, "true"), (2, "false"), (7, "true"), (7, "false"), (16, "true"), (16, "false")):
        assert "k_lk_track_row<%d, %s>" % (np_, back) in src
    assert "void launch_lk_track_row(const LkTrackArgs& a, int pixels_per_lane, hipStream_t st);" in read("stereo_vo_amd", "csrc", "svo_kernels.h")
