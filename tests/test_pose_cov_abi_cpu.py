"""The pose-covariance entry points exist and the record's Python mirror has the library's size (CPU only: loads the library, needs no GPU)."""
import ctypes as C

from stereo_vo_amd import hip
from stereo_vo_amd.abi import PoseCov

CONTEXT_SYMBOLS = ("svo_set_pose_covariance", "svo_get_pose_covariance", "svo_get_pose_covariances", "svo_copy_pose_covariances_async", "svo_pose_cov_size")
SCHEDULER_SYMBOLS = ("svo_batch_set_pose_covariance", "svo_batch_pose_covariances", "svo_fpstream_set_pose_covariance")


def test_library_exports_the_pose_covariance_symbols():
    L = hip.lib()
    for name in CONTEXT_SYMBOLS + SCHEDULER_SYMBOLS:
        assert getattr(L, name) is not None, name
    assert set(CONTEXT_SYMBOLS) <= set(hip.EXPORTS) and set(SCHEDULER_SYMBOLS) <= set(hip.BATCH_EXPORTS)


def test_record_size_matches_the_mirror():
    L = hip.lib()
    L.svo_pose_cov_size.restype = C.c_size_t
    assert L.svo_pose_cov_size() == C.sizeof(PoseCov) == 888
    r = PoseCov()
    m = r.matrix("cov_pose")
    m[1, 2] = 7.0
    assert r.cov_pose[8] == 7.0 and m.shape == (6, 6), "matrix() is a row-major view of the record"
    assert PoseCov.state.offset == 880 and PoseCov.sigma2.offset == 864
