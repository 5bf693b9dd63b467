"""ctypes binding of the HIP C-ABI (include/svo_hip.h -> stereo_vo_amd/libsvo_hip.so).

This is the product path.  There is no CPU fallback: `lib()` raises if the shared library is missing and
`Context()` raises if no HIP device is present.
"""
import ctypes as C
import os
import numpy as np

from .abi import (CameraModel, FasterStats, GfttJob, GfttParams, KltParams, KltTopupParams, Landmark, LandmarksInfo, LkImage, LkJob, LkParams, Params, PoseCov, Result, StereoCalibration, StereoCamera, StereoRectification, keypoint_dtype, dmatch_dtype, index_pair_dtype)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVO_HIP_LIB") or os.path.join(_HERE, "libsvo_hip.so")      # SVO_HIP_LIB: a library built from another commit, for A/B runs (tools/prof.sh abbench)
_LIB = None

MAX_LANES = 128
RUN_DETECT, RUN_MATCH, RUN_TRACK, RUN_OPTIMIZE, RUN_ALL = 1, 2, 4, 8, 15
FLAG_REPEAT, FLAG_NO_SHIFT, FLAG_DEVICE_IMAGES, FLAG_BGR_IMAGES, FLAG_DETECT_NO_POST, RUN_DETECT_POST, FLAG_PINNED_IMAGES = 16, 32, 64, 128, 256, 512, 1024

# every entry point include/svo_hip.h declares (tests check that the library exports all of them)
EXPORTS = [
    "svo_config_defaults", "svo_params_defaults", "svo_create", "svo_destroy", "svo_strerror", "svo_last_error",
    "svo_set_params", "svo_get_params", "svo_params_load_ini", "svo_set_fast_threshold", "svo_set_orb_threshold", "svo_get_fast_threshold",
    "svo_get_orb_threshold", "svo_set_klt_win", "svo_get_klt_win", "svo_klt_win_load_ini",
    "svo_set_dyn_fast_threshold", "svo_get_dyn_fast_threshold", "svo_dyn_fast_load_ini", "svo_get_faster_stats", "svo_faster_stats_size", "svo_faster_threshold_step",
    "svo_set_faster_adaptive_nms", "svo_get_faster_adaptive_nms", "svo_adaptive_nms",
    "svo_set_stream", "svo_get_stream", "svo_get_device", "svo_set_camera", "svo_set_rectify_map",
    "svo_stereo_rectify", "svo_set_undistort_rectify", "svo_set_stereo_calibration", "svo_debug_get_rectify_map", "svo_reset", "svo_process", "svo_process_lanes", "svo_wait", "svo_get_result", "svo_get_results", "svo_copy_results_async",
    "svo_set_pose_covariance", "svo_get_pose_covariance", "svo_get_pose_covariances", "svo_copy_pose_covariances_async", "svo_pose_cov_size",
    "svo_set_landmarks", "svo_get_landmarks_enabled", "svo_landmarks_load_ini", "svo_get_landmarks_info", "svo_get_landmarks", "svo_copy_landmarks_async", "svo_landmark_abi_size",
    "svo_get_keypoints", "svo_get_matches", "svo_get_tracked", "svo_get_residuals", "svo_get_outliers",
    "svo_get_keypoints_oct", "svo_get_matches_oct", "svo_get_tracked_oct", "svo_get_row_index", "svo_get_matches_row_index", "svo_get_match_ids", "svo_reset_ids", "svo_set_this_frame_as_kf",
    "svo_put_features", "svo_put_matches", "svo_put_tracked", "svo_put_tracked_oct", "svo_put_match_ids", "svo_save_state", "svo_load_state", "svo_change_in_pose", "svo_projected_coords", "svo_hamming_match",
    "svo_lk_default_params", "svo_lk_track", "svo_debug_lk_get_level",
    "svo_gftt_default_params", "svo_gftt_detect", "svo_debug_gftt_get_response",
    "svo_klt_default_params", "svo_klt_enable", "svo_klt_reset", "svo_klt_add_points", "svo_klt_step", "svo_klt_get_tracks", "svo_debug_klt_select",
    "svo_klt_topup_default_params", "svo_klt_topup_enable", "svo_klt_topup", "svo_klt_topup_info", "svo_debug_klt_topup_append",
    "svo_ransac_tracked", "svo_klt_set_ransac", "svo_klt_get_ransac",
    "svo_klt_set_prediction", "svo_klt_get_prediction", "svo_klt_predicted", "svo_debug_klt_predict",
    "svo_lk_track_rows", "svo_klt_set_stereo", "svo_klt_get_stereo",
    "svo_lk_set_photometric", "svo_lk_get_photometric",
    "svo_debug_get_level", "svo_debug_get_raw_keypoints", "svo_debug_get_status_word", "svo_debug_get_redo_count", "svo_debug_get_graph_count", "svo_debug_timeline", "svo_profiler_sections_enabled",
    "svo_kernel_times", "svo_kernel_times_reset", "svo_kernel_times_select", "svo_abi_sizes",
    "svo_get_values", "svo_put_features_oct", "svo_put_matches_oct", "svo_put_match_ids_oct",
    "svo_handover_bytes", "svo_export_frame", "svo_import_frame", "svo_gather_windows", "svo_get_windows_oct",
    "svo_use_graphs", "svo_record_after_post", "svo_wait_upload", "svo_host_alloc", "svo_host_free", "svo_host_register", "svo_host_unregister",
]


BATCH_EXPORTS = [
    "svo_batch_abi_sizes", "svo_batch_config_defaults", "svo_batch_create", "svo_batch_create_sized", "svo_batch_destroy", "svo_batch_last_error", "svo_batch_lanes", "svo_batch_contexts",
    "svo_batch_context", "svo_batch_set_params", "svo_batch_set_camera", "svo_batch_set_klt_win", "svo_batch_set_results_buffer", "svo_batch_switch_results_buffer", "svo_batch_step", "svo_batch_step_lanes",
    "svo_batch_wait_on_stream", "svo_batch_hold_for_event", "svo_batch_synchronize", "svo_batch_results", "svo_batch_reset",
    "svo_batch_set_pose_covariance", "svo_batch_pose_covariances", "svo_fpstream_set_pose_covariance",
    "svo_batch_set_dyn_fast_threshold", "svo_batch_faster_stats", "svo_fpstream_set_dyn_fast_threshold",
    "svo_batch_set_faster_adaptive_nms", "svo_fpstream_set_faster_adaptive_nms", "svo_fpstream_set_landmarks",
    "svo_fpstream_create", "svo_fpstream_destroy", "svo_fpstream_last_error", "svo_fpstream_contexts", "svo_fpstream_context",
    "svo_fpstream_last_owner", "svo_fpstream_set_params", "svo_fpstream_set_camera", "svo_fpstream_set_klt_win", "svo_fpstream_push", "svo_fpstream_synchronize",
]


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_lanes", C.c_int32), ("max_w", C.c_int32), ("max_h", C.c_int32),
                ("max_kps", C.c_int32), ("max_cand", C.c_int32), ("kernel_times", C.c_int32), ("max_octaves", C.c_int32),
                ("stream", C.c_void_p)]


class BatchConfig(C.Structure):
    """svo_batch_config (include/svo_batch.h)"""
    _fields_ = [("ctx", Config), ("n_contexts", C.c_int32), ("schedule", C.c_int32), ("det_priority_high", C.c_int32),
                ("post_mode", C.c_int32), ("det_streams", C.c_int32), ("rest_streams", C.c_int32), ("no_detect_ahead", C.c_int32)]


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_int64)]


class Frame(C.Structure):
    _fields_ = [("left", Image), ("right", Image)]


class Values(C.Structure):
    _fields_ = [("left_kps", C.c_void_p), ("left_desc", C.c_void_p), ("right_kps", C.c_void_p), ("right_desc", C.c_void_p),
                ("matches", C.c_void_p), ("match_ids", C.c_void_p), ("cap_kps", C.c_int32), ("cap_matches", C.c_int32),
                ("n_left", C.c_int32), ("n_right", C.c_int32), ("n_matches", C.c_int32), ("n_ids", C.c_int32)]


class SvoError(RuntimeError):
    pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise SvoError("HIP extension missing: %s (run `python -c 'import __graft_entry__ as g; g.build()'`); "
                           "there is no CPU fallback" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.svo_strerror.restype = C.c_char_p
        L.svo_last_error.restype = C.c_char_p
        L.svo_last_error.argtypes = [C.c_void_p]
        for n in ("svo_destroy", "svo_config_defaults", "svo_params_defaults", "svo_abi_sizes"):
            getattr(L, n).restype = None
        L.svo_destroy.argtypes = [C.c_void_p]
        for n in ("svo_batch_last_error", "svo_fpstream_last_error"):
            getattr(L, n).restype = C.c_char_p; getattr(L, n).argtypes = [C.c_void_p]
        for n in ("svo_batch_context", "svo_fpstream_context", "svo_fpstream_last_owner"):
            getattr(L, n).restype = C.c_void_p
        for n in ("svo_batch_destroy", "svo_fpstream_destroy", "svo_batch_config_defaults", "svo_batch_abi_sizes"):
            getattr(L, n).restype = None
        L.svo_batch_destroy.argtypes = [C.c_void_p]; L.svo_fpstream_destroy.argtypes = [C.c_void_p]
        L.svo_batch_create_sized.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
        if hasattr(L, "svo_pose_cov_size"):          # (absent from a library of an earlier commit loaded through SVO_HIP_LIB for an A/B)
            L.svo_pose_cov_size.restype = C.c_size_t; L.svo_pose_cov_size.argtypes = []
            L.svo_copy_pose_covariances_async.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        if hasattr(L, "svo_set_dyn_fast_threshold"):          # (as above: absent from a library of an earlier commit)
            L.svo_set_dyn_fast_threshold.argtypes = [C.c_void_p, C.c_int, C.c_double]
            L.svo_get_dyn_fast_threshold.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
            L.svo_dyn_fast_load_ini.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double)]
            L.svo_get_faster_stats.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            L.svo_faster_stats_size.restype = C.c_size_t; L.svo_faster_stats_size.argtypes = []
            L.svo_faster_threshold_step.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_double]
            L.svo_batch_set_dyn_fast_threshold.argtypes = [C.c_void_p, C.c_int, C.c_double]
            L.svo_batch_faster_stats.argtypes = [C.c_void_p, C.c_void_p]
            L.svo_fpstream_set_dyn_fast_threshold.argtypes = [C.c_void_p, C.c_int, C.c_double]
        if hasattr(L, "svo_set_faster_adaptive_nms"):          # (as above: absent from a library of an earlier commit)
            L.svo_set_faster_adaptive_nms.argtypes = [C.c_void_p, C.c_int]
            L.svo_get_faster_adaptive_nms.argtypes = [C.c_void_p]
            L.svo_adaptive_nms.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
            L.svo_batch_set_faster_adaptive_nms.argtypes = [C.c_void_p, C.c_int]
            L.svo_fpstream_set_faster_adaptive_nms.argtypes = [C.c_void_p, C.c_int]
        if hasattr(L, "svo_set_landmarks"):          # (as above: absent from a library of an earlier commit)
            L.svo_set_landmarks.argtypes = [C.c_void_p, C.c_int, C.c_double]
            L.svo_get_landmarks_enabled.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
            L.svo_landmarks_load_ini.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double)]
            L.svo_get_landmarks_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            L.svo_get_landmarks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.svo_copy_landmarks_async.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
            L.svo_landmark_abi_size.restype = C.c_size_t; L.svo_landmark_abi_size.argtypes = []
            L.svo_fpstream_set_landmarks.argtypes = [C.c_void_p, C.c_int, C.c_double]
        if hasattr(L, "svo_stereo_rectify"):          # (as above: absent from a library of an earlier commit)
            L.svo_stereo_rectify.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_size_t]
            L.svo_set_undistort_rectify.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.svo_set_stereo_calibration.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
            L.svo_debug_get_rectify_map.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "svo_lk_track"):          # (as above: absent from a library of an earlier commit)
            L.svo_lk_default_params.restype = None; L.svo_lk_default_params.argtypes = [C.c_void_p]
            L.svo_lk_track.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
            L.svo_debug_lk_get_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "svo_gftt_detect"):       # (as above)
            L.svo_gftt_default_params.restype = None; L.svo_gftt_default_params.argtypes = [C.c_void_p]
            L.svo_gftt_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
            L.svo_debug_gftt_get_response.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        if hasattr(L, "svo_klt_step"):          # (as above)
            L.svo_klt_default_params.restype = None; L.svo_klt_default_params.argtypes = [C.c_void_p]
            L.svo_klt_enable.argtypes = [C.c_void_p, C.c_void_p]
            L.svo_klt_reset.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            L.svo_klt_add_points.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
            L.svo_klt_step.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
            L.svo_klt_get_tracks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            L.svo_debug_klt_select.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "svo_klt_topup"):         # (as above)
            L.svo_klt_topup_default_params.restype = None; L.svo_klt_topup_default_params.argtypes = [C.c_void_p, C.c_void_p]
            L.svo_klt_topup_enable.argtypes = [C.c_void_p, C.c_void_p]
            L.svo_klt_topup.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            L.svo_klt_topup_info.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            L.svo_debug_klt_topup_append.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "svo_ransac_tracked"):    # (as above)
            L.svo_ransac_tracked.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
            L.svo_klt_set_ransac.argtypes = [C.c_void_p, C.c_int]
            L.svo_klt_get_ransac.argtypes = [C.c_void_p]
        if hasattr(L, "svo_klt_set_prediction"):    # (as above)
            L.svo_klt_set_prediction.argtypes = [C.c_void_p, C.c_int]
            L.svo_klt_get_prediction.argtypes = [C.c_void_p]
            L.svo_klt_predicted.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            L.svo_debug_klt_predict.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        if hasattr(L, "svo_lk_track_rows"):         # (as above)
            L.svo_lk_track_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_uint32]
            L.svo_klt_set_stereo.argtypes = [C.c_void_p, C.c_int]
            L.svo_klt_get_stereo.argtypes = [C.c_void_p]
        if hasattr(L, "svo_lk_set_photometric"):    # (as above)
            L.svo_lk_set_photometric.argtypes = [C.c_void_p, C.c_int]
            L.svo_lk_get_photometric.argtypes = [C.c_void_p]
        L.svo_process_lanes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
        L.svo_batch_step_lanes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]
        L.svo_gather_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        _LIB = L
    return _LIB


def default_params() -> Params:
    p = Params()
    lib().svo_params_defaults(C.byref(p))
    return p


def load_params_ini(path, sections, p: Params = None) -> Params:
    """loadParamsFromConfigFileName (H:665-672): the reference's INI keys from the seven sections
    [rectify, detect, match, if-match, least_squares, gui, general] ('' skips a group) over `p` (defaults when None)."""
    if len(sections) != 7:
        raise ValueError("seven section names expected (H:556)")
    if p is None:
        p = default_params()
    arr = (C.c_char_p * 7)(*[s.encode() if s else None for s in sections])
    rc = lib().svo_params_load_ini(str(path).encode(), arr, C.byref(p))
    if rc != 0:
        raise SvoError("svo_params_load_ini(%s): %s" % (path, lib().svo_strerror(rc).decode()))
    return p


def load_klt_win_ini(path, detect_section, klt_win=4) -> int:
    """TDetectParams::KLT_win from the DETECT section of the reference's INI file; `klt_win` when the section or key is absent"""
    v = C.c_int32(int(klt_win))
    rc = lib().svo_klt_win_load_ini(str(path).encode(), detect_section.encode() if detect_section else None, C.byref(v))
    if rc != 0:
        raise SvoError("svo_klt_win_load_ini(%s): %s" % (path, lib().svo_strerror(rc).decode()))
    return int(v.value)


def load_dyn_fast_ini(path, detect_section, target=10. / 1000.) -> float:
    """TDetectParams::target_feats_per_pixel from the DETECT section of the reference's INI file; `target` when the section or key is absent"""
    v = C.c_double(float(target))
    rc = lib().svo_dyn_fast_load_ini(str(path).encode(), detect_section.encode() if detect_section else None, C.byref(v))
    if rc != 0:
        raise SvoError("svo_dyn_fast_load_ini(%s): %s" % (path, lib().svo_strerror(rc).decode()))
    return float(v.value)


def load_landmarks_ini(path, least_squares_section, std_noise_pixels=1.0) -> float:
    """TLeastSquaresParams::std_noise_pixels from the LEAST_SQUARES section of the reference's INI file; `std_noise_pixels` when the
    section or key is absent; SvoError when the file holds a negative or non-finite value"""
    v = C.c_double(float(std_noise_pixels))
    rc = lib().svo_landmarks_load_ini(str(path).encode(), least_squares_section.encode() if least_squares_section else None, C.byref(v))
    if rc != 0:
        raise SvoError("svo_landmarks_load_ini(%s): %s" % (path, lib().svo_strerror(rc).decode()))
    return float(v.value)


def faster_threshold_step(T, n, w, h, target) -> int:
    """the rule that moves dmFASTER's threshold after a detection that found n corners in a w x h image (host only)"""
    return int(lib().svo_faster_threshold_step(int(T), int(n), int(w), int(h), float(target)))


def stereo_rectify(calib: StereoCalibration) -> StereoRectification:
    """svo_stereo_rectify: Bouguet's rectification of a calibrated rig as cv::stereoRectify does it for alpha = -1 (host only, no
    device).  SvoError with the library's text when the calibration is refused; .status holds the code."""
    out = StereoRectification()
    why = C.create_string_buffer(320)
    rc = lib().svo_stereo_rectify(C.byref(calib), C.byref(out), why, len(why))
    if rc != 0:
        e = SvoError("svo_stereo_rectify: %s [%s]" % (lib().svo_strerror(rc).decode(), why.value.decode()))
        e.status = rc
        raise e
    return out


def default_lk_params() -> LkParams:
    p = LkParams()
    lib().svo_lk_default_params(C.byref(p))
    return p


def default_klt_params() -> KltParams:
    p = KltParams()
    lib().svo_klt_default_params(C.byref(p))
    return p


def default_gftt_params() -> GfttParams:
    p = GfttParams()
    lib().svo_gftt_default_params(C.byref(p))
    return p


def _vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def lane_mask_words(active, n_lanes):
    """The active-lane mask of svo_process_lanes / svo_batch_step_lanes as a list of ceil(n_lanes / 64) ints: bit l & 63 of
    word l >> 6 selects lane l.  `active`: None (every lane), an iterable of lane indices, or a bool array of n_lanes entries."""
    n_lanes = int(n_lanes)
    if n_lanes < 1:
        raise ValueError("n_lanes must be positive")
    words = [0] * ((n_lanes + 63) // 64)
    if active is None:
        lanes = range(n_lanes)
    else:
        a = np.asarray(list(active) if not isinstance(active, np.ndarray) else active)
        if a.dtype == np.bool_:
            if a.shape != (n_lanes,):
                raise ValueError("a bool mask needs one entry per lane: %d, got shape %s" % (n_lanes, a.shape))
            lanes = np.flatnonzero(a)
        else:
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError("lane indices must be integers")
            lanes = a.reshape(-1)
    for l in lanes:
        l = int(l)
        if l < 0 or l >= n_lanes:
            raise ValueError("lane %d outside [0, %d)" % (l, n_lanes))
        words[l >> 6] |= 1 << (l & 63)
    return words


def lane_mask_lanes(words, n_lanes):
    """the lane indices a mask of lane_mask_words selects, ascending"""
    return [l for l in range(int(n_lanes)) if (int(words[l >> 6]) >> (l & 63)) & 1]


class Context:
    """n_lanes independent rso::CStereoOdometryEstimator streams driven through the HIP kernels together."""

    def __init__(self, n_lanes=1, max_w=1280, max_h=960, max_kps=4096, max_cand=1 << 17, device=0, kernel_times=False, stream=None, max_octaves=1):
        self.L = lib()
        cfg = Config()
        self.L.svo_config_defaults(C.byref(cfg))
        cfg.device, cfg.n_lanes, cfg.max_w, cfg.max_h, cfg.max_kps, cfg.max_cand = device, n_lanes, max_w, max_h, max_kps, max_cand
        cfg.kernel_times = int(kernel_times)
        cfg.max_octaves = int(max_octaves)
        cfg.stream = stream
        self.n_lanes, self.max_kps = n_lanes, max_kps
        h = C.c_void_p()
        rc = self.L.svo_create(C.byref(cfg), C.byref(h))
        self.h = h
        if rc != 0:
            msg = self._err(rc)
            if h:
                self.L.svo_destroy(h)
            self.h = None
            raise SvoError("svo_create failed: " + msg)
        self._keep = None
        self._owned = True

    @classmethod
    def from_handle(cls, handle, n_lanes, max_kps):
        """A view of a context that something else owns (svo_batch_context / svo_fpstream_context): close() leaves it alone."""
        self = cls.__new__(cls)
        self.L = lib()
        self.h = C.c_void_p(handle)
        self.n_lanes, self.max_kps = n_lanes, max_kps
        self._keep = None
        self._owned = False
        return self

    def _err(self, rc):
        s = self.L.svo_strerror(rc).decode()
        if self.h:
            le = self.L.svo_last_error(self.h)
            if le:
                s += " [" + le.decode() + "]"
        return s

    def _ck(self, rc, what):
        if rc < 0:
            raise SvoError("%s: %s" % (what, self._err(rc)))
        return rc

    def close(self):
        if getattr(self, "h", None):
            if getattr(self, "_owned", True):
                self.L.svo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- parameters ------------------------------------------------------------------------------------
    def set_params(self, p: Params):
        self._ck(self.L.svo_set_params(self.h, C.byref(p)), "svo_set_params")

    def set_camera(self, cam: StereoCamera, lane=-1):
        self._ck(self.L.svo_set_camera(self.h, lane, C.byref(cam)), "svo_set_camera")

    def set_fast_threshold(self, v):
        self._ck(self.L.svo_set_fast_threshold(self.h, int(v)), "svo_set_fast_threshold")

    def set_orb_threshold(self, v):
        self._ck(self.L.svo_set_orb_threshold(self.h, int(v)), "svo_set_orb_threshold")

    def fast_threshold(self):
        return self.L.svo_get_fast_threshold(self.h)

    def set_klt_win(self, v):
        """dmFASTER's KLT_win (1 .. 15, default 4): the response window is (2 v + 1)^2 pixels"""
        self._ck(self.L.svo_set_klt_win(self.h, int(v)), "svo_set_klt_win")

    def klt_win(self):
        return self.L.svo_get_klt_win(self.h)

    def set_dyn_fast_threshold(self, enable=True, target=10. / 1000.):
        """dmFASTER's threshold per lane and octave, adapted on the device towards `target` corners per pixel (svo_set_dyn_fast_threshold)"""
        self._ck(self.L.svo_set_dyn_fast_threshold(self.h, 1 if enable else 0, float(target)), "svo_set_dyn_fast_threshold")

    def dyn_fast_threshold(self):
        """(enabled, target corners per pixel)"""
        e, t = C.c_int(0), C.c_double(0.0)
        self._ck(self.L.svo_get_dyn_fast_threshold(self.h, C.byref(e), C.byref(t)), "svo_get_dyn_fast_threshold")
        return bool(e.value), float(t.value)

    def faster_stats(self, lane=0) -> FasterStats:
        """the lane's thresholds and corner counts (waits); SvoError while the feature is off"""
        r = FasterStats()
        self._ck(self.L.svo_get_faster_stats(self.h, lane, C.byref(r)), "svo_get_faster_stats")
        return r

    def set_faster_adaptive_nms(self, enable=True):
        """opt in to (or out of) the adaptive NMS under dmFASTER (svo_set_faster_adaptive_nms); allocates its scratch at once"""
        self._ck(self.L.svo_set_faster_adaptive_nms(self.h, 1 if enable else 0), "svo_set_faster_adaptive_nms")

    def faster_adaptive_nms(self) -> bool:
        return bool(self.L.svo_get_faster_adaptive_nms(self.h))

    def adaptive_nms(self, kps, num_out_points, img_w, img_h, cap=None):
        """m_adaptive_non_max_sup on one list (svo_adaptive_nms): the kernel of the adaptive NMS under dmFASTER on caller keypoints, for
        holding it to a reference.  kps: keypoint_dtype records in strictly ascending raster order with integer coordinates.  Returns
        (number kept, the first min(kept, cap) indices in radius-descending order); cap defaults to len(kps)."""
        kps = np.ascontiguousarray(kps, dtype=keypoint_dtype)
        cap = len(kps) if cap is None else int(cap)
        out = np.zeros(max(1, cap), np.int32)
        n = self.L.svo_adaptive_nms(self.h, _vp(kps) if len(kps) else None, len(kps), int(num_out_points), int(img_w), int(img_h), _vp(out), cap)
        if n < 0:
            self._ck(n, "svo_adaptive_nms")
        return n, out[:min(n, cap)].copy()

    def orb_threshold(self):
        return self.L.svo_get_orb_threshold(self.h)

    def reset(self, lane=-1):
        self._ck(self.L.svo_reset(self.h, lane), "svo_reset")

    # -- frames ----------------------------------------------------------------------------------------
    def _process(self, fr, flags, words):
        """svo_process (words None), or svo_process_lanes with the mask words of the lanes that take part (the others: as if not called)"""
        if words is None:
            self._ck(self.L.svo_process(self.h, fr, C.c_uint32(flags)), "svo_process")
            return
        w = list(words) + [0]
        self._ck(self.L.svo_process_lanes(self.h, fr, C.c_uint32(flags), (C.c_uint64 * 2)(w[0], w[1])), "svo_process_lanes")

    def _mask(self, active):
        """`active` consumed ONCE (it may be a generator): (mask words or None, the set of lanes that sit out)"""
        if active is None:
            return None, set()
        words = lane_mask_words(active, self.n_lanes)
        return words, set(range(self.n_lanes)) - set(lane_mask_lanes(words, self.n_lanes))

    def process_host(self, pairs, flags=RUN_ALL, active=None):
        """pairs: list of (left, right) uint8 numpy arrays [h, w], one per lane.  active: None = every lane, else an iterable of lane
        indices or a bool array; the entries of `pairs` for the other lanes are not read and may be None."""
        assert len(pairs) == self.n_lanes
        fr = (Frame * self.n_lanes)()
        keep = []
        words, idle = self._mask(active)
        for i, pr in enumerate(pairs):
            if i in idle:
                continue
            l, r = pr
            l = np.ascontiguousarray(l, np.uint8)
            r = np.ascontiguousarray(r, np.uint8)
            keep += [l, r]
            h, w = l.shape[:2]
            if l.ndim == 3:
                assert l.shape[2] == 3 and r.shape == l.shape
                flags |= FLAG_BGR_IMAGES
            fr[i].left = Image(l.ctypes.data, w, h, l.strides[0])
            fr[i].right = Image(r.ctypes.data, w, h, r.strides[0])
        self._keep = keep
        self._process(fr, flags & ~FLAG_DEVICE_IMAGES, words)

    def _ptr_frames(self, ptr_pairs, w, h, stride, active):
        assert len(ptr_pairs) == self.n_lanes
        fr = (Frame * self.n_lanes)()
        words, idle = self._mask(active)
        for i, pr in enumerate(ptr_pairs):
            if i in idle:
                continue
            fr[i].left = Image(pr[0], w, h, stride)
            fr[i].right = Image(pr[1], w, h, stride)
        return fr, words

    def process_device(self, ptr_pairs, w, h, stride, flags=RUN_ALL, active=None):
        """ptr_pairs: list of (left_ptr, right_ptr) device addresses (e.g. torch tensor.data_ptr()), one per lane; active as for
        process_host (entries of the other lanes may be None)."""
        fr, words = self._ptr_frames(ptr_pairs, w, h, stride, active)
        self._process(fr, flags | FLAG_DEVICE_IMAGES, words)

    def process_pinned(self, ptr_pairs, w, h, stride, flags=RUN_ALL, active=None):
        """ptr_pairs: (left_ptr, right_ptr) PAGE-LOCKED host addresses per lane (torch pin_memory() tensors, svo_host_alloc):
        the upload is enqueued on the context's copy stream; the buffers must stay untouched until wait_upload().  active as for
        process_host: the other lanes are not uploaded."""
        fr, words = self._ptr_frames(ptr_pairs, w, h, stride, active)
        self._process(fr, (flags | FLAG_PINNED_IMAGES) & ~FLAG_DEVICE_IMAGES, words)

    # -- windows for lists the library did not detect (svo_gather_windows) ------------------------------------
    def _gather(self, fr, flags, which, words):
        m = None
        if words is not None:
            w = list(words) + [0]
            m = (C.c_uint64 * 2)(w[0], w[1])
        self._ck(self.L.svo_gather_windows(self.h, fr, C.c_uint32(flags), int(which), m), "svo_gather_windows")

    def gather_windows(self, pairs, which=0, active=None):
        """The images of put / loaded lists: gathers the SAD windows of the current (which=0) or previous (which=1) frame of the
        active lanes.  pairs: (left, right) uint8 numpy arrays per lane, [h, w] grey or [h, w, 3] BGR; entries of idle lanes may be None."""
        assert len(pairs) == self.n_lanes
        fr = (Frame * self.n_lanes)()
        keep, flags = [], 0
        words, idle = self._mask(active)
        for i, pr in enumerate(pairs):
            if i in idle:
                continue
            l, r = (np.ascontiguousarray(x, np.uint8) for x in pr)
            keep += [l, r]
            h, w = l.shape[:2]
            if l.ndim == 3:
                assert l.shape[2] == 3 and r.shape == l.shape
                flags |= FLAG_BGR_IMAGES
            fr[i].left = Image(l.ctypes.data, w, h, l.strides[0])
            fr[i].right = Image(r.ctypes.data, w, h, r.strides[0])
        self._keep = keep
        self._gather(fr, flags, which, words)

    def gather_windows_device(self, ptr_pairs, w, h, stride, which=0, active=None, flags=0):
        """the same from device addresses (read in place under the read contract of svo_image.stride)"""
        fr, words = self._ptr_frames(ptr_pairs, w, h, stride, active)
        self._gather(fr, flags | FLAG_DEVICE_IMAGES, which, words)

    def windows(self, lane=0, which=0, side=0, octave=0):
        """(windows [n, 8, 8] uint8, border flags [n] uint8) of one list; SvoError when that frame's windows were never gathered"""
        n = self._ck(self.L.svo_get_windows_oct(self.h, lane, which, side, octave, None, None, 0), "svo_get_windows_oct")
        win = np.zeros((n, 8, 8), np.uint8)
        flag = np.zeros(n, np.uint8)
        if n:
            self._ck(self.L.svo_get_windows_oct(self.h, lane, which, side, octave, _vp(win), _vp(flag), n), "svo_get_windows_oct")
        return win, flag

    def handover_bytes(self):
        self.L.svo_handover_bytes.restype = C.c_size_t
        return int(self.L.svo_handover_bytes(self.h))

    def export_frame(self, dev_ptr, nbytes):
        """Enqueue the hand-over record ("what the next call finds as its previous frame", all lanes) into device memory."""
        self._ck(self.L.svo_export_frame(self.h, C.c_void_p(dev_ptr), C.c_size_t(nbytes)), "svo_export_frame")

    def import_frame(self, dev_ptr, nbytes):
        self._ck(self.L.svo_import_frame(self.h, C.c_void_p(dev_ptr), C.c_size_t(nbytes)), "svo_import_frame")

    def use_graphs(self, enable=True):
        """Capture each distinct svo_process call into a hipGraph and replay it (one launch per frame)."""
        self._ck(self.L.svo_use_graphs(self.h, int(enable)), "svo_use_graphs")

    def wait_upload(self):
        self._ck(self.L.svo_wait_upload(self.h), "svo_wait_upload")

    def set_stream(self, stream):
        """Later process / copy calls enqueue on this raw HIP stream (None: the stream the context was created with)."""
        self._ck(self.L.svo_set_stream(self.h, C.c_void_p(stream) if stream else None), "svo_set_stream")

    def get_stream(self):
        """the raw hipStream_t (int) calls enqueue on right now"""
        st = C.c_void_p()
        self._ck(self.L.svo_get_stream(self.h, C.byref(st)), "svo_get_stream")
        return st.value or 0

    def set_rectify_map(self, lane, side, map_x, map_y):
        """Stage-1 rectification map of one camera (HxW float32 source coordinates); None, None clears it."""
        if map_x is None:
            self._ck(self.L.svo_set_rectify_map(self.h, lane, side, None, None, 0, 0), "svo_set_rectify_map")
            return
        mx = np.ascontiguousarray(map_x, np.float32); my = np.ascontiguousarray(map_y, np.float32)
        assert mx.ndim == 2 and mx.shape == my.shape
        self._ck(self.L.svo_set_rectify_map(self.h, lane, side, C.c_void_p(mx.ctypes.data), C.c_void_p(my.ctypes.data), mx.shape[1], mx.shape[0]), "svo_set_rectify_map")

    def set_undistort_rectify(self, lane, side, cam: CameraModel, R, P, w, h):
        """cv::initUndistortRectifyMap(cam, R, P) + set_rectify_map of one camera, built on the device (svo_set_undistort_rectify).
        R: 3 x 3 rectifying rotation, P: fx' fy' cx' cy' of the rectified camera.  lane = -1: one table shared by every lane."""
        R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9)); P = np.ascontiguousarray(np.asarray(P, np.float64).reshape(4))
        self._ck(self.L.svo_set_undistort_rectify(self.h, int(lane), int(side), C.byref(cam), _vp(R), _vp(P), int(w), int(h)), "svo_set_undistort_rectify")

    def set_stereo_calibration(self, calib: StereoCalibration, lane=-1, set_camera=True) -> StereoRectification:
        """setFromCamParams: rectify the rig, build both maps on the device in one launch and (set_camera) hand the rectified camera to
        stage 5 (svo_set_stereo_calibration).  Returns the rectification; on a refusal nothing has changed."""
        out = StereoRectification()
        self._ck(self.L.svo_set_stereo_calibration(self.h, int(lane), C.byref(calib), 1 if set_camera else 0, C.byref(out)), "svo_set_stereo_calibration")
        return out

    def rectify_map_fixed(self, lane, side):
        """the fixed-point map in force for one camera, whichever setter made it: (xy, frac) flat uint32 arrays of w * h entries,
        xy = (sx + 1) | (sy + 1) << 16 (0xFFFFFFFF: wholly outside), frac = fx | fy << 8; empty arrays when the camera has no map"""
        n = self._ck(self.L.svo_debug_get_rectify_map(self.h, int(lane), int(side), None, None, 0), "svo_debug_get_rectify_map")
        xy, frac = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        if n:
            self._ck(self.L.svo_debug_get_rectify_map(self.h, int(lane), int(side), _vp(xy), _vp(frac), n), "svo_debug_get_rectify_map")
        return xy, frac

    def projected_coords(self, pre_matches, pre_left, pre_right, tracked_first, cam, change_pose):
        """getProjectedCoords (common.cpp:415-466): (B, 4) float32 pixels of the pairings whose tracked_first is -1."""
        m = np.ascontiguousarray(pre_matches, dmatch_dtype); kl = np.ascontiguousarray(pre_left, keypoint_dtype); kr = np.ascontiguousarray(pre_right, keypoint_dtype)
        tf = np.ascontiguousarray(tracked_first, np.int32); pose = np.ascontiguousarray(change_pose, np.float64)
        pix = np.zeros((max(1, len(m)), 4), np.float32)
        n = self._ck(self.L.svo_projected_coords(self.h, _vp(m), len(m), _vp(kl), len(kl), _vp(kr), len(kr), _vp(tf), C.byref(cam), _vp(pose), _vp(pix), len(pix)), "svo_projected_coords")
        return pix[:n].copy()

    def save_state(self, lane, path):
        """saveStateToFile (common.cpp:475-543) of one lane: the reference's layout with the octave-0 lists, followed -- for a context
        that works on several octaves or whose frames have SAD windows -- by the extension block (state_file.py)."""
        self._ck(self.L.svo_save_state(self.h, lane, os.fsencode(path)), "svo_save_state")

    def load_state(self, lane, path):
        """loadStateFromFile (common.cpp:261-350) into one lane; a file with the extension block brings every octave and the windows."""
        self._ck(self.L.svo_load_state(self.h, lane, os.fsencode(path)), "svo_load_state")

    def run_stages(self, flags, active=None):
        """Run stages on data already in the context (svo_put_* / previous svo_process), no prev/cur shift.  active: the mask the
        frame's first call ran with (process_host)."""
        self._process(None, (flags | FLAG_NO_SHIFT) & ~RUN_DETECT, self._mask(active)[0])

    def wait(self):
        self._ck(self.L.svo_wait(self.h), "svo_wait")

    def result(self, lane=0) -> Result:
        r = Result()
        self._ck(self.L.svo_get_result(self.h, lane, C.byref(r)), "svo_get_result")
        return r

    def results(self):
        arr = (Result * self.n_lanes)()
        self._ck(self.L.svo_get_results(self.h, arr), "svo_get_results")
        return list(arr)

    def set_pose_covariance(self, enable=True):
        """svo_set_pose_covariance: from now on every stage 5 leaves a PoseCov record per active lane"""
        self._ck(self.L.svo_set_pose_covariance(self.h, 1 if enable else 0), "svo_set_pose_covariance")

    def pose_covariance(self, lane=0) -> PoseCov:
        """the lane's record (waits); .matrix("info" | "cov_delta" | "cov_pose") are numpy 6 x 6 views of it"""
        r = PoseCov()
        self._ck(self.L.svo_get_pose_covariance(self.h, lane, C.byref(r)), "svo_get_pose_covariance")
        return r

    def pose_covariances(self):
        arr = (PoseCov * self.n_lanes)()
        self._ck(self.L.svo_get_pose_covariances(self.h, arr), "svo_get_pose_covariances")
        return list(arr)

    def copy_pose_covariances_async(self, dst_ptr, nbytes):
        self._ck(self.L.svo_copy_pose_covariances_async(self.h, C.c_void_p(dst_ptr), C.c_size_t(nbytes)), "svo_copy_pose_covariances_async")

    def set_landmarks(self, enable=True, std_noise_pixels=0.0):
        """svo_set_landmarks: from now on every stage 5 leaves one Landmark record per tracked pairing of every active lane
        (std_noise_pixels 0: the reference's default of 1)"""
        self._ck(self.L.svo_set_landmarks(self.h, 1 if enable else 0, float(std_noise_pixels)), "svo_set_landmarks")

    def landmarks_enabled(self):
        """(enabled, std_noise_pixels in force)"""
        e, s = C.c_int(0), C.c_double(0)
        self._ck(self.L.svo_get_landmarks_enabled(self.h, C.byref(e), C.byref(s)), "svo_get_landmarks_enabled")
        return bool(e.value), float(s.value)

    def landmarks_info(self, lane=0) -> LandmarksInfo:
        info = LandmarksInfo()
        self._ck(self.L.svo_get_landmarks_info(self.h, lane, C.byref(info)), "svo_get_landmarks_info")
        return info

    def landmarks(self, lane=0):
        """(LandmarksInfo, the lane's records as a numpy array of abi.Landmark) of the last stage 5 (waits)"""
        info = self.landmarks_info(lane)
        rec = np.zeros(max(0, info.n), Landmark)
        if len(rec):
            n = self._ck(self.L.svo_get_landmarks(self.h, lane, _vp(rec), len(rec)), "svo_get_landmarks")
            assert n == len(rec), (n, len(rec))
        return info, rec

    def copy_landmarks_async(self, dst_info_ptr, dst_records_ptr, nbytes):
        """svo_copy_landmarks_async: n_lanes infos and n_lanes x max_kps records into device memory, on the context's stream"""
        self._ck(self.L.svo_copy_landmarks_async(self.h, C.c_void_p(dst_info_ptr), C.c_void_p(dst_records_ptr), C.c_size_t(nbytes)), "svo_copy_landmarks_async")

    def copy_results_async(self, dst_ptr, nbytes):
        self._ck(self.L.svo_copy_results_async(self.h, C.c_void_p(dst_ptr), C.c_size_t(nbytes)), "svo_copy_results_async")

    # -- lists -----------------------------------------------------------------------------------------
    def keypoints(self, lane=0, which=0, side=0, octave=0):
        n = self._ck(self.L.svo_get_keypoints_oct(self.h, lane, which, side, octave, None, None, 0), "svo_get_keypoints_oct")
        k = np.zeros(n, keypoint_dtype)
        d = np.zeros((n, 32), np.uint8)
        if n:
            self._ck(self.L.svo_get_keypoints_oct(self.h, lane, which, side, octave, _vp(k), _vp(d), n), "svo_get_keypoints_oct")
        return k, d

    def row_index(self, lane=0, which=0, side=0, octave=0):
        n = self._ck(self.L.svo_get_row_index(self.h, lane, which, side, octave, None, 0), "svo_get_row_index")
        a = np.zeros(n, np.int32)
        if n:
            self._ck(self.L.svo_get_row_index(self.h, lane, which, side, octave, _vp(a), n), "svo_get_row_index")
        return a

    def matches_row_index(self, lane=0, which=0, octave=0):
        n = self._ck(self.L.svo_get_matches_row_index(self.h, lane, which, octave, None, 0), "svo_get_matches_row_index")
        a = np.zeros(n, np.int32)
        if n:
            self._ck(self.L.svo_get_matches_row_index(self.h, lane, which, octave, _vp(a), n), "svo_get_matches_row_index")
        return a

    def raw_keypoints(self, lane=0, side=0):
        n = self._ck(self.L.svo_debug_get_raw_keypoints(self.h, lane, side, None, None, 0), "svo_debug_get_raw_keypoints")
        k = np.zeros(n, keypoint_dtype)
        d = np.zeros((n, 32), np.uint8)
        if n:
            self._ck(self.L.svo_debug_get_raw_keypoints(self.h, lane, side, _vp(k), _vp(d), n), "svo_debug_get_raw_keypoints")
        return k, d

    def level(self, lane, side, level):
        w, h = C.c_int(0), C.c_int(0)
        n = self._ck(self.L.svo_debug_get_level(self.h, lane, side, level, None, 0, C.byref(w), C.byref(h)), "svo_debug_get_level")
        out = np.zeros((h.value, w.value), np.uint8)
        self._ck(self.L.svo_debug_get_level(self.h, lane, side, level, _vp(out), n, C.byref(w), C.byref(h)), "svo_debug_get_level")
        return out

    def redo_count(self, reset=False):
        """(image, level) pairs whose speculative FAST threshold failed (a second FAST pass at the caller's threshold) since creation / the last reset"""
        v = C.c_uint32(0)
        self._ck(self.L.svo_debug_get_redo_count(self.h, C.byref(v), int(bool(reset))), "svo_debug_get_redo_count")
        return int(v.value)

    def timeline(self, reset=False):
        """SVO_TIMELINE=1: (frame counter, array [16 frames][32 kinds][8 aux][2] of wall-clock ticks (10 ns), t0 = 2**64 - 1 where nothing ran)"""
        a = np.zeros((16, 32, 8, 2), np.uint64)
        n = self._ck(self.L.svo_debug_timeline(self.h, _vp(a), 16 * 256, int(bool(reset))), "svo_debug_timeline")
        return n, a

    def graph_count(self):
        """(graphs captured, calls served by a replay) under use_graphs since the context was created"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        self._ck(self.L.svo_debug_get_graph_count(self.h, C.byref(a), C.byref(b)), "svo_debug_get_graph_count")
        return int(a.value), int(b.value)

    def status_word(self, lane=0):
        w = C.c_uint32(0)
        self._ck(self.L.svo_debug_get_status_word(self.h, lane, C.byref(w)), "svo_debug_get_status_word")
        return w.value

    def matches(self, lane=0, which=0, octave=0):
        n = self._ck(self.L.svo_get_matches_oct(self.h, lane, which, octave, None, 0), "svo_get_matches_oct")
        m = np.zeros(n, dmatch_dtype)
        if n:
            self._ck(self.L.svo_get_matches_oct(self.h, lane, which, octave, _vp(m), n), "svo_get_matches_oct")
        return m

    def match_ids(self, lane=0, which=0, octave=0):
        n = self._ck(self.L.svo_get_match_ids(self.h, lane, which, octave, None, 0), "svo_get_match_ids")
        a = np.zeros(n, np.int32)
        if n:
            self._ck(self.L.svo_get_match_ids(self.h, lane, which, octave, _vp(a), n), "svo_get_match_ids")
        return a

    def reset_ids(self, lane=-1):
        self._ck(self.L.svo_reset_ids(self.h, lane), "svo_reset_ids")

    def set_this_frame_as_kf(self, lane=0):
        self._ck(self.L.svo_set_this_frame_as_kf(self.h, lane), "svo_set_this_frame_as_kf")

    def tracked(self, lane=0, octave=0):
        n = self._ck(self.L.svo_get_tracked_oct(self.h, lane, octave, None, 0), "svo_get_tracked_oct")
        t = np.zeros(n, index_pair_dtype)
        if n:
            self._ck(self.L.svo_get_tracked_oct(self.h, lane, octave, _vp(t), n), "svo_get_tracked_oct")
        return t

    def residuals(self, lane=0):
        n = self._ck(self.L.svo_get_residuals(self.h, lane, None, 0), "svo_get_residuals")
        r = np.zeros(n, np.float64)
        if n:
            self._ck(self.L.svo_get_residuals(self.h, lane, _vp(r), n), "svo_get_residuals")
        return r

    def outliers(self, lane=0):
        n = self._ck(self.L.svo_get_outliers(self.h, lane, None, 0), "svo_get_outliers")
        r = np.zeros(n, np.int32)
        if n:
            self._ck(self.L.svo_get_outliers(self.h, lane, _vp(r), n), "svo_get_outliers")
        return r

    def values(self, lane=0, which=0, octave=0):
        """getValues (H:704-724) in one device synchronisation: (left_kps, left_desc, right_kps, right_desc, matches, ids)."""
        mk = self.max_kps
        kl, kr = np.zeros(mk, keypoint_dtype), np.zeros(mk, keypoint_dtype)
        dl, dr = np.zeros((mk, 32), np.uint8), np.zeros((mk, 32), np.uint8)
        m, ids = np.zeros(mk, dmatch_dtype), np.zeros(mk, np.int32)
        v = Values(kl.ctypes.data, dl.ctypes.data, kr.ctypes.data, dr.ctypes.data, m.ctypes.data, ids.ctypes.data, mk, mk, 0, 0, 0, 0)
        self._ck(self.L.svo_get_values(self.h, lane, which, octave, C.byref(v)), "svo_get_values")
        return kl[:v.n_left].copy(), dl[:v.n_left].copy(), kr[:v.n_right].copy(), dr[:v.n_right].copy(), m[:v.n_matches].copy(), ids[:v.n_ids].copy()

    # -- precomputed-data bypass -------------------------------------------------------------------------
    def put_features(self, lane, which, side, kps, desc, img_w, img_h, octave=0):
        kps = np.ascontiguousarray(kps)
        desc = None if desc is None else np.ascontiguousarray(desc, np.uint8)
        self._ck(self.L.svo_put_features_oct(self.h, lane, which, side, octave, _vp(kps), _vp(desc), len(kps), img_w, img_h), "svo_put_features_oct")

    def put_matches(self, lane, which, m, octave=0):
        m = np.ascontiguousarray(m)
        self._ck(self.L.svo_put_matches_oct(self.h, lane, which, octave, _vp(m), len(m)), "svo_put_matches_oct")

    def put_match_ids(self, lane, which, ids, octave=0):
        ids = np.ascontiguousarray(ids, np.int32)
        self._ck(self.L.svo_put_match_ids_oct(self.h, lane, which, octave, _vp(ids), len(ids)), "svo_put_match_ids_oct")

    def put_tracked(self, lane, t, octave=None):
        """octave None: svo_put_tracked (octave 0, the lane's other octaves emptied); else svo_put_tracked_oct (that octave alone)"""
        t = np.ascontiguousarray(t)
        if octave is None: self._ck(self.L.svo_put_tracked(self.h, lane, _vp(t), len(t)), "svo_put_tracked")
        else: self._ck(self.L.svo_put_tracked_oct(self.h, lane, int(octave), _vp(t), len(t)), "svo_put_tracked_oct")

    def change_in_pose(self, tracked, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r, cam, init6=None):
        n = len(tracked)
        res = Result()
        residual = np.zeros(max(n, 1), np.float64)
        outl = np.zeros(max(n, 1), np.int32)
        init = None if init6 is None else np.ascontiguousarray(init6, np.float64)
        arrs = [np.ascontiguousarray(a) for a in (tracked, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r)]
        rc = self.L.svo_change_in_pose(self.h, _vp(arrs[0]), n, _vp(arrs[1]), len(pre_m), _vp(arrs[2]), len(cur_m),
                                       _vp(arrs[3]), len(pre_l), _vp(arrs[4]), len(pre_r), _vp(arrs[5]), len(cur_l), _vp(arrs[6]), len(cur_r),
                                       C.byref(cam), _vp(init), C.byref(res), _vp(residual), _vp(outl))
        self._ck(rc, "svo_change_in_pose")
        return bool(rc), res, residual[:res.n_residual], outl[:res.n_outliers]

    def hamming_match(self, q, t):
        q = np.ascontiguousarray(q, np.uint8).reshape(-1, 32)
        t = np.ascontiguousarray(t, np.uint8).reshape(-1, 32)
        idx = np.zeros(max(len(q), 1), np.int32)
        dist = np.zeros(max(len(q), 1), np.int32)
        self._ck(self.L.svo_hamming_match(self.h, _vp(q), len(q), _vp(t), len(t), _vp(idx), _vp(dist)), "svo_hamming_match")
        return idx[:len(q)], dist[:len(q)]

    # -- pyramidal Lucas-Kanade tracking on caller lists (svo_lk_track) ------------------------------------------
    def lk_track(self, jobs, params=None, device=False, pinned=False, _entry="svo_lk_track"):
        """jobs: a list of (prev, next, pts[, init]) -- prev / next uint8 [h, w] numpy arrays (any row stride; the last axis must be
        contiguous), pts / init [n, 2] float32 (x, y).  With device=True prev / next are (device address, w, h, stride) tuples, read in
        place; pinned=True declares the host arrays page-locked.  params: an LkParams (None: the defaults).  Returns a
        (next_pts [n, 2] float32, status [n] uint8, err [n] float32) triple per job.  Synchronises."""
        recs = (LkJob * max(1, len(jobs)))()
        keep, out = [], []
        for i, job in enumerate(jobs):
            prev, nxt, pts = job[0], job[1], np.ascontiguousarray(job[2], np.float32).reshape(-1, 2)
            init = None if len(job) < 4 or job[3] is None else np.ascontiguousarray(job[3], np.float32).reshape(-1, 2)
            if init is not None and len(init) != len(pts):
                raise ValueError("job %d: %d points but %d first guesses" % (i, len(pts), len(init)))
            for s, im in enumerate((prev, nxt)):
                if device:
                    rec = LkImage(int(im[0]), int(im[1]), int(im[2]), int(im[3]))
                else:
                    if im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1):
                        raise ValueError("job %d: uint8 [h, w] images with contiguous rows are expected" % i)
                    keep.append(im)
                    rec = LkImage(im.ctypes.data, im.shape[1], im.shape[0], im.strides[0])
                if s: recs[i].next = rec
                else: recs[i].prev = rec
            n = len(pts)
            res = (np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32))
            keep += [pts, init]
            recs[i].pts, recs[i].init, recs[i].n = _vp(pts) if n else None, _vp(init) if (n and init is not None) else None, n
            recs[i].next_pts, recs[i].status, recs[i].err = (_vp(a) if n else None for a in res)
            out.append(res)
        flags = FLAG_DEVICE_IMAGES if device else (FLAG_PINNED_IMAGES if pinned else 0)
        self._ck(getattr(self.L, _entry)(self.h, recs, len(jobs), C.byref(params) if params is not None else None, C.c_uint32(flags)), _entry)
        return out

    def lk_track_rows(self, jobs, params=None, device=False, pinned=False):
        """lk_track's records, flags and results with the row tracker (svo_lk_track_rows): the template of a point comes from prev at pts,
        and its partner is searched in next along the row of the guess (init, else pts) -- x alone moves, the returned y is the guess's.
        For a rectified stereo pair prev is the left image and next the right one.  Synchronises."""
        return self.lk_track(jobs, params, device, pinned, _entry="svo_lk_track_rows")

    def lk_level(self, job, which, level):
        """pyramid level `level` of image `which` (0 prev, 1 next) of job `job` of the last lk_track call as a uint8 [h, w] array; None
        when that call built no such level"""
        w, h = C.c_int(0), C.c_int(0)
        n = self._ck(self.L.svo_debug_lk_get_level(self.h, int(job), int(which), int(level), None, 0, C.byref(w), C.byref(h)), "svo_debug_lk_get_level")
        if n == 0:
            return None
        out = np.zeros((h.value, w.value), np.uint8)
        self._ck(self.L.svo_debug_lk_get_level(self.h, int(job), int(which), int(level), _vp(out), n, C.byref(w), C.byref(h)), "svo_debug_lk_get_level")
        return out

    # -- Shi-Tomasi corner detection on caller images (svo_gftt_detect) ------------------------------------------
    def gftt_detect(self, jobs, params=None, device=False, pinned=False):
        """jobs: a list of (image, seeds or None[, cap]) -- image a uint8 [h, w] numpy array (any row stride; the last axis must be
        contiguous), seeds [n, 2] float32 (x, y): points new corners keep min_distance from; cap: room for corners (default: the
        context's max_kps).  With device=True image is an (address, w, h, stride) tuple, read in place; pinned=True declares the host
        arrays page-locked.  params: a GfttParams (None: the defaults).  Returns a (pts [n, 2] float32, response [n] float32, n_cand,
        status) tuple per job.  Synchronises."""
        recs = (GfttJob * max(1, len(jobs)))()
        keep, bufs = [], []
        for i, job in enumerate(jobs):
            im = job[0]
            seeds = None if len(job) < 2 or job[1] is None else np.ascontiguousarray(job[1], np.float32).reshape(-1, 2)
            cap = int(job[2]) if len(job) > 2 and job[2] is not None else int(self.max_kps)
            if device:
                recs[i].img = LkImage(int(im[0]), int(im[1]), int(im[2]), int(im[3]))
            else:
                if im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1):
                    raise ValueError("job %d: a uint8 [h, w] image with contiguous rows is expected" % i)
                recs[i].img = LkImage(im.ctypes.data, im.shape[1], im.shape[0], im.strides[0])
            res = (np.zeros((max(cap, 0), 2), np.float32), np.zeros(max(cap, 0), np.float32), np.zeros(3, np.int32))
            keep += [im, seeds]
            recs[i].seeds, recs[i].n_seeds, recs[i].cap = _vp(seeds) if seeds is not None else None, 0 if seeds is None else len(seeds), cap
            recs[i].pts, recs[i].response, recs[i].info = (_vp(res[0]) if cap > 0 else None), (_vp(res[1]) if cap > 0 else None), _vp(res[2])
            bufs.append(res)
        flags = FLAG_DEVICE_IMAGES if device else (FLAG_PINNED_IMAGES if pinned else 0)
        self._ck(self.L.svo_gftt_detect(self.h, recs, len(jobs), C.byref(params) if params is not None else None, C.c_uint32(flags)), "svo_gftt_detect")
        return [(pts[:info[0]].copy(), resp[:info[0]].copy(), int(info[1]), int(info[2])) for pts, resp, info in bufs]

    def gftt_response(self, job):
        """the response map of job `job` of the last gftt_detect call as a float32 [h, w] array; None when that call had no such job"""
        w, h = C.c_int(0), C.c_int(0)
        n = self._ck(self.L.svo_debug_gftt_get_response(self.h, int(job), None, 0, C.byref(w), C.byref(h)), "svo_debug_gftt_get_response")
        if n == 0:
            return None
        out = np.zeros((h.value, w.value), np.float32)
        self._ck(self.L.svo_debug_gftt_get_response(self.h, int(job), _vp(out), n, C.byref(w), C.byref(h)), "svo_debug_gftt_get_response")
        return out

    # -- the resident KLT front end (svo_klt_step) -----------------------------------------------------------------
    def _words(self, active):
        if active is None:
            return None
        w = list(lane_mask_words(active, self.n_lanes)) + [0]
        return (C.c_uint64 * 2)(w[0], w[1])

    def klt_enable(self, params=None):
        """allocates the front end; params: a KltParams (None: the defaults, cap = min(1024, max_kps))"""
        self._ck(self.L.svo_klt_enable(self.h, C.byref(params) if params is not None else None), "svo_klt_enable")

    def klt_reset(self, active=None):
        """empties the tables of the lanes of `active` (None: all) and forgets their last image pairs"""
        self._ck(self.L.svo_klt_reset(self.h, self._words(active)), "svo_klt_reset")

    def klt_add_points(self, lane, left_xy, right_xy):
        """appends (left, right) point pairs ([n, 2] float32 each) to the lane's table; returns how many went in"""
        l = np.ascontiguousarray(left_xy, np.float32).reshape(-1, 2)
        r = np.ascontiguousarray(right_xy, np.float32).reshape(-1, 2)
        if len(l) != len(r):
            raise ValueError("%d left points but %d right points" % (len(l), len(r)))
        return self._ck(self.L.svo_klt_add_points(self.h, int(lane), _vp(l), _vp(r), len(l)), "svo_klt_add_points")

    def klt_step(self, frames, flags=RUN_OPTIMIZE, active=None, device=False, pinned=False):
        """frames: one (left, right) pair per lane -- uint8 [h, w] numpy arrays (any row stride), or with device=True / pinned=True
        (address, w, h, stride) tuples; the entries of lanes outside `active` are not read and may be None.  flags: RUN_OPTIMIZE or 0."""
        assert len(frames) == self.n_lanes
        fr = (Frame * self.n_lanes)()
        keep = []
        _, idle = self._mask(active)
        for i, pr in enumerate(frames):
            if i in idle:
                continue
            for s, im in enumerate(pr):
                if device or pinned:
                    rec = Image(int(im[0]), int(im[1]), int(im[2]), int(im[3]))
                else:
                    if im.dtype != np.uint8 or im.ndim != 2 or (im.shape[1] > 1 and im.strides[1] != 1):
                        raise ValueError("lane %d: uint8 [h, w] images with contiguous rows are expected" % i)
                    keep.append(im)
                    rec = Image(im.ctypes.data, im.shape[1], im.shape[0], im.strides[0])
                if s: fr[i].right = rec
                else: fr[i].left = rec
        flags = (flags & ~(FLAG_DEVICE_IMAGES | FLAG_PINNED_IMAGES)) | (FLAG_DEVICE_IMAGES if device else (FLAG_PINNED_IMAGES if pinned else 0))
        self._ck(self.L.svo_klt_step(self.h, fr, C.c_uint32(flags), self._words(active)), "svo_klt_step")

    def klt_tracks(self, lane=0):
        """(left [n, 2] float32, right [n, 2] float32, ids [n] int32, age [n] int32) of the lane's live tracks.  Synchronises."""
        n = self._ck(self.L.svo_klt_get_tracks(self.h, int(lane), None, None, None, None, 0), "svo_klt_get_tracks")
        l, r = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)
        ids, age = np.zeros(n, np.int32), np.zeros(n, np.int32)
        if n:
            self._ck(self.L.svo_klt_get_tracks(self.h, int(lane), _vp(l), _vp(r), _vp(ids), _vp(age), n), "svo_klt_get_tracks")
        return l, r, ids, age

    def klt_debug_select(self, lane, left_xy, right_xy, status_l, status_r):
        """the shift and the selection of a step on one lane, with these arrays in place of the tracker's results (svo_debug_klt_select)"""
        l = np.ascontiguousarray(left_xy, np.float32).reshape(-1, 2)
        r = np.ascontiguousarray(right_xy, np.float32).reshape(-1, 2)
        sl, sr = np.ascontiguousarray(status_l, np.uint8), np.ascontiguousarray(status_r, np.uint8)
        if not (len(l) == len(r) == len(sl) == len(sr)):
            raise ValueError("four arrays of one length are expected")
        self._ck(self.L.svo_debug_klt_select(self.h, int(lane), _vp(l), _vp(r), _vp(sl), _vp(sr), len(l)), "svo_debug_klt_select")

    # -- the resident top-up of the front end (svo_klt_topup) -------------------------------------------------------
    def klt_topup_default_params(self) -> KltTopupParams:
        """the defaults for this context's front end: below = (cap + 1) / 2, target = cap"""
        p = KltTopupParams()
        self.L.svo_klt_topup_default_params(self.h, C.byref(p))
        return p

    def klt_topup_enable(self, params=None, **fields):
        """allocates the top-up's buffers.  params: a KltTopupParams (None: the defaults); keyword arguments override single fields --
        below, target, init_disp, and max_corners, block, min_distance, quality of the detector.  Returns the parameters in force."""
        p = self.klt_topup_default_params() if params is None else params
        if fields:
            q = KltTopupParams()
            C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
            p = q
            for k, v in fields.items():
                setattr(p.gftt if k in ("max_corners", "block", "min_distance", "quality") else p, k, v)
        self._ck(self.L.svo_klt_topup_enable(self.h, C.byref(p) if (params is not None or fields) else None), "svo_klt_topup_enable")
        return p

    def klt_topup(self, active=None):
        """tops up the thinned lanes of `active` (None: all) on the device; enqueues only"""
        self._ck(self.L.svo_klt_topup(self.h, self._words(active)), "svo_klt_topup")

    def klt_topup_info(self, lane=0):
        """(corners detected, candidates, tracks appended, reason) of the lane in the last top-up; reason: abi.TOPUP_*.  Synchronises."""
        info = np.zeros(4, np.int32)
        self._ck(self.L.svo_klt_topup_info(self.h, int(lane), _vp(info)), "svo_klt_topup_info")
        return tuple(int(v) for v in info)

    def klt_debug_topup_append(self, lane, left_xy, right_xy, status):
        """the gate and the append of a top-up on one lane, with these arrays in place of the detector's corners and the tracker's
        results (svo_debug_klt_topup_append)"""
        l = np.ascontiguousarray(left_xy, np.float32).reshape(-1, 2)
        r = np.ascontiguousarray(right_xy, np.float32).reshape(-1, 2)
        st = np.ascontiguousarray(status, np.uint8)
        if not (len(l) == len(r) == len(st)):
            raise ValueError("three arrays of one length are expected")
        self._ck(self.L.svo_debug_klt_topup_append(self.h, int(lane), _vp(l), _vp(r), _vp(st), len(l)), "svo_debug_klt_topup_append")

    # -- the RANSAC gate (svo_ransac_tracked, svo_klt_set_ransac) ---------------------------------------------------
    def ransac_tracked(self, active=None):
        """stage 4's fundamental-matrix RANSAC on the tracked pairs the lanes of `active` (None: all) hold, every octave: the pairs both
        masks keep replace the list, the lane's track_stats describe the call.  Enqueues only (svo_ransac_tracked)"""
        self._ck(self.L.svo_ransac_tracked(self.h, self._words(active)), "svo_ransac_tracked")

    def klt_set_ransac(self, mode):
        """the RANSAC gate of svo_klt_step: abi.KLT_RANSAC_OFF (0, the default), KLT_RANSAC_FILTER (1: the tracked pairs are filtered) or
        KLT_RANSAC_PRUNE (2: and the rejected tracks leave the table).  After klt_enable."""
        self._ck(self.L.svo_klt_set_ransac(self.h, int(mode)), "svo_klt_set_ransac")

    def klt_ransac(self):
        """the mode svo_klt_set_ransac left"""
        return self._ck(self.L.svo_klt_get_ransac(self.h), "svo_klt_get_ransac")

    # -- the pose prediction of the front end (svo_klt_set_prediction) ------------------------------------------------
    def klt_set_prediction(self, mode):
        """where the forward pass of svo_klt_step starts: abi.KLT_PREDICT_OFF (0, the default: at the track's old position) or
        KLT_PREDICT_POSE (1: the track triangulated, moved by the lane's last pose increment and reprojected).  After klt_enable."""
        self._ck(self.L.svo_klt_set_prediction(self.h, int(mode)), "svo_klt_set_prediction")

    def klt_prediction(self):
        """the mode svo_klt_set_prediction left"""
        return self._ck(self.L.svo_klt_get_prediction(self.h), "svo_klt_get_prediction")

    # -- the stereo re-association of the front end (svo_klt_set_stereo) ----------------------------------------------
    def klt_set_stereo(self, mode):
        """how klt_step finds a track's right point: abi.KLT_STEREO_TEMPORAL (0, the default: the right list is tracked through time) or
        KLT_STEREO_ROW (1: the partner of the new left point is found in the new pair along its row).  After klt_enable."""
        self._ck(self.L.svo_klt_set_stereo(self.h, int(mode)), "svo_klt_set_stereo")

    def klt_get_stereo(self):
        """the mode svo_klt_set_stereo left"""
        return self._ck(self.L.svo_klt_get_stereo(self.h), "svo_klt_get_stereo")

    # -- the photometric mode of the trackers (svo_lk_set_photometric) ------------------------------------------------
    def lk_set_photometric(self, mode):
        """what every LK launch of the context minimises: 0 (the default) raw differences, 1 the differences with an affine brightness
        change between template and target removed per window (tests/lk_photo_ref.py).  lk_track, lk_track_rows, klt_step and klt_topup
        follow it; klt_enable does not reset it.  Any time after the context exists."""
        self._ck(self.L.svo_lk_set_photometric(self.h, int(mode)), "svo_lk_set_photometric")

    def lk_get_photometric(self):
        """the mode svo_lk_set_photometric left"""
        return self._ck(self.L.svo_lk_get_photometric(self.h), "svo_lk_get_photometric")

    def _klt_guesses(self, what, call):
        n = self._ck(call(None, None, None, 0), what)
        l, r, used = np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32), np.zeros(n, np.uint8)
        if n:
            self._ck(call(_vp(l), _vp(r), _vp(used), n), what)
        return l, r, used

    def klt_predicted(self, lane=0):
        """(left [n, 2] float32, right [n, 2] float32, used [n] uint8): the guesses the next klt_step would start the lane's live tracks
        from as things stand now; used = 0: the track's own points.  Needs mode 1.  Synchronises (svo_klt_predicted)."""
        return self._klt_guesses("svo_klt_predicted", lambda l, r, u, cap: self.L.svo_klt_predicted(self.h, int(lane), l, r, u, cap))

    def debug_klt_predict(self, lane, delta6, valid):
        """klt_predicted with `delta6` (six float64: the rotation vector, the translation) and `valid` in place of the lane's result
        record (svo_debug_klt_predict)"""
        d = np.ascontiguousarray(delta6, np.float64).reshape(6)
        return self._klt_guesses("svo_debug_klt_predict", lambda l, r, u, cap: self.L.svo_debug_klt_predict(self.h, int(lane), _vp(d), int(valid), l, r, u, cap))

    # -- timing ----------------------------------------------------------------------------------------
    FRAME_KERNEL_NAMES = 32

    def kernel_times(self, appended=False):
        """{name: (total ms, calls)} in the order of the C list.  Its first 32 names are the kernels of svo_process and of the
        hand-over calls; the names appended behind them belong to other entry points ("gather_windows": svo_gather_windows;
        "gftt_response", "gftt_candidates", "gftt_select": svo_gftt_detect, "lk_pyrdown", "lk_track": svo_lk_track and svo_klt_step, and
        "klt_select": svo_klt_step, "klt_topup": svo_klt_topup, "ransac_feed": svo_ransac_tracked and a step under klt_set_ransac,
        "klt_prune": a step in mode 2, "klt_predict": a step under klt_set_prediction(1), klt_predicted and debug_klt_predict,
        "lk_track_row": lk_track_rows and a step under klt_set_stereo(1),
        each listed once the context has made such a call) and are
        included with appended=True, so that a reader of the frame's launches finds the list it always found."""
        names = (C.c_char_p * 64)()
        tot = (C.c_double * 64)()
        calls = (C.c_int64 * 64)()
        n = self._ck(self.L.svo_kernel_times(self.h, names, tot, calls, 64), "svo_kernel_times")
        return {names[i].decode(): (tot[i], calls[i]) for i in range(n if appended else min(n, self.FRAME_KERNEL_NAMES))}

    def kernel_times_select(self, name=None):
        self._ck(self.L.svo_kernel_times_select(self.h, name.encode() if name else None), "svo_kernel_times_select")

    def kernel_times_reset(self):
        self._ck(self.L.svo_kernel_times_reset(self.h), "svo_kernel_times_reset")
