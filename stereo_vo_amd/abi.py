"""ctypes / numpy mirrors of include/svo_types.h (the POD records that cross the C-ABI).

Pure declarations: importing this module loads no native library.
"""
import ctypes as C
import numpy as np

MAX_OCTAVES = 4
DESC_BYTES = 32

# == cv::KeyPoint / cv::DMatch layouts (libstereo-odometry.h:108-109)
keypoint_dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])
dmatch_dtype = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
index_pair_dtype = np.dtype([("first", "<i4"), ("second", "<i4")])
assert keypoint_dtype.itemsize == 28 and dmatch_dtype.itemsize == 16 and index_pair_dtype.itemsize == 8

VOEC_NONE, VOEC_BAD_COND_NUMBER, VOEC_INCR_FUNC_COST_STG1, VOEC_INCR_FUNC_COST_STG2, VOEC_FIRST_ITERATION, VOEC_BAD_TRACKING = range(6)
DM_ORB, DM_FAST_ORB, DM_FASTER, DM_KLT = range(4)
SM_DESC_BF, SM_DESC_RBR, SM_SAD = range(3)
IFM_DESC_BF, IFM_DESC_WIN, IFM_SAD, IFM_OPTICAL_FLOW = range(4)


class StereoCamera(C.Structure):
    _fields_ = [("l_fx", C.c_double), ("l_fy", C.c_double), ("l_cx", C.c_double), ("l_cy", C.c_double),
                ("r_fx", C.c_double), ("r_fy", C.c_double), ("r_cx", C.c_double), ("r_cy", C.c_double),
                ("baseline", C.c_double), ("ncols", C.c_int32), ("nrows", C.c_int32)]

    @classmethod
    def simple(cls, f, cx, cy, baseline, ncols, nrows):
        return cls(f, f, cx, cy, f, f, cx, cy, baseline, ncols, nrows)


class Params(C.Structure):
    _fields_ = [
        ("nOctaves", C.c_int32),
        ("detect_method", C.c_int32), ("non_maximal_suppression", C.c_int32), ("nmsMethod", C.c_int32),
        ("min_distance", C.c_int32), ("orb_nfeats", C.c_int32), ("orb_nlevels", C.c_int32),
        ("fast_min_th", C.c_int32), ("fast_max_th", C.c_int32), ("initial_FAST_threshold", C.c_int32),
        ("minimum_ORB_response", C.c_double),
        ("match_method", C.c_int32), ("enable_robust_1to1_match", C.c_int32),
        ("orb_min_th", C.c_int32), ("orb_max_th", C.c_int32),
        ("max_y_diff", C.c_double), ("orb_max_distance", C.c_double),
        ("ifm_method", C.c_int32), ("ifm_win_w", C.c_int32), ("ifm_win_h", C.c_int32), ("filter_fund_matrix", C.c_int32),
        ("use_robust_kernel", C.c_int32), ("max_iters", C.c_int32), ("initial_max_iters", C.c_int32),
        ("max_incr_cost", C.c_int32), ("bad_tracking_th", C.c_int32), ("use_previous_pose_as_initial", C.c_int32),
        ("use_custom_initial_pose", C.c_int32), ("sad_max_distance", C.c_int32),
        ("kernel_param", C.c_double), ("min_mod_out_vector", C.c_double), ("residual_threshold", C.c_double),
        ("vo_use_matches_ids", C.c_int32), ("ifm_sad_max_distance", C.c_int32),
    ]

    def copy(self):
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        return q


class Result(C.Structure):
    _fields_ = [
        ("outPose", C.c_double * 6), ("delta", C.c_double * 6),
        ("num_it", C.c_int32), ("num_it_final", C.c_int32), ("valid", C.c_int32), ("error_code", C.c_int32),
        ("tracked_feats_from_last_KF", C.c_int32), ("tracked_feats_from_last_frame", C.c_int32),
        ("detected_left", C.c_int32 * 4), ("detected_right", C.c_int32 * 4), ("stereo_matches", C.c_int32 * 4),
        ("n_octaves", C.c_int32), ("n_outliers", C.c_int32), ("n_residual", C.c_int32), ("status", C.c_int32),
        ("track_stats", C.c_int32 * 8),
    ]

COV_NONE, COV_OK, COV_RANK_DEFICIENT, COV_NO_DOF, COV_DELTA_ONLY = range(5)


class PoseCov(C.Structure):
    """svo_pose_cov (include/svo_types.h): the covariance of a lane's pose increment; matrices 6 x 6 row-major"""
    _fields_ = [("info", C.c_double * 36), ("cov_delta", C.c_double * 36), ("cov_pose", C.c_double * 36),
                ("sigma2", C.c_double), ("n_used", C.c_int32), ("dof", C.c_int32), ("state", C.c_int32), ("reserved", C.c_int32)]

    def matrix(self, name):
        """numpy 6 x 6 view of info / cov_delta / cov_pose (shares the record's memory)"""
        return np.ctypeslib.as_array(getattr(self, name)).reshape(6, 6)


assert C.sizeof(PoseCov) == 888

# svo_landmark (include/svo_types.h): one tracked pairing of a frame as stage 5 sees it; covariances as upper triangles xx xy xz yy yz zz
LMK_FINITE, LMK_INLIER, LMK_USED, LMK_POSE, LMK_POSE_TERM = 1, 2, 4, 8, 16
LMK_NONE, LMK_OK, LMK_POINTS_ONLY = range(3)
Landmark = np.dtype([("xyz_prev", "<f8", (3,)), ("cov_prev", "<f8", (6,)), ("xyz_cur", "<f8", (3,)), ("cov_cur", "<f8", (6,)),
                     ("residual", "<f8"), ("match_id", "<i4"), ("prev_match", "<i4"), ("cur_match", "<i4"), ("octave", "<i4"),
                     ("flags", "<u4"), ("reserved", "<i4")])
assert Landmark.itemsize == 176 and Landmark.itemsize % 16 == 0


def cov3(tri):
    """the symmetric 3 x 3 matrices of upper triangles (..., 6) as stored in Landmark.cov_prev / cov_cur"""
    tri = np.asarray(tri)
    return tri[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(tri.shape[:-1] + (3, 3))


class LandmarksInfo(C.Structure):
    """svo_landmarks_info: the lane's record count, how many are finite / inliers, its state and the std_noise_pixels used"""
    _fields_ = [("n", C.c_int32), ("n_finite", C.c_int32), ("n_inliers", C.c_int32), ("state", C.c_int32),
                ("std_noise_pixels", C.c_double), ("reserved", C.c_int32 * 2)]


assert C.sizeof(LandmarksInfo) == 32


class FasterStats(C.Structure):
    """svo_faster_stats (include/svo_types.h): dmFASTER's dynamic thresholds of one lane and the corner counts that moved them, per octave"""
    _fields_ = [("next", C.c_int32 * 4), ("used_left", C.c_int32 * 4), ("used_right", C.c_int32 * 4),
                ("corners_left", C.c_int32 * 4), ("corners_right", C.c_int32 * 4), ("frame", C.c_int32), ("reserved", C.c_int32 * 3)]

    def as_dict(self, n_oct=4):
        d = {k: list(getattr(self, k))[:n_oct] for k in ("next", "used_left", "used_right", "corners_left", "corners_right")}
        d["frame"] = int(self.frame)
        return d


assert C.sizeof(FasterStats) == 96

class CameraModel(C.Structure):
    """svo_camera_model (include/svo_types.h): intrinsics and k1 k2 p1 p2 k3 k4 k5 k6 of one unrectified camera"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 8)]

    @classmethod
    def make(cls, fx, fy, cx, cy, dist=()):
        d = [float(v) for v in dist] + [0.0] * (8 - len(dist))
        return cls(float(fx), float(fy), float(cx), float(cy), (C.c_double * 8)(*d))


class StereoCalibration(C.Structure):
    """svo_stereo_calibration: x_right = R x_left + T (OpenCV's convention, R row-major); alpha must be negative"""
    _fields_ = [("left", CameraModel), ("right", CameraModel), ("R", C.c_double * 9), ("T", C.c_double * 3),
                ("w", C.c_int32), ("h", C.c_int32), ("zero_disparity", C.c_int32), ("reserved", C.c_int32), ("alpha", C.c_double)]

    @classmethod
    def make(cls, left, right, R, T, w, h, zero_disparity=False, alpha=-1.0):
        """left / right: CameraModel or (fx, fy, cx, cy, dist); R: 3 x 3; T: 3"""
        cams = [c if isinstance(c, CameraModel) else CameraModel.make(*c) for c in (left, right)]
        R = np.asarray(R, np.float64).reshape(9); T = np.asarray(T, np.float64).reshape(3)
        return cls(cams[0], cams[1], (C.c_double * 9)(*R), (C.c_double * 3)(*T), int(w), int(h), int(bool(zero_disparity)), 0, float(alpha))


class StereoRectification(C.Structure):
    """svo_stereo_rectification: R1 R2 (3 x 3 row-major), P1 P2 = fx' fy' cx' cy', tx, and the StereoCamera stage 5 works with"""
    _fields_ = [("R1", C.c_double * 9), ("R2", C.c_double * 9), ("P1", C.c_double * 4), ("P2", C.c_double * 4),
                ("tx", C.c_double), ("cam", StereoCamera)]

    def rotation(self, side):
        return np.array(self.R2 if side else self.R1).reshape(3, 3)

    def intrinsics(self, side):
        return np.array(self.P2 if side else self.P1)


assert C.sizeof(CameraModel) == 96 and C.sizeof(StereoCalibration) == 312 and C.sizeof(StereoRectification) == 296

class LkParams(C.Structure):
    """svo_lk_params (include/svo_types.h): window side (odd, 5 .. 31), deepest level (0 .. 5), iterations per level (1 .. 100), the step
    that ends a level, the minimum eigenvalue per pixel, and the forward-backward limit in pixels (0: no such pass)"""
    _fields_ = [("win", C.c_int32), ("max_level", C.c_int32), ("max_iters", C.c_int32),
                ("eps", C.c_float), ("min_eig", C.c_float), ("fb_max", C.c_float)]


class LkImage(C.Structure):
    """svo_image (include/svo_hip.h) as svo_lk_job holds it"""
    _fields_ = [("data", C.c_void_p), ("w", C.c_int32), ("h", C.c_int32), ("stride", C.c_int64)]


class LkJob(C.Structure):
    """svo_lk_job (include/svo_hip.h): one image pair with its points (host arrays) and the arrays the results go to"""
    _fields_ = [("prev", LkImage), ("next", LkImage), ("pts", C.c_void_p), ("init", C.c_void_p), ("n", C.c_int32),
                ("next_pts", C.c_void_p), ("status", C.c_void_p), ("err", C.c_void_p)]


assert C.sizeof(LkParams) == 24 and C.sizeof(LkJob) == 96


class KltParams(C.Structure):
    """svo_klt_params (include/svo_types.h): the tracker's parameters, the tracks per lane, and the gates of the selection --
    |yl - yr| <= max_dy and min_disp <= xl - xr <= max_disp"""
    _fields_ = [("lk", LkParams), ("cap", C.c_int32), ("max_dy", C.c_float), ("min_disp", C.c_float), ("max_disp", C.c_float)]


assert C.sizeof(KltParams) == 40


class GfttParams(C.Structure):
    """svo_gftt_params (include/svo_types.h): the most corners per job (0: as many as cap holds), the block side (3, 5 or 7), the minimum
    distance in pixels (0 .. 255) and the quality level in (0, 1]"""
    _fields_ = [("max_corners", C.c_int32), ("block", C.c_int32), ("min_distance", C.c_int32), ("quality", C.c_float)]


class GfttJob(C.Structure):
    """svo_gftt_job (include/svo_hip.h): one image, the seeds new corners keep their distance from (a host array) and the arrays the
    results go to"""
    _fields_ = [("img", LkImage), ("seeds", C.c_void_p), ("n_seeds", C.c_int32), ("cap", C.c_int32),
                ("pts", C.c_void_p), ("response", C.c_void_p), ("info", C.c_void_p)]


assert C.sizeof(GfttParams) == 16 and C.sizeof(GfttJob) == 64


class KltTopupParams(C.Structure):
    """svo_klt_topup_params (include/svo_types.h): the detector's parameters, the live count below which a lane is topped up, the count
    it is topped up to, and the disparity of a new corner's first guess in the right image"""
    _fields_ = [("gftt", GfttParams), ("below", C.c_int32), ("target", C.c_int32), ("init_disp", C.c_float)]


assert C.sizeof(KltTopupParams) == 28

# svo_klt_topup_info: info[3]
TOPUP_OK, TOPUP_OVERFLOW, TOPUP_ENOUGH, TOPUP_NO_PAIR, TOPUP_NOT_ASKED = range(5)

# svo_klt_set_ransac: the RANSAC gate of svo_klt_step
KLT_RANSAC_OFF, KLT_RANSAC_FILTER, KLT_RANSAC_PRUNE = range(3)

# svo_klt_set_prediction: where the forward pass of svo_klt_step starts its search
KLT_PREDICT_OFF, KLT_PREDICT_POSE = range(2)
# svo_klt_set_stereo: how svo_klt_step finds a track's right point
KLT_STEREO_TEMPORAL, KLT_STEREO_ROW = range(2)

# indices of Result.track_stats (include/svo_types.h SVO_TS_*)
TS_NAMES = ("threshold", "collision", "inliers_left", "inliers_right", "hyp_left", "hyp_right", "both_masks", "tracked")


def north_star_params(base: Params, orb_nfeats=1350) -> Params:
    """SURVEY.md 8d common parameters: ORB + BF (1-to-1, max_y_diff 1, orb_max_distance 60) + BF tracking."""
    p = base.copy()
    p.detect_method = DM_ORB
    p.orb_nfeats = orb_nfeats
    p.orb_nlevels = 8
    p.match_method = SM_DESC_BF
    p.max_y_diff = 1.0
    p.enable_robust_1to1_match = 1
    p.orb_max_distance = 60.0
    p.ifm_method = IFM_DESC_BF
    return p
