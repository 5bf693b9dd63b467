/* svo_types.h -- plain-old-data records that cross the C-ABI boundary of the MI355X stereo-VO hot path.
 *
 * They replace, field for field, the OpenCV / MRPT types that appear in the reference's public interface
 * (libstereo-odometry/include/libstereo-odometry.h, "H" below), which cannot be used here because OpenCV,
 * MRPT and Eigen are absent on both the build container and the GPU box.
 */
#ifndef SVO_TYPES_H
#define SVO_TYPES_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* == cv::KeyPoint field order (pt.x, pt.y, size, angle, response, octave, class_id), 28 bytes. H:108 */
typedef struct svo_keypoint {
    float x, y, size, angle, response;
    int32_t octave, class_id;
} svo_keypoint;

/* == cv::DMatch (queryIdx, trainIdx, imgIdx, distance), 16 bytes. H:109 */
typedef struct svo_dmatch {
    int32_t queryIdx, trainIdx, imgIdx;
    float distance;
} svo_dmatch;

/* one (previous-match-index, current-match-index) entry of rso::vector_index_pairs_t. H:139 */
typedef struct svo_index_pair {
    int32_t first, second;
} svo_index_pair;

/* the fields of mrpt::utils::TStereoCamera that the path reads (S5:185-193, 510-515; C:402-403) */
typedef struct svo_stereo_camera {
    double l_fx, l_fy, l_cx, l_cy;
    double r_fx, r_fy, r_cx, r_cy;
    double baseline;        /* rightCameraPose[0] */
    int32_t ncols, nrows;   /* leftCamera.ncols / nrows (used by getChangeInPose for the NMS grid) */
} svo_stereo_camera;

/* rso::VOErrorCode, same numeric values. H:142 */
enum {
    SVO_VOEC_NONE = 0, SVO_VOEC_BAD_COND_NUMBER = 1, SVO_VOEC_INCR_FUNC_COST_STG1 = 2,
    SVO_VOEC_INCR_FUNC_COST_STG2 = 3, SVO_VOEC_FIRST_ITERATION = 4, SVO_VOEC_BAD_TRACKING = 5
};

/* TDetectParams::TDMethod H:388, NMSMethod H:387, TSMMethod H:454, TIFMMethod H:291 */
enum { SVO_DM_ORB = 0, SVO_DM_FAST_ORB = 1, SVO_DM_FASTER = 2, SVO_DM_KLT = 3 };
enum { SVO_NMS_STANDARD = 0, SVO_NMS_ADAPTIVE = 1 };
enum { SVO_SM_DESC_BF = 0, SVO_SM_DESC_RBR = 1, SVO_SM_SAD = 2 };
enum { SVO_IFM_DESC_BF = 0, SVO_IFM_DESC_WIN = 1, SVO_IFM_SAD = 2, SVO_IFM_OPTICAL_FLOW = 3 };

/* The INI keys / struct fields that parameterise the path (H:266-508, H:554-663), one flat record.
 * Field names are the reference's. Defaults: svo_params_defaults() (S2:44-58, S3:46-57, C:69-82, S1:27-30),
 * except that the selectors default to the north-star configuration (ORB + BF + BF): the reference's own defaults are
 * dmFASTER (SVO_DM_FASTER, supported on the SAD path: svo_hip.h; its KLT_win lives on the context, svo_set_klt_win, because this
 * record's layout is frozen), smSAD (SVO_SM_SAD, supported) and none for the tracker.  Not built: SVO_DM_KLT, SVO_IFM_OPTICAL_FLOW,
 * the adaptive NMS under dmFASTER and the dynamic FAST threshold of update_dyn_thresholds. */
typedef struct svo_params {
    /* RECTIFY */
    int32_t nOctaves;
    /* DETECT */
    int32_t detect_method;
    int32_t non_maximal_suppression;
    int32_t nmsMethod;
    int32_t min_distance;
    int32_t orb_nfeats;
    int32_t orb_nlevels;
    int32_t fast_min_th, fast_max_th, initial_FAST_threshold;
    double  minimum_ORB_response;
    /* MATCH */
    int32_t match_method;
    int32_t enable_robust_1to1_match;
    int32_t orb_min_th, orb_max_th;
    double  max_y_diff;
    double  orb_max_distance;
    /* IF-MATCH */
    int32_t ifm_method;
    int32_t ifm_win_w, ifm_win_h;
    int32_t filter_fund_matrix;   /* read by the reference's INI loader, unused by it (H:304) */
    /* LEAST_SQUARES */
    int32_t use_robust_kernel;
    int32_t max_iters, initial_max_iters;
    int32_t max_incr_cost;
    int32_t bad_tracking_th;
    int32_t use_previous_pose_as_initial;
    int32_t use_custom_initial_pose;
    int32_t sad_max_distance;     /* MATCH group (H:458, kept here so that every offset of the record stays): smSAD's largest SAD of two 8 x 8
                                     windows that still counts as a match (S3:201, 334).  0 = the reference's default 200 (S3:48);
                                     negative = no threshold (the reference's unsigned wrap of a negative INI value) */
    double  kernel_param;
    double  min_mod_out_vector;
    double  residual_threshold;
    /* GENERAL */
    int32_t vo_use_matches_ids;
    int32_t ifm_sad_max_distance; /* IF-MATCH group (H:297): ifmSAD's MAX_SAD, per side (S4:448, 573, 577).  0 = 200 (the group has no
                                     constructor default, common.cpp:84; H:297 says "~200"); negative = no threshold (uint32_t wrap) */
} svo_params;

/* TStereoOdometryResult (H:235-264) without the variable-length members, which have their own getters. */
typedef struct svo_result {
    double  outPose[6];      /* x y z yaw pitch roll  (CPose3D of the inverse of delta, S5:717-718) */
    double  delta[6];        /* w1 w2 w3 t1 t2 t3 as optimised (S5:45-52) */
    int32_t num_it, num_it_final;
    int32_t valid;
    int32_t error_code;
    int32_t tracked_feats_from_last_KF, tracked_feats_from_last_frame;
    int32_t detected_left[4], detected_right[4];   /* detected_feats[octave].first/.second */
    int32_t stereo_matches[4];
    int32_t n_octaves;
    int32_t n_outliers;      /* size of result.outliers (which holds INLIER cur-match indices, S5:603-610) */
    int32_t n_residual;      /* size of result.out_residual */
    int32_t status;          /* 0, or capacity bits: 1 = a level's FAST candidate list overflowed svo_config.max_cand, 2 = a keypoint /
                                track list was cut at svo_config.max_kps (the reference has no such limits: stage2_detect.cpp:461-464),
                                4 = svo_import_frame was handed a hand-over record of another layout */
    int32_t track_stats[8];  /* where stage 4's candidates go, summed over the octaves (SVO_TS_*): no reference counterpart -- the
                                reference prints some of them at verbose level 2 (stage4_match_consecutive.cpp:205, 240) */
} svo_result;

/* indices of svo_result.track_stats: previous-frame pairings that ...                                      (ifmDescBF | ifmDescWin) */
enum {
    SVO_TS_THRESHOLD = 0,    /* pass the descriptor-distance threshold on both sides (S4:149)               | = SVO_TS_COLLISION */
    SVO_TS_COLLISION = 1,    /* survive the joint collision filter (S4:145-160): the RANSAC's input         | survivors of S4:640-679 */
    SVO_TS_INLIERS_L = 2,    /* inliers of the left-left fundamental matrix (S4:202-205); 0 = no model */
    SVO_TS_INLIERS_R = 3,    /* inliers of the right-right one (S4:237-240) */
    SVO_TS_HYP_L = 4,        /* hypotheses the left RANSAC visited before its confidence stop */
    SVO_TS_HYP_R = 5,        /* the same, right */
    SVO_TS_BOTH_MASKS = 6,   /* are inliers of both models (S4:243-255; = SVO_TS_COLLISION when a model was not found) */
    SVO_TS_TRACKED = 7       /* also pass the left/right consistency check (S4:282): tracked_pairs */
};

/* The covariance of a lane's pose increment (svo_set_pose_covariance in svo_hip.h; no reference counterpart).  All matrices 6 x 6, row-major.
 *   theta* = svo_result.delta of the same call (w1 w2 w3 t1 t2 t3); M = the tracked pairs still in stage 5's mask when it ended (the mask
 *   itself, not the `outliers` list: with initial_max_iters = 0 that list is empty while the mask is the NMS survivors).
 *   ONE MORE EVALUATION at theta*, written as m_evalRGN writes one (S5:275-390) over the landmarks as last triangulated: predicted
 *   pixels cast to float, residuals r_i in R^4 float minus float, s_i = |r_i|^2, Jacobian J_i (4 x 6); a point whose J_i is not finite is
 *   dropped (S5:322).  U = the n_used points that remain.  w_i = 1 / sqrt(1 + s_i / kernel_param^2) under use_robust_kernel, else 1.
 *   info      = A = sum_U w_i J_i^T J_i: the information for unit pixel variance.  WEIGHTED, unlike the Hessian the iteration solves with
 *               (S5:364-369 weights the gradient only)
 *   sigma2    = sum_U w_i s_i / dof, dof = 4 n_used - 6: the a-posteriori variance factor, px^2
 *   cov_delta = sigma2 * A^-1, in the order of delta
 *   cov_pose  = G cov_delta G^T, G = d outPose / d delta (x y z yaw pitch roll of the inverse transform, S5:717-718), analytic
 * state:
 *   SVO_COV_NONE            the feature is off, or this call's stage 5 did not end with valid = 1 (first frame, bad tracking, every early
 *                           return of stage 5, a cost abort): everything zero
 *   SVO_COV_NO_DOF          dof <= 0: info, n_used, dof set, the rest zero
 *   SVO_COV_RANK_DEFICIENT  A fails the positive-definiteness test of stage 5's own Cholesky solve (k_gn.hip, chol6): info, sigma2,
 *                           n_used, dof set, both covariances zero
 *   SVO_COV_DELTA_ONLY      cos^2(pitch) < 1e-12, where G is singular: cov_pose zero, the rest as for SVO_COV_OK
 *   SVO_COV_OK              every field */
enum { SVO_COV_NONE = 0, SVO_COV_OK = 1, SVO_COV_RANK_DEFICIENT = 2, SVO_COV_NO_DOF = 3, SVO_COV_DELTA_ONLY = 4 };
typedef struct svo_pose_cov {
    double info[36], cov_delta[36], cov_pose[36];
    double sigma2;
    int32_t n_used, dof, state, reserved;
} svo_pose_cov;

/* One tracked left/right pairing of a frame as stage 5 sees it (svo_set_landmarks in svo_hip.h; no reference counterpart: the
 * reference triangulates these points at S5:529-544 and keeps them to itself).  The records of a lane are in the order stage 5
 * concatenates the tracked pairs, octave by octave (S5:419-461), cut at svo_config.max_kps as stage 5 cuts them.
 *   xyz_prev   the point in the PREVIOUS left camera's frame: stage 5's own triangulation (S5:529-544) of the float pixels ul, vl
 *              (previous left) and ur (previous right x), scaled by the octave's scale_norm (S5:422), with the lane's svo_stereo_camera:
 *              den = l_fx (r_cx - ur) + r_fx (ul - l_cx);  X Y Z = baseline / den * (r_fx (ul - l_cx), r_fx (vl - l_cy), l_fx r_fx)
 *   cov_prev   std_noise_pixels^2 * J J^T, J = d(X, Y, Z) / d(ul, vl, ur), analytic (vr does not enter the triangulation): independent
 *              pixel noise of that standard deviation on the three coordinates.  Upper triangle xx xy xz yy yz zz, as cov_cur
 *   xyz_cur    R(w) xyz_prev + t with (w, t) = svo_result.delta of the same call and R the exact Rodrigues rotation: the point in the
 *              CURRENT left camera's frame, where m_evalRGN projects it (S5:180-195)
 *   cov_cur    R cov_prev R^T, plus D cov_delta D^T with D = [d(R X)/dw | I3] when the lane's svo_pose_cov of the same call is
 *              SVO_COV_OK or SVO_COV_DELTA_ONLY (SVO_LMK_POSE_TERM).  THE CROSS-COVARIANCE OF POSE AND LANDMARK IS NEGLECTED: stage 5
 *              holds the landmarks fixed while it solves for the pose, so cov_delta carries no landmark uncertainty, and the pose was
 *              estimated from these very pixels.  cov_cur is the sum of the two terms as if they were independent
 *   residual   s_i = |r_i|^2 of the one more evaluation at delta that svo_pose_cov defines (over the mask stage 5 ended with, pixels
 *              cast to float, float minus float); 0 where the pairing is not in that evaluation (SVO_LMK_USED clear)
 *   match_id   the current frame's match ID of the pairing (H:794), -1 with vo_use_matches_ids off
 *   prev_match, cur_match   the tracked pair's first / second: indices into the previous / current frame's pairings of `octave`
 * flags:
 *   SVO_LMK_FINITE     den != 0 and all of xyz_prev, cov_prev finite.  When clear EVERY double of the record is 0
 *   SVO_LMK_INLIER     in the mask stage 5 ended with (the M of svo_pose_cov)
 *   SVO_LMK_USED       in M and kept by that evaluation (finite Jacobian, S5:322): the U of svo_pose_cov
 *   SVO_LMK_POSE       xyz_cur and cov_cur are set (the lane's state is SVO_LMK_OK and the record is finite)
 *   SVO_LMK_POSE_TERM  cov_cur includes D cov_delta D^T */
enum { SVO_LMK_FINITE = 1, SVO_LMK_INLIER = 2, SVO_LMK_USED = 4, SVO_LMK_POSE = 8, SVO_LMK_POSE_TERM = 16 };
typedef struct svo_landmark {
    double xyz_prev[3], cov_prev[6];
    double xyz_cur[3], cov_cur[6];
    double residual;
    int32_t match_id, prev_match, cur_match, octave;
    uint32_t flags;
    int32_t reserved;
} svo_landmark;
/* per lane.  state:
 *   SVO_LMK_NONE         the feature is off, the lane has no previous frame, was reset, or no call has reached stage 5 yet: n = 0
 *   SVO_LMK_POINTS_ONLY  this call's stage 5 did not end with valid = 1 (bad tracking, fewer than 8 NMS survivors, every early return, a
 *                        cost abort): xyz_prev, cov_prev, the indices, IDs, octave and SVO_LMK_FINITE are set, nothing of the pose is
 *   SVO_LMK_OK           every field
 * n = records of the lane, n_finite = those with SVO_LMK_FINITE, n_inliers = those with SVO_LMK_INLIER (0 unless SVO_LMK_OK),
 * std_noise_pixels = the value cov_prev was scaled with */
enum { SVO_LMK_NONE = 0, SVO_LMK_OK = 1, SVO_LMK_POINTS_ONLY = 2 };
typedef struct svo_landmarks_info {
    int32_t n, n_finite, n_inliers, state;
    double std_noise_pixels;
    int32_t reserved[2];
} svo_landmarks_info;
#ifdef __cplusplus
static_assert(sizeof(svo_landmark) == 176 && sizeof(svo_landmark) % 16 == 0, "svo_landmark: 19 doubles, 6 words, 11 x 16 bytes");
static_assert(sizeof(svo_landmarks_info) == 32, "svo_landmarks_info");
#else
_Static_assert(sizeof(svo_landmark) == 176 && sizeof(svo_landmark) % 16 == 0, "svo_landmark: 19 doubles, 6 words, 11 x 16 bytes");
_Static_assert(sizeof(svo_landmarks_info) == 32, "svo_landmarks_info");
#endif

#define SVO_MAX_OCTAVES 4
#define SVO_DESC_BYTES 32

/* dmFASTER's dynamic threshold of one lane (svo_set_dyn_fast_threshold in svo_hip.h; stage2_detect.cpp:522-550), indexed by octave.
 * What the reference shows as GUI statistics (S2:548-549) plus the thresholds each image was detected at.  Entries of octaves the
 * parameters do not use, and all of used_* / corners_* / frame before the lane's first detection, are 0.
 *   next           m_threshold[octave]: what the lane's next left image is detected at
 *   used_left      the threshold of the last frame's left image; used_right that of its right image (= step(used_left, corners_left))
 *   corners_left   ALL FAST-12 corners found in that image, also those a full candidate list could not hold; corners_right likewise
 *   frame          detections that have moved this lane's thresholds since they were last initialised (1 after the first) */
typedef struct svo_faster_stats {
    int32_t next[SVO_MAX_OCTAVES];
    int32_t used_left[SVO_MAX_OCTAVES], used_right[SVO_MAX_OCTAVES];
    int32_t corners_left[SVO_MAX_OCTAVES], corners_right[SVO_MAX_OCTAVES];
    int32_t frame, reserved[3];
} svo_faster_stats;

/* The calibration of an unrectified stereo rig: what mrpt::vision::CStereoRectifyMap::setFromCamParams reads from the observation's
 * TStereoCamera (stage1_rectify.cpp:66-68) -- intrinsics, distortion and the pose of the right camera -- in OpenCV's conventions.
 *   dist            k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order; mrpt's TCamera::dist holds the first five, the rest 0).  Thin-prism and
 *                   tilt terms are not built.
 *   R, T            x_right = R x_left + T, R row-major: a right camera to the right of the left one has T[0] < 0
 *   zero_disparity  1: CALIB_ZERO_DISPARITY, both rectified principal points are the mean of the two; 0: only their y is (mrpt's default)
 *   alpha           must be negative (cv::stereoRectify's alpha = -1: no scaling to the inner / outer rectangle) */
typedef struct svo_camera_model {
    double fx, fy, cx, cy;
    double dist[8];
} svo_camera_model;
typedef struct svo_stereo_calibration {
    svo_camera_model left, right;
    double R[9];
    double T[3];
    int32_t w, h;
    int32_t zero_disparity;
    int32_t reserved;
    double alpha;
} svo_stereo_calibration;
/* what svo_stereo_rectify makes of it: the rotations that rectify each camera, the rectified intrinsics P = fx' fy' cx' cy' of each
 * (fx' = fy'), tx = (R2 T)[0], the translation between the rectified cameras (negative for a right camera to the right; the fourth
 * column of cv::stereoRectify's P2 is tx * fx'), and the record stage 5 works with: cam has the intrinsics of P1 / P2, baseline = -tx
 * and ncols / nrows = w / h */
typedef struct svo_stereo_rectification {
    double R1[9], R2[9];
    double P1[4], P2[4];
    double tx;
    svo_stereo_camera cam;
} svo_stereo_rectification;

/* The parameters of svo_lk_track (svo_hip.h), the pyramidal Lucas-Kanade tracker on caller lists.  svo_lk_default_params fills in the
 * defaults; the allowed ranges are checked by every call (SVO_ERR_ARG with a text).
 *   win         side of the square window in pixels: odd, 5 .. 31 (default 21)
 *   max_level   deepest pyramid level, 0 .. 5 (default 3); the pyramid of an image stops earlier, at the last level whose sides are
 *               both at least win + 4
 *   max_iters   iterations per level, 1 .. 100 (default 30)
 *   eps         an iteration whose step is at most this long (pixels) ends the level (default 0.01)
 *   min_eig     a window whose gradient matrix has a smaller minimum eigenvalue, per pixel, is not tracked at that level (default 1e-4)
 *   fb_max      > 0: track the results back into the first image and drop the points whose round trip ends farther than this many
 *               pixels from where they started (or is lost on the way); 0 (default): no such pass */
typedef struct svo_lk_params {
    int32_t win, max_level, max_iters;
    float eps, min_eig, fb_max;
} svo_lk_params;

/* The parameters of the resident KLT front end (svo_klt_enable, svo_hip.h).  svo_klt_default_params fills in the defaults.
 *   lk          the tracker's parameters, as svo_lk_track takes them and with the same ranges, fb_max included
 *   cap         tracks per lane, 1 .. max_kps (default 1024; svo_klt_enable(ctx, NULL) uses min(1024, max_kps))
 *   max_dy      a pair survives while |yl - yr| <= max_dy (default 1.5; >= 0)
 *   min_disp, max_disp   ... and min_disp <= xl - xr <= max_disp (defaults 0.5 and +infinity: no upper gate) */
typedef struct svo_klt_params {
    svo_lk_params lk;
    int32_t cap;
    float max_dy;
    float min_disp, max_disp;
} svo_klt_params;

/* The parameters of svo_gftt_detect (svo_hip.h), the Shi-Tomasi corner detector on caller images.  svo_gftt_default_params fills in the
 * defaults; the allowed ranges are checked by every call (SVO_ERR_ARG with a text).
 *   max_corners   at most this many corners per job, 0 .. max_kps; 0 (default): as many as the job's `cap` holds
 *   block         side of the window the structure tensor is summed over: 3 (default), 5 or 7
 *   min_distance  no two corners, and no corner and seed, closer than this many pixels: 0 .. 255 (default 20; 0: no such rule)
 *   quality       a corner's response exceeds this fraction of the image's largest: finite, in (0, 1] (default 0.01) */
typedef struct svo_gftt_params {
    int32_t max_corners, block, min_distance;
    float quality;
} svo_gftt_params;

/* The parameters of the resident top-up of the KLT front end (svo_klt_topup_enable, svo_hip.h).  svo_klt_topup_default_params fills in
 * the defaults, which depend on the front end's cap.
 *   gftt        the detector's parameters, as svo_gftt_detect takes them and with the same ranges
 *   below       a lane is topped up only while its live count < below: 1 .. cap (default (cap + 1) / 2)
 *   target      ... up to this many tracks: 1 .. cap (default cap)
 *   init_disp   the first guess of a new corner (x, y) in the right image is (x - init_disp, y): finite (default 0) */
typedef struct svo_klt_topup_params {
    svo_gftt_params gftt;
    int32_t below;
    int32_t target;
    float init_disp;
} svo_klt_topup_params;

#ifdef __cplusplus
}
#endif
#endif
