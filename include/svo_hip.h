/* svo_hip.h -- C-ABI of the MI355X (gfx950) stereo-VO hot path.  Shared library: stereo_vo_amd/libsvo_hip.so
 *
 * Drop-in boundary for stages 2-5 of rso::CStereoOdometryEstimator::processNewImagePair()
 * (libstereo-odometry/src/process_new_image_pair.cpp:41-385, "P"; declarations in
 * libstereo-odometry/include/libstereo-odometry.h, "H").  Plain pointers and sizes only; every call returns an
 * int status (0 = ok, <0 = error, see svo_strerror) and never throws.  Out-buffers are caller-owned with their
 * capacity passed in; device buffers are context-owned and persist across frames (the previous frame's
 * keypoints / descriptors / pairings stay in HBM).
 *
 * One context drives `n_lanes` INDEPENDENT estimator streams ("lanes") through every kernel launch together:
 * a lane is what one rso::CStereoOdometryEstimator instance is in the reference (all of its state is
 * per-instance, H:732-831), and batching lanes per launch is how a 256-CU device is filled by a workload whose
 * single-stream form is launch-latency bound.  A context with n_lanes = 1 is exactly one
 * estimator.  There is no CPU fallback: without a HIP device svo_create fails.
 */
#ifndef SVO_HIP_H
#define SVO_HIP_H
#include "svo_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_MAX_LANES 128
#define SVO_MAX_LEVELS 8

/* status codes */
enum {
    SVO_OK = 0, SVO_ERR_HIP = -1, SVO_ERR_ARG = -2, SVO_ERR_UNSUPPORTED = -3, SVO_ERR_NO_DEVICE = -4,
    SVO_ERR_CAPACITY = -5, SVO_ERR_STATE = -6
};

/* svo_process flags */
enum {
    SVO_RUN_DETECT = 1,     /* stage 2  (P:166-167 -> stage2_detect_features, H:1017)  */
    SVO_RUN_MATCH = 2,      /* stage 3  (P:269 -> stage3_match_left_right, H:1025)     */
    SVO_RUN_TRACK = 4,      /* stage 4  (P:314 -> stage4_track, H:1033)                */
    SVO_RUN_OPTIMIZE = 8,   /* stage 5  (P:338 -> stage5_optimize, H:1041)             */
    SVO_RUN_ALL = 15,
    SVO_FLAG_REPEAT = 16,   /* request_data.repeat (H:221, P:86-92)                    */
    SVO_FLAG_NO_SHIFT = 32, /* do not run the prev/cur shift of P:86-100 (staged tests and the
                               precomputed-data bypass of P:131-162 / P:219-251 after svo_put_*) */
    SVO_FLAG_DEVICE_IMAGES = 64, /* svo_image.data are device pointers (already resident in HBM) */
    SVO_FLAG_DETECT_NO_POST = 256, /* with SVO_RUN_DETECT: stop before the reference's own post-processing of the detector output
                                    (m_non_max_sup + m_update_indexes, S2:583-618: one latency-bound block per image) and the
                                    description of its survivors; both are left to a later call with SVO_RUN_DETECT_POST,
                                    e.g. on another stream */
    SVO_RUN_DETECT_POST = 512,   /* that post-processing alone, ahead of the other stages of the call */
    SVO_FLAG_BGR_IMAGES = 128,   /* svo_image.data are 8-bit 3-channel BGR (stride in bytes): stage 1's grey conversion runs
                                    on the device (stage1_rectify.cpp:50-51) */
    SVO_FLAG_DETECT_SPLIT_AT_SELECT = 2048, /* moves the split point of SVO_FLAG_DETECT_NO_POST / SVO_RUN_DETECT_POST forward: the detect call stops
                                    after the FAST kernel (pyramid + corner candidates: the throughput half), and the post call
                                    starts with the per-level selection (top-K, Harris, sort) -- pass it to BOTH calls; ORB mode only */
    SVO_FLAG_DETECT_AHEAD = 4096, /* a detect call that may run AHEAD of the stages 3-5 of the frame before it (svo_batch's pipelined
                                    schedule, round 4).  With SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST: the call writes the detector's
                                    per-image scratch ONLY (level-0 pointer table, pyramid, candidates, per-level winners) -- no lane
                                    state, no result record, no status word; capacity bits it raises are staged.  The matching
                                    SVO_RUN_DETECT_POST call carries the flag too and is issued WITHOUT SVO_FLAG_NO_SHIFT: it runs the
                                    prev/cur shift of P:86-100, clears the record and folds the staged bits in.  Everything the ahead
                                    call overwrites is last read by the post-processing of the previous frame: svo_record_after_post
                                    hands the caller an event for exactly that point */
    SVO_FLAG_PINNED_IMAGES = 1024 /* svo_image.data are PAGE-LOCKED host pointers (svo_host_alloc / svo_host_register): the upload is
                                    enqueued on the context's copy stream and svo_process returns without waiting for it; the
                                    images must stay untouched until svo_wait_upload (or svo_wait) returns.  Without this flag host
                                    images are copied into the context's own page-locked staging first, so they are only borrowed
                                    for the duration of the call, as in the reference (P:111-120) */
};

typedef struct svo_ctx svo_ctx;

typedef struct svo_config {
    int32_t device;         /* HIP device ordinal */
    int32_t n_lanes;        /* 1..SVO_MAX_LANES independent estimator streams per launch */
    int32_t max_w, max_h;   /* largest image the context will see */
    int32_t max_kps;        /* capacity of every keypoint / pairing list per octave (power of two, <= 16384; above 4096 the NMS and
                               Gauss-Newton kernels keep their sort / hash arrays in global memory instead of LDS: slower per lane.
                               16384 ranks up to 2 x 4096 corners per ORB level and holds a sampler table of about 310 MB per device) */
    int32_t max_cand;       /* capacity of the per-level FAST candidate list at level 0 (scaled by area above).  dmFASTER keeps EVERY
                               FAST-12 corner as a candidate (no score, no 3 x 3 suppression) and is dense on noisy content -- 24 % of
                               the pixels of a smoothed random texture at threshold 20 -- so size it by the image there, not by the
                               feature count: beyond it SVO_ST_CAND_OVERFLOW (status bit 1) is raised and the list is cut */
    int32_t kernel_times;   /* 1: bracket every kernel with HIP events (svo_kernel_times) */
    int32_t max_octaves;    /* 1..4: octave lists per lane (params_rectify.nOctaves of the FAST+ORB and FASTER modes); 1 suffices for ORB */
    void*   stream;         /* hipStream_t to run on; NULL = the context creates its own */
} svo_config;

/* 8-bit gray, row-major (what stage 1 hands to stage 2: S1:47-85 is outside this library) */
typedef struct svo_image {
    const uint8_t* data;
    int32_t w, h;
    int64_t stride;         /* bytes between rows, >= w * channels (1 grey, 3 with SVO_FLAG_BGR_IMAGES); svo_process refuses a
                               smaller one with SVO_ERR_ARG.  Any value from there on and any byte alignment of `data` are
                               accepted: a crop of a larger frame, a side-by-side stereo frame (stride 2 w, right = left + w),
                               odd widths held contiguously.
                               READ CONTRACT of a device frame (SVO_FLAG_DEVICE_IMAGES).  Without a rectify map, BGR or
                               svo_use_graphs the kernels read the frame IN PLACE, level 0 is never copied.  Every byte of
                               [data, data + h * stride) must be readable device memory, the padding behind the last row
                               included (k_resize fetches whole 16-byte pieces of a row up to its stride when the stride is a
                               multiple of 16; what the padding holds never reaches a result).  Nothing outside that range is
                               read and nothing of the caller's is ever written: k_fast, k_harris, k_describe, k_half and
                               k_prepare stay inside the w x h pixels.  The kernels address the frame with 32-bit byte offsets,
                               so h * stride must not exceed 2^31 - 1: svo_process refuses a larger span with SVO_ERR_ARG.
                               Both refusals happen before anything is enqueued and leave a text in svo_last_error.
                               CONSEQUENCE for sub-images: the range is h * stride bytes from `data`, not from the parent frame's
                               first byte.  For the right half of a side-by-side frame it ends w bytes behind the parent's last
                               row, for a crop at column x of the parent's bottom rows x bytes behind it -- and with a stride that
                               is a multiple of 16 k_resize does fetch there (the 16-byte pieces of the last source rows up to
                               data + h * stride).  A parent frame that is the very tail of its allocation therefore needs that
                               many readable bytes behind it (at most one stride); hipMalloc's page granularity usually provides
                               them, a sub-allocator that packs frames back to back up to the end of a mapping does not.
                               All images of one call share w, h and stride. */
} svo_image;

typedef struct svo_frame {  /* one lane's rectified stereo pair (request_data.stereo_imgs, H:208) */
    svo_image left, right;
} svo_frame;

void svo_config_defaults(svo_config* c);
void svo_params_defaults(svo_params* p);          /* reference defaults, north-star selectors (svo_types.h) */

int  svo_create(const svo_config* cfg, svo_ctx** out);
void svo_destroy(svo_ctx* ctx);
const char* svo_strerror(int status);
const char* svo_last_error(const svo_ctx* ctx);   /* text of the last HIP failure or refusal; svo_process clears it on entry */

/* loadParamsFromConfigFile (H:554-663): stores the record, then resetFASTThreshold / resetORBThreshold.  The reference has no
 * keypoint cap (stage2_detect.cpp:461-464); a request that this context's lists cannot hold (orb_nfeats against
 * svo_config.max_kps, nOctaves against max_octaves) is refused here with SVO_ERR_CAPACITY -- the numbers are in svo_last_error --
 * and the parameters in force stay as they were. */
int svo_set_params(svo_ctx* ctx, const svo_params* p);
int svo_get_params(const svo_ctx* ctx, svo_params* p);
/* The file half of loadParamsFromConfigFile / loadParamsFromConfigFileName (H:551-672): reads the reference's INI keys from the
 * seven sections {RECTIFY, DETECT, MATCH, IF-MATCH, LEAST_SQUARES, GUI, GENERAL} (an empty or NULL name skips the group) into
 * *p, keeping the current value of every key that is absent (`if_match_method` falls back to 0 as at H:611).  Host only: needs
 * no context and no GPU; follow it with svo_set_params.  SVO_ERR_ARG when the file cannot be opened (H:669 asserts it exists). */
int svo_params_load_ini(const char* path, const char* const sections[7], svo_params* p);
int svo_set_fast_threshold(svo_ctx* ctx, int v);  /* setFASTThreshold, clamped (H:531) */
int svo_set_orb_threshold(svo_ctx* ctx, int v);   /* setORBThreshold, clamped (H:538) */
int svo_get_fast_threshold(const svo_ctx* ctx);
int svo_get_orb_threshold(const svo_ctx* ctx);
/* TDetectParams::KLT_win (H:561-587, default 4 at S2:47): dmFASTER ranks its corners by CImage::KLT_response over the
 * (2 KLT_win + 1)^2 window around each.  The layout of svo_params is frozen, so the value belongs to the context, like the two
 * thresholds above; every lane shares it.  1 .. 15; anything else is SVO_ERR_ARG and the value in force stays.  May be changed
 * between frames under the rule of svo_set_params (it is an argument of the launches that follow; captured graphs are dropped). */
int svo_set_klt_win(svo_ctx* ctx, int klt_win);
int svo_get_klt_win(const svo_ctx* ctx);
/* the INI half: reads `KLT_win` from the DETECT section of a file written for the reference.  *klt_win keeps its value when the
 * section or the key is absent (an empty or NULL section name reads nothing); SVO_ERR_ARG when the file cannot be opened.  Host only. */
int svo_klt_win_load_ini(const char* path, const char* detect_section, int32_t* klt_win);
/* dmFASTER's DYNAMIC THRESHOLD (TDetectParams::target_feats_per_pixel, H:393, H:409; the controller of S2:522-550).  The reference
 * keeps one m_threshold[octave] per estimator and moves it by one after every detection so that the corner density stays within
 * +-20 % of the target -- but only under update_dyn_thresholds, which processNewImagePair never passes.  Here it is an opt-in of the
 * context (svo_params is frozen), OFF by default: while off every launch, list and result is what it always was.
 * While on, a frame of an ACTIVE lane under SVO_RUN_DETECT and dmFASTER runs the reference's two calls (P:166-167) as if each had
 * update_dyn_thresholds = true.  Per octave o, with T = the lane's m_threshold[o]:
 *     left image:   detected at T;   nL = ALL its FAST-12 corners;  T'  = step(T,  nL, w_o * h_o)
 *     right image:  detected at T';  nR likewise;                   T'' = step(T', nR, w_o * h_o);   m_threshold[o] = T''
 *     step(T, n, wh): d = n / (double)wh;  d < 0.8 target ? max(1, T - 1) : (d > 1.2 target ? T + 1 : T)        -- IEEE double
 * so the right image of a frame is detected at a threshold that depends on the left image of the SAME frame.  n is the full count:
 * a candidate list that overflows (status bit 1, as ever) cuts the list, not the rule's input.  A threshold that starts in 0 .. 255
 * stays there (at 255 nothing is a corner).  Everything downstream -- KLT response, NMS, row sort, windows, SAD stages -- is unchanged.
 * Under any other detector the setting is accepted and inert.
 * The thresholds live ON THE DEVICE, one int32 per lane and octave: no call synchronises for them, and the graphs of svo_use_graphs
 * stay valid while they move.  They are persistent detector scratch, read and committed by the detect call itself and ordered on
 * the stream it runs on, like the speculative thresholds of the ORB path: correct under SVO_FLAG_DETECT_NO_POST / SVO_RUN_DETECT_POST
 * and SVO_FLAG_DETECT_AHEAD as long as the detect calls of a context are ordered among themselves, which those schedules need anyway.
 * m_threshold[o] becomes svo_params.initial_FAST_threshold (S2:522-523)
 *     - for every lane when the feature is switched on (off -> on; a call that only changes the target moves nothing),
 *     - for the lane(s) of svo_reset,
 *     - for every lane by a svo_set_params that changes the octave count (nOctaves) -- and by no other svo_set_params: one that changes
 *       initial_FAST_threshold alone does NOT move it.
 * Nothing else moves it: not svo_gather_windows, svo_put_*, svo_import_frame, svo_load_state (hand-over records and state files do
 * not carry it: the reference's file has no such member), not a call that is refused before anything is enqueued, and not a frame the
 * lane sits out (svo_process_lanes): an idle lane keeps its thresholds and statistics.
 * svo_set_dyn_fast_threshold: target must be finite and >= 0, else SVO_ERR_ARG with a text and the values in force stay.  It allocates
 * at once, and drops the captured graphs on a change.  svo_get_dyn_fast_threshold: either pointer may be NULL; default off, 10 / 1000 (S2:46).
 * Cost while on: k_faster runs as two launches (left images, then right images; both under "faster" in svo_kernel_times). */
int svo_set_dyn_fast_threshold(svo_ctx* ctx, int enable, double target_feats_per_pixel);
int svo_get_dyn_fast_threshold(const svo_ctx* ctx, int* enable, double* target_feats_per_pixel);
/* the INI half: reads `target_feats_per_pixel` from the DETECT section of a file written for the reference, like svo_klt_win_load_ini.
 * (svo_params_load_ini keeps ignoring the key: svo_params has no field for it.) */
int svo_dyn_fast_load_ini(const char* path, const char* detect_section, double* target_feats_per_pixel);
/* the lane's thresholds and what the reference shows as GUI statistics (S2:548-549): svo_faster_stats in svo_types.h.  Implies svo_wait;
 * SVO_ERR_STATE with a text while the feature is off.  svo_faster_stats_size() = sizeof(svo_faster_stats) as compiled (96). */
int svo_get_faster_stats(svo_ctx* ctx, int lane, svo_faster_stats* out);
size_t svo_faster_stats_size(void);
/* step() above as a pure host function (no context, no device): the threshold after a detection that found n corners in a w x h image */
int svo_faster_threshold_step(int T, int n, int w, int h, double target_feats_per_pixel);
/* The adaptive NMS under dmFASTER (stage2_detect.cpp:599-606 applies m_adaptive_non_max_sup, S2:141-215, to whatever detector ran): an
 * OPT-IN of the context, off by default.  While it is off, a call under dmFASTER with non_maximal_suppression and nmsMethod =
 * SVO_NMS_ADAPTIVE is refused as it always was (SVO_ERR_UNSUPPORTED, "the adaptive NMS is not built for dmFASTER: use nmsMethod =
 * nmsmStandard") and every launch, list and record is what it was.  While it is on, such a call is accepted: behind the detector,
 * k_faster_anms runs where the grid NMS would, per octave image on EVERY FAST-12 corner with its KLT response (rank = response desc,
 * raster index asc; num_out_points = kps_to_detect[octave], min_radius_th = 0; output = radius desc, index asc), and leaves the same
 * records in the same place (x, y, size 0, angle -1, response, octave 0, class_id -1; all-zero descriptor rows).  Row sort, windows and
 * stages 3-5 follow unchanged; SVO_FLAG_DETECT_NO_POST / SVO_RUN_DETECT_POST, SVO_FLAG_DETECT_AHEAD, svo_use_graphs, svo_process_lanes
 * and svo_set_dyn_fast_threshold work as under the grid NMS.  Every other configuration launches what it launches without the opt-in:
 * under another detector, or with nmsmStandard, the setting is accepted and inert.  Hand-over records and state files carry nothing of it.
 * Why a context must ask: the setter allocates 24 bytes x 2 n_lanes x (3.3 max_cand + 8192) of scratch at once (before any graph capture),
 * and selects the most expensive selection kernel of the detect chain ("faster_nms" in svo_kernel_times counts it).  It drops the
 * captured graphs on a change.  SVO_ERR_UNSUPPORTED with a text when max_cand exceeds 2^19 (a rank is packed into 19 bits).
 * svo_get_faster_adaptive_nms: 1 / 0. */
int svo_set_faster_adaptive_nms(svo_ctx* ctx, int enable);
int svo_get_faster_adaptive_nms(const svo_ctx* ctx);
/* Switch the HIP stream that later svo_process / svo_copy_results_async calls enqueue on (NULL: the context's own).
 * Ordering between work already enqueued on the old stream and work on the new one is the caller's business (events):
 * this is what lets a caller run stage 2 of one context on a normal-priority stream and stages 3-5 of another on a
 * high-priority one (bench.py).  Stream lifetime: a stream must stay alive while calls that enqueue on it are being made; once
 * the caller has switched away it may synchronise and destroy the stream -- later svo_wait / svo_get_* / svo_destroy wait on
 * context-owned events recorded behind the work, never on the stream handle. */
int svo_set_stream(svo_ctx* ctx, void* stream);
int svo_get_device(const svo_ctx* ctx);           /* HIP device ordinal of the context (svo_config.device); < 0 on error */
/* Arms ONE hipEvent_t: the next svo_process call that runs the detector's post-processing (SVO_RUN_DETECT_POST, or SVO_RUN_DETECT
 * without SVO_FLAG_DETECT_NO_POST) records it on its stream right behind the last kernel that reads the detector's per-image
 * scratch (NMS / row sort + description), i.e. BEFORE stages 3-5 of the same call.  A detect call with SVO_FLAG_DETECT_AHEAD for
 * the next frame need wait for nothing later.  (Inside a hipGraph replay the event is recorded behind the whole graph.) */
int svo_record_after_post(svo_ctx* ctx, void* event);
/* the hipStream_t later calls enqueue on (so that a caller can order its own work -- an RCCL call, an event -- after a frame) */
int svo_get_stream(svo_ctx* ctx, void** stream);
/* request_data.stereo_cam (H:211), per lane; lane = -1 sets every lane */
int svo_set_camera(svo_ctx* ctx, int lane, const svo_stereo_camera* cam);
/* Stage 1 on the device (stage1_rectify.cpp:47-85).  Rectification maps of one camera of one lane (lane = -1: every
 * lane): HOST float arrays [h][w] of source coordinates per output pixel, as cv::initUndistortRectifyMap(CV_32FC1)
 * -- what mrpt::vision::CStereoRectifyMap::setFromCamParams (S1:66-68) precomputes -- yields.  They are converted
 * once to the 1/32-pixel fixed point of cv::remap and kept on the device; from then on svo_process rectifies that
 * camera's images (bilinear, constant-0 border, S1:70-72) before detection.  map_x = map_y = NULL clears the map
 * (areImagesRectified(), S1:61-65). */
int svo_set_rectify_map(svo_ctx* ctx, int lane, int side, const float* map_x, const float* map_y, int w, int h);
/* The same maps from a calibration, built on the device: what setFromCamParams (S1:66-68) does itself, without OpenCV and without
 * host arrays.
 * svo_stereo_rectify: Bouguet's rectification as cv::stereoRectify does it for alpha = -1 -- a pure host function, no context and no
 *   device.  Half of the rotation goes to each camera, the half-rotated baseline is aligned with the x axis (R1, R2); the common
 *   focal length is the smaller fy, shrunk where k1 < 0; each principal point centres the four undistorted image corners (five
 *   fixed-point iterations each); zero_disparity averages both coordinates of the two principal points, otherwise only y.
 *   Refused with a text in `why` (when why_cap > 0) and nothing written to `out`: SVO_ERR_UNSUPPORTED for alpha >= 0 and for a rig
 *   whose half-rotated baseline is more vertical than horizontal (or whose rotation is a half turn); SVO_ERR_ARG for a right camera
 *   that is not to the right (-tx <= 0), a non-finite field, |R^T R - I| > 1e-6 in any entry, T = 0, w or h <= 0, a NULL pointer.
 * svo_set_undistort_rectify: cv::initUndistortRectifyMap(cam, dist, R, P) + svo_set_rectify_map of one camera: the table is computed
 *   by k_rectify_map in double from (A R)^-1 and is, entry for entry, what svo_set_rectify_map makes of the float maps of the same
 *   closed form (csrc/rectify_model.hpp).  P = fx' fy' cx' cy' of the rectified camera.  lane = -1 builds the table ONCE and points
 *   every lane at that one buffer; a later per-lane set (by either setter) or clear detaches that lane only.  Arguments, the rule
 *   that all maps of a context share w and h, and the synchronisation are those of svo_set_rectify_map; a non-finite value is SVO_ERR_ARG.
 * svo_set_stereo_calibration: svo_stereo_rectify + both cameras in ONE launch.  set_camera != 0 also hands out->cam to
 *   svo_set_camera(lane): the reference leaves stereo_cam to its caller (0 is its literal behaviour), but the rectified intrinsics
 *   are what stage 5 must work with (1 is the useful one).  out may be NULL.  On a refusal nothing changes, the text is in svo_last_error.
 * svo_debug_get_rectify_map: the fixed-point entries in force for one camera, whichever setter made them: xy[i] = (sx + 1) | (sy + 1) << 16
 *   (0xFFFFFFFF: wholly outside), frac[i] = fx | fy << 8.  Returns the count w * h (0: the camera has no map) and copies min(count, cap). */
int svo_stereo_rectify(const svo_stereo_calibration* calib, svo_stereo_rectification* out, char* why, size_t why_cap);
int svo_set_undistort_rectify(svo_ctx* ctx, int lane, int side, const svo_camera_model* cam, const double* R, const double* P, int w, int h);
int svo_set_stereo_calibration(svo_ctx* ctx, int lane, const svo_stereo_calibration* calib, int set_camera, svo_stereo_rectification* out);
int svo_debug_get_rectify_map(svo_ctx* ctx, int lane, int side, uint32_t* xy, uint32_t* frac, int cap);
/* forget both frames, the warm start and the match-ID counters of one lane (a freshly constructed estimator, C:28-50); -1 = all.
 * The FAST / ORB thresholds belong to the context (all its lanes share svo_params) and stay as they are: svo_set_*_threshold.
 * dmFASTER's dynamic thresholds belong to the lane and start over (svo_set_dyn_fast_threshold). */
int svo_reset(svo_ctx* ctx, int lane);

/* processNewImagePair for every lane (P:41-385): ENQUEUES the whole frame on the context's stream and
 * returns; frames[lane] for lane in [0,n_lanes).  Nothing is copied back until svo_wait/svo_get_*. */
int svo_process(svo_ctx* ctx, const svo_frame* frames, uint32_t flags);
/* svo_process for the lanes whose bit is set: bit l & 63 of active[l >> 6] selects lane l.  Cameras do not tick in lockstep -- frames
 * are dropped, streams start late, end early or run at other rates -- and one estimator is only ever called when ITS camera has a
 * frame (H:732-831: all state is per instance).  For every lane whose bit is CLEAR the call is AS IF IT HAD NOT BEEN MADE: nothing that a
 * getter, a later frame, a hand-over record or a state file can observe changes -- the result record, both slots' keypoint /
 * descriptor / pairing / ID lists with their counts and row-index tables, the tracked list, residuals and outliers, the lane state
 * (iteration counter, m_error, which slot is the previous frame, the match-ID counters), the status word, its pose-covariance record, the speculative FAST
 * thresholds of its two images, dmFASTER's dynamic thresholds and their statistics (svo_set_dyn_fast_threshold), its gathered SAD windows and the host-side record of which of its frames have them.  No shift, no
 * zero-motion frame, no match IDs consumed.  Only per-frame scratch (pyramid, candidate lists, matcher and RANSAC tables) may be
 * rewritten.  For every lane whose bit is SET the call is exactly svo_process; with every bit set it IS svo_process, launch for launch.
 *   - frames[l] of an idle lane is not read and may hold NULL pointers; it is neither copied nor uploaded.  An active lane with NULL
 *     data is SVO_ERR_ARG, and the active lanes must agree on w / h (and on the stride of device frames).
 *   - a bit at or above n_lanes: SVO_ERR_ARG, with a text.  active == NULL: SVO_ERR_ARG.  Like every refusal of svo_process these disarm
 *     an event armed by svo_record_after_post, if the flags are those of a call that would have consumed it.
 *   - no bit set: SVO_OK; nothing is enqueued, no state moves (an armed event stays armed), svo_last_error is empty.
 *   - svo_import_frame writes every lane.  The first-frame rule of the match IDs that follows an import applies to each lane at ITS
 *     first call after the import: a lane that sits that call out keeps it for its own next frame.
 *   - ONE MASK PER FRAME.  The calls that continue a frame -- the SVO_RUN_DETECT_POST call of a SVO_FLAG_DETECT_NO_POST detect call
 *     (with or without SVO_FLAG_DETECT_AHEAD), and stages run with SVO_FLAG_NO_SHIFT -- must carry the mask of the call that began it
 *     (the last call that ran the detector or the shift; svo_process counts as all lanes).  Another mask is SVO_ERR_STATE with a text,
 *     before anything is enqueued.
 *   - a SAD stage on a frame whose windows were never gathered (below) is looked for in the active lanes only, and a lane whose
 *     previous frame is to be forgotten forgets it at ITS next active frame.
 *   - svo_use_graphs: a call with an idle lane runs as plain launches (the mask is a kernel argument); calls with every lane active go
 *     on replaying.
 * The grids stay whole: an idle lane's workgroups leave at once.  A context that is mostly idle therefore still pays for launching
 * them ("Idle lanes"). */
int svo_process_lanes(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, const uint64_t active[2]);
/* smSAD (svo_params.match_method = SVO_SM_SAD, S3:185-419) and ifmSAD (ifm_method = SVO_IFM_SAD, S4:435-738) compare the 8 x 8 image
 * windows around two keypoints (rso::compute_SAD8).  Stage 2 is the only stage that reads images, so it gathers the window of every
 * final keypoint -- from the call on in which either selector is in force; a context that never selects them allocates and launches
 * nothing.  A frame has windows when this library detected it under such parameters -- in this context, in the one whose hand-over
 * record brought it (svo_import_frame below: the records of a context that has selected a SAD method carry the windows), or in the one
 * that saved it (svo_save_state below: the file's extension block carries them) -- or when svo_gather_windows (below) was given its
 * images.  Features that came through svo_put_features(_oct) have none until then (the reference's bypass call still carries the image
 * pair, P:100-108; here the lists and the images arrive in separate calls), and neither does a frame detected while no SAD method was
 * selected, nor one loaded from a file that was saved without them.
 * A call that runs a SAD stage on a frame without windows is refused with SVO_ERR_STATE and a text in svo_last_error BEFORE anything is
 * enqueued: the lists and the lane state stay as they were.  When it is the PREVIOUS frame that lacks them (a stream that switches
 * to ifmSAD) and the call would have shifted, the refusal is remembered: the lane's next shifting call forgets that frame, i.e. it is
 * processed as the lane's first frame (voecFirstIteration; the match-ID counter runs on), and the stream is tracked with ifmSAD from the frame after.
 * dmFASTER (detect_method = SVO_DM_FASTER, the reference's default, S2:519-576): FAST-12 corners of every x1/2 octave at
 * svo_params.initial_FAST_threshold (0 .. 255, SVO_ERR_ARG otherwise; svo_set_fast_threshold does not touch it) -- constant by default, as
 * in the reference, which only moves it under update_dyn_thresholds and never passes that from processNewImagePair; with
 * svo_set_dyn_fast_threshold on it is the starting value of a per-lane, per-octave threshold that the device adapts after every image
 * (above) --, each with its KLT response (KLT_win above), then the grid NMS
 * and the row sort of the FAST+ORB path -- one list per octave, keypoint records (x, y, size 0, angle -1, response, octave 0,
 * class_id -1), all-zero descriptor rows.  It computes no descriptors, so only the SAD stages can follow it: SVO_RUN_MATCH with another
 * match_method or SVO_RUN_TRACK with ifm_method 0 / 1 is SVO_ERR_STATE, and nmsMethod = SVO_NMS_ADAPTIVE under it SVO_ERR_UNSUPPORTED
 * unless the context has opted in (svo_set_faster_adaptive_nms above: then the adaptive NMS runs in place of the grid NMS),
 * each with a text and before anything is enqueued.  minimum_KLT_response has no effect on any output of the reference's path, and
 * target_feats_per_pixel none unless update_dyn_thresholds is passed: both are accepted and ignored by svo_params_load_ini
 * (svo_dyn_fast_load_ini reads the latter for svo_set_dyn_fast_threshold).
 * SVO_IFM_OPTICAL_FLOW and SVO_DM_KLT stay SVO_ERR_UNSUPPORTED. */
/* block until every enqueued frame has finished */
int svo_wait(svo_ctx* ctx);
/* Host-fed frames (the reference's contract: P:100-120 takes host images per call).  Uploads go through a ring of two
 * device buffers on a dedicated copy stream, so the upload of frame t+1 overlaps the kernels of frame t; stage 2 of a
 * frame waits for its own upload only.  svo_wait_upload blocks until every enqueued upload has left the host buffers.
 * svo_host_alloc / svo_host_free hand out page-locked memory to callers that have no HIP headers; svo_host_register /
 * svo_host_unregister page-lock memory the caller already owns (e.g. a camera driver's frame buffers). */
int svo_wait_upload(svo_ctx* ctx);
/* One stream alone is bound by launch latency, not by its kernels (~30 launches per frame).  With graphs enabled, the
 * kernel sequence of a svo_process call is captured once into a hipGraph -- per combination of stage flags, image ring slot
 * and dynamic thresholds -- and replayed by one graph launch afterwards.  Images (host or device) then always pass
 * through the context's two-slot ring, which gives the captured kernels fixed addresses.  Calls that run stage 1 on the
 * device (rectification maps / BGR input) or have kernel timing on fall back to plain launches.  Same results. */
int svo_use_graphs(svo_ctx* ctx, int enable);
int svo_host_alloc(size_t bytes, void** out);
int svo_host_free(void* p);
int svo_host_register(void* p, size_t bytes);
int svo_host_unregister(void* p);
/* TStereoOdometryResult of the last frame, per lane (H:235-264); implies svo_wait */
int svo_get_result(svo_ctx* ctx, int lane, svo_result* res);
int svo_get_results(svo_ctx* ctx, svo_result* res /* n_lanes entries */);
/* enqueue a device-to-device copy of the n_lanes result records into caller-owned device memory (e.g. the send
 * buffer of an RCCL all-gather of poses) on the context's stream; no host synchronisation */
int svo_copy_results_async(svo_ctx* ctx, void* dst_device, size_t bytes);

/* THE COVARIANCE OF EVERY POSE INCREMENT (no reference counterpart; the quantity and the states are defined at svo_pose_cov in
 * svo_types.h).  Off by default; while off a context allocates and launches nothing for it and every result is what it was.
 * svo_set_pose_covariance(ctx, 1) allocates one record per lane (all SVO_COV_NONE) and the array stage 5 leaves its final mask in, at
 * once (before any graph capture); from then on every call that runs stage 5 -- svo_process / svo_process_lanes with SVO_RUN_OPTIMIZE,
 * and svo_change_in_pose -- launches k_pose_covariance behind k_gauss_newton ("pose_covariance" in svo_kernel_times, a name listed only while the
 * feature is on: with it off the list is the one it always was), which rewrites the
 * record of every ACTIVE lane: one more evaluation at the returned delta over the mask stage 5 ended with.  `info` is WEIGHTED by the
 * robust kernel's weights, unlike the Hessian the iteration solves with (S5:364-369).  A record is SVO_COV_NONE unless the stage 5 of
 * that very call ended with valid = 1: the kernel is told so by k_gauss_newton itself, not by svo_result.valid, so nothing stale can
 * leak in on any path.  svo_change_in_pose writes lane 0's record, as it uses lane 0's warm start.  A change of value drops the
 * captured graphs (svo_use_graphs); a call with idle lanes still runs as plain launches, and an idle lane keeps its record.
 * Other entry points treat the record as they treat the lane's svo_result: svo_reset zeroes it; svo_import_frame and svo_load_state
 * leave it as it is (they bring lists and inherited members, not results; hand-over records and state files do not carry it).
 * The getters imply svo_wait; with the feature off they and the copy return SVO_ERR_STATE with a text in svo_last_error.
 * svo_copy_pose_covariances_async is the twin of svo_copy_results_async: n_lanes records, device to device, on the context's stream.
 * svo_pose_cov_size() = sizeof(svo_pose_cov) as this library was compiled (888), for a binding to check its mirror. */
int svo_set_pose_covariance(svo_ctx* ctx, int enable);
int svo_get_pose_covariance(svo_ctx* ctx, int lane, svo_pose_cov* cov);
int svo_get_pose_covariances(svo_ctx* ctx, svo_pose_cov* cov /* n_lanes entries */);
int svo_copy_pose_covariances_async(svo_ctx* ctx, void* dst_device, size_t bytes);
size_t svo_pose_cov_size(void);

/* THE LANDMARKS OF EVERY FRAME, WITH THEIR COVARIANCES (no reference counterpart: the reference triangulates them at S5:529-544 and keeps
 * them; the record, its flags and the lane states are defined at svo_landmark / svo_landmarks_info in svo_types.h).  Off by default;
 * while off a context allocates and launches nothing for it and every result is what it was.
 * svo_set_landmarks(ctx, 1, std_noise_pixels) allocates, at once (before any graph capture), n_lanes x max_kps records of 176 bytes -- the
 * one large allocation a context makes after svo_create (96 x 16384: 277 MB); when it fails the call is SVO_ERR_CAPACITY with the number
 * in svo_last_error -- one info per lane (all SVO_LMK_NONE) and, unless the pose covariance made it, the array stage 5 leaves its final
 * mask in.  std_noise_pixels is TLeastSquaresParams::std_noise_pixels (H:628), which the reference reads and never uses: 0 = its default
 * of 1; negative or not finite is SVO_ERR_ARG with a text and the values in force stay.  It travels through this setter because
 * svo_params' layout is frozen; svo_landmarks_load_ini reads it from the LEAST_SQUARES section of a file written for the reference
 * (needs no device; the value is kept when the key is absent, SVO_ERR_ARG when the file holds a negative one).
 * From then on every svo_process / svo_process_lanes with SVO_RUN_OPTIMIZE launches k_landmarks once behind k_gauss_newton -- behind
 * k_pose_covariance when that is on, whose cov_delta then enters cov_cur -- ("landmarks" in svo_kernel_times, listed only while the feature is
 * on), inside the captured graph under svo_use_graphs.  It rewrites the records and the info of every ACTIVE lane; an idle lane keeps both.
 * A change of the switch or of the value drops the captured graphs.  svo_pose_cov is bit for bit what it is with the feature off.
 * svo_reset sets the lane's info to SVO_LMK_NONE with n = 0.  svo_change_in_pose writes no records.  Hand-over records, state files and
 * the RCCL companion do not carry them, and frame-parallel streams refuse the feature (svo_fpstream_set_landmarks, svo_batch.h).
 * The getters imply svo_wait; with the feature off they and the copy return SVO_ERR_STATE with a text in svo_last_error.
 * svo_get_landmarks returns the lane's count n and writes min(n, cap) records (one synchronisation).
 * svo_copy_landmarks_async: n_lanes infos to dst_info and n_lanes x max_kps records (lane after lane; only the first info.n of a lane
 * mean anything) to dst_records, device to device on the context's stream; either may be NULL; bytes = the size of dst_records.
 * svo_landmark_abi_size() = sizeof(svo_landmark) as this library was compiled (176); callable without a device. */
int svo_set_landmarks(svo_ctx* ctx, int enable, double std_noise_pixels);
int svo_get_landmarks_enabled(const svo_ctx* ctx, int* enable, double* std_noise_pixels);   /* either pointer may be NULL */
int svo_landmarks_load_ini(const char* path, const char* least_squares_section, double* std_noise_pixels);
int svo_get_landmarks_info(svo_ctx* ctx, int lane, svo_landmarks_info* info);
int svo_get_landmarks(svo_ctx* ctx, int lane, svo_landmark* out, int cap);
int svo_copy_landmarks_async(svo_ctx* ctx, void* dst_info_device, void* dst_records_device, size_t bytes);
size_t svo_landmark_abi_size(void);

/* getValues (H:704-724) and friends.  which: 0 = current frame, 1 = previous frame; side: 0 left, 1 right.
 * Each returns the list length (possibly > cap; only min(len,cap) entries are written) or <0. */
int svo_get_keypoints(svo_ctx* ctx, int lane, int which, int side, svo_keypoint* kps, uint8_t* desc, int cap);
int svo_get_matches(svo_ctx* ctx, int lane, int which, svo_dmatch* m, int cap);
int svo_get_tracked(svo_ctx* ctx, int lane, svo_index_pair* t, int cap);          /* tracked_pairs[0] (H:823) */
int svo_get_residuals(svo_ctx* ctx, int lane, double* r, int cap);                /* result.out_residual */
int svo_get_outliers(svo_ctx* ctx, int lane, int32_t* idx, int cap);              /* result.outliers */
/* the same lists of one octave (the FAST+ORB mode keeps one list per x1/2 octave, H:760-764, H:799), the row table
 * of m_update_indexes (pyr_feats_index, H:763; img_h entries) and matches_lr_row_index (H:789; img_h + 1 entries) */
int svo_get_keypoints_oct(svo_ctx* ctx, int lane, int which, int side, int octave, svo_keypoint* kps, uint8_t* desc, int cap);
int svo_get_matches_oct(svo_ctx* ctx, int lane, int which, int octave, svo_dmatch* m, int cap);
int svo_get_tracked_oct(svo_ctx* ctx, int lane, int octave, svo_index_pair* t, int cap);
int svo_get_row_index(svo_ctx* ctx, int lane, int which, int side, int octave, int32_t* idx, int cap);
int svo_get_matches_row_index(svo_ctx* ctx, int lane, int which, int octave, int32_t* idx, int cap);
/* match-ID bookkeeping of params_general.vo_use_matches_ids: matches_IDs (H:794, getRefCurrentIDs H:701),
 * resetIds (H:684) and setThisFrameAsKF (H:675-683); result.tracked_feats_from_last_KF counts against the key frame */
int svo_get_match_ids(svo_ctx* ctx, int lane, int which, int octave, int32_t* ids, int cap);
/* getValues (H:704-724) in ONE device synchronisation: every list of one octave of one frame of one lane.  The caller
 * fills the array pointers (any may be NULL) and the two capacities; the call fills the four counts (the full list
 * lengths, possibly above the capacities; min(length, capacity) entries are written).  The lists are packed on the
 * device, copied to the context's page-locked staging in one transfer, and unpacked on the host: one stream
 * synchronisation per call where the individual getters above pay one or two each. */
typedef struct svo_values {
    svo_keypoint* left_kps;  uint8_t* left_desc;      /* cap_kps entries / cap_kps * 32 bytes */
    svo_keypoint* right_kps; uint8_t* right_desc;
    svo_dmatch* matches;     int32_t* match_ids;      /* cap_matches entries each */
    int32_t cap_kps, cap_matches;
    int32_t n_left, n_right, n_matches, n_ids;        /* out */
} svo_values;
int svo_get_values(svo_ctx* ctx, int lane, int which, int octave, svo_values* v);
int svo_reset_ids(svo_ctx* ctx, int lane);
int svo_set_this_frame_as_kf(svo_ctx* ctx, int lane);   /* H:675-683; SVO_ERR_STATE while the lane has no current frame with pairings */

/* the precomputed-data bypass (request_data.use_precomputed_data, H:214-218, P:131-162, P:219-251):
 * load caller-supplied features / pairings into a lane's current (which=0) or previous (which=1) frame. */
int svo_put_features(svo_ctx* ctx, int lane, int which, int side, const svo_keypoint* kps, const uint8_t* desc, int n,
                     int img_w, int img_h);
/* (Coordinates are taken as they come, as in the reference: none is checked against img_w x img_h.  One claim depends on them: stage 4's
 * inlier counts on the matrix cores -- contexts of more than 8 lane-octaves -- are the reference's bit for bit for keypoints with
 * |x| <= img_w and |y| <= img_h (proven with a margin up to about 1.6 times that; lists reaching from -1 to 4 times the image size are
 * tested and agree, without a proof).  A caller whose coordinates lie outside the image declares an img_w x img_h that covers them;
 * contexts of up to 8 lane-octaves evaluate the reference's own expression and need no such premise.) */
/* (Order: a keypoint list is put in ascending row order -- (int)y never falls from one keypoint to the next --, as every list of the
 * reference is after stage 2.  The row-by-row stereo matchers smDescRbR and smSAD rest on it: they find a keypoint's row iteration from its
 * own row, where the reference walks index ranges of the row table, and the two agree for lists in row order only; a list in another
 * order is matched without a fault and without SVO_ST_INTERNAL, every keypoint paired at most once, but not to the reference's pairings.
 * Rows below 0 and from img_h on are no breach of it: they are taken as they come, and the reference's loops never visit them.
 * The brute-force matcher needs the order for the pairings' row table alone.  The windowed tracker ifmDescWin takes every previous
 * pairing's row iteration from the pairings' row table itself and equals the reference's walk for pairing lists in ANY order, negative
 * rows included: a pairing whose left keypoint has y <= 0 is visited in iteration 0.  tests/test_gpu_match_scenes.py holds both.) */
/* (svo_put_matches also builds the list's matches_lr_row_index (S3:425-445) from the LEFT keypoints put before it: the reference builds that
 * index in stage 3 only, which this path skips (P:219-251), and its windowed tracker (S4:517-530) would read an index nobody built.) */
int svo_put_matches(svo_ctx* ctx, int lane, int which, const svo_dmatch* m, int n);
int svo_put_tracked(svo_ctx* ctx, int lane, const svo_index_pair* t, int n);   /* octave 0; the lane's other octaves are emptied */
/* the tracked pairs of one octave < svo_config.max_octaves; the lane's other octaves keep theirs.  (A caller that feeds stage 5 with
 * the tracked pairs of several octaves, which it concatenates octave by octave, S5:419-461, and cuts at svo_config.max_kps.) */
int svo_put_tracked_oct(svo_ctx* ctx, int lane, int octave, const svo_index_pair* t, int n);
/* request_data.precomputed_matches_ID (H:218, P:233-244): the IDs of the octave-0 pairings put before; m_last_match_ID
 * becomes their maximum (P:236-243).  Honoured by the pipeline only when vo_use_matches_ids is set (P:246-250). */
int svo_put_match_ids(svo_ctx* ctx, int lane, int which, const int32_t* ids, int n);
/* the same per OCTAVE (P:141-161 and P:219-244 loop over params_rectify.nOctaves lists): octave < svo_config.max_octaves and,
 * in the FAST+ORB mode, < nOctaves.  img_w / img_h stay the size of the octave-0 image.  svo_put_match_ids_oct: octave 0
 * restarts m_last_match_ID at its maximum ID, higher octaves raise it (call in ascending octave order, as P:236-243 does). */
int svo_put_features_oct(svo_ctx* ctx, int lane, int which, int side, int octave, const svo_keypoint* kps, const uint8_t* desc, int n,
                         int img_w, int img_h);
int svo_put_matches_oct(svo_ctx* ctx, int lane, int which, int octave, const svo_dmatch* m, int n);
int svo_put_match_ids_oct(svo_ctx* ctx, int lane, int which, int octave, const int32_t* ids, int n);
/* (svo_put_features(_oct) also builds the list's row table pyr_feats_index (m_update_indexes, S2:103-129) from the keypoints' rows, as
 * stage 2 would have: the row-by-row stereo matchers smDescRbR and smSAD read it, S3:253-256.) */

/* The images of a frame whose lists were put (or loaded without windows): what makes smSAD / ifmSAD work on the precomputed-data bypass.
 * In the reference a bypass call still carries the image pair: stage 1 builds the octave images (P:100-108) and ifmSAD reads its
 * windows from them (S4:572, 576).  Here: put the lists of a frame, then hand its images to this call.
 *   frames   taken exactly as svo_process takes them: host frames, SVO_FLAG_PINNED_IMAGES, SVO_FLAG_DEVICE_IMAGES (read in place under the
 *            read contract of svo_image.stride), SVO_FLAG_BGR_IMAGES, a rectify map.  Any other flag bit is SVO_ERR_ARG.
 *   which    0: the lists of the current frame, 1: those of the previous one.
 *   active   as in svo_process_lanes; NULL = every lane.  frames[l] of an idle lane is not read; its windows and the host-side record
 *            of which of its frames have them stay as they were.  No bit set: SVO_OK, nothing is enqueued.
 * In the FAST+ORB / dmFASTER geometry the call builds the x1/2 octave images (n_oct - 1 launches); in ORB mode the windows come from
 * level 0.  ONE launch then gathers the window and the border flag of every keypoint of that slot, for every active lane, side and
 * octave: (int)pt, rows y - 3 .. y + 4, the float border rule of S3:290-293, exactly as stage 2 gathers them for a frame it detected;
 * nothing outside the w x h pixels is read.  A NaN coordinate is flagged.  The window buffers are allocated on first use.
 * The call only enqueues on the context's stream and returns.  It marks the frame of every active lane as having windows and touches
 * NOTHING ELSE: no prev/cur shift, no counters, result records, lists, row tables or status words, no match IDs; whether the
 * context's hand-over records carry windows stays as it is.
 * SCHEDULING.  The call overwrites the detector's per-image scratch -- the level-0 pointer table, the upload ring slot, the octave
 * pyramid -- as a detect call does: in a pipelined schedule it TAKES A DETECT CALL'S PLACE (it may not overlap the detection or the
 * post-processing of another frame of this context, and the next detect call must be ordered behind it).  It always runs as plain
 * launches: it is neither captured nor replayed under svo_use_graphs.  svo_kernel_times counts its gather launch as "gather_windows".
 * Refusals, all before anything is enqueued and with a text in svo_last_error:
 *   SVO_ERR_ARG    which not 0 / 1; frames == NULL; a flag bit other than the three above; a mask bit at or above n_lanes; NULL data,
 *                  disagreeing sizes, stride or span violations of an active lane, as svo_process refuses them
 *   SVO_ERR_STATE  no geometry yet (no lists were put or loaded since the last svo_set_params); a frame size other than the one the
 *                  lists were put with */
int svo_gather_windows(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, int which, const uint64_t active[2] /* NULL = all lanes */);
/* the gathered windows of one list, like the other list getters (size query with cap 0; returns the list's length): win receives
 * min(length, cap) x 64 bytes (rows top to bottom), flag as many bytes (1: too close to the border for a window, S3:290-293; the 64 bytes
 * of such a keypoint mean nothing).  0 when the lane has no such frame; SVO_ERR_STATE with a text when that frame's windows were never
 * gathered. */
int svo_get_windows_oct(svo_ctx* ctx, int lane, int which, int side, int octave, uint8_t* win /* n x 64 */, uint8_t* flag /* n */, int cap);

/* getProjectedCoords (H:175-182, C:415-466): pixel coordinates (uL vL uR vR, 4 floats each) that the previous
 * pairings NOT marked as tracked (tracked_first[m] == -1, C:430-431) take after the change in pose: triangulation as
 * in stage 5, then m_pinhole_stereo_projection with the inverse of change_pose (x y z yaw pitch roll).  Returns the
 * number B of such pairings; nothing is written when pix is NULL or cap < B (size query). */
int svo_projected_coords(svo_ctx* ctx, const svo_dmatch* pre_matches, int n_pre, const svo_keypoint* pre_left, int n_left,
                         const svo_keypoint* pre_right, int n_right, const int32_t* tracked_first,
                         const svo_stereo_camera* cam, const double* change_pose6, float* pix, int cap);

/* Frame-parallelism WITHIN one stream: consecutive frames of a stream dealt round-robin to several
 * contexts (one GPU or several).  Stages 2-3 of a frame need only its images; stages 4-5 need the previous frame's lists
 * and the members a call inherits from the one before (m_error for the recovery rule P:86-95, m_last_computed_pose
 * S5:506-507, the match-ID counters H:735-742).  The owner of frame t-1 exports them once its stages 4-5 are enqueued,
 * the owner of frame t imports them after its own stages 2-3 and before its stages 4-5:
 *     owner(t):   svo_process(frames, SVO_RUN_DETECT | SVO_RUN_MATCH);            // overlaps owner(t-1)'s stages 4-5
 *                 <wait for owner(t-1)'s export>  svo_import_frame(blob);
 *                 svo_process(NULL, SVO_RUN_TRACK | SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT);  svo_export_frame(blob');
 * The record is one flat DEVICE buffer of svo_handover_bytes() bytes (all lanes): hand it over device-to-device, or with
 * ncclSend / ncclRecv between GPUs.  Both calls only enqueue on the context's stream; ordering between the two
 * contexts' streams is the caller's (an event, or the send/recv pair).  The run equals the sequential one list for
 * list and pose for pose: nothing is dropped, not even the warm start.
 * Two kinds of record.  A context that has never selected smSAD or ifmSAD writes layout version 2: lists, row tables, inherited members.
 * From the first svo_set_params that selects either -- and for the rest of its life -- a context CARRIES WINDOWS: its records are version
 * 3, the same sections followed by the border flags and the 8 x 8 windows of the exported frame's keypoints (2 * max_kps * 65 bytes more
 * per lane and octave), so that frame-parallel runs work under the SAD matchers, dmFASTER's only ones.  svo_handover_bytes() answers for
 * the context's kind at the time of the call: query it AFTER svo_set_params, and again after a later svo_set_params that selects SAD for
 * the first time (svo_fpstream_set_params does).  The buffer of a context that carries windows must be 16-byte aligned (SVO_ERR_ARG).
 * Which records a context takes: one that carries no windows takes version 2 only; one that does takes version 3 and version 2 (then
 * `bytes` may be the smaller size), and also a version 3 record whose frame had no windows gathered.  A frame that arrives without
 * windows is enough for a descriptor tracker (smSAD + ifmDescBF / ifmDescWin).  Under ifmSAD it cannot be tracked from: the lane then
 * starts afresh at the importer's frame (voecFirstIteration; the match-ID counter runs on) -- where the sequential path's refusal rule
 * above arrives one frame later -- and THE PARAMETERS IN FORCE AT THE IMPORT decide that, not those of the svo_process call after it.
 * Anything else -- a version 3 record handed to a context that carries no windows, other list capacities, lanes or octaves, a buffer too
 * short for its records -- is another layout: nothing is copied, status bit 4 is raised for the lane. */
size_t svo_handover_bytes(const svo_ctx* ctx);
int svo_export_frame(svo_ctx* ctx, void* dev_blob, size_t bytes);
int svo_import_frame(svo_ctx* ctx, const void* dev_blob, size_t bytes);

/* saveStateToFile / loadStateFromFile (H:184-185, C:475-543, C:261-350): the state of one lane in the reference's
 * binary layout -- npyr; then for PRE and CUR: left keypoints, right keypoints (count, then x y response size angle as
 * float and octave class_id as int per keypoint, then rows cols type and the descriptor bytes), pairings (count,
 * id count, then [id] queryIdx trainIdx distance imgIdx each); then m_reset (1 byte) and m_lastID,
 * m_num_tracked_pairs_from_last_kf, m_num_tracked_pairs_from_last_frame, m_last_match_ID, m_kf_max_match_ID as
 * 8-byte integers.  These bytes come first and hold the octave-0 lists: old readers, the reference's included, still get octave 0;
 * npyr is the context's octave count (C:488-489).  svo_load_state reads what svo_save_state (and
 * the reference's saveStateToFile) writes; the reference's own loader expects one more 8-byte word before
 * m_last_match_ID that its saver never writes (C:342-343 vs C:533-539) -- deviation, see SURVEY.md appendix A #18.
 * After a load both frames are present, m_error is cleared and the warm start is the identity.
 * THE EXTENSION BLOCK follows the tail directly, little-endian, no padding.  It is written only when the context works on more than
 * one octave or at least one of the two frames has SAD windows (above); a single-octave context that never selected SAD writes the
 * bytes it always wrote.  Byte for byte:
 *     magic   u32  0x58455653 ("SVEX")        version  u32  1
 *     n_oct   u32  1 .. 4                      w, h     u32 each: the octave-0 image size (the reference's file has none)
 *     has_windows  u8 x 2: PRE, CUR (0 / 1)
 *     for octave 1 .. n_oct - 1:  the PRE group, then the CUR group, each in the sub-layout above (left keypoints, right keypoints,
 *                                 pairings + ids)
 *     for frame in (PRE, CUR) with has_windows, for octave 0 .. n_oct - 1, for side in (left, right):
 *                                 count u64 (= that list's keypoint count), count flag bytes, count x 64 window bytes (all zero where
 *                                 the flag is set)
 * svo_load_state: a file without the block loads into a single-octave context as it always did (image size: the last geometry, or the
 * context's maximum).  A file with the block needs n_oct equal to the octave count the context's parameters give (SVO_ERR_ARG with both
 * numbers otherwise, also for a file without the block offered to a multi-octave context) and w x h within max_w x max_h; per octave and
 * slot it restores the lists, pairings, IDs and row tables, the windows and flags, and from the has_windows bytes which frames have
 * windows: a frame saved without them loads without them and the refusal rule above applies unchanged.  A malformed file --
 * truncated anywhere, a count above max_kps, a windows count different from its list's, a wrong magic or version, bytes behind the
 * block -- is SVO_ERR_ARG with a text; the WHOLE file is validated before the first write to the lane, which is left as it was.
 * (Parser and writer: stereo_vo_amd/csrc/state_format.cpp, host only; stereo_vo_amd/state_file.py reads the same layout independently.) */
int svo_save_state(svo_ctx* ctx, int lane, const char* path);
int svo_load_state(svo_ctx* ctx, int lane, const char* path);

/* getChangeInPose (H:162-172, C:355-413): stage 5 alone on caller arrays, lane 0 of the context.
 * residual: n_tracked doubles; outliers: n_tracked int32 (holds INLIER cur-match indices, S5:603-610).
 * init6 may be NULL.  Returns result.valid (0/1) or <0. */
int svo_change_in_pose(svo_ctx* ctx, const svo_index_pair* tracked, int n_tracked,
                       const svo_dmatch* pre_matches, int n_pre, const svo_dmatch* cur_matches, int n_cur,
                       const svo_keypoint* pre_left, int n_pl, const svo_keypoint* pre_right, int n_pr,
                       const svo_keypoint* cur_left, int n_cl, const svo_keypoint* cur_right, int n_cr,
                       const svo_stereo_camera* cam, const double* init6,
                       svo_result* res, double* residual, int32_t* outliers);

/* cv::BFMatcher(NORM_HAMMING,false).match stand-in (S3:88-94, S4:141-142) on caller arrays (host pointers):
 * for each of nq 32-byte query rows the FIRST minimum-distance train row.  idx = -1 when nt == 0. */
int svo_hamming_match(svo_ctx* ctx, const uint8_t* query, int nq, const uint8_t* train, int nt,
                      int32_t* idx, int32_t* dist);

/* m_adaptive_non_max_sup stand-in (S2:141-215, min_radius_th = 0) on caller arrays (host pointers), like svo_hamming_match: runs the
 * SAME device code as the adaptive NMS under dmFASTER on one list.  It exists so that the kernel can be held to a reference on hand-built
 * lists; it needs no opt-in, touches no lane state and synchronises.  Returns the number kept, min(num_out_points, n) -- possibly
 * > cap --, with the first min(., cap) indices into kps written to out_order in (radius desc, index asc) order.  Requires: integer-valued
 * x, y inside img_w x img_h; img_w * img_h < 2^24; strictly ascending raster order (y * img_w + x), so that index order is position
 * order; no NaN response; n <= the context's level-0 candidate capacity (max(1024, max_cand)); min(num_out_points, n) <= max_kps.
 * Anything else is SVO_ERR_ARG with a text. */
int svo_adaptive_nms(svo_ctx* ctx, const svo_keypoint* kps, int n, int num_out_points, int img_w, int img_h,
                     int32_t* out_order, int cap);

/* Pyramidal Lucas-Kanade tracking on caller lists, batched over many image pairs: the capability under the reference's ifmOpticalFlow
 * (stage4_match_consecutive.cpp:333-431), offered like svo_hamming_match as a primitive -- SVO_IFM_OPTICAL_FLOW and SVO_DM_KLT stay
 * SVO_ERR_UNSUPPORTED in svo_process.  Each job follows n points of `prev` into `next` with sub-pixel accuracy; nothing is detected or
 * described in `next`.  The arithmetic is THIS PROJECT'S (tests/lk_ref.py is its definition and the device equals it bit for bit:
 * fixed-point bilinear samples, integer Scharr derivatives, exact integer sums, one stated order for the double 2 x 2 solve).  It follows
 * Bouguet's algorithm with the constants cv::calcOpticalFlowPyrLK documents, but equality with OpenCV is NOT claimed.
 *   prev, next   8-bit grey images of the same w, h (strides may differ): host pointers, page-locked host pointers
 *                (SVO_FLAG_PINNED_IMAGES) or device pointers read in place under the read contract of svo_image.stride
 *                (SVO_FLAG_DEVICE_IMAGES, h * stride <= 2^31 - 1).  Any other flag bit is SVO_ERR_ARG.
 *   pts, init    host arrays of n x 2 floats (x, y); init (may be NULL) is the first guess of each point in `next`, pts otherwise
 *   next_pts     n x 2 floats: where each point ended (for a lost point: the guess it had when it was lost)
 *   status       n bytes: 1 tracked, 0 lost (window outside the image at level 0, too little texture, a NaN or infinite coordinate, or
 *                the forward-backward check)
 *   err          NULL or n floats: mean |difference| of the window in grey levels; 0 for a point the forward pass lost
 * Limits, refused up front with SVO_ERR_CAPACITY and the numbers in svo_last_error: n <= max_kps per job, n_jobs <= 4 * n_lanes *
 * max_octaves, images within max_w x max_h.  SVO_ERR_ARG with a text: NULL pointers, win / max_level / max_iters outside their ranges,
 * negative n or n_jobs, prev and next of different sizes, a stride smaller than a row, a device image that spans more than 2^31 - 1
 * bytes.  Every refusal happens before anything is enqueued and leaves the outputs untouched.  n = 0 jobs (their images are still
 * checked, and their pyramids built) and n_jobs = 0 are SVO_OK.
 * The call synchronises.  It touches no lane state and none of the detector's scratch: its pyramids and point lists are buffers of their
 * own, allocated by the first call, grown on demand and freed with the context.  It needs no svo_set_params and never runs inside a
 * captured graph.  p == NULL: the defaults. */
typedef struct svo_lk_job {
    svo_image prev, next;
    const float* pts;
    const float* init;
    int32_t n;
    float* next_pts;
    uint8_t* status;
    float* err;
} svo_lk_job;
void svo_lk_default_params(svo_lk_params* p);
int svo_lk_track(svo_ctx* ctx, const svo_lk_job* jobs, int n_jobs, const svo_lk_params* p, uint32_t flags);
/* one pyramid level of the last svo_lk_track call: job, which = 0 prev / 1 next, level 0 = the image as the tracker read it.  Returns
 * w * h (with out == NULL: the size only); 0 when the call built no such level (or no call was made); SVO_ERR_CAPACITY when cap < w * h.
 * Level 0 of a device image is read from the caller's memory, which must still hold it. */
int svo_debug_lk_get_level(svo_ctx* ctx, int job, int which, int level, uint8_t* out, int cap, int* w, int* h);
/* THE ROW TRACKER: svo_lk_track with one unknown.  The template of a point is taken from `prev` at pts, and its partner is searched in
 * `next` ALONG THE ROW of the guess (init, else pts): x alone moves, with the gradient Ix alone, so it also follows a vertical edge, on
 * which the two-dimensional tracker gives up.  For a rectified stereo pair prev is the left image and next the right one.  It takes the
 * records, flags and limits of svo_lk_track, makes the same refusals in the same order, uses the same buffers and pyramid kernel,
 * synchronises as it does, never runs inside a captured graph, and svo_debug_lk_get_level answers for it as for svo_lk_track.
 * tests/lk_row_ref.py is its definition and the device equals it bit for bit; against svo_lk_track:
 *   - the guess's y is never updated: next_pts[i].y is the guess's y (init's bit pattern, else the point's);
 *   - A11 = sum Ix^2; a level is skipped (at level 0 the point is lost) when A11 / win^2 < min_eig;
 *   - an iteration moves x by -b1 / A11, b1 = sum (J - I) Ix, and stops on |dx| <= eps, on the oscillation rule applied to dx, or
 *     after max_iters;
 *   - under fb_max the way back runs from next to prev along the row of the forward result, and the distance is |back.x - pts.x|.
 * svo_lk_track itself is untouched by it. */
int svo_lk_track_rows(svo_ctx* ctx, const svo_lk_job* jobs, int n_jobs, const svo_lk_params* p, uint32_t flags);
/* PHOTOMETRIC COMPENSATION: a mode of the context's TRACKER.  In mode 0 (the default) both trackers minimise sum (J - I)^2 on raw grey
 * values: a patch has to keep its brightness from prev to next.  In mode 1 every LK launch of the context estimates and removes an
 * affine brightness change J ~ (1 + a) I + b between template and target -- per window, per level and per iteration, so auto-exposure,
 * two cameras with gains and offsets of their own and slow vignetting no longer move or lose the points.  a and b are eliminated in
 * closed form from exact integer window sums; nothing photometric is carried between iterations or levels and nothing new is returned.
 * tests/lk_photo_ref.py is the definition of mode 1 and the device equals it bit for bit; against tests/lk_ref.py / lk_row_ref.py:
 *   - the gradient matrix and the right-hand side are the centred window moments with the template's own direction removed
 *     (A11 = (Cxx - CxI^2 / CII) / n, b1 = (Cdx - CxI CdI / CII) / n, ...; n = win^2, C.. = n S.. - S. S.);
 *   - a template flat to 1/32 grey level (CII == 0) skips the level like a small eigenvalue does; a template that is an exact ramp cannot
 *     be told from an offset and is lost by the min_eig test on the reduced matrix;
 *   - err is the mean |difference - its window mean| in grey levels: the offset is removed from it, the gain is not;
 *   - the forward-backward pass (fb_max > 0) is compensated too, with the image roles swapped.
 * The mode applies to svo_lk_track, svo_lk_track_rows, the tracker passes of svo_klt_step (the temporal passes and the row pass of
 * svo_klt_set_stereo(1)) and the left-to-right pass of svo_klt_topup.  It is read when a call is enqueued.  Every contract of the front
 * end below that is phrased as "what this recipe of public calls leaves" holds verbatim in mode 1: the recipe's svo_lk_track /
 * svo_lk_track_rows calls run on a context in the same mode.  Launch counts and kernel-time names ("lk_track", "lk_track_row") are those
 * of mode 0.
 * The setter is accepted at any time after svo_create: it needs no svo_set_params and no svo_klt_enable.  The mode belongs to the
 * tracker, not to the front end: an svo_klt_enable that re-makes the front end's buffers does NOT reset it.  Any mode but 0 and 1 is
 * SVO_ERR_ARG with a text, and inside a captured graph the setter is SVO_ERR_STATE; a refused call leaves the mode as it was. */
int svo_lk_set_photometric(svo_ctx* ctx, int mode);   /* 0 raw differences (default), 1 gain and bias removed per window */
int svo_lk_get_photometric(const svo_ctx* ctx);

/* Shi-Tomasi corner detection on caller images, batched over many images: the capability under the reference's dmKLT
 * (stage2_detect.cpp:444-449: cv::goodFeaturesToTrack with quality 0.01, minimum distance 20, block 3), offered like svo_lk_track as a
 * primitive -- SVO_DM_KLT stays SVO_ERR_UNSUPPORTED in svo_process.  The arithmetic is THIS PROJECT'S (tests/gftt_ref.py is its
 * definition and the device equals it bit for bit): integer Sobel derivatives and block sums with reflect-101 borders, the smaller
 * eigenvalue 0.5 * ((a + c) - sqrt((a - c)^2 + 4 b^2)) in double with one operation per operator, rounded to float32; the threshold
 * float32(quality * the image's largest response); candidates = pixels off the border ring above the threshold and not below any of
 * their eight neighbours; candidates walked by descending response (ties: raster order) and accepted unless a corner accepted before
 * (integer dx^2 + dy^2 < min_distance^2) or a seed (the same in float32) is closer than min_distance.  Equality with OpenCV is NOT
 * claimed.
 *   img        8-bit grey image with both sides >= 8: a host pointer, a page-locked host pointer (SVO_FLAG_PINNED_IMAGES) or a device
 *              pointer read in place under the read contract of svo_image.stride (SVO_FLAG_DEVICE_IMAGES, h * stride <= 2^31 - 1).
 *              Any other flag bit is SVO_ERR_ARG.
 *   seeds      NULL or n_seeds x 2 floats (x, y), a host array: points the caller already follows.  New corners keep min_distance from
 *              them; they are never output.  A seed that is not finite or lies outside [0, w) x [0, h) is ignored.
 *   cap        room in pts / response (may be 0)
 *   pts        cap x 2 floats: the corners (x, y) in walk order; response (NULL or cap floats): their responses
 *   info       3 ints: corners written = min(accepted, cap, max_corners if > 0); the number of candidates before the distance rule;
 *              status: 0, or 1 when the job had more candidates than max(1024, svo_config.max_cand) -- then no corner is written,
 *              the count is still the true one and the other jobs of the call are unaffected.
 * Limits, refused up front with SVO_ERR_CAPACITY and the numbers in svo_last_error: cap, n_seeds, max_corners <= max_kps, n_jobs <=
 * 4 * n_lanes * max_octaves, images within max_w x max_h, and a response-map buffer (4 bytes per pixel of the call) that cannot be
 * allocated; a context whose max_cand exceeds 2^24 is refused too.  SVO_ERR_ARG with a text: NULL pointers, parameters outside their ranges (svo_types.h), negative counts, a side below 8,
 * a stride smaller than a row, a device image that spans more than 2^31 - 1 bytes.  Every refusal happens before anything is enqueued
 * and leaves the outputs untouched.  n_jobs = 0 is SVO_OK.
 * The call synchronises.  It touches no lane state and none of the detector's scratch: its buffers are its own, allocated by the first
 * call, grown on demand and freed with the context.  It needs no svo_set_params and never runs inside a captured graph.  p == NULL: the
 * defaults. */
typedef struct svo_gftt_job {
    svo_image img;
    const float* seeds;
    int32_t n_seeds, cap;
    float* pts;
    float* response;
    int32_t* info;
} svo_gftt_job;
void svo_gftt_default_params(svo_gftt_params* p);
int svo_gftt_detect(svo_ctx* ctx, const svo_gftt_job* jobs, int n_jobs, const svo_gftt_params* p, uint32_t flags);
/* the response map of one job of the last svo_gftt_detect call, w * h floats in raster order.  Returns w * h (with out == NULL: the size
 * only); 0 when the last call had no such job (or no call was made); SVO_ERR_CAPACITY when cap < w * h. */
int svo_debug_gftt_get_response(svo_ctx* ctx, int job, float* out, int cap, int* w, int* h);

/* A KLT FRONT END RESIDENT ON THE DEVICE: a per-context track table and one call per frame that follows every lane's tracks into the
 * new stereo pair with the tracker of svo_lk_track, gates and compacts them, writes the lane's current-frame lists as the
 * precomputed-data bypass would, and optionally runs stage 5.  Nothing synchronises inside a step.  The selectors SVO_DM_KLT and
 * SVO_IFM_OPTICAL_FLOW stay refused by svo_process.  Tracks only die in a step: svo_klt_topup (below) replaces them on the device; the host
 * recipe it equals is svo_klt_get_tracks, svo_gftt_detect (the tracks as seeds), svo_lk_track (left to right) and svo_klt_add_points.
 * THE CONTRACT: after a step every getter of the lane -- keypoints, pairings, tracked pairs, pairing IDs, both row tables, the values
 * record, the result with residuals and outliers -- returns, byte for byte, what this host recipe leaves: a call that only shifts
 * (svo_process_lanes with no run bit), svo_lk_track with svo_klt_params.lk on the lane's (left[t-1], left[t], left points) and
 * (right[t-1], right[t], right points), the gate below on the host, then svo_put_features_oct (both sides, descriptors NULL),
 * svo_put_matches_oct, svo_put_match_ids_oct, svo_put_tracked_oct for octave 0 of the current frame, and svo_process_lanes with
 * SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT.  tests/klt_ref.py holds that recipe and the walk of the selection.
 * A lane's table holds up to `cap` tracks: left point, right point, ID, age, its index in the list of the last step and its index p in
 * the list of the lane's PREVIOUS slot (-1: none).  svo_klt_step, for every lane of the mask (an idle lane keeps its table, its
 * pyramids, its lists and its record, as if the call had not been made):
 *   1. the prev/cur shift of svo_process, its recovery rule included (a lane whose last call ended in voecBadTracking or
 *      voecBadCondNumber keeps its previous frame);
 *   2. level 0 of both images is copied into the front end's own buffers and the pyramid levels are built; the pyramid of the lane's
 *      last pair is still there and is not rebuilt.  HOST images (with or without SVO_FLAG_PINNED_IMAGES) are free once the call returns
 *      unless they are pinned, DEVICE images (SVO_FLAG_DEVICE_IMAGES) and pinned ones once the enqueued work has run (svo_wait);
 *   3. both lists are tracked from the lane's last pair into the new one (forward-backward as well when lk.fb_max > 0).  A lane without
 *      a last pair -- its first step, or the first after svo_klt_reset -- tracks nothing: its points stand as they are, status 1;
 *   4. a slot survives when both statuses are 1, all four coordinates are finite, |yl - yr| <= max_dy and min_disp <= xl - xr <=
 *      max_disp (float32 compares as written).  Survivors keep their order and become keypoint i of both lists (size = lk.win, angle
 *      -1, response 0, octave 0, class_id = the track's ID), pairing i -> i (imgIdx 0, distance 0), pairing ID i = the track's ID, and
 *      one tracked pair (p, i) per survivor that has a p: the index the track had in the list of the last step when the lane shifted
 *      in 1, its old p when the lane held its previous frame.  The compacted table (age + 1) replaces the old one;
 *   5. stage 5 with SVO_RUN_OPTIMIZE, as svo_process enqueues it (pose covariance and landmarks included while they are on).
 * flags: SVO_RUN_OPTIMIZE, SVO_FLAG_DEVICE_IMAGES or SVO_FLAG_PINNED_IMAGES; any other bit is SVO_ERR_ARG, SVO_FLAG_BGR_IMAGES included.
 * svo_klt_enable allocates (NULL: the defaults, cap = min(1024, max_kps)); called again with other parameters it returns SVO_ERR_STATE
 * unless every table is empty.  A context that never calls it allocates and launches nothing for the front end.
 * svo_klt_add_points appends behind the lane's live count: fresh IDs (the lane's last ID + 1 ..., from 0), age 0, no indices; points
 * beyond cap are dropped and the number appended is returned.  It and svo_klt_get_tracks (returns the live count, writes min(count, cap)
 * entries; any array may be NULL) synchronise.  svo_klt_reset empties the tables of the lanes of the mask (NULL: all), forgets
 * their last pairs and starts their IDs over from 0: such a lane is a fresh stream.
 * svo_debug_klt_select runs 1 and 4 on ONE lane with the caller's arrays in place of the tracker's results (n must be the live count,
 * else SVO_ERR_ARG): the selection on inputs no image could produce.
 * Refusals, all before anything is enqueued, with the outputs untouched and a text in svo_last_error: SVO_ERR_STATE when the front end
 * is not enabled, when svo_set_params has not been called, inside a captured graph, or for a member context of a frame-parallel
 * stream (svo_batch.h; svo_klt_enable refuses it already); SVO_ERR_ARG / SVO_ERR_CAPACITY for parameters out
 * of range (cap > max_kps: capacity), a mask bit at or above n_lanes, NULL images, images not of one size, below 64 x 64 or above
 * max_w x max_h (capacity), strides below a row, device spans above 2^31 - 1 bytes; and whatever svo_process refuses for a
 * SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT call under the parameters in force.
 * Not carried by state files, hand-over records or the RCCL companion; no svo_batch / frame-parallel form; octave 0 only. */
void svo_klt_default_params(svo_klt_params* p);
int svo_klt_enable(svo_ctx* ctx, const svo_klt_params* p);
int svo_klt_reset(svo_ctx* ctx, const uint64_t lanes[2] /* NULL = all lanes */);
int svo_klt_add_points(svo_ctx* ctx, int lane, const float* left_xy, const float* right_xy, int n);
int svo_klt_step(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, const uint64_t lanes[2] /* NULL = all lanes */);
int svo_klt_get_tracks(svo_ctx* ctx, int lane, float* left_xy, float* right_xy, int32_t* ids, int32_t* age, int cap);
int svo_debug_klt_select(svo_ctx* ctx, int lane, const float* left_xy, const float* right_xy,
                         const uint8_t* status_l, const uint8_t* status_r, int n);

/* THE TOP-UP OF THE KLT FRONT END, RESIDENT ON THE DEVICE: tracks only die in svo_klt_step; svo_klt_topup replaces them without a host
 * round trip.  One call looks at every lane of the mask, decides ON THE DEVICE which of them have thinned, detects new corners there
 * with the detector of svo_gftt_detect (the live tracks as seeds), finds their partners in the right image with the tracker of
 * svo_lk_track, gates the pairs and appends the survivors to the lane's table.  Nothing synchronises inside the call and the host
 * reads nothing back.
 * THE CONTRACT: after a svo_klt_topup call and svo_wait, svo_klt_get_tracks (points, IDs, ages, count) of every lane, and every getter
 * after any later svo_klt_step, return byte for byte what this host recipe leaves, lane by lane for the lanes of the mask that have a
 * last pair in the front end, n being the lane's live count:
 *   1. n >= below: nothing happens.  Otherwise want = max(min(target, cap) - n, 0);
 *   2. svo_gftt_detect with one job: the left level-0 image of the lane's last pair, tightly packed, as the last svo_klt_step copied
 *      it; seeds = the n live left points; the job's cap = want; the parameters `gftt`;
 *   3. svo_lk_track with one job: (left, right) of that last pair, pts = the new corners, init = the corners shifted by
 *      (-init_disp, 0) in float32, the parameters svo_klt_params.lk as enabled (fb_max included: the left-right-left check);
 *   4. the gate of svo_klt_step item 4 on (corner, partner): status 1, four finite coordinates, |yl - yr| <= max_dy and
 *      min_disp <= xl - xr <= max_disp (float32 compares as written);
 *   5. svo_klt_add_points with the survivors in walk order: fresh IDs from the lane's next ID, age 0, no indices; what lies beyond cap
 *      is dropped.
 * A lane outside the mask, at or above `below`, or without a last pair (never stepped, or reset since) keeps its table bit for bit,
 * the NaN tail included.  Lane lists, records, results, stage 5 outputs and the pyramids are never touched.  tests/klt_topup_ref.py
 * holds the recipe.
 * svo_klt_topup_info (synchronises): info[0] corners detected, info[1] candidates before the distance rule, info[2] tracks appended,
 * info[3] why, for the lane in the last call: 0 topped up; 1 more candidates than max(1024, svo_config.max_cand), nothing is written,
 * as in svo_gftt_detect; 2 not below the threshold; 3 no last pair; 4 not in the mask.
 * svo_klt_topup_enable allocates the top-up's own buffers (NULL: the defaults), the response maps among them: 4 bytes per pixel for
 * n_lanes images of max_w x max_h; a context that never calls it allocates and launches nothing for the top-up.  svo_gftt_detect and
 * svo_lk_track calls made in between are undisturbed, and their debug getters keep answering for the caller's last call.  A
 * svo_klt_enable that re-makes the front end's buffers (other parameters, empty tables) drops the top-up: enable it again.
 * svo_debug_klt_topup_append runs items 4 and 5 alone on ONE lane with the caller's arrays in place of the detector's corners and the
 * tracker's results (0 <= n <= cap; no threshold applies); it synchronises.
 * Refusals, all before anything is enqueued, with the outputs untouched and a text in svo_last_error: SVO_ERR_STATE when the front end
 * or the top-up is not enabled, inside a captured graph, or when svo_klt_topup_enable is called again with other parameters after a
 * top-up has run while a table holds tracks; SVO_ERR_ARG / SVO_ERR_CAPACITY for parameters out of range (the gftt ranges of
 * svo_types.h, below or target outside 1 .. cap, a non-finite init_disp), a mask bit at or above n_lanes, a context whose max_cand
 * exceeds 2^24 (capacity), and a response-map buffer the device cannot provide (capacity). */
void svo_klt_topup_default_params(const svo_ctx* ctx, svo_klt_topup_params* p);   /* needs cap: after svo_klt_enable (before: cap = min(1024, max_kps)) */
int svo_klt_topup_enable(svo_ctx* ctx, const svo_klt_topup_params* p);
int svo_klt_topup(svo_ctx* ctx, const uint64_t lanes[2] /* NULL = all lanes */);
int svo_klt_topup_info(svo_ctx* ctx, int lane, int32_t info[4]);
int svo_debug_klt_topup_append(svo_ctx* ctx, int lane, const float* left_xy, const float* right_xy, const uint8_t* status, int n);

/* STAGE 4'S RANSAC ON THE TRACKED PAIRS A LANE HOLDS, AND AS A GATE INSIDE svo_klt_step.  The detect-match-track path verifies its
 * tracked pairs with cv::findFundamentalMat(FM_RANSAC, 1.0, 0.99) on the left and on the right point pairs (stage4_match_consecutive.cpp:
 * 202-255, 684-699); lists that arrive through the precomputed-data bypass (svo_put_tracked_oct) and the lists of the resident KLT front
 * end had no such verification.  svo_ransac_tracked runs the same device RANSAC -- the sampler of cv::RNG, the LMedS registrator for 8 to
 * 14 pairs, the direct path for 7 -- on what the lanes hold.  It enqueues on the context's stream and never synchronises.
 * For every lane of the mask (NULL: all) and every octave below n_octaves:
 *   candidates   the lane-octave's tracked pairs (first, second) in list order; first indexes the pairings of the lane's PREVIOUS slot,
 *                second those of its current slot.  The left point pair is the previous left keypoint of pairing `first` (queryIdx) and
 *                the current left keypoint of pairing `second`; the right pair the same through trainIdx.  A pair with an index outside
 *                its pairing list, or whose pairings point outside their keypoint lists, is no candidate and never reaches the output
 *                (the puts validate nothing; this call does);
 *   the rule     one RANSAC per side on the candidates (oracle: svo_oracle_ransac_fundamental); use_f = both inlier counts >= 8.  With
 *                use_f a candidate survives iff both masks hold it; without it -- 0 to 7 candidates, the 7-pair direct path, a side that
 *                finds no model -- every candidate survives.  There is no consistency check, no bad-tracking gate and no min_pairs rule;
 *   the output   the survivors keep their order and replace the list (svo_get_tracked_oct); nothing else of the lists changes;
 *   track_stats  the lane's eight counters describe THIS call alone, summed over the octaves: SVO_TS_THRESHOLD = pairs in the list before
 *                the call, SVO_TS_COLLISION = candidates, SVO_TS_INLIERS_L / _R and SVO_TS_HYP_L / _R = each side's inlier count and
 *                hypotheses visited, SVO_TS_BOTH_MASKS = SVO_TS_TRACKED = survivors.  No other field of the record is written.
 * A lane of the mask without a previous frame gets empty lists and zero counters (no error code is written); a lane outside the mask is
 * untouched.  Refusals, before anything is enqueued, with a text in svo_last_error: SVO_ERR_STATE before svo_set_params, before the
 * context has a geometry (put or load lists, or process a frame, first) and inside a captured graph; SVO_ERR_ARG for a mask bit at or
 * above n_lanes.  tests/ransac_tracked_ref.py holds the walk.
 * ONE BEHAVIOUR OF THE REFERENCE'S ARITHMETIC TO KNOW: with 8 to 14 candidates OpenCV's LMedS path runs, and it can reject half of a
 * clean list (the oracle, on synthetic stereo tracks: 9 of 14 pairs rejected, 2 of them planted outliers).  With 15 or more clean pairs
 * it rejected none; with 40 to 1024 pairs and 15-20 % planted outliers it rejected 85-100 % of those and at most 2 % of the good pairs.
 *
 * svo_klt_set_ransac(ctx, mode) makes the same sequence a gate inside svo_klt_step and svo_debug_klt_select, between the selection
 * (item 4) and stage 5, for the step's active lanes.  It is accepted once svo_klt_enable has succeeded (SVO_ERR_STATE before, and inside
 * a captured graph; SVO_ERR_ARG for another mode); svo_klt_get_ransac returns the mode.
 *   0 (default)  a step allocates, launches and returns exactly what it did without this call;
 *   1            the tracked pairs are filtered and the lane's track_stats filled; the current-frame lists and the table stay as the
 *                selection wrote them;
 *   2            as 1, and the tracks whose pair was rejected leave the table: the live tracks are compacted in order, the slots behind
 *                the new count become empty, the survivors keep the index they have in the step's lists, no ID is given out again.  A
 *                lane that rejected nothing writes nothing.  Under the LMedS behaviour above a lane with 8 to 14 tracked pairs can lose
 *                half of them in a step; svo_klt_topup then finds a thinner table and refills it.
 * THE CONTRACT is svo_klt_step's with public calls added: after a step every getter and svo_klt_get_tracks return byte for byte what
 * this leaves: the recipe of svo_klt_step up to and including its puts; svo_ransac_tracked on the step's lanes; for mode 2
 * svo_get_tracked, and every track that had a tracked pair and lost it removed from the host's table; then svo_process_lanes with
 * SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT.  That last call starts the lane's record afresh, track_stats included, so the gate's counters
 * are there to read after a step WITHOUT SVO_RUN_OPTIMIZE (and after svo_debug_klt_select) and are zero after a step with it: to have
 * both, step without the flag, read them, and make the svo_process_lanes call of the recipe.  svo_klt_topup is unchanged.  No svo_batch, frame-parallel or graph-captured form. */
int svo_ransac_tracked(svo_ctx* ctx, const uint64_t lanes[2] /* NULL = all lanes */);
int svo_klt_set_ransac(svo_ctx* ctx, int mode);
int svo_klt_get_ransac(const svo_ctx* ctx);

/* POSE-PREDICTED FIRST GUESSES FOR svo_klt_step.  A step starts the search for every track at the track's old position; the lane holds
 * what a stereo front end predicts from instead: the depth of every track (xl, yl, xr and the camera stage 5 runs with) and the pose
 * increment stage 5 estimated a frame ago (svo_result.delta).  svo_klt_set_prediction(ctx, 1) makes a step triangulate each track, move it
 * by that increment (constant velocity), reproject it into both cameras and start the forward tracking pass there; nothing is read back
 * and nothing synchronises.  It is accepted once svo_klt_enable has succeeded (SVO_ERR_STATE before, and inside a captured graph;
 * SVO_ERR_ARG for a mode other than 0 and 1); svo_klt_get_prediction returns the mode.
 *   0 (default)  a step allocates, launches and returns exactly what it did without this call;
 *   1            the first call allocates the one buffer of the mode (a float2 per lane, side and slot, a byte per lane and slot).  A
 *                svo_klt_enable that re-makes the front end's buffers drops it and returns to mode 0, as it drops the top-up.
 * THE RULE, for a lane of the step's mask that tracks (it has a last pair) and slot s below its live count, (xl, yl), (xr, yr) the slot's
 * float32 points.  The device's definition is k_project_points (k_gn.hip), its restatement svo_oracle_project; every compare is written
 * as it is evaluated:
 *   1  the lane predicts iff svo_result.valid != 0 and all six delta values are finite, the record taken as svo_get_result would
 *      return it immediately before the step.  Nothing else is consulted, neither ages nor error codes: after a step without
 *      SVO_RUN_OPTIMIZE, or one that ended invalid, the record says so and the lane does not predict;
 *   2  triangulate in double, one operation per operator, with ul = xl, vl = yl, ur = xr: disparity = fl*(cur - ur) + fr*(ul - cul),
 *      b_d = baseline/disparity, X = (b_d*fr*(ul - cul), b_d*fr*(vl - cvl), b_d*fl*fr);
 *   3  move and project: the rotation R of delta's first three values (the reference's Rodrigues formula with its small-angle
 *      branch), Xc = R X + t, and the four float32 pixels uL vL uR vR exactly as k_project_points stores them;
 *   4  the slot is predicted (used = 1) iff the lane predicts, disparity > 0 and Z1c > 0 (compared in double), all four pixels are
 *      finite, and both guesses lie inside the image: 0 <= x <= w - 1 and 0 <= y <= h - 1, compared in float32 against the level-0
 *      size of the lane's last pair.  Then the left guess is (uL, vL) and the right guess (uR, vR); otherwise used = 0 and both
 *      guesses are the slot's own points, bit for bit -- which tracks exactly as no guess does;
 *   5  the slots behind the live count get NaN guesses and used = 0.
 * Lanes that do not predict, lanes outside the mask and lanes without a last pair get their own points and used = 0.  Only the forward
 * pass starts from the guesses: the forward-backward pass under fb_max, the gate, the RANSAC gate, svo_klt_topup and stage 5 are as
 * they were.  A lost point reports the guess it had when it was lost (svo_lk_track): with the prediction on, the predicted one.
 * THE CONTRACT is svo_klt_step's with public calls added: after a step in mode 1 every getter of the lane and svo_klt_get_tracks return
 * byte for byte what the recipe of svo_klt_step leaves when svo_get_result and svo_klt_get_tracks are read before its shift call, the
 * guesses are computed by the rule on the host, and they are passed as `init` of both svo_lk_track jobs of the lane
 * (tests/klt_predict_ref.py holds the walk and the recipe).
 * svo_klt_predicted synchronises and returns, for the lane's live tracks, the guesses the next svo_klt_step would start from as things
 * stand now (the lane's record and table of this moment; a lane without a last pair does not predict): it returns the live count, like
 * svo_klt_get_tracks, and writes min(count, cap) entries of left_xy / right_xy (x, y pairs) and `used`; any array may be NULL.
 * svo_debug_klt_predict runs the same kernel on the lane's table with the caller's delta6 and valid in place of the lane's record:
 * the rule on inputs no sequence could produce, the counterpart of svo_debug_klt_select.  Neither changes a table, a list or a record.
 * Both are refused with SVO_ERR_STATE before svo_klt_enable, before svo_set_params, inside a captured graph and while the mode is 0,
 * and with SVO_ERR_ARG for a lane outside the context, cap < 0 or delta6 == NULL, in that order.
 * No constant-image-flow mode for lanes without a valid pose, no prediction from a caller's pose or an IMU, no automatic choice of the
 * pyramid depth, no prediction inside svo_klt_topup; no svo_batch, frame-parallel or graph-captured form. */
int svo_klt_set_prediction(svo_ctx* ctx, int mode);     /* 0 off (default), 1 constant-velocity pose prediction */
int svo_klt_get_prediction(const svo_ctx* ctx);
int svo_klt_predicted(svo_ctx* ctx, int lane, float* left_xy, float* right_xy, uint8_t* used, int cap);
int svo_debug_klt_predict(svo_ctx* ctx, int lane, const double* delta6, int valid,
                          float* left_xy, float* right_xy, uint8_t* used, int cap);

/* STEREO RE-ASSOCIATION FOR svo_klt_step.  A step follows a track's left and right point independently through time, and nothing ties
 * the halves of a pair to each other again: each drifts on its own until the gate drops the pair.  svo_klt_set_stereo(ctx, 1) makes a
 * step track the LEFT list through time only and find every right point afresh in the NEW pair, along the row of the new left point,
 * with the row tracker of svo_lk_track_rows.  It is accepted once svo_klt_enable has succeeded (SVO_ERR_STATE before, and inside a
 * captured graph; SVO_ERR_ARG for a mode other than 0 and 1); svo_klt_get_stereo returns the mode.
 *   0 (default)  a step allocates, launches and returns exactly what it did without this call;
 *   1            the first call allocates the buffers of the mode (a job record per lane, a float2 per lane, side and slot).  A
 *                svo_klt_enable that re-makes the front end's buffers drops them and returns to mode 0, as it drops the top-up.
 * In mode 1 item 3 of a step becomes, for every active lane:
 *   3a  the left list is tracked through time exactly as in mode 0 (prediction guesses, fb_max; a lane without a last pair: its
 *       points stand with status 1);
 *   3b  for each slot the right point is found by svo_lk_track_rows' tracker on (left[t], right[t]) -- the pyramids the step has just
 *       built -- with pts = the left results of 3a and init = (xl' - (xl - xr), yl') in float32 as written, (xl, xr) the table's old
 *       points and (xl', yl') the result of 3a; svo_klt_params.lk applies, fb_max included (left, right and back along the row).  A
 *       lane without a last pair runs 3b too: it needs the new pair only.  Right status and right point go where the pass through
 *       time put them; the gate, the RANSAC gate, the prune, stage 5 and svo_klt_topup are as they were.  Every surviving pair has
 *       yr == yl bit for bit.  The predicted right guesses of svo_klt_set_prediction(1) are not used; svo_klt_predicted is unchanged.
 * Nothing synchronises, nothing is read back and nothing is allocated per step.
 * THE CONTRACT is svo_klt_step's with public calls: after a step in mode 1 every getter of the lane and svo_klt_get_tracks return byte
 * for byte what the recipe of svo_klt_step leaves when its second svo_lk_track job (the right list through time) is replaced by a
 * svo_lk_track_rows job on (left[t], right[t], pts = the left job's next_pts, init as above) (tests/klt_stereo_ref.py holds it).
 * No row association inside svo_klt_topup, no predicted disparity as the guess, no unrectified pairs, no bound on the row search; no
 * svo_batch, frame-parallel or graph-captured form. */
int svo_klt_set_stereo(svo_ctx* ctx, int mode);         /* 0 the right list through time (default), 1 the right partner along the row */
int svo_klt_get_stereo(const svo_ctx* ctx);

/* debugging / parity probes */
int svo_debug_get_level(svo_ctx* ctx, int lane, int side, int level, uint8_t* out, int cap, int* w, int* h);
int svo_debug_get_raw_keypoints(svo_ctx* ctx, int lane, int side, svo_keypoint* kps, uint8_t* desc, int cap);
int svo_debug_get_status_word(svo_ctx* ctx, int lane, uint32_t* w);   /* capacity-overflow bits */
/* svo_use_graphs bookkeeping: graphs this context holds (one per distinct captured call) and calls served by replaying one since
 * svo_create; either pointer may be NULL.  A call that runs as plain launches moves neither. */
int svo_debug_get_graph_count(svo_ctx* ctx, uint32_t* captured, uint32_t* replayed);
/* 1 when the reference's profiler sections (CTimeLogger names: "processNewImagePair", "_stg1" .. "_stg5", "stg3.find_pairings",
 * "stg4.track") are being emitted as roctx ranges around the enqueue of each stage: SVO_ROCTX=1 in the environment, or a rocprofv3
 * session (it sets ROCP_TOOL_LIBRARIES); the roctx library is looked up with dlopen, never linked. */
int svo_profiler_sections_enabled(void);
/* How often the speculative FAST threshold of k_fast failed since svo_create (or the last reset = 1 call): (image, level) pairs
 * that a frame had to run again at the caller's threshold (k_fast_redo + the second k_select pass).  Waits for the enqueued work. */
int svo_debug_get_redo_count(svo_ctx* ctx, uint32_t* pairs, int reset);
/* What was really in flight (SVO_TIMELINE=1 in the environment of svo_create; a measuring knob, off in production): every kernel stamps
 * the hull [first wave in, last wave out] of its launch on the device-wide 100 MHz wall clock.  out receives 4096 records of two uint64
 * (t0, t1; t0 = ~0: no such launch) for the last 16 frames: index = (frame % 16) * 256 + kind * 8 + aux, kinds in bench.py's
 * TIMELINE_KINDS order.  Returns the context's frame counter (0: the knob is off); reset = 1 clears the table.  Waits for the work. */
int svo_debug_timeline(svo_ctx* ctx, uint64_t* out, int cap_records, int reset);

/* per-kernel HIP-event timing (svo_config.kernel_times = 1): names[i] points to static storage.
 * total_ms[i] / calls[i] accumulate since the last svo_kernel_times_reset. Returns number of kernels.
 * THE NUMBER RETURNED DEPENDS ON THE CONTEXT'S STATE in one respect: the last two names are listed only on request -- "pose_covariance"
 * while svo_set_pose_covariance is on, and "landmarks" behind it while svo_set_landmarks is on (then with "pose_covariance" before it
 * whatever that switch says) --, so a context that has both off returns the list (and the count) it always did.  Size arrays by the
 * value of the same call, or for the largest list (cap 64 always suffices).
 * "gftt_response", "gftt_candidates" and "gftt_select" are appended behind whatever that rule lists, once the context has made a
 * svo_gftt_detect call; "lk_pyrdown" and "lk_track" behind those, once the context has made a svo_lk_track call or a svo_klt_step
 * (whose pyramid and tracking launches count there); "klt_select" behind the lk names, once the context has made a svo_klt_step or a
 * svo_debug_klt_select; "klt_topup" behind that, once the context has made a svo_klt_topup or svo_debug_klt_topup_append call (its
 * three kernels count there, its detector and tracker launches under the gftt and lk names, which are then listed as well, and
 * "klt_select" with them); "ransac_feed" behind all of those, once the context has made a svo_ransac_tracked call or a step under
 * svo_klt_set_ransac (the RANSAC launches behind it count under "ransac_hyp" .. "track_finalize"), "klt_prune" behind it, once a step
 * in mode 2 has run, "klt_predict" behind it, once the context has made a step under svo_klt_set_prediction(1) or a svo_klt_predicted /
 * svo_debug_klt_predict call, and "lk_track_row" last, once the context has made a svo_lk_track_rows call or a step under
 * svo_klt_set_stereo(1) (whose guess kernel counts there too). */
int svo_kernel_times(svo_ctx* ctx, const char** names, double* total_ms, int64_t* calls, int cap);
int svo_kernel_times_reset(svo_ctx* ctx);
/* time only the kernel of that name from now on (NULL or "": all again): two events per kernel cost a few percent of
 * a step, a benchmark that needs the live duration of one kernel need not pay for the others */
int svo_kernel_times_select(svo_ctx* ctx, const char* name);

/* sizeof() of the ABI records as this library was compiled: out[0..5] = keypoint, dmatch, stereo_camera,
 * params, result, config.  Lets a binding verify its mirror of svo_types.h. */
void svo_abi_sizes(int32_t* out6);

#ifdef __cplusplus
}
#endif
#endif
