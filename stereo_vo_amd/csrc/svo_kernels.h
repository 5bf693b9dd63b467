// svo_kernels.h -- host-side launchers of the HIP kernels (defined in k_detect.hip, k_match.hip, k_gn.hip).  The launchers that consult a
// run-time knob take the context's Knobs (svo_knobs.hpp); none reads the environment.
#pragma once
#include "svo_device.h"
#include "rectify_model.hpp"

struct GNParams {
    int use_robust_kernel, max_iters, initial_max_iters, max_incr_cost;
    int use_previous_pose_as_initial, use_custom_initial_pose;
    int min_distance, img_w, img_h;      // grid of the stage-5 NMS mask (S5:465-468)
    int pmax;                            // power of two >= max_kps (LDS carve)
    int standalone;                      // 1: getChangeInPose entry (no prev/bad-tracking gate)
    int pad;
    double kernel_param, min_mod_out_vector, residual_threshold;
    double init[6];
    uint8_t* mask_out;                   // nullptr, or the array k_gauss_newton leaves its final mask in for k_pose_covariance and k_landmarks (gn_mask_bytes_per_lane each)
};

// Which kernel forms are the PRODUCT and which are kept as A/B anchors only.  Every form below is compiled and run
// against the oracle by tests/test_gpu_parity.py (test_every_ransac_kernel_form_gives_the_oracle_models,
// test_kernel_launch_knobs_do_not_change_results); the launchers pick the product form unless a debug knob says otherwise.
//   product, many lanes (> 8 lane-octaves):  k_hamming_f4, k_ransac_hyp_thread, k_ransac_count_mfma16
//   product, few lanes (one stream alone):   k_hamming_f4, k_ransac_hyp (16 lanes per sample), k_ransac_count<4> (VALU, for latency)
//   product, other entry points:             k_hamming_plain (svo_hamming_match), k_track_gate (multi-octave contexts), k_project_points,
//                                            k_faster_anms (svo_set_faster_adaptive_nms) and k_anms_list (svo_adaptive_nms), one body
//   A/B only (never launched by default):    k_hamming + k_gather_mdesc (the int8 matcher, SVO_HAM_FP4=0), k_ransac_count_mfma (4 x 4 tiles,
//                                            SVO_DEBUG_MODE=52), k_ransac_count<16> (SVO_DEBUG_MODE=14).  Since round 6 these are compiled only
//                                            under -DSVO_AB_KERNELS: the product libsvo_hip.so does not contain them (svo_create refuses the
//                                            knobs there), libsvo_hip_ab.so does -- tests and A/B runs load it through SVO_HIP_LIB.
bool svo_ab_kernels_built();                   // k_match.hip: compiled with -DSVO_AB_KERNELS (libsvo_hip_ab.so)
// (svo_ab_form_requested(const Knobs&), svo_knobs.hpp: SVO_HAM_FP4=0 or SVO_DEBUG_MODE 14 / 52 in the environment of svo_create)
hipError_t svo_upload_tables();
// hipFuncAttributeMaxDynamicSharedMemorySize belongs to (kernel, DEVICE) and is shared by every context of the process on that
// device: keyed by both, only ever raised -- a later, smaller context must not lower the limit under an earlier context's launches,
// and a host with one thread per GPU must set it on every device it uses (the calling thread's current device is the context's).
hipError_t svo_raise_dyn_smem(const void* kernel, size_t bytes);
// stage 1 (k_prepare.hip)
struct PrepArgs {
    const uint8_t* src[2 * SVO_MAX_LANES];   // source image pointers (device memory), by value in the kernel arguments
    const uint2* const* maps;         // device table [n_img] of fixed-point maps (nullptr entries: no rectification), or nullptr
    uint8_t* dst; long long dst_img_stride; int dst_pitch;
    long long src_stride; int channels, w, h;
    LaneMask idle;                    // lanes that sit the call out (DevCtx.idle): their images are neither read nor written
};
void launch_prepare(const PrepArgs& a, int n_img, hipStream_t st);
// the fixed-point map of one image from its calibration (rectify_model.hpp): what k_rectify_map reads per image.  dst holds w * h entries.
struct RectifyImage { RectifyModel m; uint2* dst; };
void launch_rectify_map(const RectifyImage* d_models, int n_img, int w, int h, hipStream_t st);   // d_models: device memory; only the map setters launch it
// frame hand-over between contexts (k_handover.hip)
size_t handover_record_bytes(const DevCtx& c);                  // of the context's kind (DevCtx.carry_win)
size_t handover_record_bytes(const DevCtx& c, bool windows);    // version 2 (false) / version 3 with the SAD windows (true)
void launch_export_frame(const DevCtx& c, uint8_t* blob, const LaneMask& win_cur, const LaneMask& win_prev, hipStream_t st);
void launch_import_frame(const DevCtx& c, const uint8_t* blob, size_t blob_bytes, int need_windows, hipStream_t st);
void launch_pack_values(const DevCtx& c, int lane, int which, int octave, uint8_t* dst, hipStream_t st);
void launch_begin_frame(const DevCtx& c, const uint8_t* const* ptrs, unsigned flags, const LaneMask& drop_prev, hipStream_t st);
void launch_resize(const DevCtx& c, int level, hipStream_t st);
void launch_fast(const DevCtx& c, hipStream_t st);
void launch_select(const DevCtx& c, hipStream_t st);
void launch_describe(const DevCtx& c, const Knobs& k, int pre, hipStream_t st);
void launch_sad_patch(const DevCtx& c, hipStream_t st);       // needs DevCtx.sad_patch / sad_flag (allocated when a SAD selector is first in force)
void launch_publish_img0(const DevCtx& c, const uint8_t* const* ptrs, hipStream_t st);      // svo_gather_windows: the level-0 pointer table of the active lanes, nothing else
void launch_sad_patch_slot(const DevCtx& c, int which, hipStream_t st);                    // the same gather for slot `which` (0 current, 1 previous) of put / loaded lists
hipError_t configure_nms_rowsort(const DevCtx& c);
size_t nms_rowsort_scratch_bytes(int n_img, int oct_cap, int n_keys);      // DevCtx::big_scratch for lists of up to n_keys keys (0 up to 4096: all in LDS)
int nms_rowsort_items(const DevCtx& c);           // keys per thread of the k_nms_rowsort instantiation this geometry launches: 4, 8 or 16
void launch_nms_rowsort(const DevCtx& c, const Knobs& k, int do_nms, int min_distance, int pre, hipStream_t st);
void launch_half(const DevCtx& c, int level, hipStream_t st);
void launch_fastorb_anms(const DevCtx& c, uint32_t* scratch3, hipStream_t st);     // scratch3: fastorb_anms_scratch_words(n_img, cand_total) words
size_t fastorb_anms_scratch_words(int n_img, int cand_total);
void launch_fastorb_nms(const DevCtx& c, int do_nms, int min_distance, hipStream_t st);
// dmFASTER (k_detect.hip): cand64 = [n_img][cand_total] 64-bit keys, allocated by the first svo_process made while it is selected
void launch_faster(const DevCtx& c, unsigned long long* cand64, int fast_th, int klt_win, hipStream_t st);
hipError_t configure_faster_nms(const DevCtx& c);
void launch_faster_nms(const DevCtx& c, const unsigned long long* cand64, int do_nms, int min_distance, hipStream_t st);
// ... under svo_set_dyn_fast_threshold: stats = [n_lanes] records whose next[octave] is the lane's m_threshold.  Two k_faster_dyn launches
// (left images, then right images) read it; the NMS launch behind them commits the new thresholds and the statistics
void launch_faster_dyn(const DevCtx& c, unsigned long long* cand64, const svo_faster_stats* stats, double target, int klt_win, hipStream_t st);
void launch_faster_nms_dyn(const DevCtx& c, const unsigned long long* cand64, int do_nms, int min_distance, svo_faster_stats* stats, double target, hipStream_t st);
// ... under svo_set_faster_adaptive_nms with nmsmAdaptive: k_faster_anms in place of k_faster_nms(_dyn).  scratch = faster_anms_scratch_words()
// 64-bit words; stats = nullptr, or the records above (the launch then commits them as launch_faster_nms_dyn does).  A level holds at most
// faster_anms_max_candidates() candidates.  launch_anms_list: the same device code on one list of keys (svo_adaptive_nms)
hipError_t configure_faster_anms(int max_kps);
size_t faster_anms_scratch_words(int n_img, int cand_total);
int faster_anms_max_candidates();
void launch_faster_anms(const DevCtx& c, const unsigned long long* cand64, unsigned long long* scratch, svo_faster_stats* stats, double target, hipStream_t st);
void launch_anms_list(const unsigned long long* keys, int n, int w, int h, int actual, int max_kps, unsigned long long* scratch, int n_cap, uint32_t* out_pos, hipStream_t st);
void launch_hamming(const DevCtx& c, const Knobs& k, int mode, int nsplit, hipStream_t st);
void launch_match_lr_filter(const DevCtx& c, int one_to_one, double max_y_diff, hipStream_t st);
void launch_track_filter(const DevCtx& c, hipStream_t st);
void launch_ransac_hyp(const DevCtx& c, int chunk, hipStream_t st);
void launch_ransac_count(const DevCtx& c, const Knobs& k, int chunk, hipStream_t st);
void launch_track_finalize(const DevCtx& c, int bad_tracking_th, int win_mode, hipStream_t st);
// svo_ransac_tracked (k_match.hip): k_ransac_feed hands the tracked pairs the lanes HOLD to the RANSAC -- set DevCtx.rs_c0 / rs_c1 first,
// phase 0 of the sample schedule rides in it --, then the three chunks as a frame launches them, then k_track_finalize on the survivor
// list with no bad-tracking gate and no k_track_gate
void launch_ransac_feed(const DevCtx& c, hipStream_t st);
void launch_ransac_stats_clear(const DevCtx& c, hipStream_t st);     // its zeroing phase alone (a gated svo_klt_step ahead of stage 5)
void launch_track_finalize_ungated(const DevCtx& c, hipStream_t st);
// sad = false: smDescRbR / ifmDescWin on the descriptors; sad = true: smSAD / ifmSAD on the windows of launch_sad_patch (max_sad: ifmSAD's threshold)
void launch_match_lr_rbr(const DevCtx& c, bool sad, int one_to_one, double max_y_diff, double minimum_response, int max_distance, hipStream_t st);
void launch_track_win(const DevCtx& c, bool sad, int win_w, int win_h, unsigned max_sad, hipStream_t st);
void launch_match_ids(const DevCtx& c, unsigned flags, hipStream_t st);
void launch_hamming_plain(const uint8_t* q, int nq, const uint8_t* t, int nt, unsigned* out, int nsplit, hipStream_t st);
hipError_t configure_gauss_newton(int pmax);
size_t gn_scratch_bytes_per_lane(int pmax);
hipError_t configure_match(int max_kps);
void launch_project_points(const float* uvu, int n, const svo_stereo_camera& cam, const double* delta6, float* pix, hipStream_t st);
void launch_gauss_newton(const DevCtx& c, const Knobs& k, const GNParams& P, hipStream_t st);
// svo_set_pose_covariance: P as handed to launch_gauss_newton just before (mask_out set), out = one record per lane
size_t gn_mask_bytes_per_lane(int pmax);
// consume: the launch is the last reader of the mask record and clears its ended_valid (false when launch_landmarks follows)
void launch_pose_covariance(const DevCtx& c, const Knobs& k, const GNParams& P, svo_pose_cov* out, bool consume, hipStream_t st);
// svo_set_landmarks: P as handed to launch_gauss_newton just before (mask_out set).  rec = [n_lanes][max_kps] records, info = one per
// lane, cnt = [n_lanes][4] ints that are zero between launches (the blocks of a lane add their counts and take a ticket there),
// cov = the records launch_pose_covariance has just written, or nullptr while svo_set_pose_covariance is off
struct LmkArgs {
    svo_landmark* rec; svo_landmarks_info* info; int* cnt; const svo_pose_cov* cov;
    double std_px, var_px;               // std_noise_pixels and its square
    int ids_on, pad;                     // svo_params.vo_use_matches_ids
};
void launch_landmarks(const DevCtx& c, const GNParams& P, const LmkArgs& A, hipStream_t st);
// svo_lk_track (k_lk.hip).  One record per job, in device memory: the levels of its two images (img[0] prev, img[1] next; level 0 is the
// caller's device image or its copy in the context's pyramid buffer, the others lie in that buffer), the level sizes (lk_call.hpp), the
// job's first index in the flat point arrays and its point count
struct LkJobDev {
    const uint8_t* img[2][6]; int pitch[2][6];
    int w[6], h[6];
    int nl, pt0, n, has_init;
};
// backward = 0: the forward pass (pts -> out, status, err; aux = the first guesses, read for jobs with has_init).  backward = 1: the
// forward-backward check with the image roles swapped: pts = the forward results, aux = the points they came from; only status is written.
// photo: the context's svo_lk_set_photometric mode when the launch is enqueued (1: the PHOTO instantiations, tests/lk_photo_ref.py)
struct LkTrackArgs {
    const LkJobDev* jobs; int n_jobs, n_pts;
    const float2* pts; const float2* aux;
    float2* out; uint8_t* status; float* err;
    svo_lk_params p; int backward, photo;
};
void launch_lk_pyrdown(const LkJobDev* jobs, int n_jobs, int level, int max_w, int max_h, hipStream_t st);   // max_w x max_h: the largest level `level` of the call
void launch_lk_track(const LkTrackArgs& a, int pixels_per_lane, hipStream_t st);                             // pixels_per_lane: lk_pixels_per_lane(win)
// svo_lk_track_rows (k_lk_track_row in k_lk.hip): the same arguments; the search runs along the row of the guess, the backward pass compares
// x alone.  A point index behind its job's count (gp - pt0 >= n) is nobody's and is left alone: a step's row records leave such gaps
void launch_lk_track_row(const LkTrackArgs& a, int pixels_per_lane, hipStream_t st);
// svo_gftt_detect (k_gftt.hip).  One record per job, in device memory: its image (the caller's device image or its copy in the context's
// buffer), its response map, where its seeds and its results lie in the flat arrays, and the cell grid of the distance rule
// (gftt_call.hpp: cell side >= min_distance, at most 64 x 64 cells)
struct GfttJobDev {
    const uint8_t* img; float* map;
    int pitch, w, h;
    int seed0, n_seeds, pts0, cap;
    int cell, gw, gh;
};
// cand_cap: candidates a job may collect; key_stride: keys per job in `keys` (cand_cap rounded up to a power of two, the sort pads to
// one); items: items_stride = 5 * cand_cap + 2 * seed_cap ints per job, rounded up to a multiple of 4; state: cand_cap bytes per job; info: 4 ints per job (corners written, candidates
// counted, status, the bit pattern of the largest response), zeroed before the first kernel
struct GfttArgs {
    const GfttJobDev* jobs; int n_jobs;
    int cand_cap, key_stride, seed_cap, items_stride;
    unsigned long long* keys; int* items; uint8_t* state;
    const float2* seeds; float2* pts; float* resp; int* info;
    svo_gftt_params p;
};
void launch_gftt_response(const GfttArgs& a, int max_w, int max_h, hipStream_t st);      // max_w x max_h: the largest image of the call
void launch_gftt_candidates(const GfttArgs& a, int max_w, int max_h, hipStream_t st);
void launch_gftt_select(const GfttArgs& a, hipStream_t st);
// the resident KLT front end (k_klt.hip; the buffer plan: klt_call.hpp).  The table of a lane: cap slots, the first n of them live.
struct KltLaneDev {
    int n;                // live tracks
    int next_id;          // the ID the next appended track gets
    int seen_slot;        // LaneState::prev_slot as the front end saw it last: another value after k_begin_frame means the lane shifted
    int pad;
};
enum { KLT_ID = 0, KLT_AGE, KLT_IDX, KLT_PIDX, KLT_META };     // the rows of a lane's meta block
struct KltDev {
    int n_lanes, cap;
    float2* pts[2];       // [half][n_lanes][2 sides][cap]: NaN behind the live count
    int* meta[2];         // [half][n_lanes][KLT_META][cap]: ID, age, index in the list of the last step, index in the previous slot's list (-1: none)
    KltLaneDev* lane;     // [n_lanes]
    float2* out; uint8_t* status; float* err;      // the tracker's results (or svo_debug_klt_select's arrays): [n_lanes][2 sides][cap]
    int* appended;        // what the last k_klt_append launch appended
};
struct KltSelectArgs {
    KltDev t; int half;   // the half that is read; the other one is written
    LaneMask fresh;       // lanes without a last pair: their points stand as they are, status 1
    float max_dy, min_disp, max_disp, kp_size;
    int H;                // rows of the two row tables: min(octave-0 image height, DevCtx.max_h)
};
// the job records of a step, built on the device from the step's geometry: n_lanes pyramid records (img[0] / img[1] = the left / right
// image of the NEW pair) and 2 * n_lanes tracking records (job 2 * lane + side: img[0] the side's last image, img[1] its new one).
// parity: the pyramid buffer the lane's new pair is in; empty: lanes that track nothing (idle, or without a last pair) -- their
// tracking records describe a 0 x 0 image, on which the tracker retires every point before it reads a pixel
// row_jobs (svo_klt_set_stereo(1), else NULL): n_lanes more records, lane l's with img[0] / img[1] = the left / right image of the NEW pair
// and the slots [2 l cap, 2 l cap + cap) -- the left results are its points, the right results lie cap behind them; an idle lane's has
// no point.  The tracking records of the right side then describe a 0 x 0 image: the right list is not tracked through time
struct KltJobArgs {
    LkJobDev* pyr_jobs; LkJobDev* trk_jobs; LkJobDev* row_jobs;
    uint8_t* pyr; long long img_stride;
    int n_lanes, cap, nl;
    int w[6], h[6]; long long off[6];
    LaneMask parity, empty, idle;
};
size_t klt_select_lds_bytes(int H);
// has_init: what every tracking record gets (1 under svo_klt_set_prediction(1): the forward launch then reads its first guesses from aux)
void launch_klt_jobs(const KltJobArgs& a, int has_init, hipStream_t st);
// svo_klt_set_prediction(1) (k_klt_predict in k_gn.hip, beside k_project_points): the first guesses of a step's forward tracking launch.
// For lane l and slot s < cap: guess[(2 * l + side) * cap + s] and used[l * cap + s].  A lane of `tracks` whose record (DevCtx.results, or
// forced_valid / forced_delta under `forced`) is valid with a finite delta moves its live slots by that increment; every other slot gets
// its own points (NaN behind the live count) and used = 0.  only_lane >= 0: that lane alone (grid.y = 1)
struct KltPredictArgs {
    KltDev t; int half;               // the live half, read only
    float2* guess; uint8_t* used;
    LaneMask tracks;                  // the lanes of the step's mask that have a last pair
    float x_max, y_max;               // w - 1 and h - 1 of level 0 of that pair
    int only_lane;
    int forced, forced_valid; double forced_delta[6];
};
void launch_klt_predict(const DevCtx& c, const KltPredictArgs& a, hipStream_t st);
// svo_klt_set_stereo(1), behind the step's tracking launches (k_klt_row_guess in k_klt.hip): the first guesses of the row pass.  For an
// active lane l and slot s < cap: guess[2 l cap + s] = (xl' - (xl - xr), yl') in float32 as written, (xl, xr) the table's old points and
// (xl', yl') the left result; NaN where the left status is not 1 (the row pass then reads nothing for the slot).  A lane of `fresh` has
// no last pair: its left points stand -- they are copied to the results with status 1 -- and are the (xl', yl') of its guesses
struct KltRowGuessArgs {
    KltDev t; int half;               // the live half, read only
    float2* guess;                    // [n_lanes][2][cap], the first cap of a lane used
    LaneMask active, fresh;
};
void launch_klt_row_guess(const KltRowGuessArgs& a, hipStream_t st);
void launch_klt_select(const DevCtx& c, const KltSelectArgs& a, hipStream_t st);
void launch_klt_append(const KltDev& t, int half, int lane, const float2* left, const float2* right, int n, hipStream_t st);
// empties the tables of the lanes of the mask in `half` and starts their IDs over
void launch_klt_clear(const DevCtx& c, const KltDev& t, int half, const LaneMask& lanes, hipStream_t st);
// svo_klt_set_ransac(2): behind k_track_finalize, the tracks whose pair the RANSAC rejected leave the live half `half` (k_klt_prune)
void launch_klt_prune(const DevCtx& c, const KltDev& t, int half, hipStream_t st);
// svo_klt_topup: what its three kernels read.  One detector job and one tracking job (left -> right) per lane; lane l owns slots
// [l * cap, (l + 1) * cap) of the flat arrays.  ginfo: the detector's four ints per job; tinfo: four ints per lane (svo_klt_topup_info)
enum { KLT_TOPUP_OK = 0, KLT_TOPUP_OVERFLOW, KLT_TOPUP_ENOUGH, KLT_TOPUP_NO_PAIR, KLT_TOPUP_NOT_ASKED };
struct KltTopupArgs {
    KltDev t; int half;
    GfttJobDev* gjobs; int* ginfo; int* tinfo;
    float* map; long long map_stride;             // one response map of map_stride floats per lane
    LkJobDev* lk_jobs;
    const uint8_t* pyr; long long img_stride;     // the front end's pyramid buffer (KltJobArgs)
    int nl, w[6], h[6]; long long off[6];         // the geometry of the last step's images
    int cell, gw, gh;                             // gftt_cells of level 0
    int below, target;
    float init_disp, max_dy, min_disp, max_disp;
    LaneMask lanes, has_img, parity;              // the call's mask; the lanes with a last pair; the parity that pair is in
    float2* corners; float2* init; float2* out; uint8_t* status;     // the detector's corners, the first guesses, the tracker's results
};
void launch_klt_topup_jobs(const KltTopupArgs& a, hipStream_t st);
void launch_klt_topup_prepare(const KltTopupArgs& a, hipStream_t st);
// one block per lane, or with only_lane >= 0 that lane alone (svo_debug_klt_topup_append)
void launch_klt_topup_append(const KltTopupArgs& a, int only_lane, hipStream_t st);
