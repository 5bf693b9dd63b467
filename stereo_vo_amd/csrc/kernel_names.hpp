// kernel_names.hpp -- the names svo_kernel_times lists: one id per timed name, one table row per id (kernel_names.cpp), and the rule
// that says which of them a context lists.  Host only, no HIP: svo_ctx.hpp includes it for the ids, svo_api.hip lists and selects with
// it, and tools/kernel_names_check.cpp holds the rule and the lookup to the contract of svo_hip.h under the sanitizers on the CPU
// (`make hostcheck`).  A new timed name is one more id here and one more row there, nothing else.
#pragma once

// the ids, in the order of the listing.  A span is counted under its id; bit id of svo_ctx::kt_mask selects it (svo_kernel_times_select)
enum KernelTimeId : int {
    KT_BEGIN, KT_RESIZE, KT_FAST, KT_SELECT, KT_DESCRIBE, KT_NMS, KT_HAM_LR, KT_LR_FILTER, KT_HAM_TRK, KT_TRK_FILTER,
    KT_RANSAC_HYP, KT_RANSAC_CNT, KT_TRK_FINAL, KT_GN, KT_RANSAC_HYP1, KT_RANSAC_CNT1, KT_RANSAC_HYP2, KT_RANSAC_CNT2,
    KT_SAD_PATCH, KT_LR_SAD, KT_TRK_SAD,
    // the instantiations that only a 16384-entry context launches, under names of their own (a context with max_kps <= 8192 never counts a call here)
    KT_SELECT_8192, KT_NMS_16, KT_HAM_LR_WIDE, KT_HAM_TRK_WIDE, KT_TRK_FILTER_64,
    // svo_export_frame / svo_import_frame: the kernels of a context that carries no SAD windows, then those of one that does
    KT_EXPORT, KT_IMPORT, KT_EXPORT_WIN, KT_IMPORT_WIN,
    KT_FASTER, KT_FASTER_NMS,          // dmFASTER (only a context that selects it counts a call here)
    KT_GATHER_WIN,                     // svo_gather_windows (only a caller of that entry point counts a call here)
    KT_POSE_COV, KT_LANDMARKS,         // svo_set_pose_covariance, svo_set_landmarks
    KT_GFTT_RESPONSE, KT_GFTT_CANDIDATES, KT_GFTT_SELECT,      // svo_gftt_detect and the detector of a top-up
    KT_LK_PYRDOWN, KT_LK_TRACK,        // svo_lk_track, the pyramids and tracking launches of svo_klt_step and of a top-up
    KT_KLT_SELECT,                     // the selection of svo_klt_step
    KT_KLT_TOPUP,                      // the three kernels of k_klt.hip around the detector and the tracker of svo_klt_topup
    KT_RANSAC_FEED,                    // svo_ransac_tracked, or a step under svo_klt_set_ransac (the RANSAC launches count under their names of a frame)
    KT_KLT_PRUNE,                      // a step under svo_klt_set_ransac(2)
    KT_KLT_PREDICT,                    // a step under svo_klt_set_prediction(1), svo_klt_predicted, svo_debug_klt_predict
    KT_LK_TRACK_ROW,                   // svo_lk_track_rows, or a step under svo_klt_set_stereo(1)
    KT_COUNT
};
static_assert(KT_COUNT <= 64, "kt_mask is one 64-bit word, and Context.kernel_times reads 64 names");

// what decides whether a name is listed: KG_ALWAYS always, KG_POSE_COV and KG_LANDMARKS while their switch is on, every other group once
// the context has done what the group stands for (svo_ctx::kt_seen holds one bit per group, set where that happens)
enum KernelTimeGroup : int {
    KG_ALWAYS, KG_POSE_COV, KG_LANDMARKS, KG_GFTT, KG_LK, KG_KLT_SELECT, KG_KLT_TOPUP, KG_RANSAC_FEED, KG_KLT_PRUNE, KG_KLT_PREDICT, KG_LK_TRACK_ROW,
    KG_COUNT
};

struct KernelName { int id; const char* name; int group; };
extern const KernelName kernel_names[KT_COUNT];            // in listing order; row i has id i

// the ids a context lists, in order, into ids[KT_COUNT]; returns how many.  seen: the groups of the calls the context has made
int kernel_time_listing(unsigned seen, bool pose_cov, bool landmarks, int* ids);
// the id of a name, -1 when there is no such name
int kernel_time_id(const char* name);
