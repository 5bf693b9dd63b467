// kernel_names.cpp -- the one table of timed names and the listing rule (kernel_names.hpp).
#include "kernel_names.hpp"
#include <string.h>

const KernelName kernel_names[KT_COUNT] = {
    { KT_BEGIN, "begin_frame", KG_ALWAYS }, { KT_RESIZE, "resize", KG_ALWAYS }, { KT_FAST, "fast", KG_ALWAYS }, { KT_SELECT, "select", KG_ALWAYS }, { KT_DESCRIBE, "describe", KG_ALWAYS },
    { KT_NMS, "nms_rowsort", KG_ALWAYS }, { KT_HAM_LR, "hamming_lr", KG_ALWAYS }, { KT_LR_FILTER, "match_lr_filter", KG_ALWAYS }, { KT_HAM_TRK, "hamming_track", KG_ALWAYS }, { KT_TRK_FILTER, "track_filter", KG_ALWAYS },
    { KT_RANSAC_HYP, "ransac_hyp", KG_ALWAYS }, { KT_RANSAC_CNT, "ransac_count", KG_ALWAYS }, { KT_TRK_FINAL, "track_finalize", KG_ALWAYS }, { KT_GN, "gauss_newton", KG_ALWAYS },
    { KT_RANSAC_HYP1, "ransac_hyp_1", KG_ALWAYS }, { KT_RANSAC_CNT1, "ransac_count_1", KG_ALWAYS }, { KT_RANSAC_HYP2, "ransac_hyp_2", KG_ALWAYS }, { KT_RANSAC_CNT2, "ransac_count_2", KG_ALWAYS },
    { KT_SAD_PATCH, "sad_patch", KG_ALWAYS }, { KT_LR_SAD, "match_lr_sad", KG_ALWAYS }, { KT_TRK_SAD, "track_sad", KG_ALWAYS },
    { KT_SELECT_8192, "select_8192", KG_ALWAYS }, { KT_NMS_16, "nms_rowsort_16", KG_ALWAYS }, { KT_HAM_LR_WIDE, "hamming_lr_wide", KG_ALWAYS }, { KT_HAM_TRK_WIDE, "hamming_track_wide", KG_ALWAYS }, { KT_TRK_FILTER_64, "track_filter_64", KG_ALWAYS },
    { KT_EXPORT, "export_frame", KG_ALWAYS }, { KT_IMPORT, "import_frame", KG_ALWAYS }, { KT_EXPORT_WIN, "export_frame_win", KG_ALWAYS }, { KT_IMPORT_WIN, "import_frame_win", KG_ALWAYS },
    { KT_FASTER, "faster", KG_ALWAYS }, { KT_FASTER_NMS, "faster_nms", KG_ALWAYS }, { KT_GATHER_WIN, "gather_windows", KG_ALWAYS },
    { KT_POSE_COV, "pose_covariance", KG_POSE_COV }, { KT_LANDMARKS, "landmarks", KG_LANDMARKS },
    { KT_GFTT_RESPONSE, "gftt_response", KG_GFTT }, { KT_GFTT_CANDIDATES, "gftt_candidates", KG_GFTT }, { KT_GFTT_SELECT, "gftt_select", KG_GFTT },
    { KT_LK_PYRDOWN, "lk_pyrdown", KG_LK }, { KT_LK_TRACK, "lk_track", KG_LK },
    { KT_KLT_SELECT, "klt_select", KG_KLT_SELECT }, { KT_KLT_TOPUP, "klt_topup", KG_KLT_TOPUP },
    { KT_RANSAC_FEED, "ransac_feed", KG_RANSAC_FEED }, { KT_KLT_PRUNE, "klt_prune", KG_KLT_PRUNE }, { KT_KLT_PREDICT, "klt_predict", KG_KLT_PREDICT }, { KT_LK_TRACK_ROW, "lk_track_row", KG_LK_TRACK_ROW },
};

// the groups that list a group's names.  Landmarks list "pose_covariance" with their own name; a top-up launches the detector, the
// tracker and the selection, a selection the tracker: their names come with it
#define G(g) (1u << KG_##g)
static const unsigned listed_by[KG_COUNT] = { G(ALWAYS), G(POSE_COV) | G(LANDMARKS), G(LANDMARKS), G(GFTT) | G(KLT_TOPUP), G(LK) | G(KLT_SELECT) | G(KLT_TOPUP),
                                              G(KLT_SELECT) | G(KLT_TOPUP), G(KLT_TOPUP), G(RANSAC_FEED), G(KLT_PRUNE), G(KLT_PREDICT), G(LK_TRACK_ROW) };

int kernel_time_listing(unsigned seen, bool pose_cov, bool landmarks, int* ids)
{
    // the switches count while they are on, whatever the context has seen
    const unsigned on = (seen & ~(G(POSE_COV) | G(LANDMARKS))) | G(ALWAYS) | (pose_cov ? G(POSE_COV) : 0u) | (landmarks ? G(LANDMARKS) : 0u);
    int n = 0;
    for (const KernelName& k : kernel_names) if (on & listed_by[k.group]) ids[n++] = k.id;
    return n;
}

int kernel_time_id(const char* name)
{
    for (const KernelName& k : kernel_names) if (!strcmp(name, k.name)) return k.id;
    return -1;
}
