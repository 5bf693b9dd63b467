// kernel_names_check.cpp -- the table of timed names and the listing rule (stereo_vo_amd/csrc/kernel_names.cpp), under the address and
// undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc hostcheck && tools/kernel_names_check
//
// The expected listing below is written from the rules include/svo_hip.h states for svo_kernel_times, name by name, not taken from a
// run of kernel_time_listing.  Exit status 0 and a last line "ok" when everything held.
#include "kernel_names.hpp"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s   [seen %#x, pose_cov %d, landmarks %d]\n", __FILE__, __LINE__, #cond, cur_seen, cur_cov, cur_lmk); failures++; } } while (0)
static unsigned cur_seen = 0;
static int cur_cov = 0, cur_lmk = 0;

// the names a context always lists
static const char* const ALWAYS[] = { "begin_frame", "resize", "fast", "select", "describe", "nms_rowsort", "hamming_lr", "match_lr_filter", "hamming_track",
    "track_filter", "ransac_hyp", "ransac_count", "track_finalize", "gauss_newton", "ransac_hyp_1", "ransac_count_1", "ransac_hyp_2", "ransac_count_2",
    "sad_patch", "match_lr_sad", "track_sad", "select_8192", "nms_rowsort_16", "hamming_lr_wide", "hamming_track_wide", "track_filter_64",
    "export_frame", "import_frame", "export_frame_win", "import_frame_win", "faster", "faster_nms", "gather_windows" };

// the rules, one line each
static std::vector<std::string> expected(unsigned seen, bool pose_cov, bool landmarks)
{
    auto has = [&](int g) { return (seen >> g & 1u) != 0; };
    std::vector<std::string> out(ALWAYS, ALWAYS + sizeof(ALWAYS) / sizeof(ALWAYS[0]));
    if (pose_cov || landmarks) out.push_back("pose_covariance");
    if (landmarks) out.push_back("landmarks");
    if (has(KG_GFTT) || has(KG_KLT_TOPUP)) { out.push_back("gftt_response"); out.push_back("gftt_candidates"); out.push_back("gftt_select"); }
    if (has(KG_LK) || has(KG_KLT_SELECT) || has(KG_KLT_TOPUP)) { out.push_back("lk_pyrdown"); out.push_back("lk_track"); }
    if (has(KG_KLT_SELECT) || has(KG_KLT_TOPUP)) out.push_back("klt_select");
    if (has(KG_KLT_TOPUP)) out.push_back("klt_topup");
    if (has(KG_RANSAC_FEED)) out.push_back("ransac_feed");
    if (has(KG_KLT_PRUNE)) out.push_back("klt_prune");
    if (has(KG_KLT_PREDICT)) out.push_back("klt_predict");
    if (has(KG_LK_TRACK_ROW)) out.push_back("lk_track_row");
    return out;
}

static void check_table()
{
    CHECK(sizeof(ALWAYS) / sizeof(ALWAYS[0]) == 33 && KT_COUNT == 46 && KG_COUNT == 11);
    for (int i = 0; i < KT_COUNT; i++) {
        CHECK(kernel_names[i].id == i && kernel_names[i].name && kernel_names[i].name[0]);
        CHECK(kernel_names[i].group >= 0 && kernel_names[i].group < KG_COUNT);
        CHECK(i == 0 || kernel_names[i].group >= kernel_names[i - 1].group);          // the groups lie one behind the other
        CHECK(kernel_time_id(kernel_names[i].name) == i);                              // (which also says that no name occurs twice)
    }
    CHECK(kernel_time_id("no_such_kernel") == -1 && kernel_time_id("") == -1 && kernel_time_id("lk_trac") == -1 && kernel_time_id("lk_track_") == -1);
}

static void check_listing()
{
    // every set of groups, the bits of the two switches and of KG_ALWAYS included (they must not matter), with every setting of the switches
    for (unsigned seen = 0; seen < (1u << KG_COUNT); seen++) {
        for (int sw = 0; sw < 4; sw++) {
            const bool cov = sw & 1, lmk = (sw & 2) != 0;
            cur_seen = seen; cur_cov = cov; cur_lmk = lmk;
            int ids[KT_COUNT];
            const int n = kernel_time_listing(seen, cov, lmk, ids);
            const std::vector<std::string> want = expected(seen, cov, lmk);
            CHECK(n == (int)want.size() && n <= KT_COUNT);
            for (int i = 0; i < n && i < (int)want.size(); i++) {
                CHECK(ids[i] >= 0 && ids[i] < KT_COUNT);
                if (ids[i] >= 0 && ids[i] < KT_COUNT) CHECK(want[(size_t)i] == kernel_names[ids[i]].name);
            }
        }
    }
}

int main()
{
    check_table();
    check_listing();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
