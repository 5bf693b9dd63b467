// klt_call.hpp -- what the calls of the resident KLT front end ARE, decided on the host without a device: the parameter ranges of
// svo_klt_params, every refusal of svo_klt_enable / svo_klt_step / svo_klt_add_points / svo_klt_get_tracks / svo_klt_reset /
// svo_debug_klt_select in the order they are made, and the buffer plan (pyramid ping-pong, table ping-pong, job records); the same for
// the top-up, the RANSAC gate and the pose prediction.
// Host only, no HIP: svo_api.hip acts on these decisions, k_klt.hip reads the buffers they size, and tools/klt_check.cpp drives them
// under the sanitizers on the CPU (`make hostcheck`).
#pragma once
#include "../../include/svo_hip.h"
#include "frame_call.hpp"
#include "lk_call.hpp"
#include <stdint.h>
#include <string>

namespace svo_klt {

// what the context can take (svo_config) and what it is doing
struct Caps { int n_lanes, max_kps, max_w, max_h; };
struct State {
    bool enabled;         // svo_klt_enable has succeeded
    bool params_set;      // svo_set_params has been called
    bool capturing;       // the context's stream is capturing a graph
    bool frame_parallel;  // the context is a member of a frame-parallel stream (svo_batch.h): its frames travel between contexts, a table would not
};

// NULL parameters of svo_klt_enable: the defaults with cap = min(1024, max_kps)
svo_klt_params klt_resolve_params(const svo_klt_params* p, int max_kps);
// the ranges of svo_klt_params: SVO_OK, SVO_ERR_ARG, or SVO_ERR_CAPACITY (cap > max_kps), with the numbers in `why`
int check_klt_params(const svo_klt_params& p, const Caps& caps, std::string& why);
// svo_klt_enable: the parameters, then -- for a context that is enabled already -- other parameters than those in force while a table
// holds tracks (SVO_ERR_STATE); a member of a frame-parallel stream is refused first (SVO_ERR_STATE).  realloc: the call must (re)make the buffers
int check_klt_enable(const svo_klt_params& p, const Caps& caps, bool enabled, const svo_klt_params& in_force, bool tables_empty, bool frame_parallel, bool& realloc, std::string& why);
// what every other entry point asks first: enabled, parameters set, not inside a capture
int check_klt_ready(const State& s, const char* entry, std::string& why);
// svo_klt_step, in order: ready, flags, frames, the mask, then the images of the active lanes (NULL data, one size, the 64 x 64 floor,
// max_w x max_h, strides, device spans).  active / idle: the parsed mask.  w, h: the size of the call's images
int check_klt_step(const svo_frame* frames, uint32_t flags, const uint64_t* lanes, const Caps& caps, const State& s,
                   LaneMask& active, LaneMask& idle, int& w, int& h, std::string& why);
// svo_klt_add_points / svo_klt_get_tracks / svo_debug_klt_select: ready, the lane, the arrays and the count
int check_klt_lane_call(const State& s, const char* entry, int lane, int n, bool arrays_ok, const Caps& caps, std::string& why);


// ---- the RANSAC gate (svo_ransac_tracked / svo_klt_set_ransac; tools/klt_ransac_check.cpp drives these) ----
enum { KLT_RANSAC_OFF = 0, KLT_RANSAC_FILTER = 1, KLT_RANSAC_PRUNE = 2 };
// svo_ransac_tracked, in order: no svo_set_params yet, no geometry yet, a capturing stream (SVO_ERR_STATE), then the mask (NULL = all
// lanes; a bit at or above n_lanes: SVO_ERR_ARG).  The front end need not be enabled.  active / idle: the parsed mask
int check_ransac_tracked(bool params_set, bool geom_ready, bool capturing, const uint64_t* lanes, int n_lanes, LaneMask& active, LaneMask& idle, std::string& why);
// svo_klt_set_ransac: the front end enabled and no capture (SVO_ERR_STATE), then the mode, 0 .. 2 (SVO_ERR_ARG)
int check_klt_set_ransac(const State& s, int mode, std::string& why);

// ---- the pose prediction (svo_klt_set_prediction / svo_klt_get_prediction / svo_klt_predicted / svo_debug_klt_predict;
//      tools/klt_predict_check.cpp drives these) ----
enum { KLT_PREDICT_OFF = 0, KLT_PREDICT_POSE = 1 };
// svo_klt_set_prediction: the front end enabled and no capture (SVO_ERR_STATE), then the mode, 0 .. 1 (SVO_ERR_ARG).  alloc: the call
// must make the guess buffer (mode 1 and no buffer yet)
int check_klt_set_prediction(const State& s, int mode, bool have_buffer, bool& alloc, std::string& why);
// svo_klt_predicted / svo_debug_klt_predict, in order: ready (check_klt_ready), the prediction on (SVO_ERR_STATE), then the lane, a count
// >= 0 and the arrays (SVO_ERR_ARG; delta_ok: svo_debug_klt_predict's delta6 is there)
int check_klt_predict_call(const State& s, const char* entry, int mode, int lane, int cap, bool delta_ok, const Caps& caps, std::string& why);
// the one buffer of the prediction: the guesses [n_lanes][2 sides][cap] float2, laid out as the tracker's results are (job 2 * lane + side
// owns slots [job * cap, (job + 1) * cap)), and a byte per slot [n_lanes][cap]
struct PredictPlan {
    long long n_guess;              // float2: n_lanes * 2 * cap
    long long n_used;               // bytes: n_lanes * cap
    int blocks_x;                   // k_klt_predict's grid: (ceil(cap / 256), n_lanes)
};
PredictPlan plan_predict(const svo_klt_params& p, const Caps& caps);

// ---- the stereo re-association (svo_klt_set_stereo / svo_klt_get_stereo; tools/klt_stereo_check.cpp drives these) ----
// 0: the right list is tracked through time; 1: the right partner is found along the row in the new pair (svo_lk_track_rows' kernel)
enum { KLT_STEREO_TEMPORAL = 0, KLT_STEREO_ROW = 1 };
// svo_klt_set_stereo: the front end enabled and no capture (SVO_ERR_STATE), then the mode, 0 .. 1 (SVO_ERR_ARG).  alloc: the call must
// make the buffers of mode 1 (mode 1 and none yet)
int check_klt_set_stereo(const State& s, int mode, bool have_buffers, bool& alloc, std::string& why);
// the buffers of mode 1: one row record per lane, and the first guesses of the row pass laid out as the tracker's results are (lane l's
// at [2 l cap, 2 l cap + cap): the row pass indexes its points, guesses and -- cap behind -- results with one number)
struct StereoPlan {
    int n_jobs;                     // LkJobDev: n_lanes
    long long n_guess;              // float2: n_lanes * 2 * cap
    long long n_pts;                // the point indices a row launch covers: (2 * n_lanes - 1) * cap
};
StereoPlan plan_stereo(const svo_klt_params& p, const Caps& caps);

// the buffers of an enabled context, sized for max_w x max_h images:
//   pyramids  [2 parities][n_lanes][2 sides] blocks of img_stride bytes, the levels of one image tightly packed (lk_geometry with
//              level 0).  A lane's new pair goes to the parity its last pair did NOT go to: the other parity still holds frame t - 1
//   table      [2 halves] x ( points [n_lanes][2 sides][cap] float2 + meta [n_lanes][4][cap] int32: id, age, index in the list of the
//              last step, index in the lane's previous-slot list ).  k_klt_select reads one half and writes the other
//   results    the tracker's out / status / err, [n_lanes][2 sides][cap]: job 2 * lane + side owns slots [job * cap, (job + 1) * cap)
//   jobs       n_lanes pyramid records (left and right image of the NEW pair) and 2 * n_lanes tracking records
struct Plan {
    long long img_stride, pyr_bytes;
    long long n_slots;              // n_lanes * 2 * cap
    long long meta_ints;            // n_lanes * 4 * cap
    int n_pyr_jobs, n_trk_jobs;
    long long select_lds_bytes;     // dynamic LDS of k_klt_select: three row tables of max_h + 1 ints
};
Plan plan_klt(const svo_klt_params& p, const Caps& caps);
// the geometry of a step's images (every lane has the same size)
svo_lk::Geometry klt_geometry(const svo_klt_params& p, int w, int h);

// ---- the resident top-up (svo_klt_topup_enable / svo_klt_topup / svo_klt_topup_info / svo_debug_klt_topup_append) ----
// what the top-up asks of the context besides Caps: the front end's cap and svo_config.max_cand
struct TopupCaps { int cap, max_cand; };
// the defaults for a front end of `cap` tracks per lane: the detector's defaults, below = (cap + 1) / 2, target = cap, init_disp = 0
svo_klt_topup_params topup_default_params(int cap);
// the ranges of svo_klt_topup_params: the gftt ranges (max_corners against max_kps is a capacity), below and target in 1 .. cap, a
// finite init_disp (SVO_ERR_ARG), a context whose max_cand exceeds 2^24 (SVO_ERR_CAPACITY, as svo_gftt_detect has it)
int check_topup_params(const svo_klt_topup_params& p, const Caps& caps, const TopupCaps& tc, std::string& why);
// svo_klt_topup_enable, in order: the front end enabled and no capture (SVO_ERR_STATE), the parameters, then -- for a top-up that is
// enabled already -- other parameters than those in force after a top-up has run while a table holds tracks (SVO_ERR_STATE).
// realloc: the call must make the buffers; adopt: only the parameters change
int check_topup_enable(const svo_klt_topup_params& p, const Caps& caps, const TopupCaps& tc, const State& s, bool topup_enabled,
                       const svo_klt_topup_params& in_force, bool has_run, bool tables_empty, bool& realloc, bool& adopt, std::string& why);
// what svo_klt_topup, svo_klt_topup_info and svo_debug_klt_topup_append ask first: both enabled, not inside a capture
int check_topup_ready(const State& s, bool topup_enabled, const char* entry, std::string& why);
// svo_klt_topup: ready, then the mask (NULL = all lanes)
int check_topup_call(const State& s, bool topup_enabled, const uint64_t* lanes, const Caps& caps, LaneMask& active, std::string& why);
// svo_klt_topup_info / svo_debug_klt_topup_append: ready, the lane, the arrays, 0 <= n <= cap
int check_topup_lane_call(const State& s, bool topup_enabled, const char* entry, int lane, int n, bool arrays_ok, const Caps& caps, const TopupCaps& tc, std::string& why);

// the buffers of an enabled top-up, its own (svo_gftt_detect's and svo_lk_track's are not touched):
//   maps       n_lanes response maps of map_stride floats (max_w x max_h rounded up to 64 floats): the large one
//   detector   per lane cand_cap candidates in a row of key_stride 64-bit keys, items_stride ints of cell lists (seed capacity = cap),
//              cand_cap state bytes, 4 counters
//   points     corners, responses, first guesses, tracked points, status, error: n_lanes * cap each
//   jobs       n_lanes detector records and n_lanes tracking records; 4 ints of svo_klt_topup_info per lane
struct TopupPlan {
    long long map_stride, map_floats;
    int cand_cap, key_stride; long long items_stride;
    long long n_keys, n_items, n_state;
    long long n_pts;
    int n_jobs;
};
TopupPlan plan_topup(const svo_klt_params& kp, const Caps& caps, const TopupCaps& tc);

}
