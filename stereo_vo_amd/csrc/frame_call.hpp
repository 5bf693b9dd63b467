// frame_call.hpp -- what one svo_process / svo_process_lanes / svo_gather_windows call IS, decided on the host without a device: who takes
// part (the lane mask), what the flags and parameters in force ask for (FrameCall), whether that is acceptable (check_frame_call) and what
// the call does to the per-lane record of gathered SAD windows (sad_window_step).  Host only, no HIP: svo_api.hip acts on these decisions,
// and tools/frame_call_check.cpp drives them under the sanitizers on the CPU (`make hostcheck`).
#pragma once
#include "../../include/svo_hip.h"
#include <stdint.h>
#include <string>
#include <vector>

// one bit per lane: bit l of w[l >> 6] (kernel argument of k_begin_frame and the hand-over kernels, and DevCtx.idle)
struct LaneMask { unsigned long long w[(SVO_MAX_LANES + 63) / 64]; };
static inline bool lane_in(const LaneMask& m, int l) { return ((m.w[l >> 6] >> (l & 63)) & 1ull) != 0; }
static inline bool lane_any(const LaneMask& m) { return (m.w[0] | m.w[1]) != 0; }
static_assert(SVO_MAX_LANES <= 128, "lane_any reads two mask words");

namespace svo_call {

// The mask of a call: words == NULL stands for every lane, except on the masked entry point (svo_process_lanes), where it is refused.
// active = the lanes below n_lanes whose bit is set, idle = the others below n_lanes.  False with the text in `why` when the mask is
// not acceptable; the caller decides when to report it (svo_process_lanes only after it has armed the post-event disarm).
bool parse_lane_mask(const uint64_t* words, bool masked, int n_lanes, LaneMask& active, LaneMask& idle, std::string& why);

// The facts of one call, from (flags, parameters in force) alone.  Computed once; every later use reads the struct.
struct FrameCall {
    uint32_t flags;
    bool faster;             // dmFASTER: keypoints without descriptors
    bool ahead;              // SVO_FLAG_DETECT_AHEAD: the detect call that leaves lane state alone, or the post call that completes it
    bool continuation;       // continues the frame in flight (its post call, a SVO_FLAG_NO_SHIFT stage): must carry that frame's mask
    bool runs_post;          // the call runs the detector's post-processing: it leaves final lists (and consumes an armed post event)
    bool select_in_post;     // SVO_FLAG_DETECT_SPLIT_AT_SELECT: k_select belongs to the post call, not to the detect call
    bool shifts, repeat;     // runs the prev/cur shift of P:86-100; request_data.repeat
    bool sad_m, sad_t, sad_any;      // stage 3 / stage 4 / either compares 8 x 8 windows
    int nms_mode;            // launch_nms_rowsort after k_select (dmORB): 0 none, 1 standard, 2 adaptive
    int nms_mode_oct;        // launch_nms_rowsort after the x1/2-octave detectors: 0 the NMS ran in the detector, 3 none (raster order)
    int max_sad_match;       // smSAD: size_t(sad_max_distance) (S3:201): 0 = the reference's 200 (S3:48), negative = no threshold
    unsigned max_sad_track;  // ifmSAD: uint32_t MAX_SAD (S4:448): 0 = "~200" (H:297), negative wraps to no threshold
    double minresp;          // S3:189-193: minimum_ORB_response under dmORB, 0 otherwise
    bool faster_anms_on;     // svo_set_faster_adaptive_nms: the context has opted in to the adaptive NMS under dmFASTER
    bool faster_anms;        // ... and this call's parameters select it: dmFASTER + non_maximal_suppression + nmsmAdaptive
};
FrameCall make_frame_call(uint32_t flags, const svo_params& p, bool faster_adaptive_nms = false);

// The refusals a call meets before anything is enqueued or noted, in their order: selectors, variants outside the hot path, dmFASTER's
// rules, the detect-ahead flag combinations, then the one-mask-per-frame rule (frame_active: the mask of the frame in flight, NULL when
// there is none).  SVO_OK, or the status with the text (empty where the status says it all) in `why`.
int check_frame_call(const FrameCall& call, const svo_params& p, const LaneMask& active, const LaneMask* frame_active, std::string& why);

// Which frames of a lane have their windows, per lane (svo_ctx: sad_cur, sad_prev, sad_drop).  "true" also stands for "no such frame yet".
struct SadWindows { std::vector<uint8_t> cur, prev, drop; };
// What the call does to that record.  bad_lane < 0: `next` is the record after the call and drop_prev the lanes whose shift forgets their
// previous frame.  Otherwise the call is refused (SVO_ERR_STATE) for that lane with `why`, and `next` is the record as it was, plus -- when
// it is the PREVIOUS frame that lacks windows and the call would have shifted -- sad_drop on every active lane that cannot be tracked
// from with SAD: its next frame starts the lane's track afresh.  Either way the caller commits `next`.
struct SadStep { SadWindows next; LaneMask drop_prev; bool any_drop; int bad_lane; std::string why; };
SadStep sad_window_step(const SadWindows& now, const LaneMask& idle, const FrameCall& call);

// svo_set_dyn_fast_threshold: target_feats_per_pixel must be finite and >= 0; SVO_ERR_ARG with the text otherwise
int check_dyn_fast_target(double target, std::string& why);
// ... and whether a svo_set_params re-initialises the lanes' thresholds: when the number of octaves m_threshold is sized by changes
// (S2:522-523: m_threshold.size() != nOctaves), and for no other field -- initial_FAST_threshold included
bool dyn_fast_octaves_changed(const svo_params& before, const svo_params& after);

// svo_adaptive_nms: the argument rules that need no device.  kps must be n keypoints in strictly ascending raster order with integer
// coordinates inside img_w x img_h and no NaN response, img_w * img_h < 2^24, n <= cand_cap (the context's level-0 candidate capacity),
// min(num_out_points, n) <= max_kps (the selection sorts that many keys in LDS).  SVO_OK, or SVO_ERR_ARG with the text.
int check_adaptive_nms_args(const svo_keypoint* kps, int n, int num_out_points, int img_w, int img_h, const int32_t* out_order, int cap,
                            int cand_cap, int max_kps, std::string& why);

}
