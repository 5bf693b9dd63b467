// frame_call.cpp -- the per-call decisions of svo_api.hip that need no device (frame_call.hpp).  Host only, built with g++.
#include "frame_call.hpp"
#include "faster_dyn.hpp"
#include <float.h>
#include <limits.h>
#include <stdio.h>
#include <string.h>

namespace svo_call {

bool parse_lane_mask(const uint64_t* words, bool masked, int n_lanes, LaneMask& active, LaneMask& idle, std::string& why)
{
    bool ok = true;
    why.clear();
    if (masked && !words) { why = "active == NULL"; ok = false; }
    for (int wd = 0; wd < 2; wd++) {
        const int n = n_lanes - wd * 64 < 0 ? 0 : (n_lanes - wd * 64 > 64 ? 64 : n_lanes - wd * 64);
        const unsigned long long all = n == 64 ? ~0ull : ((1ull << n) - 1ull), a = words ? (unsigned long long)words[wd] : all;
        if ((a & ~all) && ok) {
            char msg[160];
            snprintf(msg, sizeof(msg), "active[%d] = %016llx selects a lane at or above n_lanes = %d", wd, a, n_lanes);
            why = msg; ok = false;
        }
        active.w[wd] = a & all; idle.w[wd] = all & ~a;
    }
    return ok;
}

FrameCall make_frame_call(uint32_t flags, const svo_params& p, bool faster_adaptive_nms)
{
    FrameCall c;
    c.flags = flags;
    c.faster = p.detect_method == SVO_DM_FASTER;
    c.ahead = (flags & SVO_FLAG_DETECT_AHEAD) != 0;
    c.continuation = !(flags & SVO_RUN_DETECT) && (flags & (SVO_FLAG_NO_SHIFT | SVO_RUN_DETECT_POST));
    c.runs_post = (flags & SVO_RUN_DETECT_POST) || ((flags & SVO_RUN_DETECT) && !(flags & SVO_FLAG_DETECT_NO_POST));
    c.select_in_post = (flags & SVO_FLAG_DETECT_SPLIT_AT_SELECT) && (!(flags & SVO_RUN_DETECT) || (flags & SVO_FLAG_DETECT_NO_POST));
    c.shifts = !(flags & SVO_FLAG_NO_SHIFT) && !(c.ahead && (flags & SVO_RUN_DETECT));
    c.repeat = (flags & SVO_FLAG_REPEAT) != 0;
    c.sad_m = p.match_method == SVO_SM_SAD; c.sad_t = p.ifm_method == SVO_IFM_SAD; c.sad_any = c.sad_m || c.sad_t;
    c.nms_mode = p.non_maximal_suppression ? (p.nmsMethod == SVO_NMS_ADAPTIVE ? 2 : 1) : 0;
    c.nms_mode_oct = p.non_maximal_suppression ? 0 : 3;
    c.max_sad_match = p.sad_max_distance == 0 ? 200 : (p.sad_max_distance < 0 ? INT32_MAX : p.sad_max_distance);
    c.max_sad_track = p.ifm_sad_max_distance == 0 ? 200u : (unsigned)p.ifm_sad_max_distance;
    c.minresp = p.detect_method == SVO_DM_ORB ? p.minimum_ORB_response : 0.0;
    c.faster_anms_on = faster_adaptive_nms;
    c.faster_anms = faster_adaptive_nms && c.faster && c.nms_mode == 2;
    return c;
}

int check_frame_call(const FrameCall& call, const svo_params& p, const LaneMask& active, const LaneMask* frame_active, std::string& why)
{
    const uint32_t flags = call.flags;
    why.clear();
    // P:54-76: invalid selectors are hard errors; the variants outside the hot path are refused explicitly
    if (p.detect_method < 0 || p.detect_method > 3 || p.match_method < 0 || p.match_method > 2 || p.ifm_method < 0 || p.ifm_method > 3) return SVO_ERR_ARG;
    if ((flags & SVO_RUN_DETECT) && p.detect_method == SVO_DM_KLT) return SVO_ERR_UNSUPPORTED;                                         // dmKLT: out of scope
    if ((flags & SVO_RUN_TRACK) && p.ifm_method == SVO_IFM_OPTICAL_FLOW) return SVO_ERR_UNSUPPORTED;                                   // optical flow: out of scope
    if (p.non_maximal_suppression && p.nmsMethod != SVO_NMS_STANDARD && p.nmsMethod != SVO_NMS_ADAPTIVE) return SVO_ERR_ARG;          // S2:608
    if (p.min_distance < 2) return SVO_ERR_ARG;            // cell size 0 divides by zero in the reference (S2:331-332)
    // dmFASTER (S2:519-576) produces keypoints without descriptors: only the SAD stages can consume its lists
    if (call.faster) {
        if ((flags & SVO_RUN_MATCH) && p.match_method != SVO_SM_SAD) { why = "dmFASTER computes no descriptors: stage 3 needs match_method = smSAD"; return SVO_ERR_STATE; }
        if ((flags & SVO_RUN_TRACK) && p.ifm_method != SVO_IFM_SAD) { why = "dmFASTER computes no descriptors: stage 4 needs ifm_method = ifmSAD"; return SVO_ERR_STATE; }
        // ... unless the context has asked for it (svo_set_faster_adaptive_nms): the refusal and its text are what they were while it has not
        if (!call.faster_anms_on && (flags & (SVO_RUN_DETECT | SVO_RUN_DETECT_POST)) && p.non_maximal_suppression && p.nmsMethod == SVO_NMS_ADAPTIVE) {
            why = "the adaptive NMS is not built for dmFASTER: use nmsMethod = nmsmStandard"; return SVO_ERR_UNSUPPORTED;
        }
        if ((flags & SVO_RUN_DETECT) && (p.initial_FAST_threshold < 0 || p.initial_FAST_threshold > 255)) {
            char msg[128]; snprintf(msg, sizeof(msg), "initial_FAST_threshold %d: dmFASTER takes 0 .. 255", p.initial_FAST_threshold);
            why = msg; return SVO_ERR_ARG;
        }
    }
    // SVO_FLAG_DETECT_AHEAD: a detect call that leaves lane state and records alone (it may overlap stages 3-5 of the frame before),
    // or the post call that completes it (and therefore runs the shift itself)
    if (call.ahead) {
        if (flags & SVO_RUN_DETECT) { if (!(flags & SVO_FLAG_DETECT_NO_POST) || (flags & (SVO_RUN_MATCH | SVO_RUN_TRACK | SVO_RUN_OPTIMIZE | SVO_RUN_DETECT_POST))) return SVO_ERR_ARG; }
        else if (!(flags & SVO_RUN_DETECT_POST) || (flags & SVO_FLAG_NO_SHIFT)) return SVO_ERR_ARG;
    }
    // the calls of one frame carry one mask: what a frame's first call (any call that is not a continuation) ran with is what its
    // post call and its SVO_FLAG_NO_SHIFT stages must run with
    if (call.continuation && frame_active && memcmp(&active, frame_active, sizeof(active)) != 0) {
        char msg[256];
        snprintf(msg, sizeof(msg), "active lanes %016llx:%016llx, but the frame in flight began with %016llx:%016llx: every call of a frame carries the same mask",
                 active.w[1], active.w[0], frame_active->w[1], frame_active->w[0]);
        why = msg; return SVO_ERR_STATE;
    }
    return SVO_OK;
}

SadStep sad_window_step(const SadWindows& now, const LaneMask& idle, const FrameCall& call)
{
    const uint32_t flags = call.flags;
    const int n_lanes = (int)now.cur.size();
    SadStep r;
    r.next = now; memset(&r.drop_prev, 0, sizeof(r.drop_prev)); r.any_drop = false; r.bad_lane = -1;
    std::vector<uint8_t>& cur = r.next.cur, & prev = r.next.prev, & drop = r.next.drop;
    bool bad_prev = false;
    for (int l = 0; l < n_lanes; l++) {
        if (lane_in(idle, l)) continue;                  // (sad_drop of an idle lane waits for the lane's next active frame)
        if (call.shifts) {
            if (drop[l]) { r.drop_prev.w[l >> 6] |= 1ull << (l & 63); r.any_drop = true; prev[l] = 1; drop[l] = 0; }
            else if (!call.repeat) prev[l] = prev[l] && cur[l];
            cur[l] = 0;                                  // an empty list until the post-processing has run
        }
        if (call.runs_post) cur[l] = call.sad_any ? 1 : 0;
        if (r.bad_lane < 0 && (flags & SVO_RUN_MATCH) && call.sad_m && !cur[l]) r.bad_lane = l;
        if (r.bad_lane < 0 && (flags & SVO_RUN_TRACK) && call.sad_t && !(cur[l] && prev[l])) { r.bad_lane = l; bad_prev = cur[l] != 0; }
    }
    if (r.bad_lane < 0) return r;
    const bool afresh = bad_prev && call.shifts && !call.repeat;
    char msg[320];
    snprintf(msg, sizeof(msg), "lane %d: %s selects SAD but the 8 x 8 windows of its %s frame were never gathered (features put, loaded or imported, "
             "or detected while no SAD method was selected)%s", r.bad_lane, bad_prev ? "ifm_method" : (((flags & SVO_RUN_MATCH) && call.sad_m) ? "match_method" : "ifm_method"),
             bad_prev ? "previous" : "current", afresh ? ": this frame is refused, the next one starts the lane's track afresh" : "");
    r.why = msg;
    // refused: nothing of the record moves, except that the frame before cannot be tracked from with SAD and its image is gone -- the
    // next frame of such a lane forgets it
    r.next = now; memset(&r.drop_prev, 0, sizeof(r.drop_prev)); r.any_drop = false;
    if (afresh) for (int l = 0; l < n_lanes; l++) if (!lane_in(idle, l) && (!now.prev[l] || !now.cur[l])) r.next.drop[l] = 1;
    return r;
}

int check_dyn_fast_target(double target, std::string& why)
{
    why.clear();
    if (target >= 0.0 && target <= DBL_MAX) return SVO_OK;             // (a NaN fails both comparisons)
    char msg[128]; snprintf(msg, sizeof(msg), "target_feats_per_pixel %g: a finite value >= 0 is expected", target);
    why = msg; return SVO_ERR_ARG;
}

int check_adaptive_nms_args(const svo_keypoint* kps, int n, int num_out_points, int img_w, int img_h, const int32_t* out_order, int cap,
                            int cand_cap, int max_kps, std::string& why)
{
    char msg[200]; msg[0] = 0;
    why.clear();
    if (n < 0 || (n > 0 && !kps)) snprintf(msg, sizeof(msg), "kps: %d keypoints at %s", n, kps ? "an address" : "NULL");
    else if (cap < 0 || (cap > 0 && !out_order)) snprintf(msg, sizeof(msg), "out_order: room for %d indices at %s", cap, out_order ? "an address" : "NULL");
    else if (img_w < 1 || img_h < 1 || img_w > 65535 || img_h > 65535 || (long long)img_w * img_h >= (1 << 24))
        snprintf(msg, sizeof(msg), "image %d x %d: sizes of 1 .. 65535 with img_w * img_h < 2^24 are expected", img_w, img_h);
    else if (n > cand_cap) snprintf(msg, sizeof(msg), "%d keypoints: the context's level-0 candidate capacity is %d", n, cand_cap);
    else if ((num_out_points < n ? num_out_points : n) > max_kps)
        snprintf(msg, sizeof(msg), "min(num_out_points, n) = %d: the selection keeps at most max_kps = %d", num_out_points < n ? num_out_points : n, max_kps);
    long long last = -1;
    for (int i = 0; i < n && !msg[0]; i++) {
        const float x = kps[i].x, y = kps[i].y;
        if (!(x >= 0.0f && x < (float)img_w && y >= 0.0f && y < (float)img_h) || x != (float)(int)x || y != (float)(int)y)
            snprintf(msg, sizeof(msg), "keypoint %d at (%g, %g): integer coordinates inside %d x %d are expected", i, (double)x, (double)y, img_w, img_h);
        else if (kps[i].response != kps[i].response) snprintf(msg, sizeof(msg), "keypoint %d: its response is NaN", i);
        else {
            const long long pos = (long long)(int)y * img_w + (int)x;
            if (pos <= last) snprintf(msg, sizeof(msg), "keypoint %d at (%d, %d): strictly ascending raster order is expected", i, (int)x, (int)y);
            last = pos;
        }
    }
    if (!msg[0]) return SVO_OK;
    why = msg; return SVO_ERR_ARG;
}

bool dyn_fast_octaves_changed(const svo_params& before, const svo_params& after)
{
    const int a = before.nOctaves < 1 ? 1 : before.nOctaves, b = after.nOctaves < 1 ? 1 : after.nOctaves;
    return a != b;
}

}

// the rule that moves dmFASTER's threshold, as the kernels compile it (faster_dyn.hpp), for a host that predicts or checks a sequence
extern "C" int svo_faster_threshold_step(int T, int n, int w, int h, double target_feats_per_pixel)
{
    return faster_dyn_step(T, (unsigned)n, w, h, target_feats_per_pixel);
}
