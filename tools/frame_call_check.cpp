// frame_call_check.cpp -- the per-call decisions of svo_process / svo_process_lanes / svo_gather_windows (stereo_vo_amd/csrc/frame_call.cpp)
// against the contract of include/svo_hip.h, under the address and undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc hostcheck && tools/frame_call_check
//
// Every expected value below is written from the contract (svo_hip.h: svo_process_lanes, the SAD paragraph, the flag comments), not
// taken from a run.  Exit status 0 and a last line "ok" when everything held.
#include "frame_call.hpp"
#include <stdio.h>
#include <string.h>

using namespace svo_call;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static svo_params good_params()
{
    svo_params p; memset(&p, 0, sizeof(p));
    p.detect_method = SVO_DM_ORB; p.non_maximal_suppression = 1; p.nmsMethod = SVO_NMS_STANDARD; p.min_distance = 3;
    p.match_method = SVO_SM_DESC_BF; p.ifm_method = SVO_IFM_DESC_BF; p.initial_FAST_threshold = 20; p.minimum_ORB_response = 0.25;
    return p;
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

// ---- the mask ---------------------------------------------------------------------------------------------------------------
static void check_masks()
{
    LaneMask a, i; std::string why;
    // every lane count: all lanes set is accepted, active = the n lowest bits, nobody idle; NULL on the unmasked entry is the same
    const int counts[5] = { 1, 63, 64, 65, 128 };
    for (int n : counts) {
        uint64_t all[2] = { n >= 64 ? ~0ull : (1ull << n) - 1, n <= 64 ? 0 : (n == 128 ? ~0ull : (1ull << (n - 64)) - 1) };
        CHECK(parse_lane_mask(all, true, n, a, i, why) && why.empty());
        CHECK(a.w[0] == all[0] && a.w[1] == all[1] && i.w[0] == 0 && i.w[1] == 0);
        int cnt = 0; for (int l = 0; l < SVO_MAX_LANES; l++) cnt += lane_in(a, l) ? 1 : 0;
        CHECK(cnt == n && lane_in(a, n - 1) && (n == SVO_MAX_LANES || !lane_in(a, n)));
        LaneMask a2, i2;
        CHECK(parse_lane_mask(nullptr, false, n, a2, i2, why) && !memcmp(&a2, &a, sizeof(a)) && !memcmp(&i2, &i, sizeof(i)));
        // only the last lane: everybody else idle
        uint64_t last[2] = { n <= 64 ? 1ull << (n - 1) : 0, n > 64 ? 1ull << (n - 65) : 0 };
        CHECK(parse_lane_mask(last, true, n, a, i, why));
        CHECK(lane_in(a, n - 1) && !lane_in(i, n - 1) && (n == 1 || (lane_in(i, 0) && !lane_in(a, 0))));
        CHECK((a.w[0] | i.w[0]) == all[0] && (a.w[1] | i.w[1]) == all[1] && (a.w[0] & i.w[0]) == 0 && (a.w[1] & i.w[1]) == 0);
        // all clear: accepted, nobody active (the caller returns SVO_OK without enqueueing)
        uint64_t none[2] = { 0, 0 };
        CHECK(parse_lane_mask(none, true, n, a, i, why) && !lane_any(a) && i.w[0] == all[0] && i.w[1] == all[1]);
        // the first bit at or above n_lanes: refused with a text that names the word, its value and n_lanes
        if (n < SVO_MAX_LANES) {
            uint64_t stray[2] = { all[0], all[1] }; stray[n >> 6] |= 1ull << (n & 63);
            CHECK(!parse_lane_mask(stray, true, n, a, i, why));
            char want[160]; snprintf(want, sizeof(want), "active[%d] = %016llx selects a lane at or above n_lanes = %d", n >> 6, (unsigned long long)stray[n >> 6], n);
            CHECK(why == want);
            CHECK(!parse_lane_mask(stray, false, n, a, i, why) && why == want);      // svo_gather_windows: the same text
        }
    }
    {   // a stray bit in word 0 and in word 1 at once: the first word is reported
        uint64_t m[2] = { 0x10, 0x1 };
        CHECK(!parse_lane_mask(m, true, 3, a, i, why) && why == "active[0] = 0000000000000010 selects a lane at or above n_lanes = 3");
        uint64_t m1[2] = { 0x7, 0x8000000000000000ull };
        CHECK(!parse_lane_mask(m1, true, 3, a, i, why) && why == "active[1] = 8000000000000000 selects a lane at or above n_lanes = 3");
    }
    // NULL on the masked entry point: refused
    CHECK(!parse_lane_mask(nullptr, true, 4, a, i, why) && why == "active == NULL");
}

// ---- the call facts ---------------------------------------------------------------------------------------------------------
static void check_facts()
{
    svo_params p = good_params();
    FrameCall c = make_frame_call(SVO_RUN_ALL, p);
    CHECK(c.runs_post && c.shifts && !c.repeat && !c.ahead && !c.continuation && !c.faster && !c.sad_any && !c.select_in_post);
    CHECK(c.nms_mode == 1 && c.nms_mode_oct == 0 && c.minresp == 0.25);
    c = make_frame_call(SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST, p);
    CHECK(!c.runs_post && c.shifts && !c.continuation);
    c = make_frame_call(SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST | SVO_FLAG_DETECT_SPLIT_AT_SELECT, p);
    CHECK(!c.runs_post && c.select_in_post);
    c = make_frame_call(SVO_RUN_DETECT | SVO_FLAG_DETECT_SPLIT_AT_SELECT, p);        // nothing is left out: nothing moves
    CHECK(c.runs_post && !c.select_in_post);
    c = make_frame_call(SVO_RUN_DETECT_POST | SVO_FLAG_DETECT_SPLIT_AT_SELECT | SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, p);
    CHECK(c.runs_post && c.select_in_post && c.continuation && !c.shifts);
    c = make_frame_call(SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST | SVO_FLAG_DETECT_AHEAD, p);   // leaves lane state alone
    CHECK(c.ahead && !c.shifts && !c.runs_post && !c.continuation);
    c = make_frame_call(SVO_RUN_DETECT_POST | SVO_FLAG_DETECT_AHEAD | SVO_RUN_MATCH, p);        // completes it: runs the shift itself
    CHECK(c.ahead && c.shifts && c.runs_post && c.continuation);
    c = make_frame_call(SVO_RUN_TRACK | SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT, p);
    CHECK(!c.shifts && c.continuation && !c.runs_post);
    c = make_frame_call(SVO_RUN_ALL | SVO_FLAG_REPEAT, p);
    CHECK(c.repeat && c.shifts);
    p.non_maximal_suppression = 0; c = make_frame_call(SVO_RUN_ALL, p); CHECK(c.nms_mode == 0 && c.nms_mode_oct == 3);
    p.non_maximal_suppression = 1; p.nmsMethod = SVO_NMS_ADAPTIVE; c = make_frame_call(SVO_RUN_ALL, p); CHECK(c.nms_mode == 2 && c.nms_mode_oct == 0);
    p.detect_method = SVO_DM_FAST_ORB; c = make_frame_call(SVO_RUN_ALL, p); CHECK(c.minresp == 0.0 && !c.faster);
    p.detect_method = SVO_DM_FASTER; p.match_method = SVO_SM_SAD; c = make_frame_call(SVO_RUN_ALL, p); CHECK(c.faster && c.sad_m && !c.sad_t && c.sad_any);
    p.match_method = SVO_SM_DESC_BF; p.ifm_method = SVO_IFM_SAD; c = make_frame_call(SVO_RUN_ALL, p); CHECK(!c.sad_m && c.sad_t && c.sad_any);
    // the two SAD thresholds: 0 is the reference's 200 for both; a negative one is "none" -- INT32_MAX in stage 3, the wrapped unsigned in stage 4
    p.sad_max_distance = 0; p.ifm_sad_max_distance = 0; c = make_frame_call(0, p); CHECK(c.max_sad_match == 200 && c.max_sad_track == 200u);
    p.sad_max_distance = 350; p.ifm_sad_max_distance = 90; c = make_frame_call(0, p); CHECK(c.max_sad_match == 350 && c.max_sad_track == 90u);
    p.sad_max_distance = -1; p.ifm_sad_max_distance = -1; c = make_frame_call(0, p); CHECK(c.max_sad_match == 2147483647 && c.max_sad_track == 4294967295u);
}

// ---- the refusals, each once, with its code -----------------------------------------------------------------------------------
static int refusal(uint32_t flags, const svo_params& p, std::string& why, const LaneMask* active = nullptr, const LaneMask* frame = nullptr)
{
    LaneMask all; all.w[0] = 0xF; all.w[1] = 0;
    return check_frame_call(make_frame_call(flags, p), p, active ? *active : all, frame, why);
}
static void check_refusals()
{
    std::string why;
    const svo_params g = good_params();
    CHECK(refusal(SVO_RUN_ALL, g, why) == SVO_OK && why.empty());
    svo_params p;
    // selectors out of range: hard errors, no text
    p = g; p.detect_method = 4; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_ARG && why.empty());
    p = g; p.detect_method = -1; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_ARG);
    p = g; p.match_method = 3; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_ARG);
    p = g; p.ifm_method = 4; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_ARG);
    // the variants outside the hot path, only where the call runs their stage
    p = g; p.detect_method = SVO_DM_KLT; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_UNSUPPORTED && refusal(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, p, why) == SVO_OK);
    p = g; p.ifm_method = SVO_IFM_OPTICAL_FLOW; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_UNSUPPORTED && refusal(SVO_RUN_DETECT | SVO_RUN_MATCH, p, why) == SVO_OK);
    p = g; p.nmsMethod = 2; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_ARG);
    p.non_maximal_suppression = 0; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_OK);          // (the method is not looked at while the NMS is off)
    p = g; p.min_distance = 1; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_ARG);
    // dmFASTER: only the SAD stages can follow it, no adaptive NMS, a threshold of 0 .. 255 -- each with a text
    svo_params f = g; f.detect_method = SVO_DM_FASTER; f.match_method = SVO_SM_SAD; f.ifm_method = SVO_IFM_SAD;
    CHECK(refusal(SVO_RUN_ALL, f, why) == SVO_OK);
    p = f; p.match_method = SVO_SM_DESC_RBR; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_STATE && why == "dmFASTER computes no descriptors: stage 3 needs match_method = smSAD");
    CHECK(refusal(SVO_RUN_DETECT, p, why) == SVO_OK);
    p = f; p.ifm_method = SVO_IFM_DESC_WIN; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_STATE && why == "dmFASTER computes no descriptors: stage 4 needs ifm_method = ifmSAD");
    p = f; p.nmsMethod = SVO_NMS_ADAPTIVE; CHECK(refusal(SVO_RUN_DETECT, p, why) == SVO_ERR_UNSUPPORTED && why == "the adaptive NMS is not built for dmFASTER: use nmsMethod = nmsmStandard");
    CHECK(refusal(SVO_RUN_DETECT_POST | SVO_FLAG_NO_SHIFT, p, why) == SVO_ERR_UNSUPPORTED && refusal(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, p, why) == SVO_OK);
    p = f; p.initial_FAST_threshold = 256; CHECK(refusal(SVO_RUN_DETECT, p, why) == SVO_ERR_ARG && why == "initial_FAST_threshold 256: dmFASTER takes 0 .. 255");
    p.initial_FAST_threshold = -1; CHECK(refusal(SVO_RUN_DETECT, p, why) == SVO_ERR_ARG && why == "initial_FAST_threshold -1: dmFASTER takes 0 .. 255");
    // the order stays: a call that breaks two rules reports the earlier one
    p = f; p.match_method = SVO_SM_DESC_BF; p.initial_FAST_threshold = 300; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_STATE && has(why, "stage 3"));
    p = g; p.min_distance = 0; p.detect_method = SVO_DM_KLT; CHECK(refusal(SVO_RUN_ALL, p, why) == SVO_ERR_UNSUPPORTED);
    // SVO_FLAG_DETECT_AHEAD: DETECT | NO_POST alone, or a post call that shifts
    const uint32_t A = SVO_FLAG_DETECT_AHEAD;
    CHECK(refusal(A | SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST, g, why) == SVO_OK);
    CHECK(refusal(A | SVO_RUN_DETECT, g, why) == SVO_ERR_ARG && why.empty());
    CHECK(refusal(A | SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST | SVO_RUN_MATCH, g, why) == SVO_ERR_ARG);
    CHECK(refusal(A | SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST | SVO_RUN_DETECT_POST, g, why) == SVO_ERR_ARG);
    CHECK(refusal(A | SVO_RUN_DETECT_POST | SVO_RUN_MATCH | SVO_RUN_TRACK | SVO_RUN_OPTIMIZE, g, why) == SVO_OK);
    CHECK(refusal(A | SVO_RUN_MATCH, g, why) == SVO_ERR_ARG);
    CHECK(refusal(A | SVO_RUN_DETECT_POST | SVO_FLAG_NO_SHIFT, g, why) == SVO_ERR_ARG);
    // one mask per frame: a continuation with another mask than the frame's is SVO_ERR_STATE with both masks in the text
    LaneMask began; began.w[0] = 0x5; began.w[1] = 0x1;
    LaneMask other; other.w[0] = 0x7; other.w[1] = 0x1;
    CHECK(refusal(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, g, why, &began, &began) == SVO_OK);
    CHECK(refusal(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, g, why, &other, &began) == SVO_ERR_STATE);
    CHECK(why == "active lanes 0000000000000001:0000000000000007, but the frame in flight began with 0000000000000001:0000000000000005: every call of a frame carries the same mask");
    CHECK(refusal(SVO_RUN_DETECT_POST | SVO_RUN_MATCH, g, why, &other, &began) == SVO_ERR_STATE);
    CHECK(refusal(SVO_RUN_ALL, g, why, &other, &began) == SVO_OK);                       // a call that begins a frame brings its own mask
    CHECK(refusal(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, g, why, &other, nullptr) == SVO_OK);  // no frame in flight yet
}

// ---- the record of gathered windows -----------------------------------------------------------------------------------------
static SadWindows rec(std::vector<uint8_t> cur, std::vector<uint8_t> prev, std::vector<uint8_t> drop) { SadWindows w; w.cur = cur; w.prev = prev; w.drop = drop; return w; }
static bool same(const SadWindows& w, std::vector<uint8_t> cur, std::vector<uint8_t> prev, std::vector<uint8_t> drop) { return w.cur == cur && w.prev == prev && w.drop == drop; }
static void check_window_step()
{
    LaneMask nobody_idle; memset(&nobody_idle, 0, sizeof(nobody_idle));
    svo_params sad = good_params(); sad.match_method = SVO_SM_SAD; sad.ifm_method = SVO_IFM_SAD;
    svo_params plain = good_params();
    // a whole frame under SAD: the previous frame has windows when both candidates for it had them (the device decides the shift), the
    // current one gets them from the post-processing.  Lane 0 had both, lane 1 lacked the previous, lane 2 lacked the current.
    SadStep r = sad_window_step(rec({ 1, 1, 0 }, { 1, 0, 1 }, { 0, 0, 0 }), nobody_idle, make_frame_call(SVO_RUN_DETECT | SVO_RUN_MATCH, sad));
    CHECK(r.bad_lane < 0 && r.why.empty() && !r.any_drop && !lane_any(r.drop_prev) && same(r.next, { 1, 1, 1 }, { 1, 0, 0 }, { 0, 0, 0 }));
    // SVO_FLAG_REPEAT: the current frame is replaced, the previous one stays what it was
    r = sad_window_step(rec({ 1, 1, 0 }, { 1, 0, 1 }, { 0, 0, 0 }), nobody_idle, make_frame_call(SVO_RUN_DETECT | SVO_RUN_MATCH | SVO_FLAG_REPEAT, sad));
    CHECK(r.bad_lane < 0 && same(r.next, { 1, 1, 1 }, { 1, 0, 1 }, { 0, 0, 0 }));
    // no SAD method selected: a detected frame has no windows
    r = sad_window_step(rec({ 1, 1 }, { 1, 1 }, { 0, 0 }), nobody_idle, make_frame_call(SVO_RUN_ALL, plain));
    CHECK(r.bad_lane < 0 && same(r.next, { 0, 0 }, { 1, 1 }, { 0, 0 }));
    // a detect call that leaves the post-processing out: an empty list until the post call has run; that one (NO_SHIFT) marks it
    r = sad_window_step(rec({ 1 }, { 1 }, { 0 }), nobody_idle, make_frame_call(SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST, sad));
    CHECK(r.bad_lane < 0 && same(r.next, { 0 }, { 1 }, { 0 }));
    r = sad_window_step(r.next, nobody_idle, make_frame_call(SVO_RUN_DETECT_POST | SVO_RUN_MATCH | SVO_RUN_TRACK | SVO_FLAG_NO_SHIFT, sad));
    CHECK(r.bad_lane < 0 && same(r.next, { 1 }, { 1 }, { 0 }));
    // a pending sad_drop: the shift forgets the previous frame -- the lane is in drop_prev, "no such frame" counts as having windows, the mark goes
    r = sad_window_step(rec({ 1, 1 }, { 0, 1 }, { 1, 0 }), nobody_idle, make_frame_call(SVO_RUN_ALL, sad));
    CHECK(r.bad_lane < 0 && r.any_drop && r.drop_prev.w[0] == 1 && r.drop_prev.w[1] == 0 && same(r.next, { 1, 1 }, { 1, 1 }, { 0, 0 }));
    // ... at the lane's next ACTIVE frame: an idle lane keeps its sad_drop and everything else
    LaneMask idle0; idle0.w[0] = 1; idle0.w[1] = 0;
    r = sad_window_step(rec({ 0, 1 }, { 0, 1 }, { 1, 0 }), idle0, make_frame_call(SVO_RUN_ALL, sad));
    CHECK(r.bad_lane < 0 && !r.any_drop && !lane_any(r.drop_prev) && same(r.next, { 0, 1 }, { 0, 1 }, { 1, 0 }));
    // a call without a shift does not consume the mark either
    r = sad_window_step(rec({ 1 }, { 1 }, { 1 }), nobody_idle, make_frame_call(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, sad));
    CHECK(r.bad_lane < 0 && !r.any_drop && same(r.next, { 1 }, { 1 }, { 1 }));
    // the detect-ahead call does not shift (its post call does): the record stays as it is
    r = sad_window_step(rec({ 1, 0 }, { 0, 1 }, { 0, 1 }), nobody_idle, make_frame_call(SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST | SVO_FLAG_DETECT_AHEAD, sad));
    CHECK(r.bad_lane < 0 && !r.any_drop && same(r.next, { 1, 0 }, { 0, 1 }, { 0, 1 }));
    r = sad_window_step(rec({ 1, 0 }, { 1, 1 }, { 0, 1 }), nobody_idle, make_frame_call(SVO_RUN_DETECT_POST | SVO_FLAG_DETECT_AHEAD | SVO_RUN_MATCH | SVO_RUN_TRACK, sad));
    CHECK(r.bad_lane < 0 && r.any_drop && r.drop_prev.w[0] == 2 && same(r.next, { 1, 1 }, { 1, 1 }, { 0, 0 }));
    // refusal 1, the CURRENT frame: stage 3 with smSAD on put features (no shift, no post-processing in the call).  Nothing moves.
    const SadWindows put = rec({ 1, 0 }, { 1, 1 }, { 0, 0 });
    r = sad_window_step(put, nobody_idle, make_frame_call(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, sad));
    CHECK(r.bad_lane == 1 && same(r.next, put.cur, put.prev, put.drop) && !r.any_drop && !lane_any(r.drop_prev));
    CHECK(r.why == "lane 1: match_method selects SAD but the 8 x 8 windows of its current frame were never gathered (features put, loaded or imported, "
                   "or detected while no SAD method was selected)");
    // ... the same for the tracker alone: the current frame again, named by ifm_method
    svo_params sad_t = good_params(); sad_t.ifm_method = SVO_IFM_SAD;
    r = sad_window_step(put, nobody_idle, make_frame_call(SVO_RUN_TRACK | SVO_FLAG_NO_SHIFT, sad_t));
    CHECK(r.bad_lane == 1 && has(r.why, "lane 1: ifm_method selects SAD") && has(r.why, "of its current frame") && !has(r.why, "afresh") && same(r.next, put.cur, put.prev, put.drop));
    // ... and only in the active lanes
    LaneMask idle1; idle1.w[0] = 2; idle1.w[1] = 0;
    r = sad_window_step(put, idle1, make_frame_call(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, sad));
    CHECK(r.bad_lane < 0 && same(r.next, put.cur, put.prev, put.drop));
    // refusal 2, the PREVIOUS frame: a stream that switches to ifmSAD -- lane 1's last frame was detected without windows.  The call
    // would have shifted: refused, the record stays, and the lane is marked so that its next frame starts afresh (lane 0 is not, lane 2 is idle)
    const SadWindows sw = rec({ 1, 0, 0 }, { 1, 1, 0 }, { 0, 0, 0 });
    LaneMask idle2; idle2.w[0] = 4; idle2.w[1] = 0;
    r = sad_window_step(sw, idle2, make_frame_call(SVO_RUN_ALL, sad_t));
    CHECK(r.bad_lane == 1 && !r.any_drop && !lane_any(r.drop_prev) && same(r.next, { 1, 0, 0 }, { 1, 1, 0 }, { 0, 1, 0 }));
    CHECK(r.why == "lane 1: ifm_method selects SAD but the 8 x 8 windows of its previous frame were never gathered (features put, loaded or imported, "
                   "or detected while no SAD method was selected): this frame is refused, the next one starts the lane's track afresh");
    // the frame after: the mark is consumed, the lane forgets its previous frame and the call goes through
    r = sad_window_step(r.next, idle2, make_frame_call(SVO_RUN_ALL, sad_t));
    CHECK(r.bad_lane < 0 && r.any_drop && r.drop_prev.w[0] == 2 && same(r.next, { 1, 1, 0 }, { 1, 1, 0 }, { 0, 0, 0 }));
    // the previous frame lacks windows but the call does not shift (or repeats): refused, and nothing is remembered
    r = sad_window_step(rec({ 1 }, { 0 }, { 0 }), nobody_idle, make_frame_call(SVO_RUN_TRACK | SVO_FLAG_NO_SHIFT, sad_t));
    CHECK(r.bad_lane == 0 && has(r.why, "of its previous frame") && !has(r.why, "afresh") && same(r.next, { 1 }, { 0 }, { 0 }));
    r = sad_window_step(rec({ 1 }, { 0 }, { 0 }), nobody_idle, make_frame_call(SVO_RUN_ALL | SVO_FLAG_REPEAT, sad_t));
    CHECK(r.bad_lane == 0 && has(r.why, "of its previous frame") && !has(r.why, "afresh") && same(r.next, { 1 }, { 0 }, { 0 }));
    // 128 lanes: the last lane's bit is bit 63 of word 1
    SadWindows big = rec(std::vector<uint8_t>(128, 1), std::vector<uint8_t>(128, 1), std::vector<uint8_t>(128, 0)); big.drop[127] = 1; big.drop[64] = 1;
    r = sad_window_step(big, nobody_idle, make_frame_call(SVO_RUN_ALL, sad));
    CHECK(r.bad_lane < 0 && r.drop_prev.w[0] == 0 && r.drop_prev.w[1] == (0x8000000000000000ull | 1ull) && r.next.drop == std::vector<uint8_t>(128, 0));
}

int main()
{
    check_masks();
    check_facts();
    check_refusals();
    check_window_step();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
