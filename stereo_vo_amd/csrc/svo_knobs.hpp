// svo_knobs.hpp -- the run-time knobs: every SVO_* environment variable the library consults, read ONCE per context by svo_create
// (knobs_read) into a Knobs that the context keeps, and the names of the SVO_DEBUG_MODE values.  Host only, no HIP: svo_device.h
// includes it so that the kernels see the names, svo_api.hip hands the context's Knobs to the launchers that consult one, and
// tools/knobs_check.cpp drives the parsing under the sanitizers on the CPU (`make hostcheck`).
// (SVO_ROCTX / ROCP_TOOL_LIBRARIES are not knobs of a context: they decide whether a library is loaded into the process -- RoctxApi
// in svo_api.hip.)
#pragma once

// ---- SVO_DEBUG_MODE -----------------------------------------------------------------------------------------------------------------
// 0 in production.  The NUMBERS are the knob's public face (tests, tests/dev, tools and INTEGRATION.md pass them) and never change;
// the code compares with the names.  Three groups, one predicate each below:
//   forms      other kernel forms or orders with the SAME results, in both libraries: the parity tests run them against the oracle
//   A/B forms  the same, but compiled only into libsvo_hip_ab.so (-DSVO_AB_KERNELS); svo_create refuses them elsewhere
//   ablations  a kernel stops early or leaves work out, for timing: the results are MEANINGLESS
enum DebugMode : int {
    DBG_NONE = 0,
    // ablations of k_fast
    DBG_FAST_STOP_STAGED = 1,        // returns after staging its tile
    DBG_FAST_STOP_COMPACTED = 2,     // ... after compacting the candidate pixels
    DBG_FAST_STOP_SCORED = 3,        // ... after the corner scores
    DBG_FAST_NO_PUBLISH = 4,         // runs to the end but publishes no corner
    // ablations of k_resize
    DBG_RESIZE_NO_STAGING = 5,       // without staging the source rows
    DBG_RESIZE_NO_BLEND = 6,         // returns before the blend
    DBG_RESIZE_NO_STORE = 7,         // blends but stores nothing
    // forms
    DBG_LINEAR_TILES = 8,            // linear (not XCD-chunked) tile orders in k_resize, k_fast, k_harris and k_describe
    DBG_DESCRIBE_BEFORE_NMS = 9,     // detector order: describe every raw keypoint, then NMS (what svo_debug_get_raw_keypoints shows)
    // ablations of k_gauss_newton
    DBG_GN_STOP_SETUP = 10,          // returns after its set-up
    DBG_GN_ONE_ITER = 11,            // one iteration per phase
    // forms
    DBG_NO_SPEC_FAST_TH = 12,        // no speculative FAST threshold: k_fast runs at the base threshold
    DBG_RC_REPLAY_ALL = 13,          // RANSAC count: every verdict replayed through the oracle's own expression
    DBG_RC_VALU16 = 14,              // [A/B] RANSAC count: k_ransac_count<16>, sixteen models per block on the VALU
    DBG_RC_NO_EARLY_STOP = 16,       // RANSAC count: never stops early on a hopeless model
    // ablations of k_nms_rowsort (tests/dev/nms_breakdown.py): returns after ...
    DBG_NMS_STOP_KEYS = 21,          // ... building its keys
    DBG_NMS_STOP_SORT = 22,          // ... the sort by response
    DBG_NMS_STOP_GRID = 23,          // ... the grid NMS
    DBG_NMS_STOP_ACCEPT = 24,        // ... the list of accepted keypoints
    DBG_NMS_STOP_ROWSORT = 25,       // ... the row sort
    DBG_NMS_STOP_CELLS = 26,         // ... the grid cells, before the grid NMS
    // ablations of k_select / k_select_sort: returns after ...
    DBG_SELECT_STOP_HIST = 31,       // k_select: ... the score histogram
    DBG_SSORT_STOP_RANGE = 41,       // k_select_sort: ... the wave-level key range
    DBG_SSORT_STOP_BUCKETS = 42,     // ... the bucket counts
    DBG_SSORT_STOP_OFFSETS = 43,     // ... the bucket offsets
    DBG_SSORT_STOP_SCATTER = 44,     // ... the scatter into buckets
    DBG_SSORT_STOP_RANK = 45,        // ... the ranking inside the buckets
    DBG_DESCRIBE_NO_TRIG = 46,       // ablation of k_describe: no trigonometry for the orientation
    // forms of the RANSAC launchers (k_match.hip)
    DBG_RH_LANES16 = 50,             // hypotheses: k_ransac_hyp (16 lanes per sample) whatever the lane count
    DBG_RH_THREAD = 51,              // hypotheses: k_ransac_hyp_thread (one thread per sample) whatever the lane count
    DBG_RC_MFMA4 = 52,               // [A/B] count: k_ransac_count_mfma, the 4 x 4-component matrix-core tiles
    DBG_RC_MFMA16 = 53,              // count: k_ransac_count_mfma16, the 16 x 16 tiles, whatever the lane count
    DBG_RC_MFMA16_REPLAY = 54,       // ... with every verdict replayed through the oracle's own expression
    // ablations of k_gauss_newton's iteration (tests/dev/gn_breakdown.py): one iteration per phase, and
    DBG_GN_NO_TRACK_LOOP = 60,       // ... without the per-track loop
    DBG_GN_NO_SOLVE = 61,            // ... without the solve
    DBG_GN_NO_ROT_UPDATE = 62,       // ... without the rotation update
    DBG_GN_NO_SOLVE_NO_ROT = 63,     // ... without either
    // ablations of k_gauss_newton's set-up, phase by phase (tests/dev/gn_breakdown.py): returns after ...
    DBG_GN_STOP_GATHER = 64,         // ... gathering the tracked observations
    DBG_GN_STOP_SORT = 65,           // ... the sort by response
    DBG_GN_STOP_MASK = 66,           // ... the NMS mask
    DBG_GN_STOP_TRIANGULATE = 67,    // ... the triangulation
};

constexpr bool dbg_in(int m, int lo, int hi) { return m >= lo && m <= hi; }
// the iteration ablations of k_gauss_newton, which all run one iteration per phase
constexpr bool debug_mode_gn_loop_ablation(int m) { return m >= DBG_GN_NO_TRACK_LOOP && m <= DBG_GN_NO_SOLVE_NO_ROT; }
// results unchanged, in both libraries
constexpr bool debug_mode_is_form(int m)
{
    return m == DBG_LINEAR_TILES || m == DBG_DESCRIBE_BEFORE_NMS || m == DBG_NO_SPEC_FAST_TH || m == DBG_RC_REPLAY_ALL || m == DBG_RC_NO_EARLY_STOP ||
           m == DBG_RH_LANES16 || m == DBG_RH_THREAD || m == DBG_RC_MFMA16 || m == DBG_RC_MFMA16_REPLAY;
}
// results unchanged, libsvo_hip_ab.so only
constexpr bool debug_mode_is_ab_form(int m) { return m == DBG_RC_VALU16 || m == DBG_RC_MFMA4; }
// results meaningless: for timing
constexpr bool debug_mode_is_ablation(int m)
{
    return dbg_in(m, DBG_FAST_STOP_STAGED, DBG_RESIZE_NO_STORE) || m == DBG_GN_STOP_SETUP || m == DBG_GN_ONE_ITER || dbg_in(m, DBG_NMS_STOP_KEYS, DBG_NMS_STOP_CELLS) ||
           m == DBG_SELECT_STOP_HIST || dbg_in(m, DBG_SSORT_STOP_RANGE, DBG_DESCRIBE_NO_TRIG) || dbg_in(m, DBG_GN_NO_TRACK_LOOP, DBG_GN_STOP_TRIANGULATE);
}

// ---- constants the knobs are validated against (the kernels use them too) ---------------------------------------------------------------
#define SVO_RANSAC_CHUNK0 32        // samples [0, CHUNK0) are evaluated unconditionally, [CHUNK0, CHUNK1) and [CHUNK1, HYP) only as far as
#define SVO_RANSAC_FEW 320          // both chunk ends for a handful of lanes (DevCtx.rs_c0 / rs_c1): one hypothesis + count pair covers what the stop rule usually visits
#ifndef SVO_RANSAC_CHUNK1
#define SVO_RANSAC_CHUNK1 160       // the 0.99-confidence stop of the sequential algorithm can still reach (rs_bound)
#endif
#define RC16_NSPLIT0 1              // blocks the pairs of a lane are split over in chunk 0 of k_ransac_count_mfma16 (chunks 1, 2: one; launch_ransac_count)

// ---- the knobs, validated ---------------------------------------------------------------------------------------------------------------
struct Knobs {
    int debug_mode;           // SVO_DEBUG_MODE: atoi, default 0; any integer is accepted (copied into DevCtx.debug_mode)
    int rest_prio;            // SVO_REST_PRIO: atoi & 3, default 0 (copied into DevCtx.rest_prio)
    bool timeline;            // SVO_TIMELINE: on iff its first character is '1'
    bool ham_fp4;             // SVO_HAM_FP4: the FP4 brute-force matcher (k_hamming_f4) unless set and atoi == 0 = the int8 form [A/B]
                              //   (default FP4: 32.1 against 45.0 us per launch at 64 lanes, profiles/r04n, r04o)
    int ham_splits;           // SVO_HAM_SPLITS: > 0 forces the matcher's train-side splits, 0 = derive from the lane count (hamming_splits)
    bool copy_prio_normal;    // SVO_COPY_PRIO: the upload stream at normal priority iff set and atoi == 0 (default: the highest)
    int rs_c0;                // SVO_RS_C0: SVO_RANSAC_CHUNK0 / CHUNK1 / FEW forces the end of chunk 0, anything else 0 = derive (enqueue_track)
    int rc_split[3];          // SVO_RC_SPLIT = s0[,s1[,s2]]: blocks per lane and side of k_ransac_count_mfma16 in chunk 0, 1, 2; entries not given
                              //   repeat the last one given; each 1..8, otherwise its default (RC16_NSPLIT0, 1, 1)
    int gn_nt;                // SVO_GN_NT: threads per lane of k_gauss_newton / k_pose_covariance, 256 / 384 / 512, else 384
    int desc_kpw;             // SVO_DESC_KPW: keypoints per wave of k_describe, 1..64 (a wave keeps its work items one per lane), else 8
    bool desc_tl;             // SVO_DESC_TL: k_describe's operands in LDS unless set and atoi == 0 = in registers
                              //   (default LDS: 0.204 -> 0.198 ms at 64 lanes, profiles/r04i)
    int nms_nt;               // SVO_NMS_NT: atoi; 512 takes effect where the lists fit 2048 keys (launch_nms_rowsort), anything else is 1024
};

// The only place that parses.  get(name) returns the variable's text or NULL: svo_create passes knobs_env, the check program a table.
void knobs_read(Knobs* k, const char* (*get)(const char*));
const char* knobs_env(const char* name);      // the process environment

// SVO_HAM_FP4=0 or SVO_DEBUG_MODE 14 / 52: a kernel form that only libsvo_hip_ab.so holds
inline bool svo_ab_form_requested(const Knobs& k) { return !k.ham_fp4 || debug_mode_is_ab_form(k.debug_mode); }
