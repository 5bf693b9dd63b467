// svo_ctx.hpp -- what the units behind the C-ABI share (private; include/svo_hip.h is the public face): the context, the error and
// timing idioms of an entry point, and the few pipeline helpers of svo_api.hip that the front ends call.  svo_api.hip holds the context's
// life, the geometry and the frame pipeline; svo_lk.hip, svo_gftt.hip and svo_klt.hip hold the front ends.
#pragma once
#include "svo_device.h"
#include "svo_kernels.h"
#include "frame_call.hpp"
#include "lk_call.hpp"
#include "gftt_call.hpp"
#include "klt_call.hpp"
#include "kernel_names.hpp"
#include <string.h>
#include <initializer_list>
#include <string>
#include <vector>

#define HIPCHECK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { ctx->last_error = std::string(#expr) + ": " + hipGetErrorString(_e); return SVO_ERR_HIP; } } while (0)
// how an entry point that makes a call of its own begins: no context, no call; the context's device; the last error cleared
#define SVO_ENTER(ctx) do { if (!(ctx)) return SVO_ERR_ARG; use_device(ctx); (ctx)->last_error.clear(); } while (0)
// a decision unit's verdict on the call: `check` writes its reason to `why`; a refused call leaves it in last_error and returns the status
#define SVO_REFUSE(check) do { std::string why; const int _rc = (check); if (_rc) { ctx->last_error = why; return _rc; } } while (0)

struct TimedSpan { int id; hipEvent_t a, b; };

struct svo_ctx {
    svo_config cfg;
    Knobs knobs;                                       // the SVO_* environment of svo_create (svo_knobs.hpp): read once, before the first allocation
    svo_params params;
    int fast_th, orb_th;
    int klt_win;                                       // TDetectParams::KLT_win (S2:47): the window of dmFASTER's response, (2 klt_win + 1)^2 pixels
    hipStream_t stream, stream0; bool own_stream;      // stream0: the stream the context was created with / owns
    DevCtx dc;
    bool geom_ready, geom_once;                        // geom_once: DevCtx has held a frame's geometry (svo_set_params clears geom_ready only; the lists of the last frame keep theirs)
    int geom_w, geom_h, geom_nfe, geom_nlevels, geom_method, geom_noct;
    int raw_cap_alloc;
    uint8_t* d_img0; int img0_pitch_internal;
    // host-fed frames (process_new_image_pair.cpp:100-120 hands over host images): a ring of two device level-0 buffers
    // filled by a dedicated copy stream, so that the upload of frame t+1 overlaps the kernels of frame t
    uint8_t* d_img0_ring[2]; uint8_t* h_stage[2]; size_t slot_bytes;
    hipStream_t s_copy; hipEvent_t ev_h2d[2], ev_det[2]; bool ev_det_valid[2], ev_h2d_valid[2], up_ready; int up_slot, det_slot;
    long long pyr_bytes_alloc; int cand_total_alloc, rtab_alloc, tile_tab_alloc;
    std::vector<void*> allocs;
    std::string last_error;
    std::vector<TimedSpan> spans; std::vector<hipEvent_t> free_events;
    double kt_total[KT_COUNT]; long long kt_calls[KT_COUNT]; unsigned long long kt_mask;
    // svo_kernel_times: one bit per KernelTimeGroup (kernel_names.hpp), set where the context does what the group stands for
    unsigned kt_seen;
    void seen(int group) { kt_seen |= 1u << group; }
    bool has_seen(int group) const { return (kt_seen >> group & 1u) != 0; }
    unsigned* d_ham_out; uint8_t* d_ham_q, *d_ham_t; int ham_cap_q, ham_cap_t;
    // svo_lk_track: buffers of its own, made by its first call, grown on demand, freed with the context -- the pyramids of the call's
    // images, the job records, the flat point arrays (pts, init, out: float2; status; err).  lk_jobs: the records of the last call, for
    // svo_debug_lk_get_level
    uint8_t* d_lk_pyr; size_t lk_pyr_cap; LkJobDev* d_lk_jobs; int lk_jobs_cap;
    float2* d_lk_pts, *d_lk_init, *d_lk_out; uint8_t* d_lk_status; float* d_lk_err; int lk_pts_cap;
    std::vector<LkJobDev> lk_jobs;
    // svo_lk_set_photometric: 0 raw differences, 1 gain and bias removed per window.  The tracker's, not the front end's: every LK launch
    // of the context reads it when it is enqueued, and svo_klt_enable leaves it alone
    int lk_photo;
    // svo_gftt_detect: buffers of its own as well -- the response maps, the copies of host images, the job records, per job the
    // candidate keys, the cell lists and the decision states, the flat seed and result arrays, four counters per job.  gftt_jobs: the
    // records of the last call, for svo_debug_gftt_get_response
    float* d_gftt_map; size_t gftt_map_cap; uint8_t* d_gftt_img; size_t gftt_img_cap; GfttJobDev* d_gftt_jobs; int gftt_jobs_cap;
    unsigned long long* d_gftt_keys; int* d_gftt_items; uint8_t* d_gftt_state; int* d_gftt_info;
    float2* d_gftt_seeds; int gftt_seeds_cap; float2* d_gftt_pts; float* d_gftt_resp; int gftt_pts_cap;
    std::vector<GfttJobDev> gftt_jobs;
    // the resident KLT front end (svo_klt_enable; the plan: klt_call.hpp): nothing is allocated until it is enabled.  Host side: the
    // parameters in force, the table half that is live (every lane's: k_klt_select moves idle lanes along), per lane the pyramid parity
    // its last pair went to and whether it has a last pair, the image size of the last step.  klt_free zeroes the whole struct
    struct Klt {
        bool enabled; svo_klt_params p; svo_klt::Plan plan;
        KltDev dev; uint8_t* d_pyr; LkJobDev* d_pyr_jobs, * d_trk_jobs; float2* d_stage;
        int half, w, h; LaneMask parity, has_img;
        int ransac;                                    // svo_klt_set_ransac: 0 off, 1 filter the tracked pairs, 2 and drop the rejected tracks
        // svo_klt_set_prediction: 0 off, 1 constant-velocity pose prediction.  The one buffer of mode 1 (klt_call.hpp: plan_predict), made
        // by the first call with mode 1 and dropped with the front end's buffers: the guesses and a byte per slot
        int predict; float2* d_guess; uint8_t* d_gused;
        // svo_klt_set_stereo: 0 the right list is tracked through time, 1 it is found along the row in the new pair.  The buffers of mode 1
        // (klt_call.hpp: plan_stereo), made by the first call with mode 1 and dropped with the front end's buffers
        int stereo; LkJobDev* d_row_jobs; float2* d_row_guess;
        // the resident top-up (svo_klt_topup_enable; the plan: klt_call.hpp), buffers of its own: the response maps, the detector's job
        // records, keys, cell lists, states and counters, the corners with their responses, the first guesses, the tracker's records and
        // results, four ints per lane for svo_klt_topup_info
        bool topup_enabled; svo_klt_topup_params tp; svo_klt::TopupPlan tplan;
        float* d_tmap; GfttJobDev* d_tgjobs; unsigned long long* d_tkeys; int* d_titems; uint8_t* d_tstate; int* d_tginfo, * d_tinfo;
        float2* d_tcorners, * d_tinit, * d_tout; float* d_tresp, * d_terr; uint8_t* d_tstatus; LkJobDev* d_tlk_jobs;
    } klt;
    // where the device buffers of the front end (those of the prediction and the stereo mode with them) and of the top-up live: each
    // address is noted by the call that allocates it (klt_alloc), and the group is freed from its list
    std::vector<void**> klt_bufs, topup_bufs;
    bool params_set;                                   // svo_set_params has been called (the front end needs the parameters stage 5 runs with)
    bool frame_parallel;                               // the context is a member of a frame-parallel stream (svo_internal_mark_frame_parallel): no KLT front end
    // stage 1 (svo_set_rectify_map, SVO_FLAG_BGR_IMAGES): all allocated on first use
    uint8_t* d_src; int src_pitch;                    // staging of host source images (grey or BGR)
    uint2** d_map_ptrs; std::vector<uint2*> map_ptrs;  // per image: fixed-point map on the device or nullptr
    int map_w, map_h, n_maps;
    std::vector<uint2*> map_bufs;                      // per image: the allocation of its own behind map_ptrs (kept across clear / set cycles)
    // maps from a calibration (svo_set_undistort_rectify, svo_set_stereo_calibration): the table of a side that lane = -1 built ONCE and
    // every lane's map_ptrs entry points at until the lane is set or cleared on its own; the models k_rectify_map reads.  First use.
    uint2* map_shared[2]; RectifyImage* d_rect_models;
    // getChangeInPose works on temporaries (common.cpp:362-400): a one-lane scratch view of the device context
    DevCtx cip; bool cip_ready;
    // svo_get_values: device packing buffer and its page-locked host mirror
    uint8_t* d_vals; uint8_t* h_vals; size_t vals_bytes;
    uint32_t* d_anms;                                  // scratch of k_fastorb_anms (3 x n_img x cand_total), allocated on first use
    // svo_set_pose_covariance: one record per lane and the array k_gauss_newton leaves its final mask in; nullptr until first enabled
    bool pose_cov; svo_pose_cov* d_cov; uint8_t* d_cov_mask;      // (d_cov_mask: made by whichever of this feature and the next is enabled first)
    // svo_set_landmarks: [n_lanes][max_kps] records, one info per lane, the 4 counter words per lane of k_landmarks; nullptr until first enabled
    bool landmarks; double lmk_std; svo_landmark* d_lmk; svo_landmarks_info* d_lmk_info; int* d_lmk_cnt;
    // svo_set_dyn_fast_threshold: dmFASTER's m_threshold[octave] of every lane (the `next` member) with its statistics; nullptr until first enabled.
    // Persistent detector scratch: read and written by detect calls alone, ordered on the stream they run on, like fast_th_dyn
    bool dyn_fast; double dyn_target; svo_faster_stats* d_fstats;
    // svo_set_faster_adaptive_nms: the opt-in, and the scratch of k_faster_anms (3 x n_img x cand_total 64-bit words), allocated by the setter.
    // svo_adaptive_nms has buffers of its own (keys, scratch, positions out), allocated by its first call: it touches nothing a frame uses
    bool faster_anms; unsigned long long* d_fanms; unsigned long long* d_anms_list; uint32_t* d_anms_pos;
    unsigned long long* d_cand64;                      // dmFASTER's 64-bit candidate keys (n_img x cand_total), allocated by the first svo_process made while it is selected
    // smSAD / ifmSAD (k_sad_patch): which frames of a lane have their 8 x 8 windows in DevCtx.sad_patch.  Kept on the HOST, per lane,
    // so that a stage that selects SAD on a frame without them is refused before anything is enqueued.  "true" also stands for "no
    // such frame yet" (the kernels then read nothing).  The device decides the prev/cur shift (the recovery rule of P:86-95 needs
    // m_error), so the previous frame after a shift is known to have patches only when both candidates for it had them.
    svo_call::SadWindows sad;                          // sad.drop: the lane's next shift forgets its previous frame (svo_hip.h)
    LaneMask imported;                                 // lanes that svo_import_frame has written and that have not had a svo_process call since (an idle lane keeps its bit)
    // svo_process_lanes: the active mask of the call that began the frame in flight.  The later calls of a multi-call frame (the post
    // call of a detect call, stages run with SVO_FLAG_NO_SHIFT) must carry the same one.
    LaneMask frame_active; bool frame_active_set;
    int sampler_nmax;                                  // > 0: holds a reference on the shared sampler table of (device, sampler_nmax)
    hipEvent_t post_event;                             // svo_record_after_post: armed for the next call that runs the detector's post-processing
    // svo_use_graphs: the kernel sequence of a frame captured once per (flags, ring slot, thresholds) and replayed
    struct GraphEntry { uint32_t flags; int slot, fast_th, orb_th; hipGraphExec_t exec; };
    std::vector<GraphEntry> graphs; bool use_graphs; unsigned graph_replays;      // graph_replays: calls served by an earlier capture (svo_debug_get_graph_count)
    bool capturing;                                    // the call being enqueued is capturing its launches on the stream (CaptureGuard)
    // every stream that has had work of this context enqueued since the last full synchronisation (svo_set_stream), each with
    // a context-owned event recorded behind the last work enqueued on it.  Synchronising waits on the EVENTS, never on the
    // foreign stream handles: a caller may synchronise and destroy its own stream and switch back with svo_set_stream(NULL);
    // an event recorded on a stream that has since been destroyed is simply complete.
    struct UsedStream { hipStream_t s; hipEvent_t ev; bool dirty; };
    std::vector<UsedStream> used_streams;
};

// Every entry point runs on the context's GPU whatever device the calling thread had current (a host may own one
// estimator per GPU and call them from one thread, or from one thread each: SURVEY.md 8b "Threading")
static inline void use_device(const svo_ctx* ctx)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != ctx->cfg.device) (void)hipSetDevice(ctx->cfg.device);
}

// ---- svo_api.hip ------------------------------------------------------------------------------------------------------------------
void note_stream(svo_ctx* ctx);
void mark_stream(svo_ctx* ctx);
hipEvent_t get_event(svo_ctx* ctx);
int ensure_geometry(svo_ctx* ctx, int w, int h);
void enqueue_ransac_tracked(svo_ctx* ctx, hipStream_t st);
void enqueue_optimize(svo_ctx* ctx, const svo_call::FrameCall&, hipStream_t st);

// the launches between its construction and its destruction count under kernel-time name `id` (kernel_names.hpp)
struct Span {
    svo_ctx* ctx; int id; hipEvent_t a, b; bool on; hipStream_t st;
    Span(svo_ctx* c, int i, hipStream_t on_stream = nullptr) : ctx(c), id(i), on(c->cfg.kernel_times != 0 && ((c->kt_mask >> i) & 1ull)), st(on_stream ? on_stream : c->stream) { if (on) { a = get_event(ctx); b = get_event(ctx); hipEventRecord(a, st); } }
    ~Span() { if (on) { hipEventRecord(b, st); ctx->spans.push_back({ id, a, b }); } }
};
struct MarkGuard { svo_ctx* c; ~MarkGuard() { mark_stream(c); } };
struct IdleGuard { DevCtx* d; ~IdleGuard() { memset(&d->idle, 0, sizeof(d->idle)); } };

// ---- the front ends' buffers ------------------------------------------------------------------------------------------------------
template <typename T>
static hipError_t lk_realloc(T** p, size_t n)
{
    if (*p) { (void)hipFree(*p); *p = nullptr; }
    return hipMalloc((void**)p, n * sizeof(T));
}
// the first error of a run of allocations (every one of them is made)
static inline hipError_t first_error(std::initializer_list<hipError_t> all)
{
    for (hipError_t e : all) if (e != hipSuccess) return e;
    return hipSuccess;
}
// the on-demand buffers of svo_lk_track and svo_gftt_detect: where `cap` is short of `n`, `alloc` reallocates what the capacity stands
// for.  A failed growth leaves the capacity at 0, so that the next call allocates afresh
template <typename N, typename F>
static hipError_t grow(N& cap, N n, F alloc)
{
    if (n <= cap) return hipSuccess;
    cap = 0;
    const hipError_t e = alloc();
    if (e == hipSuccess) cap = n;
    return e;
}

// ---- svo_lk.hip -------------------------------------------------------------------------------------------------------------------
// the tracking launch (rows: k_lk_track_row) and, under fb_max > 0, the way back: the same kernel with the image roles swapped, from
// the results to the points they came from
void enqueue_lk_track(const LkTrackArgs& a, bool rows, hipStream_t st);

// ---- svo_klt.hip ------------------------------------------------------------------------------------------------------------------
void klt_free(svo_ctx* ctx);                           // svo_destroy drops the front end's buffers with the context
