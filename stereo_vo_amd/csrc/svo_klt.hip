// svo_klt.hip -- the resident KLT front end: svo_klt_enable .. svo_klt_step, the RANSAC gate with svo_ransac_tracked, the pose prediction,
// the stereo re-association and the resident top-up (svo_hip.h; the decisions: klt_call.hpp; the kernels: k_klt.hip, k_lk.hip, k_gftt.hip
// and k_klt_predict in k_gn.hip).  No kernel lives here: the unit uses the HIP runtime and the launchers.
#include "svo_ctx.hpp"
#include <stdio.h>
#include <algorithm>

using namespace svo_call;

// ---- the resident KLT front end (svo_hip.h; the decisions: klt_call.hpp, the kernels: k_klt.hip and k_lk.hip) ----------------------
// a device buffer of the front end (owned: svo_ctx::klt_bufs) or of the top-up (topup_bufs): allocated, and its address noted in the
// list its group is freed from
template <typename T>
static hipError_t klt_alloc(std::vector<void**>& owned, T** p, size_t n)
{
    const hipError_t e = lk_realloc(p, n);
    if (e == hipSuccess) owned.push_back((void**)p);
    return e;
}
// the two buffers of a mode 1 (prediction, stereo): both or neither
template <typename A, typename B>
static hipError_t klt_alloc_both(svo_ctx* ctx, A** a, size_t na, B** b, size_t nb)
{
    std::vector<void**> both;
    const hipError_t e = first_error({ klt_alloc(both, a, na), klt_alloc(both, b, nb) });
    if (e == hipSuccess) ctx->klt_bufs.insert(ctx->klt_bufs.end(), both.begin(), both.end());
    else { (void)hipGetLastError(); for (void** p : both) { (void)hipFree(*p); *p = nullptr; } }
    return e;
}
static void free_bufs(std::vector<void**>& owned)
{
    for (void** p : owned) { if (*p) (void)hipFree(*p); *p = nullptr; }
    owned.clear();
}
static void topup_free(svo_ctx* ctx) { free_bufs(ctx->topup_bufs); ctx->klt.topup_enabled = false; }
// (the marks behind "klt_select", "klt_topup" and "klt_prune" go with the struct, as the booleans they replace did)
void klt_free(svo_ctx* ctx)
{
    free_bufs(ctx->klt_bufs); free_bufs(ctx->topup_bufs);
    ctx->kt_seen &= ~(1u << KG_KLT_SELECT | 1u << KG_KLT_TOPUP | 1u << KG_KLT_PRUNE);
    memset(&ctx->klt, 0, sizeof(ctx->klt));
}
static svo_klt::Caps klt_caps(const svo_ctx* ctx) { return { ctx->cfg.n_lanes, ctx->dc.max_kps, ctx->cfg.max_w, ctx->cfg.max_h }; }
static svo_klt::State klt_state(svo_ctx* ctx)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    return { ctx->klt.enabled, ctx->params_set, ctx->capturing || cs != hipStreamCaptureStatusNone, ctx->frame_parallel };
}
static LaneMask klt_all_lanes(const svo_ctx* ctx)
{
    LaneMask a, i; std::string why;
    parse_lane_mask(nullptr, false, ctx->cfg.n_lanes, a, i, why);
    return a;
}

// the live count of one lane's table, read back (the caller has waited for the stream)
static int klt_lane_count(svo_ctx* ctx, int lane, int& n)
{
    KltLaneDev kl;
    HIPCHECK(hipMemcpy(&kl, ctx->klt.dev.lane + lane, sizeof(kl), hipMemcpyDeviceToHost));
    n = kl.n;
    return SVO_OK;
}
// whether no lane's table holds a track: waits, then reads every lane's count back
static int klt_tables_empty(svo_ctx* ctx, bool& empty)
{
    if (const int rc = svo_wait(ctx)) return rc;
    empty = true;
    for (int l = 0, n = 0; l < ctx->cfg.n_lanes; l++) { if (const int rc = klt_lane_count(ctx, l, n)) return rc; if (n > 0) empty = false; }
    return SVO_OK;
}
// the pyramid geometry into the arguments of a kernel that builds job records
template <typename Args>
static void set_geometry(Args& a, const svo_lk::Geometry& g)
{
    a.nl = g.nl;
    for (int l = 0; l < g.nl; l++) { a.w[l] = g.w[l]; a.h[l] = g.h[l]; a.off[l] = g.off[l]; }
}

// svo_fpstream_create tells its member contexts what they are (svo_batch.cpp; not part of the public interface)
extern "C" void svo_internal_mark_frame_parallel(svo_ctx* ctx) { if (ctx) ctx->frame_parallel = true; }

extern "C" int svo_klt_enable(svo_ctx* ctx, const svo_klt_params* params)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    const svo_klt::Caps caps = klt_caps(ctx);
    const svo_klt_params p = svo_klt::klt_resolve_params(params, caps.max_kps);
    bool empty = true;
    if (k.enabled && memcmp(&p, &k.p, sizeof(p)) != 0) {                // other parameters: only while no lane holds a track
        if (const int rc = klt_tables_empty(ctx, empty)) return rc;
    }
    bool realloc = false;
    SVO_REFUSE(svo_klt::check_klt_enable(p, caps, k.enabled, k.p, empty, ctx->frame_parallel, realloc, why));
    if (!realloc) return SVO_OK;
    const svo_klt::Plan plan = svo_klt::plan_klt(p, caps);
    if (plan.select_lds_bytes > 60 * 1024) {
        char msg[160]; snprintf(msg, sizeof(msg), "max_h = %d: the selection keeps three row tables of max_h + 1 words in 60 KB of LDS", caps.max_h);
        ctx->last_error = msg; return SVO_ERR_UNSUPPORTED;
    }
    { const int rc = svo_wait(ctx); if (rc) return rc; }
    const int ransac = k.ransac;                            // (the mode outlives the buffers)
    klt_free(ctx);
    k.ransac = ransac;
    k.p = p; k.plan = plan;
    k.dev.n_lanes = caps.n_lanes; k.dev.cap = p.cap;
    const size_t NS = (size_t)plan.n_slots;
    std::vector<void**>& own = ctx->klt_bufs;
    for (int hf = 0; hf < 2; hf++) { HIPCHECK(klt_alloc(own, &k.dev.pts[hf], NS)); HIPCHECK(klt_alloc(own, &k.dev.meta[hf], (size_t)plan.meta_ints)); }
    HIPCHECK(klt_alloc(own, &k.dev.lane, (size_t)caps.n_lanes)); HIPCHECK(klt_alloc(own, &k.dev.appended, (size_t)1));
    HIPCHECK(klt_alloc(own, &k.dev.out, NS)); HIPCHECK(klt_alloc(own, &k.dev.status, NS)); HIPCHECK(klt_alloc(own, &k.dev.err, NS));
    HIPCHECK(klt_alloc(own, &k.d_pyr, (size_t)plan.pyr_bytes));
    HIPCHECK(klt_alloc(own, &k.d_pyr_jobs, (size_t)plan.n_pyr_jobs)); HIPCHECK(klt_alloc(own, &k.d_trk_jobs, (size_t)plan.n_trk_jobs));
    HIPCHECK(klt_alloc(own, &k.d_stage, 2 * (size_t)p.cap));
    HIPCHECK(hipMemsetAsync(k.dev.status, 0, NS, ctx->stream));
    HIPCHECK(hipMemsetAsync(k.dev.out, 0, sizeof(float2) * NS, ctx->stream));
    const LaneMask all = klt_all_lanes(ctx);
    note_stream(ctx);
    launch_klt_clear(ctx->dc, k.dev, 0, all, ctx->stream);
    launch_klt_clear(ctx->dc, k.dev, 1, all, ctx->stream);
    mark_stream(ctx);
    HIPCHECK(hipGetLastError());
    k.enabled = true;
    return SVO_OK;
}

extern "C" int svo_klt_reset(svo_ctx* ctx, const uint64_t lanes[2])
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_klt_ready(klt_state(ctx), "svo_klt_reset", why));
    LaneMask active, idle; std::string why;
    if (!parse_lane_mask(lanes, false, ctx->cfg.n_lanes, active, idle, why)) { ctx->last_error = why; return SVO_ERR_ARG; }
    note_stream(ctx);
    launch_klt_clear(ctx->dc, k.dev, k.half, active, ctx->stream);
    mark_stream(ctx);
    for (int wd = 0; wd < 2; wd++) k.has_img.w[wd] &= ~active.w[wd];
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_klt_add_points(svo_ctx* ctx, int lane, const float* left_xy, const float* right_xy, int n)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_klt_lane_call(klt_state(ctx), "svo_klt_add_points", lane, n, n <= 0 || (left_xy && right_xy), klt_caps(ctx), why));
    if (n == 0) return 0;
    const int m = n < k.p.cap ? n : k.p.cap;                             // (what lies beyond cap cannot go in whatever the live count is)
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    HIPCHECK(hipMemcpyAsync(k.d_stage, left_xy, sizeof(float2) * (size_t)m, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(k.d_stage + k.p.cap, right_xy, sizeof(float2) * (size_t)m, hipMemcpyHostToDevice, st));
    launch_klt_append(k.dev, k.half, lane, k.d_stage, k.d_stage + k.p.cap, m, st);
    int appended = 0;
    HIPCHECK(hipMemcpyAsync(&appended, k.dev.appended, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipGetLastError());
    return appended;
}

extern "C" int svo_klt_get_tracks(svo_ctx* ctx, int lane, float* left_xy, float* right_xy, int32_t* ids, int32_t* age, int cap)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_klt_lane_call(klt_state(ctx), "svo_klt_get_tracks", lane, cap, true, klt_caps(ctx), why));
    { const int rc = svo_wait(ctx); if (rc) return rc; }
    int n = 0;
    if (const int rc = klt_lane_count(ctx, lane, n)) return rc;
    const int m = n < cap ? n : cap, C = k.p.cap;
    if (m <= 0) return n;
    const float2* pts = k.dev.pts[k.half] + (size_t)lane * 2 * C;
    const int* meta = k.dev.meta[k.half] + (size_t)lane * KLT_META * C;
    if (left_xy) HIPCHECK(hipMemcpy(left_xy, pts, sizeof(float2) * (size_t)m, hipMemcpyDeviceToHost));
    if (right_xy) HIPCHECK(hipMemcpy(right_xy, pts + C, sizeof(float2) * (size_t)m, hipMemcpyDeviceToHost));
    if (ids) HIPCHECK(hipMemcpy(ids, meta + KLT_ID * C, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    if (age) HIPCHECK(hipMemcpy(age, meta + KLT_AGE * C, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    return n;
}

// steps 1 and 4 of a step for the lanes of `active`: the shift (k_begin_frame as a svo_process call without a run bit launches it, with
// that call's host bookkeeping) and the selection.  fresh: the lanes whose points stand as they are
static int klt_shift(svo_ctx* ctx, const LaneMask& active, const LaneMask& idle, hipStream_t st)
{
    DevCtx& d = ctx->dc;
    const FrameCall shift = make_frame_call(0, ctx->params, ctx->faster_anms);
    SadStep step = sad_window_step(ctx->sad, idle, shift);              // (no SAD stage runs: never a bad lane)
    ctx->sad = std::move(step.next);
    ctx->frame_active = active; ctx->frame_active_set = true;
    for (int wd = 0; wd < 2; wd++) ctx->imported.w[wd] &= ~active.w[wd];
    d.fast_th = ctx->fast_th; d.orb_th = ctx->orb_th; d.det_ahead = 0;
    { Span s(ctx, KT_BEGIN); launch_begin_frame(d, nullptr, 0, step.drop_prev, st); }
    return SVO_OK;
}
static void klt_select(svo_ctx* ctx, const LaneMask& active, const LaneMask& fresh, hipStream_t st)
{
    svo_ctx::Klt& k = ctx->klt; const DevCtx& d = ctx->dc;
    KltSelectArgs a; memset(&a, 0, sizeof(a));
    a.t = k.dev; a.half = k.half; a.fresh = fresh;
    a.max_dy = k.p.max_dy; a.min_disp = k.p.min_disp; a.max_disp = k.p.max_disp; a.kp_size = (float)k.p.lk.win;
    a.H = std::max(0, std::min(d.oh[0], d.max_h));
    { Span s(ctx, KT_KLT_SELECT); launch_klt_select(d, a, st); }
    k.half ^= 1; ctx->seen(KG_KLT_SELECT);
    for (int l = 0; l < d.n_lanes; l++) if (lane_in(active, l)) ctx->sad.cur[(size_t)l] = 0;      // lists without an image behind them: no SAD windows
}
// between the selection and stage 5, under svo_klt_set_ransac: the RANSAC on the tracked pairs the selection wrote, for the step's active
// lanes (DevCtx.idle is the step's); mode 2: the rejected tracks then leave the live half
static void klt_ransac_gate(svo_ctx* ctx, hipStream_t st)
{
    svo_ctx::Klt& k = ctx->klt;
    if (k.ransac == svo_klt::KLT_RANSAC_OFF) return;
    enqueue_ransac_tracked(ctx, st);
    if (k.ransac == svo_klt::KLT_RANSAC_PRUNE) { Span s(ctx, KT_KLT_PRUNE); launch_klt_prune(ctx->dc, k.dev, k.half, st); ctx->seen(KG_KLT_PRUNE); }
}

extern "C" int svo_klt_set_ransac(svo_ctx* ctx, int mode)
{
    SVO_ENTER(ctx);
    SVO_REFUSE(svo_klt::check_klt_set_ransac(klt_state(ctx), mode, why));
    ctx->klt.ransac = mode;
    return SVO_OK;
}
extern "C" int svo_klt_get_ransac(const svo_ctx* ctx) { return ctx ? ctx->klt.ransac : SVO_ERR_ARG; }

// ---- the pose prediction of the front end (svo_hip.h; the decisions: klt_call.hpp; the kernel: k_klt_predict in k_gn.hip) ----
// the guesses for the table as it stands: the lanes of `tracks` may predict; only_lane >= 0: that lane alone; delta6: the caller's
// increment and `valid` in place of the lanes' records (svo_debug_klt_predict)
static void klt_predict(svo_ctx* ctx, const LaneMask& tracks, int only_lane, const double* delta6, int valid, hipStream_t st)
{
    svo_ctx::Klt& k = ctx->klt;
    KltPredictArgs a; memset(&a, 0, sizeof(a));
    a.t = k.dev; a.half = k.half;
    a.guess = k.d_guess; a.used = k.d_gused;
    a.tracks = tracks;
    a.x_max = (float)(k.w - 1); a.y_max = (float)(k.h - 1);
    a.only_lane = only_lane;
    if (delta6) { a.forced = 1; a.forced_valid = valid; for (int i = 0; i < 6; i++) a.forced_delta[i] = delta6[i]; }
    { Span s(ctx, KT_KLT_PREDICT); launch_klt_predict(ctx->dc, a, st); }
    ctx->seen(KG_KLT_PREDICT);
}

extern "C" int svo_klt_set_prediction(svo_ctx* ctx, int mode)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    bool alloc = false;
    SVO_REFUSE(svo_klt::check_klt_set_prediction(klt_state(ctx), mode, k.d_guess != nullptr, alloc, why));
    if (alloc) {
        const svo_klt::PredictPlan plan = svo_klt::plan_predict(k.p, klt_caps(ctx));
        const hipError_t e = klt_alloc_both(ctx, &k.d_guess, (size_t)plan.n_guess, &k.d_gused, (size_t)plan.n_used);
        HIPCHECK(e);                                        // the mode stays as it was
    }
    k.predict = mode;
    return SVO_OK;
}
extern "C" int svo_klt_get_prediction(const svo_ctx* ctx) { return ctx ? ctx->klt.predict : SVO_ERR_ARG; }

// ---- the stereo re-association of the front end (svo_hip.h; the decisions: klt_call.hpp; the kernels: k_lk_track_row, k_klt_row_guess) ----
extern "C" int svo_klt_set_stereo(svo_ctx* ctx, int mode)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    bool alloc = false;
    SVO_REFUSE(svo_klt::check_klt_set_stereo(klt_state(ctx), mode, k.d_row_jobs != nullptr, alloc, why));
    if (alloc) {
        const svo_klt::StereoPlan plan = svo_klt::plan_stereo(k.p, klt_caps(ctx));
        const hipError_t e = klt_alloc_both(ctx, &k.d_row_jobs, (size_t)plan.n_jobs, &k.d_row_guess, (size_t)plan.n_guess);
        HIPCHECK(e);                                        // the mode stays as it was
    }
    k.stereo = mode;
    return SVO_OK;
}
extern "C" int svo_klt_get_stereo(const svo_ctx* ctx) { return ctx ? ctx->klt.stereo : SVO_ERR_ARG; }

// svo_klt_predicted and svo_debug_klt_predict: the kernel on one lane, then the lane's count and its guesses back
static int klt_predict_lane(svo_ctx* ctx, const char* entry, int lane, const double* delta6, bool forced, int valid, float* left_xy, float* right_xy, uint8_t* used, int cap)
{
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_klt_predict_call(klt_state(ctx), entry, k.predict, lane, cap, !forced || delta6 != nullptr, klt_caps(ctx), why));
    { const int rc = svo_wait(ctx); if (rc) return rc; }
    LaneMask tracks; memset(&tracks, 0, sizeof(tracks));
    if (lane_in(k.has_img, lane)) tracks.w[lane >> 6] = 1ull << (lane & 63);
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    klt_predict(ctx, tracks, lane, forced ? delta6 : nullptr, valid, st);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(st));
    int live = 0;
    if (const int rc = klt_lane_count(ctx, lane, live)) return rc;
    const int C = k.p.cap, n = live < C ? live : C, m = n < cap ? n : cap;
    if (m <= 0) return n;
    const float2* g = k.d_guess + (size_t)lane * 2 * C;
    if (left_xy) HIPCHECK(hipMemcpy(left_xy, g, sizeof(float2) * (size_t)m, hipMemcpyDeviceToHost));
    if (right_xy) HIPCHECK(hipMemcpy(right_xy, g + C, sizeof(float2) * (size_t)m, hipMemcpyDeviceToHost));
    if (used) HIPCHECK(hipMemcpy(used, k.d_gused + (size_t)lane * C, (size_t)m, hipMemcpyDeviceToHost));
    return n;
}

extern "C" int svo_klt_predicted(svo_ctx* ctx, int lane, float* left_xy, float* right_xy, uint8_t* used, int cap)
{
    SVO_ENTER(ctx);
    return klt_predict_lane(ctx, "svo_klt_predicted", lane, nullptr, false, 0, left_xy, right_xy, used, cap);
}

extern "C" int svo_debug_klt_predict(svo_ctx* ctx, int lane, const double* delta6, int valid, float* left_xy, float* right_xy, uint8_t* used, int cap)
{
    SVO_ENTER(ctx);
    return klt_predict_lane(ctx, "svo_debug_klt_predict", lane, delta6, true, valid, left_xy, right_xy, used, cap);
}

extern "C" int svo_ransac_tracked(svo_ctx* ctx, const uint64_t lanes[2])
{
    SVO_ENTER(ctx);
    LaneMask active, idle;
    SVO_REFUSE(svo_klt::check_ransac_tracked(ctx->params_set, ctx->geom_ready, klt_state(ctx).capturing, lanes, ctx->cfg.n_lanes, active, idle, why));
    if (!lane_any(active)) return SVO_OK;                   // nobody takes part: nothing is enqueued
    DevCtx& d = ctx->dc;
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    d.idle = idle;
    IdleGuard idle_guard{ &d };
    enqueue_ransac_tracked(ctx, st);
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_klt_step(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, const uint64_t lanes[2])
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    const svo_klt::Caps caps = klt_caps(ctx);
    LaneMask active, idle; int w = 0, h = 0;
    SVO_REFUSE(svo_klt::check_klt_step(frames, flags, lanes, caps, klt_state(ctx), active, idle, w, h, why));
    if (!lane_any(active)) return SVO_OK;                   // nobody takes part: nothing is enqueued
    const FrameCall opt = make_frame_call(SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT, ctx->params, ctx->faster_anms);
    SVO_REFUSE(check_frame_call(opt, ctx->params, active, nullptr, why));
    { const int rc = ensure_geometry(ctx, w, h); if (rc) return rc; }
    DevCtx& d = ctx->dc;
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    d.idle = idle;
    IdleGuard idle_guard{ &d };
    // 0. under svo_klt_set_prediction(1): the first guesses of the lanes that will track, AHEAD of the shift -- k_begin_frame starts the
    //    lanes' records afresh, and the prediction reads them as the last step left them (images of another size track nothing)
    if (k.predict == svo_klt::KLT_PREDICT_POSE) {
        LaneMask tracks; memset(&tracks, 0, sizeof(tracks));
        if (w == k.w && h == k.h) for (int wd = 0; wd < 2; wd++) tracks.w[wd] = active.w[wd] & k.has_img.w[wd];
        klt_predict(ctx, tracks, -1, nullptr, 0, st);
    }
    // 1. the shift
    { const int rc = klt_shift(ctx, active, idle, st); if (rc) return rc; }
    // 2. the new pair of every active lane into the parity its last pair did not go to; images of another size than the last step's
    //    cannot be tracked from it
    if (w != k.w || h != k.h) { memset(&k.has_img, 0, sizeof(k.has_img)); k.w = w; k.h = h; }
    const svo_lk::Geometry g = svo_klt::klt_geometry(k.p, w, h);
    const hipMemcpyKind kind = (flags & SVO_FLAG_DEVICE_IMAGES) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    LaneMask fresh, empty = idle;
    bool any_tracks = false;
    for (int wd = 0; wd < 2; wd++) { k.parity.w[wd] ^= active.w[wd]; fresh.w[wd] = active.w[wd] & ~k.has_img.w[wd]; empty.w[wd] |= fresh.w[wd]; any_tracks |= (active.w[wd] & k.has_img.w[wd]) != 0; }
    for (int l = 0; l < d.n_lanes; l++) {
        if (!lane_in(active, l)) continue;
        for (int sd = 0; sd < 2; sd++) {
            const svo_image& im = sd ? frames[l].right : frames[l].left;
            uint8_t* block = k.d_pyr + ((long long)((lane_in(k.parity, l) ? 1 : 0) * d.n_lanes + l) * 2 + sd) * k.plan.img_stride;
            HIPCHECK(hipMemcpy2DAsync(block, (size_t)w, im.data, (size_t)im.stride, (size_t)w, (size_t)h, kind, st));
        }
    }
    KltJobArgs ja; memset(&ja, 0, sizeof(ja));
    const bool rows = k.stereo == svo_klt::KLT_STEREO_ROW;
    ja.pyr_jobs = k.d_pyr_jobs; ja.trk_jobs = k.d_trk_jobs; ja.row_jobs = rows ? k.d_row_jobs : nullptr; ja.pyr = k.d_pyr; ja.img_stride = k.plan.img_stride;
    ja.n_lanes = d.n_lanes; ja.cap = k.p.cap;
    set_geometry(ja, g);
    ja.parity = k.parity; ja.empty = empty; ja.idle = idle;
    { Span s(ctx, KT_LK_PYRDOWN); launch_klt_jobs(ja, k.predict == svo_klt::KLT_PREDICT_POSE ? 1 : 0, st); for (int l = 1; l < g.nl; l++) launch_lk_pyrdown(k.d_pyr_jobs, d.n_lanes, l, g.w[l], g.h[l], st); }
    // 3. one tracking launch over every lane's two jobs (and the way back under fb_max); no lane has a last pair: nothing to track
    if (any_tracks) {
        const float2* guess = k.predict == svo_klt::KLT_PREDICT_POSE ? k.d_guess : nullptr;                     // (read for records with has_init)
        const LkTrackArgs a{ k.d_trk_jobs, 2 * d.n_lanes, 2 * d.n_lanes * k.p.cap, k.dev.pts[k.half], guess, k.dev.out, k.dev.status, k.dev.err, k.p.lk, 0, ctx->lk_photo };
        Span s(ctx, KT_LK_TRACK);
        enqueue_lk_track(a, false, st);
    }
    // 3b. under svo_klt_set_stereo(1) the right records of 3 were empty: the right partner of every left result is found in the NEW pair
    //     along the row (and back under fb_max), from guesses formed on the device.  A lane without a last pair takes part: its left
    //     points stand (k_klt_row_guess writes them as results with status 1), so the selection has no fresh lane to treat apart
    if (rows) {
        KltRowGuessArgs ga; memset(&ga, 0, sizeof(ga));
        ga.t = k.dev; ga.half = k.half; ga.guess = k.d_row_guess; ga.active = active; ga.fresh = fresh;
        const int C = k.p.cap;
        // lane l: slots [2 l C, 2 l C + C), results C behind
        const LkTrackArgs a{ k.d_row_jobs, d.n_lanes, (2 * d.n_lanes - 1) * C, k.dev.out, k.d_row_guess, k.dev.out + C, k.dev.status + C, k.dev.err + C, k.p.lk, 0, ctx->lk_photo };
        Span s(ctx, KT_LK_TRACK_ROW);
        launch_klt_row_guess(ga, st);
        enqueue_lk_track(a, true, st);
        ctx->seen(KG_LK_TRACK_ROW);
        memset(&fresh, 0, sizeof(fresh));
    }
    // 4. the selection
    klt_select(ctx, active, fresh, st);
    klt_ransac_gate(ctx, st);
    for (int wd = 0; wd < 2; wd++) k.has_img.w[wd] |= active.w[wd];
    // 5. stage 5.  The recipe's stage-5 call starts the lane's record afresh (k_begin_frame), the gate's counters included: a gated
    //    step that optimises leaves them at zero as well, one that does not leaves them standing
    if (flags & SVO_RUN_OPTIMIZE) {
        if (k.ransac != svo_klt::KLT_RANSAC_OFF) { Span s(ctx, KT_RANSAC_FEED); launch_ransac_stats_clear(d, st); }
        enqueue_optimize(ctx, opt, st);
    }
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_debug_klt_select(svo_ctx* ctx, int lane, const float* left_xy, const float* right_xy, const uint8_t* status_l, const uint8_t* status_r, int n)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_klt_lane_call(klt_state(ctx), "svo_debug_klt_select", lane, n, n <= 0 || (left_xy && right_xy && status_l && status_r), klt_caps(ctx), why));
    if (!ctx->geom_ready) { ctx->last_error = "svo_debug_klt_select: no geometry yet: the row tables need the image size of a step or of put lists"; return SVO_ERR_STATE; }
    { const int rc = svo_wait(ctx); if (rc) return rc; }
    int live = 0;
    if (const int rc = klt_lane_count(ctx, lane, live)) return rc;
    if (n != live) { char msg[128]; snprintf(msg, sizeof(msg), "svo_debug_klt_select: n = %d, the lane's table holds %d tracks", n, live); ctx->last_error = msg; return SVO_ERR_ARG; }
    const uint64_t words[2] = { lane < 64 ? 1ull << lane : 0ull, lane >= 64 ? 1ull << (lane - 64) : 0ull };
    LaneMask active, idle, fresh; std::string why;
    parse_lane_mask(words, true, ctx->cfg.n_lanes, active, idle, why);
    memset(&fresh, 0, sizeof(fresh));
    DevCtx& d = ctx->dc;
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    const size_t C = (size_t)k.p.cap, o = (size_t)(2 * lane) * C;
    if (n > 0) {
        HIPCHECK(hipMemcpyAsync(k.dev.out + o, left_xy, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(k.dev.out + o + C, right_xy, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(k.dev.status + o, status_l, (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(k.dev.status + o + C, status_r, (size_t)n, hipMemcpyHostToDevice, st));
    }
    d.idle = idle;
    IdleGuard idle_guard{ &d };
    { const int rc = klt_shift(ctx, active, idle, st); if (rc) return rc; }
    klt_select(ctx, active, fresh, st);
    klt_ransac_gate(ctx, st);
    HIPCHECK(hipStreamSynchronize(st));                      // the caller's arrays are free
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

// ---- the resident top-up of the front end (svo_hip.h; the decisions: klt_call.hpp; the kernels: k_klt.hip around k_gftt.hip and k_lk.hip) ----
static svo_klt::TopupCaps topup_caps(const svo_ctx* ctx)
{
    const int cap = ctx->klt.enabled ? ctx->klt.p.cap : std::min(1024, ctx->dc.max_kps);
    return { cap, ctx->cfg.max_cand };
}
extern "C" void svo_klt_topup_default_params(const svo_ctx* ctx, svo_klt_topup_params* p)
{
    if (!p) return;
    *p = svo_klt::topup_default_params(ctx ? topup_caps(ctx).cap : 1024);
}

extern "C" int svo_klt_topup_enable(svo_ctx* ctx, const svo_klt_topup_params* params)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    const svo_klt::Caps caps = klt_caps(ctx);
    const svo_klt::TopupCaps tc = topup_caps(ctx);
    const svo_klt_topup_params p = params ? *params : svo_klt::topup_default_params(tc.cap);
    const bool has_run = ctx->has_seen(KG_KLT_TOPUP);        // a top-up has run
    bool empty = true;
    if (k.enabled && k.topup_enabled && has_run && memcmp(&p, &k.tp, sizeof(p)) != 0) {          // other parameters after a top-up: only while no lane holds a track
        if (const int rc = klt_tables_empty(ctx, empty)) return rc;
    }
    bool realloc = false, adopt = false;
    SVO_REFUSE(svo_klt::check_topup_enable(p, caps, tc, klt_state(ctx), k.topup_enabled, k.tp, has_run, empty, realloc, adopt, why));
    if (adopt) { k.tp = p; return SVO_OK; }
    if (!realloc) return SVO_OK;
    const svo_klt::TopupPlan plan = svo_klt::plan_topup(k.p, caps, tc);
    { const int rc = svo_wait(ctx); if (rc) return rc; }
    // the response maps are the large buffer (4 bytes per pixel of n_lanes images of max_w x max_h): failing to get them is a capacity refusal
    std::vector<void**>& own = ctx->topup_bufs;
    if (klt_alloc(own, &k.d_tmap, (size_t)plan.map_floats) != hipSuccess) {
        (void)hipGetLastError(); k.d_tmap = nullptr;
        char msg[200]; snprintf(msg, sizeof(msg), "%d lanes of %d x %d need a response-map buffer of %lld bytes, which the device could not provide", caps.n_lanes, caps.max_w, caps.max_h, plan.map_floats * 4ll);
        ctx->last_error = msg; return SVO_ERR_CAPACITY;
    }
    const size_t NP = (size_t)plan.n_pts, NJ = (size_t)plan.n_jobs;
    const hipError_t e = first_error({
        klt_alloc(own, &k.d_tgjobs, NJ), klt_alloc(own, &k.d_tginfo, 4 * NJ), klt_alloc(own, &k.d_tinfo, 4 * NJ), klt_alloc(own, &k.d_tlk_jobs, NJ),
        klt_alloc(own, &k.d_tkeys, (size_t)plan.n_keys), klt_alloc(own, &k.d_titems, (size_t)plan.n_items), klt_alloc(own, &k.d_tstate, (size_t)plan.n_state),
        klt_alloc(own, &k.d_tcorners, NP), klt_alloc(own, &k.d_tinit, NP), klt_alloc(own, &k.d_tout, NP),
        klt_alloc(own, &k.d_tresp, NP), klt_alloc(own, &k.d_terr, NP), klt_alloc(own, &k.d_tstatus, NP) });
    if (e != hipSuccess) { (void)hipGetLastError(); topup_free(ctx); HIPCHECK(e); }
    // before the first call every lane's record says "not in the mask"
    std::vector<int> none(4 * NJ, 0);
    for (size_t l = 0; l < NJ; l++) none[4 * l + 3] = KLT_TOPUP_NOT_ASKED;
    HIPCHECK(hipMemcpy(k.d_tinfo, none.data(), sizeof(int) * none.size(), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(k.d_tginfo, 0, sizeof(int) * 4 * NJ));
    k.tp = p; k.tplan = plan; k.topup_enabled = true;
    return SVO_OK;
}

// the arguments of the three kernels for the front end's state as it is
static KltTopupArgs topup_args(svo_ctx* ctx, const LaneMask& lanes)
{
    svo_ctx::Klt& k = ctx->klt;
    KltTopupArgs a; memset(&a, 0, sizeof(a));
    a.t = k.dev; a.half = k.half;
    a.gjobs = k.d_tgjobs; a.ginfo = k.d_tginfo; a.tinfo = k.d_tinfo;
    a.map = k.d_tmap; a.map_stride = k.tplan.map_stride;
    a.lk_jobs = k.d_tlk_jobs; a.pyr = k.d_pyr; a.img_stride = k.plan.img_stride;
    a.cell = 1;
    if (k.w > 0 && k.h > 0) {
        const svo_lk::Geometry g = svo_klt::klt_geometry(k.p, k.w, k.h);
        set_geometry(a, g);
        const svo_gftt::Cells cells = svo_gftt::gftt_cells(k.w, k.h, k.tp.gftt.min_distance);
        a.cell = cells.cell; a.gw = cells.gw; a.gh = cells.gh;
    }
    a.below = k.tp.below; a.target = k.tp.target; a.init_disp = k.tp.init_disp;
    a.max_dy = k.p.max_dy; a.min_disp = k.p.min_disp; a.max_disp = k.p.max_disp;
    a.lanes = lanes; a.has_img = k.has_img; a.parity = k.parity;
    a.corners = k.d_tcorners; a.init = k.d_tinit; a.out = k.d_tout; a.status = k.d_tstatus;
    return a;
}

extern "C" int svo_klt_topup(svo_ctx* ctx, const uint64_t lanes[2])
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    LaneMask active;
    SVO_REFUSE(svo_klt::check_topup_call(klt_state(ctx), k.topup_enabled, lanes, klt_caps(ctx), active, why));
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    const KltTopupArgs a = topup_args(ctx, active);
    const int n_lanes = k.dev.n_lanes;
    bool any = false;                                        // a lane of the mask has a last pair: only then is there an image to look at
    for (int wd = 0; wd < 2; wd++) any |= (active.w[wd] & k.has_img.w[wd]) != 0;
    ctx->seen(KG_KLT_TOPUP);
    // 1. the detector's records, decided on the device from the live counts
    { Span s(ctx, KT_KLT_TOPUP); launch_klt_topup_jobs(a, st); }
    if (any && a.nl > 0) {
        // 2 .. 4. the detector as svo_gftt_detect launches it, on the top-up's own buffers; the seeds are the table's left points
        GfttArgs g;
        g.jobs = k.d_tgjobs; g.n_jobs = n_lanes; g.cand_cap = k.tplan.cand_cap; g.key_stride = k.tplan.key_stride; g.seed_cap = k.p.cap; g.items_stride = (int)k.tplan.items_stride;
        g.keys = k.d_tkeys; g.items = k.d_titems; g.state = k.d_tstate;
        g.seeds = k.dev.pts[k.half]; g.pts = k.d_tcorners; g.resp = k.d_tresp; g.info = k.d_tginfo; g.p = k.tp.gftt;
        { Span s(ctx, KT_GFTT_RESPONSE); launch_gftt_response(g, k.w, k.h, st); }
        { Span s(ctx, KT_GFTT_CANDIDATES); launch_gftt_candidates(g, k.w, k.h, st); }
        { Span s(ctx, KT_GFTT_SELECT); launch_gftt_select(g, st); }
        // 5. the tracking records and the first guesses
        { Span s(ctx, KT_KLT_TOPUP); launch_klt_topup_prepare(a, st); }
        // 6. left -> right over every lane (and the way back under fb_max), as svo_lk_track launches it
        const LkTrackArgs t{ k.d_tlk_jobs, n_lanes, n_lanes * k.p.cap, k.d_tcorners, k.d_tinit, k.d_tout, k.d_tstatus, k.d_terr, k.p.lk, 0, ctx->lk_photo };
        Span s(ctx, KT_LK_TRACK);
        enqueue_lk_track(t, false, st);
    }
    // 7. the gate and the append
    { Span s(ctx, KT_KLT_TOPUP); launch_klt_topup_append(a, -1, st); }
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_klt_topup_info(svo_ctx* ctx, int lane, int32_t info[4])
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_topup_lane_call(klt_state(ctx), k.topup_enabled, "svo_klt_topup_info", lane, 0, info != nullptr, klt_caps(ctx), topup_caps(ctx), why));
    { const int rc = svo_wait(ctx); if (rc) return rc; }
    HIPCHECK(hipMemcpy(info, k.d_tinfo + 4 * lane, sizeof(int32_t) * 4, hipMemcpyDeviceToHost));
    return SVO_OK;
}

extern "C" int svo_debug_klt_topup_append(svo_ctx* ctx, int lane, const float* left_xy, const float* right_xy, const uint8_t* status, int n)
{
    SVO_ENTER(ctx);
    svo_ctx::Klt& k = ctx->klt;
    SVO_REFUSE(svo_klt::check_topup_lane_call(klt_state(ctx), k.topup_enabled, "svo_debug_klt_topup_append", lane, n, n <= 0 || (left_xy && right_xy && status), klt_caps(ctx), topup_caps(ctx), why));
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    LaneMask none; memset(&none, 0, sizeof(none));
    const KltTopupArgs a = topup_args(ctx, none);
    const size_t o = (size_t)lane * (size_t)k.p.cap;
    if (n > 0) {
        HIPCHECK(hipMemcpyAsync(k.d_tcorners + o, left_xy, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(k.d_tout + o, right_xy, sizeof(float2) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(k.d_tstatus + o, status, (size_t)n, hipMemcpyHostToDevice, st));
    }
    // the records the kernel reads: n corners, no overflow, the lane takes part
    const int ginfo[4] = { n, n, 0, 0 }, tinfo[4] = { 0, 0, 0, KLT_TOPUP_OK };
    HIPCHECK(hipMemcpyAsync(k.d_tginfo + 4 * lane, ginfo, sizeof(ginfo), hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(k.d_tinfo + 4 * lane, tinfo, sizeof(tinfo), hipMemcpyHostToDevice, st));
    ctx->seen(KG_KLT_TOPUP);
    { Span s(ctx, KT_KLT_TOPUP); launch_klt_topup_append(a, lane, st); }
    HIPCHECK(hipStreamSynchronize(st));                      // the caller's arrays (and the two records above) are free
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}
