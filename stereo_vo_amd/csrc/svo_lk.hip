// svo_lk.hip -- pyramidal Lucas-Kanade tracking on caller lists: svo_lk_track, svo_lk_track_rows, svo_lk_set_photometric, svo_debug_lk_get_level
// (svo_hip.h; the decisions: lk_call.hpp, the kernels: k_lk.hip).  No kernel lives here: the unit uses the HIP runtime and the launchers.
#include "svo_ctx.hpp"

void enqueue_lk_track(const LkTrackArgs& a, bool rows, hipStream_t st)
{
    const int ppl = svo_lk::lk_pixels_per_lane(a.p.win);
    const auto launch = [&](const LkTrackArgs& x) { if (rows) launch_lk_track_row(x, ppl, st); else launch_lk_track(x, ppl, st); };
    launch(a);
    if (a.p.fb_max > 0.0f) {
        LkTrackArgs b = a;
        b.pts = a.out; b.aux = a.pts; b.out = nullptr; b.err = nullptr; b.backward = 1;
        launch(b);
    }
}

// svo_lk_track and svo_lk_track_rows: one call, the tracker apart (rows: k_lk_track_row, counted under its own name)
static int lk_track_call(svo_ctx* ctx, const svo_lk_job* jobs, int n_jobs, const svo_lk_params* params, uint32_t flags, bool rows)
{
    SVO_ENTER(ctx);
    svo_lk_params p;
    if (params) p = *params; else svo_lk_default_params(&p);
    const svo_lk::Caps caps{ ctx->dc.max_kps, 4 * ctx->cfg.n_lanes * ctx->dc.oct_cap, ctx->cfg.max_w, ctx->cfg.max_h };
    SVO_REFUSE(svo_lk::check_lk_call(jobs, n_jobs, p, flags, caps, why));
    if (n_jobs == 0) return SVO_OK;
    const bool dev = (flags & SVO_FLAG_DEVICE_IMAGES) != 0;
    const svo_lk::Plan plan = svo_lk::plan_lk_call(jobs, n_jobs, p, dev);
    const size_t NP = (size_t)plan.n_pts;
    ctx->lk_jobs.clear();
    HIPCHECK(grow(ctx->lk_pyr_cap, (size_t)plan.pyr_bytes, [&] { return lk_realloc(&ctx->d_lk_pyr, (size_t)plan.pyr_bytes); }));
    HIPCHECK(grow(ctx->lk_jobs_cap, n_jobs, [&] { return lk_realloc(&ctx->d_lk_jobs, (size_t)n_jobs); }));
    HIPCHECK(grow(ctx->lk_pts_cap, plan.n_pts, [&] {
        return first_error({ lk_realloc(&ctx->d_lk_pts, NP), lk_realloc(&ctx->d_lk_init, NP), lk_realloc(&ctx->d_lk_out, NP), lk_realloc(&ctx->d_lk_status, NP), lk_realloc(&ctx->d_lk_err, NP) });
    }));
    ctx->seen(KG_LK);
    if (rows) ctx->seen(KG_LK_TRACK_ROW);
    const hipStream_t st = ctx->stream;
    // the job records; host images go to level 0 of their block, device images are read where they are
    std::vector<LkJobDev> recs((size_t)n_jobs);
    int lw[svo_lk::LK_MAX_LEVELS] = { 0 }, lh[svo_lk::LK_MAX_LEVELS] = { 0 };
    for (int j = 0; j < n_jobs; j++) {
        const svo_lk::Geometry& g = plan.geom[(size_t)j];
        LkJobDev& r = recs[(size_t)j];
        memset(&r, 0, sizeof(r));
        r.nl = g.nl; r.pt0 = plan.pt0[(size_t)j]; r.n = jobs[j].n; r.has_init = (jobs[j].n > 0 && jobs[j].init) ? 1 : 0;
        for (int l = 0; l < g.nl; l++) { r.w[l] = g.w[l]; r.h[l] = g.h[l]; if (g.w[l] > lw[l]) lw[l] = g.w[l]; if (g.h[l] > lh[l]) lh[l] = g.h[l]; }
        for (int s = 0; s < 2; s++) {
            const svo_image& im = s ? jobs[j].next : jobs[j].prev;
            uint8_t* block = ctx->d_lk_pyr + plan.img_off[(size_t)(2 * j + s)];
            for (int l = 1; l < g.nl; l++) { r.img[s][l] = block + g.off[l]; r.pitch[s][l] = g.w[l]; }
            if (dev) { r.img[s][0] = im.data; r.pitch[s][0] = (int)im.stride; }
            else {
                r.img[s][0] = block; r.pitch[s][0] = g.w[0];
                HIPCHECK(hipMemcpy2DAsync(block, (size_t)g.w[0], im.data, (size_t)im.stride, (size_t)g.w[0], (size_t)g.h[0], hipMemcpyHostToDevice, st));
            }
        }
    }
    HIPCHECK(hipMemcpyAsync(ctx->d_lk_jobs, recs.data(), sizeof(LkJobDev) * (size_t)n_jobs, hipMemcpyHostToDevice, st));
    std::vector<float> h_pts(2 * NP), h_init(plan.any_init ? 2 * NP : 0);
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].n <= 0) continue;
        const size_t o = 2 * (size_t)plan.pt0[(size_t)j], nb = sizeof(float) * 2 * (size_t)jobs[j].n;
        memcpy(h_pts.data() + o, jobs[j].pts, nb);
        if (jobs[j].init) memcpy(h_init.data() + o, jobs[j].init, nb);
    }
    if (NP) HIPCHECK(hipMemcpyAsync(ctx->d_lk_pts, h_pts.data(), sizeof(float) * 2 * NP, hipMemcpyHostToDevice, st));
    if (NP && plan.any_init) HIPCHECK(hipMemcpyAsync(ctx->d_lk_init, h_init.data(), sizeof(float) * 2 * NP, hipMemcpyHostToDevice, st));
    { Span s(ctx, KT_LK_PYRDOWN); for (int l = 1; l < plan.max_nl; l++) launch_lk_pyrdown(ctx->d_lk_jobs, n_jobs, l, lw[l], lh[l], st); }
    // (jobs, n_jobs, n_pts; pts, aux: the first guesses; out, status, err; the parameters; forward; the context's photometric mode)
    const LkTrackArgs a{ ctx->d_lk_jobs, n_jobs, plan.n_pts, ctx->d_lk_pts, ctx->d_lk_init, ctx->d_lk_out, ctx->d_lk_status, ctx->d_lk_err, p, 0, ctx->lk_photo };
    { Span s(ctx, rows ? KT_LK_TRACK_ROW : KT_LK_TRACK); enqueue_lk_track(a, rows, st); }
    HIPCHECK(hipGetLastError());
    std::vector<float> h_out(2 * NP), h_err(NP);
    std::vector<uint8_t> h_status(NP);
    if (NP) {
        HIPCHECK(hipMemcpyAsync(h_out.data(), ctx->d_lk_out, sizeof(float) * 2 * NP, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(h_status.data(), ctx->d_lk_status, NP, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(h_err.data(), ctx->d_lk_err, sizeof(float) * NP, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipStreamSynchronize(st));
    ctx->lk_jobs = recs;
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].n <= 0) continue;
        const size_t o = (size_t)plan.pt0[(size_t)j], n = (size_t)jobs[j].n;
        memcpy(jobs[j].next_pts, h_out.data() + 2 * o, sizeof(float) * 2 * n);
        memcpy(jobs[j].status, h_status.data() + o, n);
        if (jobs[j].err) memcpy(jobs[j].err, h_err.data() + o, sizeof(float) * n);
    }
    return SVO_OK;
}

extern "C" int svo_lk_track(svo_ctx* ctx, const svo_lk_job* jobs, int n_jobs, const svo_lk_params* params, uint32_t flags)
{
    return lk_track_call(ctx, jobs, n_jobs, params, flags, false);
}

extern "C" int svo_lk_track_rows(svo_ctx* ctx, const svo_lk_job* jobs, int n_jobs, const svo_lk_params* params, uint32_t flags)
{
    return lk_track_call(ctx, jobs, n_jobs, params, flags, true);
}

// svo_lk_set_photometric / svo_lk_get_photometric: the mode every later LK launch of the context carries (LkTrackArgs::photo)
extern "C" int svo_lk_set_photometric(svo_ctx* ctx, int mode)
{
    SVO_ENTER(ctx);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(ctx->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    SVO_REFUSE(svo_lk::check_lk_set_photometric(mode, ctx->capturing || cs != hipStreamCaptureStatusNone, why));
    ctx->lk_photo = mode;
    return SVO_OK;
}
extern "C" int svo_lk_get_photometric(const svo_ctx* ctx) { return ctx ? ctx->lk_photo : SVO_ERR_ARG; }

extern "C" int svo_debug_lk_get_level(svo_ctx* ctx, int job, int which, int level, uint8_t* out, int cap, int* w, int* h)
{
    if (ctx) use_device(ctx);
    if (!ctx || which < 0 || which > 1 || job < 0 || level < 0) return SVO_ERR_ARG;
    if ((size_t)job >= ctx->lk_jobs.size() || level >= ctx->lk_jobs[(size_t)job].nl) return 0;
    int rc = svo_wait(ctx); if (rc) return rc;
    const LkJobDev& r = ctx->lk_jobs[(size_t)job];
    if (w) *w = r.w[level]; if (h) *h = r.h[level];
    if (!out) return r.w[level] * r.h[level];
    if (cap < r.w[level] * r.h[level]) return SVO_ERR_CAPACITY;
    HIPCHECK(hipMemcpy2D(out, (size_t)r.w[level], r.img[which][level], (size_t)r.pitch[which][level], (size_t)r.w[level], (size_t)r.h[level], hipMemcpyDeviceToHost));
    return r.w[level] * r.h[level];
}
