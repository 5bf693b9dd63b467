// svo_gftt.hip -- Shi-Tomasi corner detection on caller images: svo_gftt_detect, svo_debug_gftt_get_response
// (svo_hip.h; the decisions: gftt_call.hpp, the kernels: k_gftt.hip).  No kernel lives here: the unit uses the HIP runtime and the launchers.
#include "svo_ctx.hpp"
#include <stdio.h>

extern "C" int svo_gftt_detect(svo_ctx* ctx, const svo_gftt_job* jobs, int n_jobs, const svo_gftt_params* params, uint32_t flags)
{
    SVO_ENTER(ctx);
    svo_gftt_params p;
    if (params) p = *params; else svo_gftt_default_params(&p);
    const svo_gftt::Caps caps{ ctx->dc.max_kps, 4 * ctx->cfg.n_lanes * ctx->dc.oct_cap, ctx->cfg.max_w, ctx->cfg.max_h, ctx->cfg.max_cand };
    SVO_REFUSE(svo_gftt::check_gftt_call(jobs, n_jobs, p, flags, caps, why));
    if (n_jobs == 0) return SVO_OK;
    const bool dev = (flags & SVO_FLAG_DEVICE_IMAGES) != 0;
    const svo_gftt::Plan plan = svo_gftt::plan_gftt_call(jobs, n_jobs, p, dev);
    const int cand_cap = svo_gftt::gftt_cand_cap(ctx->cfg.max_cand), key_stride = svo_gftt::gftt_key_stride(cand_cap), seed_cap = ctx->dc.max_kps;
    const long long items_stride = (5ll * cand_cap + 2ll * seed_cap + 3) / 4 * 4;
    // the buffers.  The map buffer is the large one (4 bytes per pixel of the call): failing to get it is a capacity refusal, before
    // anything is enqueued
    ctx->gftt_jobs.clear();
    if (grow(ctx->gftt_map_cap, (size_t)plan.map_floats, [&] { return lk_realloc(&ctx->d_gftt_map, (size_t)plan.map_floats); }) != hipSuccess) {
        (void)hipGetLastError(); ctx->d_gftt_map = nullptr;
        char msg[200]; snprintf(msg, sizeof(msg), "%d jobs need a response-map buffer of %lld bytes, which the device could not provide", n_jobs, plan.map_floats * 4ll);
        ctx->last_error = msg; return SVO_ERR_CAPACITY;
    }
    HIPCHECK(grow(ctx->gftt_img_cap, (size_t)plan.img_bytes, [&] { return lk_realloc(&ctx->d_gftt_img, (size_t)plan.img_bytes); }));
    HIPCHECK(grow(ctx->gftt_jobs_cap, n_jobs, [&] {
        const size_t NJ = (size_t)n_jobs;
        return first_error({ lk_realloc(&ctx->d_gftt_jobs, NJ), lk_realloc(&ctx->d_gftt_info, 4 * NJ), lk_realloc(&ctx->d_gftt_keys, NJ * (size_t)key_stride),
                             lk_realloc(&ctx->d_gftt_state, NJ * (size_t)cand_cap), lk_realloc(&ctx->d_gftt_items, NJ * (size_t)items_stride) });
    }));
    HIPCHECK(grow(ctx->gftt_seeds_cap, plan.n_seeds, [&] { return lk_realloc(&ctx->d_gftt_seeds, (size_t)plan.n_seeds); }));
    HIPCHECK(grow(ctx->gftt_pts_cap, plan.n_pts, [&] { return first_error({ lk_realloc(&ctx->d_gftt_pts, (size_t)plan.n_pts), lk_realloc(&ctx->d_gftt_resp, (size_t)plan.n_pts) }); }));
    ctx->seen(KG_GFTT);
    const hipStream_t st = ctx->stream;
    // the job records; host images are copied tightly packed, device images are read where they are
    std::vector<GfttJobDev> recs((size_t)n_jobs);
    std::vector<float> h_seeds(2 * (size_t)plan.n_seeds);
    for (int j = 0; j < n_jobs; j++) {
        const svo_image& im = jobs[j].img;
        GfttJobDev& r = recs[(size_t)j];
        memset(&r, 0, sizeof(r));
        r.w = im.w; r.h = im.h; r.map = ctx->d_gftt_map + plan.map_off[(size_t)j];
        r.seed0 = plan.seed0[(size_t)j]; r.n_seeds = jobs[j].n_seeds; r.pts0 = plan.pts0[(size_t)j]; r.cap = jobs[j].cap;
        r.cell = plan.cells[(size_t)j].cell; r.gw = plan.cells[(size_t)j].gw; r.gh = plan.cells[(size_t)j].gh;
        if (dev) { r.img = im.data; r.pitch = (int)im.stride; }
        else {
            uint8_t* copy = ctx->d_gftt_img + plan.img_off[(size_t)j];
            r.img = copy; r.pitch = im.w;
            HIPCHECK(hipMemcpy2DAsync(copy, (size_t)im.w, im.data, (size_t)im.stride, (size_t)im.w, (size_t)im.h, hipMemcpyHostToDevice, st));
        }
        if (jobs[j].n_seeds > 0) memcpy(h_seeds.data() + 2 * (size_t)r.seed0, jobs[j].seeds, sizeof(float) * 2 * (size_t)jobs[j].n_seeds);
    }
    HIPCHECK(hipMemcpyAsync(ctx->d_gftt_jobs, recs.data(), sizeof(GfttJobDev) * (size_t)n_jobs, hipMemcpyHostToDevice, st));
    if (plan.n_seeds) HIPCHECK(hipMemcpyAsync(ctx->d_gftt_seeds, h_seeds.data(), sizeof(float) * 2 * (size_t)plan.n_seeds, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(ctx->d_gftt_info, 0, sizeof(int) * 4 * (size_t)n_jobs, st));
    GfttArgs a;
    a.jobs = ctx->d_gftt_jobs; a.n_jobs = n_jobs; a.cand_cap = cand_cap; a.key_stride = key_stride; a.seed_cap = seed_cap; a.items_stride = (int)items_stride;
    a.keys = ctx->d_gftt_keys; a.items = ctx->d_gftt_items; a.state = ctx->d_gftt_state;
    a.seeds = ctx->d_gftt_seeds; a.pts = ctx->d_gftt_pts; a.resp = ctx->d_gftt_resp; a.info = ctx->d_gftt_info; a.p = p;
    { Span s(ctx, KT_GFTT_RESPONSE); launch_gftt_response(a, plan.max_w, plan.max_h, st); }
    { Span s(ctx, KT_GFTT_CANDIDATES); launch_gftt_candidates(a, plan.max_w, plan.max_h, st); }
    { Span s(ctx, KT_GFTT_SELECT); launch_gftt_select(a, st); }
    HIPCHECK(hipGetLastError());
    std::vector<int> h_info(4 * (size_t)n_jobs);
    std::vector<float> h_pts(2 * (size_t)plan.n_pts), h_resp((size_t)plan.n_pts);
    HIPCHECK(hipMemcpyAsync(h_info.data(), ctx->d_gftt_info, sizeof(int) * 4 * (size_t)n_jobs, hipMemcpyDeviceToHost, st));
    if (plan.n_pts) {
        HIPCHECK(hipMemcpyAsync(h_pts.data(), ctx->d_gftt_pts, sizeof(float) * 2 * (size_t)plan.n_pts, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(h_resp.data(), ctx->d_gftt_resp, sizeof(float) * (size_t)plan.n_pts, hipMemcpyDeviceToHost, st));
    }
    HIPCHECK(hipStreamSynchronize(st));
    ctx->gftt_jobs = recs;
    for (int j = 0; j < n_jobs; j++) {
        const int* inf = h_info.data() + 4 * (size_t)j;
        const size_t o = (size_t)plan.pts0[(size_t)j], n = (size_t)(inf[0] < jobs[j].cap ? inf[0] : jobs[j].cap);
        if (n) {
            memcpy(jobs[j].pts, h_pts.data() + 2 * o, sizeof(float) * 2 * n);
            if (jobs[j].response) memcpy(jobs[j].response, h_resp.data() + o, sizeof(float) * n);
        }
        jobs[j].info[0] = (int32_t)n; jobs[j].info[1] = inf[1]; jobs[j].info[2] = inf[2];
    }
    return SVO_OK;
}

extern "C" int svo_debug_gftt_get_response(svo_ctx* ctx, int job, float* out, int cap, int* w, int* h)
{
    if (ctx) use_device(ctx);
    if (!ctx || job < 0) return SVO_ERR_ARG;
    if ((size_t)job >= ctx->gftt_jobs.size()) return 0;
    int rc = svo_wait(ctx); if (rc) return rc;
    const GfttJobDev& r = ctx->gftt_jobs[(size_t)job];
    if (w) *w = r.w; if (h) *h = r.h;
    if (!out) return r.w * r.h;
    if (cap < r.w * r.h) return SVO_ERR_CAPACITY;
    HIPCHECK(hipMemcpy(out, r.map, sizeof(float) * (size_t)r.w * (size_t)r.h, hipMemcpyDeviceToHost));
    return r.w * r.h;
}
