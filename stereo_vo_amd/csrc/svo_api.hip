// svo_api.hip -- the C-ABI of include/svo_hip.h: context, geometry, frame pipeline, getters.
//
// svo_process enqueues one frame of every lane on the context's stream as a fixed sequence of ~20 kernel
// launches; every data-dependent size (keypoint, pairing, track counts) stays in device memory, so there is no
// host synchronisation inside a frame and frames can be enqueued back to back.
#include "svo_ctx.hpp"
#include "state_format.hpp"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <mutex>
#include <map>
#include <memory>
#include <condition_variable>

// ---- profiler sections ---------------------------------------------------------------------------------------------------
// The reference brackets its stages with mrpt's CTimeLogger: m_profiler.enter / leave("processNewImagePair", "_stg1" ... "_stg5",
// "stg3.find_pairings", "stg4.track", ...: process_new_image_pair.cpp:79, 377; stage1_rectify.cpp:41-86; stage2_detect.cpp:392, 670;
// stage3_match_left_right.cpp:64-473; stage4_match_consecutive.cpp:76-800; stage5_optimization.cpp:398, 729).  Here the same names
// are roctx ranges around the ENQUEUE of each stage (the kernels run asynchronously: rocprofv3 --marker-trace --kernel-trace ties a
// kernel to the range it was launched in).  The roctx library is looked up at run time and only when asked for (SVO_ROCTX=1, or a
// rocprofv3 session: ROCP_TOOL_LIBRARIES is set), so libsvo_hip.so has no link-time dependency on the profiler SDK.
#include <dlfcn.h>
namespace {
struct RoctxApi {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    RoctxApi()
    {
        const char* e = getenv("SVO_ROCTX");
        if (e && e[0] == '0') return;
        if (!(e && e[0] == '1') && !getenv("ROCP_TOOL_LIBRARIES")) return;
        for (const char* name : { "librocprofiler-sdk-roctx.so.1", "librocprofiler-sdk-roctx.so", "libroctx64.so.4", "libroctx64.so" }) {
            void* h = dlopen(name, RTLD_LAZY | RTLD_GLOBAL);
            if (!h) continue;
            push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) return;
            push = nullptr; pop = nullptr;
        }
    }
};
RoctxApi& roctx_api() { static RoctxApi a; return a; }
struct Section {                                       // m_profiler.enter(name) ... leave(name)
    bool on;
    explicit Section(const char* name) : on(roctx_api().push != nullptr) { if (on) roctx_api().push(name); }
    ~Section() { if (on) roctx_api().pop(); }
    Section(const Section&) = delete; Section& operator=(const Section&) = delete;
};
}
extern "C" int svo_profiler_sections_enabled(void) { return roctx_api().push != nullptr; }

using namespace svo_call;
static void drop_graphs(svo_ctx* ctx);
static int dyn_fast_init(svo_ctx* ctx, int lane);
static int ensure_sad_buffers(svo_ctx* ctx);
static int sampler_table_acquire(svo_ctx* ctx, int nmax);
static void sampler_table_release(int device, int nmax);
void note_stream(svo_ctx* ctx)
{
    for (auto& u : ctx->used_streams) if (u.s == ctx->stream) { u.dirty = true; return; }
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;      // mark_stream then synchronises the stream itself
    ctx->used_streams.push_back({ ctx->stream, ev, true });
}
// record "everything enqueued so far" on the current stream (behind the last launch of an entry point, on its error exits too;
// never while capturing)
void mark_stream(svo_ctx* ctx)
{
    if (ctx->stream == ctx->stream0 && ctx->own_stream) return;  // the context's own stream is synchronised by handle
    for (auto& u : ctx->used_streams) if (u.s == ctx->stream) {
        if (u.ev) (void)hipEventRecord(u.ev, ctx->stream);
        else { (void)hipStreamSynchronize(ctx->stream); u.dirty = false; }   // no event to leave behind: wait now, while the handle is certainly alive
        return;
    }
}
// wait for what this context left on streams other than the current one
static hipError_t sync_foreign(svo_ctx* ctx)
{
    hipError_t first = hipSuccess;
    for (auto& u : ctx->used_streams) {
        if (!u.dirty || u.s == ctx->stream) continue;
        hipError_t e = hipSuccess;
        if (u.s == ctx->stream0 && ctx->own_stream) e = hipStreamSynchronize(u.s);
        else if (u.ev) e = hipEventSynchronize(u.ev);                    // (an entry without an event was synchronised when it was marked)
        if (first == hipSuccess) first = e;
        u.dirty = false;
    }
    return first;
}
// wait for everything this context has enqueued, on whichever stream (a caller that switched streams with
// svo_set_stream may have left work on the earlier ones)
static hipError_t sync_all(svo_ctx* ctx)
{
    hipError_t first = sync_foreign(ctx);
    if (ctx->up_ready) { const hipError_t e2 = hipStreamSynchronize(ctx->s_copy); if (first == hipSuccess) first = e2; }
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    if (first == hipSuccess) first = e;
    // everything is complete: forget the foreign streams the caller has switched away from (a host that makes a stream per frame
    // would otherwise leave one entry and one event behind per frame)
    size_t keep = 0;
    for (auto& u : ctx->used_streams) {
        u.dirty = false;
        if (u.s == ctx->stream || (u.s == ctx->stream0 && ctx->own_stream)) ctx->used_streams[keep++] = u;
        else if (u.ev) (void)hipEventDestroy(u.ev);
    }
    ctx->used_streams.resize(keep);
    return first;
}

static int align_up(int v, int a) { return (v + a - 1) / a * a; }

extern "C" void svo_config_defaults(svo_config* c)
{
    memset(c, 0, sizeof(*c));
    c->device = 0; c->n_lanes = 1; c->max_w = 1280; c->max_h = 960; c->max_kps = 4096; c->max_cand = 1 << 17; c->kernel_times = 0; c->max_octaves = 1; c->stream = nullptr;
}

extern "C" void svo_params_defaults(svo_params* p)
{
    memset(p, 0, sizeof(*p));
    p->nOctaves = 3;                                   // stage1_rectify.cpp:27-30
    p->detect_method = SVO_DM_ORB;                     // north-star selector (reference default dmFASTER, stage2_detect.cpp:45)
    p->non_maximal_suppression = 1; p->nmsMethod = SVO_NMS_STANDARD; p->min_distance = 3;   // stage2_detect.cpp:49-51
    p->orb_nfeats = 500; p->orb_nlevels = 8; p->minimum_ORB_response = 0.0;                 // stage2_detect.cpp:52-54
    p->fast_min_th = 5; p->fast_max_th = 30; p->initial_FAST_threshold = 20;                // stage2_detect.cpp:55-56
    p->match_method = SVO_SM_DESC_BF;                  // north-star selector (reference default smSAD, stage3:47)
    p->orb_max_distance = 40; p->orb_min_th = 30; p->orb_max_th = 100;                      // stage3_match_left_right.cpp:50-51
    p->enable_robust_1to1_match = 0; p->max_y_diff = 0;                                     // stage3_match_left_right.cpp:52-54
    p->ifm_method = SVO_IFM_DESC_BF; p->ifm_win_w = 16; p->ifm_win_h = 16; p->filter_fund_matrix = 0;   // H:610; no reference defaults (common.cpp:84)
    p->use_robust_kernel = 1; p->kernel_param = 3.0; p->max_iters = 100; p->initial_max_iters = 10;     // common.cpp:69-82
    p->min_mod_out_vector = 1e-3; p->max_incr_cost = 3; p->residual_threshold = 10.0; p->bad_tracking_th = 5;
    p->use_previous_pose_as_initial = 1; p->use_custom_initial_pose = 0;
    p->vo_use_matches_ids = 0;                         // process_new_image_pair.cpp:35
}

extern "C" const char* svo_strerror(int s)
{
    switch (s) {
        case SVO_OK: return "ok";
        case SVO_ERR_HIP: return "HIP runtime error (see svo_last_error)";
        case SVO_ERR_ARG: return "invalid argument";
        case SVO_ERR_UNSUPPORTED: return "configuration outside the supported hot path";
        case SVO_ERR_NO_DEVICE: return "no HIP device (this library has no CPU fallback)";
        case SVO_ERR_CAPACITY: return "context capacity exceeded";
        case SVO_ERR_STATE: return "call not valid in the current state";
        default: return "unknown status";
    }
}
extern "C" const char* svo_last_error(const svo_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }

extern "C" void svo_abi_sizes(int32_t* out)
{
    out[0] = sizeof(svo_keypoint); out[1] = sizeof(svo_dmatch); out[2] = sizeof(svo_stereo_camera);
    out[3] = sizeof(svo_params); out[4] = sizeof(svo_result); out[5] = sizeof(svo_config);
}

template <typename T>
static hipError_t dev_alloc(svo_ctx* ctx, T** p, size_t n)
{
    void* q = nullptr;
    hipError_t e = hipMalloc(&q, n * sizeof(T) + 256);
    if (e != hipSuccess) return e;
    e = hipMemset(q, 0, n * sizeof(T) + 256);
    if (e != hipSuccess) { hipFree(q); return e; }
    ctx->allocs.push_back(q);
    *p = (T*)q;
    return hipSuccess;
}

static void level_sizes(int w, int h, int nlevels, int* lw, int* lh, float* sc)
{
    for (int l = 0; l < nlevels; l++) {                      // same expression as oracle svo_oracle_pyramid_sizes
        const float sf = (float)pow(1.2, (double)l);
        sc[l] = sf; lw[l] = (int)lrintf((float)w / sf); lh[l] = (int)lrintf((float)h / sf);
    }
}

static long long pyramid_bytes(int w, int h, int nlevels)
{
    int lw[SVO_MAX_LEVELS], lh[SVO_MAX_LEVELS]; float sc[SVO_MAX_LEVELS];
    level_sizes(w, h, nlevels, lw, lh, sc);
    long long b = 0;
    for (int l = 1; l < nlevels; l++) b += (long long)align_up(lw[l], 64) * lh[l];
    return align_up((int)((b + 255) & ~255LL), 256);
}

// ---- the sampler's attempt table ---------------------------------------------------------------------------------------------
// cv::RNG from the seed RANSACPointSetRegistrator::run uses, (uint64)-1 -- state = (uint32)state * 4164903690 + (state >> 32), output
// (uint32)state --, rng.uniform(0, n) = next() % n, a draw that repeats an index of the same attempt is drawn again (getSubset); the
// collinearity rejection depends on the data and stays on the device.  The attempts depend on the point count n alone: tabulated once per
// process and nmax on the host (~0.1 s, 18 KB per n: 84 MB at max_kps 4096, about 310 MB at 16384) and uploaded ONCE per (device, nmax) -- three contexts of a
// batch used to hold three copies -- together with the generator's state at the end of every row, from which the device
// continues the stream when a lane needs more attempts than its row holds (rs_schedule_block).  The host mutex covers the maps only,
// not the upload of another device's copy.
namespace {
struct SamplerHost { std::vector<uint16_t> att; std::vector<uint64_t> state; };
struct SamplerDev { uint16_t* att = nullptr; uint64_t* state = nullptr; int refs = 0; bool ready = false; hipError_t err = hipSuccess; };
std::mutex g_sampler_mu;
std::map<int, std::shared_ptr<SamplerHost>> g_sampler_host;                 // by nmax
std::map<std::pair<int, int>, std::shared_ptr<SamplerDev>> g_sampler_dev;   // by (device, nmax)
std::condition_variable g_sampler_cv;
size_t sampler_row_off(int n) { return n < SVO_RS_SMALL_N ? (size_t)(n - 8) * SVO_RS_ATT_SMALL : (size_t)(SVO_RS_SMALL_N - 8) * SVO_RS_ATT_SMALL + (size_t)(n - SVO_RS_SMALL_N) * SVO_RS_ATT; }
std::shared_ptr<SamplerHost> sampler_build(int nmax)
{
    auto h = std::make_shared<SamplerHost>();
    h->att.assign(sampler_row_off(nmax + 1) * 8, 0);
    h->state.assign((size_t)nmax + 1, 0xFFFFFFFFFFFFFFFFULL);
    for (int n = 8; n <= nmax; n++) {
        uint64_t stt = 0xFFFFFFFFFFFFFFFFULL;
        uint16_t* row = h->att.data() + sampler_row_off(n) * 8;
        const int n_att = n < SVO_RS_SMALL_N ? SVO_RS_ATT_SMALL : SVO_RS_ATT;
        for (int a = 0; a < n_att; a++) {
            uint16_t* s7 = row + (size_t)a * 8;
            for (int i = 0; i < 7; i++) {
                for (;;) {
                    stt = (uint64_t)(uint32_t)stt * 4164903690ULL + (uint32_t)(stt >> 32);
                    const uint16_t v = (uint16_t)((uint32_t)stt % (uint32_t)n);
                    bool dup = false;
                    for (int k = 0; k < i; k++) dup = dup || s7[k] == v;
                    if (!dup) { s7[i] = v; break; }
                }
            }
        }
        h->state[(size_t)n] = stt;
    }
    return h;
}
}
static int sampler_table_acquire(svo_ctx* ctx, int nmax)
{
    const std::pair<int, int> key(ctx->cfg.device, nmax);
    std::shared_ptr<SamplerDev> dv; std::shared_ptr<SamplerHost> host; bool mine = false;
    {
        std::unique_lock<std::mutex> lock(g_sampler_mu);
        auto& slot = g_sampler_dev[key];
        if (!slot) { slot = std::make_shared<SamplerDev>(); mine = true; }
        dv = slot; dv->refs++;
        if (!mine) g_sampler_cv.wait(lock, [&] { return dv->ready; });      // another thread is uploading this very copy: wait for THAT one only
        else {
            auto& hs = g_sampler_host[nmax];
            if (!hs) hs = sampler_build(nmax);                               // (built under the lock: once per process and nmax)
            host = hs;
        }
    }
    if (mine) {                                                              // the upload runs WITHOUT the lock: contexts on other devices / of other sizes go on
        hipError_t e = hipMalloc((void**)&dv->att, host->att.size() * sizeof(uint16_t) + 256);
        if (e == hipSuccess) e = hipMalloc((void**)&dv->state, host->state.size() * sizeof(uint64_t) + 256);
        if (e == hipSuccess) e = hipMemcpy(dv->att, host->att.data(), host->att.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dv->state, host->state.data(), host->state.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
        std::lock_guard<std::mutex> lock(g_sampler_mu);
        dv->err = e; dv->ready = true;
        g_sampler_cv.notify_all();
    }
    if (dv->err != hipSuccess) { ctx->last_error = std::string("sampler table: ") + hipGetErrorString(dv->err); sampler_table_release(ctx->cfg.device, nmax); return SVO_ERR_HIP; }
    ctx->dc.rs_att = dv->att; ctx->dc.rs_att_state = (const unsigned long long*)dv->state; ctx->dc.rs_att_nmax = nmax;
    ctx->sampler_nmax = nmax;
    return SVO_OK;
}
static void sampler_table_release(int device, int nmax)
{
    std::lock_guard<std::mutex> lock(g_sampler_mu);
    auto it = g_sampler_dev.find(std::make_pair(device, nmax));
    if (it == g_sampler_dev.end()) return;
    if (--it->second->refs > 0) return;
    if (it->second->att) hipFree(it->second->att);
    if (it->second->state) hipFree(it->second->state);
    g_sampler_dev.erase(it);
}

extern "C" int svo_create(const svo_config* cfg, svo_ctx** out)
{
    if (!cfg || !out) return SVO_ERR_ARG;
    *out = nullptr;
    if (cfg->n_lanes < 1 || cfg->n_lanes > SVO_MAX_LANES || cfg->max_w < 64 || cfg->max_h < 64) return SVO_ERR_ARG;
    if (cfg->max_kps < 64 || cfg->max_kps > 16384 || (cfg->max_kps & (cfg->max_kps - 1))) return SVO_ERR_ARG;   // above 4096 the NMS / GN kernels keep their sort and hash arrays in global scratch
    if ((long long)cfg->max_w * cfg->max_h >= (1 << 24)) return SVO_ERR_UNSUPPORTED;      // position packs into 24 bits
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device >= ndev) return SVO_ERR_NO_DEVICE;
    svo_ctx* ctx = new svo_ctx();
    ctx->cfg = *cfg;
    svo_params_defaults(&ctx->params);
    ctx->fast_th = 20; ctx->orb_th = 60;                  // common.cpp:35-36
    ctx->klt_win = 4; ctx->d_cand64 = nullptr;            // stage2_detect.cpp:47
    ctx->dyn_fast = false; ctx->dyn_target = 10. / 1000.; ctx->d_fstats = nullptr;      // stage2_detect.cpp:46; update_dyn_thresholds = false (H:1020)
    ctx->faster_anms = false; ctx->d_fanms = nullptr; ctx->d_anms_list = nullptr; ctx->d_anms_pos = nullptr;
    ctx->sampler_nmax = 0;
    ctx->geom_ready = false; ctx->geom_once = false;
    ctx->d_ham_out = nullptr; ctx->d_ham_q = ctx->d_ham_t = nullptr; ctx->ham_cap_q = ctx->ham_cap_t = 0;
    ctx->lk_photo = 0; ctx->d_lk_pyr = nullptr; ctx->lk_pyr_cap = 0; ctx->d_lk_jobs = nullptr; ctx->lk_jobs_cap = 0; ctx->lk_pts_cap = 0;
    ctx->d_lk_pts = ctx->d_lk_init = ctx->d_lk_out = nullptr; ctx->d_lk_status = nullptr; ctx->d_lk_err = nullptr;
    ctx->d_gftt_map = nullptr; ctx->gftt_map_cap = 0; ctx->d_gftt_img = nullptr; ctx->gftt_img_cap = 0; ctx->d_gftt_jobs = nullptr; ctx->gftt_jobs_cap = 0;
    ctx->d_gftt_keys = nullptr; ctx->d_gftt_items = nullptr; ctx->d_gftt_state = nullptr; ctx->d_gftt_info = nullptr;
    ctx->d_gftt_seeds = nullptr; ctx->gftt_seeds_cap = 0; ctx->d_gftt_pts = nullptr; ctx->d_gftt_resp = nullptr; ctx->gftt_pts_cap = 0;
    memset(&ctx->klt, 0, sizeof(ctx->klt)); ctx->params_set = false; ctx->frame_parallel = false; ctx->kt_seen = 0;
    ctx->d_src = nullptr; ctx->src_pitch = 0; ctx->d_map_ptrs = nullptr; ctx->map_w = ctx->map_h = ctx->n_maps = 0;
    ctx->map_shared[0] = ctx->map_shared[1] = nullptr; ctx->d_rect_models = nullptr;
    memset(&ctx->imported, 0, sizeof(ctx->imported)); ctx->graph_replays = 0; ctx->capturing = false; ctx->frame_active_set = false; memset(&ctx->frame_active, 0, sizeof(ctx->frame_active)); ctx->use_graphs = false; ctx->d_anms = nullptr; ctx->post_event = nullptr; ctx->pose_cov = false; ctx->d_cov = nullptr; ctx->d_cov_mask = nullptr;
    ctx->landmarks = false; ctx->lmk_std = 1.0; ctx->d_lmk = nullptr; ctx->d_lmk_info = nullptr; ctx->d_lmk_cnt = nullptr;
    ctx->sad.cur.assign((size_t)cfg->n_lanes, 1); ctx->sad.prev.assign((size_t)cfg->n_lanes, 1); ctx->sad.drop.assign((size_t)cfg->n_lanes, 0);
    ctx->cip_ready = false; ctx->d_vals = nullptr; ctx->h_vals = nullptr; ctx->vals_bytes = 0;
    ctx->up_ready = false; ctx->up_slot = 0; ctx->det_slot = -1; ctx->s_copy = nullptr; ctx->slot_bytes = 0;
    for (int i = 0; i < 2; i++) { ctx->d_img0_ring[i] = nullptr; ctx->h_stage[i] = nullptr; ctx->ev_det_valid[i] = ctx->ev_h2d_valid[i] = false; }
    for (int i = 0; i < KT_COUNT; i++) { ctx->kt_total[i] = 0; ctx->kt_calls[i] = 0; }
    ctx->kt_mask = ~0ull;
    *out = ctx;                                           // so that the caller can read last_error and destroy
    knobs_read(&ctx->knobs, knobs_env);
    if (svo_ab_form_requested(ctx->knobs) && !svo_ab_kernels_built()) {
        ctx->last_error = "SVO_HAM_FP4=0 / SVO_DEBUG_MODE=14 / 52 ask for an A/B kernel form that this library was built without: load libsvo_hip_ab.so (SVO_HIP_LIB) or build with -DSVO_AB_KERNELS";
        return SVO_ERR_UNSUPPORTED;
    }
    HIPCHECK(hipSetDevice(cfg->device));
    if (cfg->stream) { ctx->stream = (hipStream_t)cfg->stream; ctx->own_stream = false; }
    else { HIPCHECK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    ctx->stream0 = ctx->stream;
    HIPCHECK(svo_upload_tables());
    DevCtx& d = ctx->dc;
    memset(&d, 0, sizeof(d));
    const int L = cfg->n_lanes, NI = 2 * L, MK = cfg->max_kps;
    const int OC = cfg->max_octaves < 1 ? 1 : (cfg->max_octaves > SVO_MAX_OCTAVES ? SVO_MAX_OCTAVES : cfg->max_octaves);
    const int NV = L * OC;                                  // lane-octaves
    d.n_lanes = L; d.n_img = NI; d.max_kps = MK; d.n_levels = SVO_MAX_LEVELS; d.oct_cap = OC; d.n_oct = 1; d.max_h = cfg->max_h;
    ctx->raw_cap_alloc = 2 * MK;
    ctx->pyr_bytes_alloc = pyramid_bytes(cfg->max_w, cfg->max_h, SVO_MAX_LEVELS);
    ctx->cand_total_alloc = (int)((long long)cfg->max_cand * 33 / 10) + 8 * 1024;
    ctx->rtab_alloc = 2 * (cfg->max_w + cfg->max_h) * SVO_MAX_LEVELS;
    ctx->img0_pitch_internal = align_up(cfg->max_w, 64);
    HIPCHECK(dev_alloc(ctx, &ctx->d_img0, (size_t)NI * ctx->img0_pitch_internal * cfg->max_h));
    HIPCHECK(dev_alloc(ctx, (uint8_t***)&d.img0, (size_t)NI));
    HIPCHECK(dev_alloc(ctx, &d.pyr, (size_t)NI * ctx->pyr_bytes_alloc));
    HIPCHECK(dev_alloc(ctx, &d.rtab, (size_t)ctx->rtab_alloc));
    // FAST tile table: the level tilings of an image of the largest size, all levels (scale 1.2: 3.3 x level 0; x1/2 octaves: 1.34 x)
    ctx->tile_tab_alloc = 4 * ((cfg->max_w / SVO_FT_W + 2) * (cfg->max_h / SVO_FT_H + 2)) + 64;
    HIPCHECK(dev_alloc(ctx, (uint4**)&d.fast_tiles, (size_t)ctx->tile_tab_alloc));
    HIPCHECK(dev_alloc(ctx, &d.cand_keys, (size_t)NI * ctx->cand_total_alloc));
    HIPCHECK(dev_alloc(ctx, &d.cand_cnt, (size_t)NI * SVO_MAX_LEVELS * SVO_CNT_STRIDE));
    HIPCHECK(dev_alloc(ctx, &d.fast_th_dyn, (size_t)NI * SVO_MAX_LEVELS * 4 + 32));
    d.fast_th_used = d.fast_th_dyn + (size_t)NI * SVO_MAX_LEVELS; d.redo_flag = d.fast_th_used + (size_t)NI * SVO_MAX_LEVELS;
    d.redo_list = d.redo_flag + (size_t)NI * SVO_MAX_LEVELS; d.redo_n = d.redo_list + (size_t)NI * SVO_MAX_LEVELS;
    HIPCHECK(dev_alloc(ctx, &d.lvl_pos, (size_t)NI * ctx->raw_cap_alloc));
    HIPCHECK(dev_alloc(ctx, &d.lvl_resp, (size_t)NI * ctx->raw_cap_alloc));
    d.sel_max = MK > 8192 ? 4 * SVO_SEL_MAX : (MK > 4096 ? 2 * SVO_SEL_MAX : SVO_SEL_MAX);
    HIPCHECK(dev_alloc(ctx, &d.sel_keys, (size_t)NI * SVO_MAX_LEVELS * d.sel_max));
    HIPCHECK(dev_alloc(ctx, &d.sel_resp, (size_t)NI * SVO_MAX_LEVELS * d.sel_max));
    d.big_scratch = nullptr; d.gn_scratch = nullptr;
    // (the geometry, and with it the kernel's own list length, is not known yet: room for lists of max_kps keys)
    if (const size_t bytes = nms_rowsort_scratch_bytes(NI, OC, MK)) HIPCHECK(dev_alloc(ctx, &d.big_scratch, bytes));
    HIPCHECK(dev_alloc(ctx, &d.gn_scratch, (size_t)L * gn_scratch_bytes_per_lane(MK)));      // lanes that track more than GN_LCAP pairs (k_gn.hip)
    HIPCHECK(dev_alloc(ctx, &d.sel_n, (size_t)NI * SVO_MAX_LEVELS));
    HIPCHECK(dev_alloc(ctx, &d.lvl_n, (size_t)NI * SVO_MAX_LEVELS));
    HIPCHECK(dev_alloc(ctx, &d.raw_kps, (size_t)NI * ctx->raw_cap_alloc));
    HIPCHECK(dev_alloc(ctx, &d.raw_desc, (size_t)NI * ctx->raw_cap_alloc * 32));
    HIPCHECK(dev_alloc(ctx, &d.raw_n, (size_t)NI));
    HIPCHECK(dev_alloc(ctx, &d.desc_work, (size_t)NI * ctx->raw_cap_alloc + 8));
    HIPCHECK(dev_alloc(ctx, &d.desc_n, (size_t)NI));
    HIPCHECK(dev_alloc(ctx, &d.kps, (size_t)NV * 4 * MK));
    HIPCHECK(dev_alloc(ctx, &d.desc, (size_t)NV * 4 * MK * 32));
    HIPCHECK(dev_alloc(ctx, &d.mdesc, (size_t)NV * 4 * MK * 32));
    HIPCHECK(dev_alloc(ctx, &d.final_slot, (size_t)NV * 4 * MK));
    HIPCHECK(dev_alloc(ctx, &d.n_kps, (size_t)NV * 4));
    HIPCHECK(dev_alloc(ctx, &d.matches, (size_t)NV * 2 * MK));
    HIPCHECK(dev_alloc(ctx, &d.n_matches, (size_t)NV * 2));
    HIPCHECK(dev_alloc(ctx, &d.row_index, (size_t)NV * 4 * cfg->max_h));
    HIPCHECK(dev_alloc(ctx, &d.mrow_index, (size_t)NV * 2 * (cfg->max_h + 1)));
    HIPCHECK(dev_alloc(ctx, &d.ids, (size_t)NV * 2 * MK));
    HIPCHECK(dev_alloc(ctx, &d.n_ids, (size_t)NV * 2));
    HIPCHECK(dev_alloc(ctx, &d.bf_idx, (size_t)NV * 3 * MK));
    HIPCHECK(dev_alloc(ctx, &d.trk_kq, (size_t)NV * MK));
    HIPCHECK(dev_alloc(ctx, &d.trk_nk, (size_t)NV));
    HIPCHECK(dev_alloc(ctx, &d.trk_pts, (size_t)NV * 2 * MK * 4));
    HIPCHECK(dev_alloc(ctx, &d.rs_F, (size_t)NV * 2 * SVO_RANSAC_SLOTS * 9));
    HIPCHECK(dev_alloc(ctx, &d.rs_guard, (size_t)NV * 2 * SVO_RANSAC_SLOTS * 2));
    HIPCHECK(dev_alloc(ctx, &d.rs_cnt, (size_t)NV * 2 * SVO_RANSAC_SLOTS));
    HIPCHECK(dev_alloc(ctx, &d.rs_k, (size_t)NV * 2 * SVO_RANSAC_SLOTS));
    HIPCHECK(dev_alloc(ctx, &d.rs_nvalid, (size_t)NV * 2 * (SVO_RANSAC_PAD / SVO_RANSAC_REG)));
    HIPCHECK(dev_alloc(ctx, &d.rs_bound, (size_t)NV * 2));
    HIPCHECK(dev_alloc(ctx, &d.rs_gen, (size_t)NV * 2));
    HIPCHECK(dev_alloc(ctx, &d.rs_floor, (size_t)NV * 4));
    HIPCHECK(dev_alloc(ctx, &d.rs_ticket, (size_t)NV * 2 * (SVO_RANSAC_SLOTS / 16)));
    HIPCHECK(dev_alloc(ctx, &d.rs_smp, (size_t)NV * 2 * SVO_RANSAC_PAD * 8));
    HIPCHECK(dev_alloc(ctx, &d.rs_sched, (size_t)NV * SVO_RS_ST));
    {   // The attempts of cv::findFundamentalMat's sampler for every point count a context can meet (k_match.hip, k_ransac_schedule):
        // ONE device copy per (device, max_kps), shared by every context of the process and freed with the last of them (sampler_table_*).
        int rc_t = sampler_table_acquire(ctx, MK); if (rc_t) return rc_t;
    }
    HIPCHECK(dev_alloc(ctx, &d.tracked, (size_t)NV * MK));
    HIPCHECK(dev_alloc(ctx, &d.n_tracked, (size_t)NV));
    HIPCHECK(dev_alloc(ctx, &d.gn_lmk, (size_t)L * MK * 3));
    HIPCHECK(dev_alloc(ctx, &d.gn_obs, (size_t)L * MK * 8));
    HIPCHECK(dev_alloc(ctx, &d.residual, (size_t)L * MK));
    HIPCHECK(dev_alloc(ctx, &d.outliers, (size_t)L * MK));
    HIPCHECK(dev_alloc(ctx, &d.cams, (size_t)L));
    HIPCHECK(dev_alloc(ctx, &d.lane, (size_t)L));
    HIPCHECK(dev_alloc(ctx, &d.results, (size_t)L));
    HIPCHECK(dev_alloc(ctx, &d.status, (size_t)L));
    HIPCHECK(dev_alloc(ctx, &d.det_status, (size_t)L)); d.det_ahead = 0;
    d.sad_patch = nullptr; d.sad_flag = nullptr; d.carry_win = 0;
    d.bf_dist = nullptr;
    d.debug_mode = ctx->knobs.debug_mode; d.rest_prio = ctx->knobs.rest_prio;
    d.rs_c0 = SVO_RANSAC_CHUNK0; d.rs_c1 = SVO_RANSAC_CHUNK1;      // (set per call where the RANSAC is launched)
    // SVO_TIMELINE=1: every kernel stamps the hull of its launch on the device's wall clock (svo_device.h, TlScope; svo_debug_timeline)
    d.tl = nullptr; d.tl_step = 0;
    if (ctx->knobs.timeline) { HIPCHECK(dev_alloc(ctx, &d.tl, (size_t)SVO_TL_STEPS * 256 * SVO_TL_SUB)); HIPCHECK(svo_debug_timeline(ctx, nullptr, 0, 1) < 0 ? hipErrorUnknown : hipSuccess); }
    HIPCHECK(configure_gauss_newton(MK));
    HIPCHECK(configure_match(MK));
    return SVO_OK;
}

extern "C" void svo_destroy(svo_ctx* ctx)
{
    if (ctx) use_device(ctx);
    if (!ctx) return;
    sync_all(ctx);                                        // work may still be running on a stream the caller switched away from
    for (void* p : ctx->allocs) hipFree(p);
    if (ctx->sampler_nmax > 0) sampler_table_release(ctx->cfg.device, ctx->sampler_nmax);
    for (auto& g : ctx->graphs) hipGraphExecDestroy(g.exec);
    if (ctx->h_vals) hipHostFree(ctx->h_vals);
    if (ctx->d_ham_out) hipFree(ctx->d_ham_out);
    if (ctx->d_ham_q) hipFree(ctx->d_ham_q);
    if (ctx->d_ham_t) hipFree(ctx->d_ham_t);
    for (void* p : { (void*)ctx->d_lk_pyr, (void*)ctx->d_lk_jobs, (void*)ctx->d_lk_pts, (void*)ctx->d_lk_init, (void*)ctx->d_lk_out, (void*)ctx->d_lk_status, (void*)ctx->d_lk_err }) if (p) hipFree(p);
    for (void* p : { (void*)ctx->d_gftt_map, (void*)ctx->d_gftt_img, (void*)ctx->d_gftt_jobs, (void*)ctx->d_gftt_keys, (void*)ctx->d_gftt_items, (void*)ctx->d_gftt_state,
                     (void*)ctx->d_gftt_info, (void*)ctx->d_gftt_seeds, (void*)ctx->d_gftt_pts, (void*)ctx->d_gftt_resp }) if (p) hipFree(p);
    klt_free(ctx);
    if (ctx->up_ready) {
        hipStreamSynchronize(ctx->s_copy);
        for (int i = 0; i < 2; i++) { hipEventDestroy(ctx->ev_h2d[i]); hipEventDestroy(ctx->ev_det[i]); if (ctx->h_stage[i]) hipHostFree(ctx->h_stage[i]); }
        hipStreamDestroy(ctx->s_copy);
    }
    for (auto& u : ctx->used_streams) if (u.ev) hipEventDestroy(u.ev);
    for (auto& s : ctx->spans) { hipEventDestroy(s.a); hipEventDestroy(s.b); }
    for (auto e : ctx->free_events) hipEventDestroy(e);
    if (ctx->own_stream) hipStreamDestroy(ctx->stream0);
    delete ctx;
}

void level_quota(int nfeatures, int nlevels, int* q);

// The reference has no keypoint cap (stage2_detect.cpp:461-464: orb_nfeats is free); a context has one (svo_config.max_kps).
// A request that cannot fit whatever the image size is refused HERE, when the parameters are loaded, with SVO_ERR_CAPACITY and
// the numbers in svo_last_error -- not at the first frame, and never by cutting a list silently.  (What depends on the image
// size -- pyramid and candidate buffers -- is still checked by the first svo_process.)
static int params_fit(svo_ctx* ctx, const svo_params& p)
{
    const bool fast_orb = p.detect_method == SVO_DM_FAST_ORB || p.detect_method == SVO_DM_FASTER;      // one list per x1/2 octave
    if (p.detect_method != SVO_DM_ORB && !fast_orb) return SVO_OK;          // refused as unsupported by svo_process
    char msg[256];
    const int MK = ctx->dc.max_kps;
    if (p.orb_nfeats <= 0) { snprintf(msg, sizeof(msg), "orb_nfeats %d: the detector needs a positive feature count", p.orb_nfeats); ctx->last_error = msg; return SVO_ERR_ARG; }
    if (fast_orb) {
        const int noct = p.nOctaves < 1 ? 1 : p.nOctaves;
        if (noct > ctx->dc.oct_cap) { snprintf(msg, sizeof(msg), "nOctaves %d exceeds svo_config.max_octaves %d", noct, ctx->dc.oct_cap); ctx->last_error = msg; return SVO_ERR_CAPACITY; }
        if (p.non_maximal_suppression) {
            const size_t k0 = (size_t)((double)(size_t)p.orb_nfeats * (double)(2 * noct) / (pow(2, noct) - 1));            // S2:404-407
            if ((long long)k0 > MK) { snprintf(msg, sizeof(msg), "orb_nfeats %d keeps up to %zu keypoints in octave 0, svo_config.max_kps is %d", p.orb_nfeats, k0, MK); ctx->last_error = msg; return SVO_ERR_CAPACITY; }
        }
        return SVO_OK;
    }
    const int nfe = p.non_maximal_suppression ? (int)(size_t)(1.5 * (double)(size_t)p.orb_nfeats) : p.orb_nfeats;       // S2:461-464
    int nlev = p.orb_nlevels < 1 ? 1 : p.orb_nlevels;
    if (nlev > SVO_MAX_LEVELS) return SVO_OK;                                  // refused as unsupported by the first frame
    if (nfe > MK) { snprintf(msg, sizeof(msg), "orb_nfeats %d asks the detector for %d keypoints, svo_config.max_kps is %d (largest supported: 16384)", p.orb_nfeats, nfe, MK); ctx->last_error = msg; return SVO_ERR_CAPACITY; }
    int quota[SVO_MAX_LEVELS];
    level_quota(nfe, nlev, quota);
    for (int l = 0; l < nlev; l++)
        if (2 * quota[l] > ctx->dc.sel_max) { snprintf(msg, sizeof(msg), "level %d ranks 2 x %d corners, the selection list of this context holds %d (2048; 4096 with max_kps 8192, 8192 with max_kps 16384)", l, quota[l], ctx->dc.sel_max); ctx->last_error = msg; return SVO_ERR_CAPACITY; }
    return SVO_OK;
}

extern "C" int svo_set_params(svo_ctx* ctx, const svo_params* p)
{
    if (ctx) use_device(ctx);
    if (!ctx || !p) return SVO_ERR_ARG;
    { const int rc = params_fit(ctx, *p); if (rc) return rc; }
    const bool dyn_reinit = ctx->dyn_fast && dyn_fast_octaves_changed(ctx->params, *p);
    ctx->params = *p; ctx->params_set = true;
    if (dyn_reinit) { const int rc = dyn_fast_init(ctx, -1); if (rc) return rc; }      // S2:522-523: m_threshold.assign(nOctaves, initial_FAST_threshold)
    // a context that has once selected a SAD method hands its frames over with their 8 x 8 windows (k_handover.hip, version 3), for good:
    // svo_handover_bytes grows here and never shrinks again
    if (p->match_method == SVO_SM_SAD || p->ifm_method == SVO_IFM_SAD) ctx->dc.carry_win = 1;
    ctx->fast_th = p->initial_FAST_threshold;            // resetFASTThreshold (H:532, 661)
    ctx->orb_th = (int)p->orb_max_distance;              // resetORBThreshold (H:539, 662)
    ctx->geom_ready = false;
    drop_graphs(ctx);
    return SVO_OK;
}
extern "C" int svo_get_params(const svo_ctx* ctx, svo_params* p) { if (!ctx || !p) return SVO_ERR_ARG; *p = ctx->params; return SVO_OK; }
extern "C" int svo_set_fast_threshold(svo_ctx* ctx, int v)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    const int lo = ctx->params.fast_min_th, hi = ctx->params.fast_max_th, m = v > lo ? v : lo;
    ctx->fast_th = hi < m ? hi : m;
    return SVO_OK;
}
extern "C" int svo_set_orb_threshold(svo_ctx* ctx, int v)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    const int lo = ctx->params.orb_min_th, hi = ctx->params.orb_max_th, m = v > lo ? v : lo;
    ctx->orb_th = hi < m ? hi : m;
    return SVO_OK;
}
extern "C" int svo_get_fast_threshold(const svo_ctx* ctx) { return ctx ? ctx->fast_th : SVO_ERR_ARG; }
extern "C" int svo_get_orb_threshold(const svo_ctx* ctx) { return ctx ? ctx->orb_th : SVO_ERR_ARG; }
// TDetectParams::KLT_win: svo_params has no room for it (its layout is frozen), so it lives on the context like the two thresholds.
// A kernel argument of the launches that follow: like svo_set_params it needs no synchronisation, only the captured graphs go.
extern "C" int svo_set_klt_win(svo_ctx* ctx, int v)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (v < 1 || v > 15) { char msg[96]; snprintf(msg, sizeof(msg), "KLT_win %d: 1 .. 15 are supported", v); ctx->last_error = msg; return SVO_ERR_ARG; }
    if (v != ctx->klt_win) drop_graphs(ctx);
    ctx->klt_win = v;
    return SVO_OK;
}
extern "C" int svo_get_klt_win(const svo_ctx* ctx) { return ctx ? ctx->klt_win : SVO_ERR_ARG; }

// The covariance of every pose increment (svo_types.h, svo_pose_cov).  Off: nothing is allocated, nothing launched.  The buffers are made
// here and not at the first frame: hipMalloc / hipMemset are refused on a capturing thread (as d_anms).  The launch sequence of a
// frame changes with the value, so the captured graphs go.
extern "C" int svo_set_pose_covariance(svo_ctx* ctx, int enable)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    const bool on = enable != 0;
    if (on == ctx->pose_cov) return SVO_OK;
    drop_graphs(ctx);
    HIPCHECK(sync_all(ctx));
    if (on) {
        const size_t L = (size_t)ctx->cfg.n_lanes, mb = gn_mask_bytes_per_lane(ctx->dc.max_kps) * L;
        if (!ctx->d_cov) HIPCHECK(dev_alloc(ctx, &ctx->d_cov, L));
        if (!ctx->d_cov_mask) HIPCHECK(dev_alloc(ctx, &ctx->d_cov_mask, mb));      // (each on its own: a failed second allocation is made again by the next call)
        HIPCHECK(hipMemset(ctx->d_cov, 0, sizeof(svo_pose_cov) * L));          // SVO_COV_NONE until a stage 5 has run
        HIPCHECK(hipMemset(ctx->d_cov_mask, 0, mb));
    }
    ctx->pose_cov = on;
    return SVO_OK;
}
static int pose_cov_ready(svo_ctx* ctx)
{
    if (ctx->pose_cov) return SVO_OK;
    ctx->last_error = "the pose covariance is off: svo_set_pose_covariance(ctx, 1) before the frame";
    return SVO_ERR_STATE;
}
extern "C" size_t svo_pose_cov_size(void) { return sizeof(svo_pose_cov); }
extern "C" int svo_get_pose_covariances(svo_ctx* ctx, svo_pose_cov* cov)
{
    if (ctx) use_device(ctx);
    if (!ctx || !cov) return SVO_ERR_ARG;
    int rc = pose_cov_ready(ctx); if (rc) return rc;
    rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(cov, ctx->d_cov, sizeof(svo_pose_cov) * ctx->cfg.n_lanes, hipMemcpyDeviceToHost));
    return SVO_OK;
}
extern "C" int svo_get_pose_covariance(svo_ctx* ctx, int lane, svo_pose_cov* cov)
{
    if (ctx) use_device(ctx);
    if (!ctx || !cov || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    int rc = pose_cov_ready(ctx); if (rc) return rc;
    rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(cov, ctx->d_cov + lane, sizeof(svo_pose_cov), hipMemcpyDeviceToHost));
    return SVO_OK;
}
extern "C" int svo_copy_pose_covariances_async(svo_ctx* ctx, void* dst, size_t bytes)
{
    if (ctx) use_device(ctx);
    if (!ctx || !dst || bytes < sizeof(svo_pose_cov) * (size_t)ctx->cfg.n_lanes) return SVO_ERR_ARG;
    { const int rc = pose_cov_ready(ctx); if (rc) return rc; }
    note_stream(ctx);
    HIPCHECK(hipMemcpyAsync(dst, ctx->d_cov, sizeof(svo_pose_cov) * ctx->cfg.n_lanes, hipMemcpyDeviceToDevice, ctx->stream));
    mark_stream(ctx);
    return SVO_OK;
}

// The landmarks of every frame (svo_types.h, svo_landmark).  Off: nothing is allocated, nothing launched.  As for the pose covariance the
// buffers are made here, before any graph capture, and a change of the switch or of std_noise_pixels (a kernel argument) drops the
// captured graphs.  The record array is the one large allocation a context makes after svo_create: refused with the number when it fails.
extern "C" size_t svo_landmark_abi_size(void) { return sizeof(svo_landmark); }
extern "C" int svo_set_landmarks(svo_ctx* ctx, int enable, double std_noise_pixels)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (!(std_noise_pixels >= 0.0 && std_noise_pixels <= 1.7976931348623157e308)) {
        char msg[128]; snprintf(msg, sizeof(msg), "std_noise_pixels %g: a finite value >= 0 is expected (0 = the reference's default, 1)", std_noise_pixels);
        ctx->last_error = msg; return SVO_ERR_ARG;
    }
    const bool on = enable != 0;
    const double sd = std_noise_pixels == 0.0 ? 1.0 : std_noise_pixels;       // TLeastSquaresParams::std_noise_pixels defaults to 1
    if (on == ctx->landmarks && (!on || sd == ctx->lmk_std)) return SVO_OK;
    drop_graphs(ctx);
    HIPCHECK(sync_all(ctx));
    if (on) {
        const size_t L = (size_t)ctx->cfg.n_lanes, MK = (size_t)ctx->dc.max_kps, mb = gn_mask_bytes_per_lane(ctx->dc.max_kps) * L;
        if (!ctx->d_lmk) {
            const hipError_t e = dev_alloc(ctx, &ctx->d_lmk, L * MK);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                char msg[200]; snprintf(msg, sizeof(msg), "svo_set_landmarks: %zu bytes for %zu lanes x %zu records of %zu bytes could not be allocated (%s)", L * MK * sizeof(svo_landmark), L, MK, sizeof(svo_landmark), hipGetErrorString(e));
                ctx->last_error = msg; return SVO_ERR_CAPACITY;
            }
        }
        if (!ctx->d_lmk_info) HIPCHECK(dev_alloc(ctx, &ctx->d_lmk_info, L));
        if (!ctx->d_lmk_cnt) HIPCHECK(dev_alloc(ctx, &ctx->d_lmk_cnt, 4 * L));
        if (!ctx->d_cov_mask) { HIPCHECK(dev_alloc(ctx, &ctx->d_cov_mask, mb)); }
        else if (!ctx->pose_cov) HIPCHECK(hipMemset(ctx->d_cov_mask, 0, mb));      // (while the pose covariance is on the array is in use and consistent)
        if (!ctx->landmarks) {                                                       // SVO_LMK_NONE until a stage 5 has run
            HIPCHECK(hipMemset(ctx->d_lmk_info, 0, sizeof(svo_landmarks_info) * L));
            HIPCHECK(hipMemset(ctx->d_lmk_cnt, 0, sizeof(int) * 4 * L));
        }
        ctx->lmk_std = sd;
    }
    ctx->landmarks = on;
    return SVO_OK;
}
extern "C" int svo_get_landmarks_enabled(const svo_ctx* ctx, int* enable, double* std_noise_pixels)
{
    if (!ctx) return SVO_ERR_ARG;
    if (enable) *enable = ctx->landmarks ? 1 : 0;
    if (std_noise_pixels) *std_noise_pixels = ctx->lmk_std;
    return SVO_OK;
}
static int landmarks_ready(svo_ctx* ctx)
{
    if (ctx->landmarks) return SVO_OK;
    ctx->last_error = "the landmarks are off: svo_set_landmarks(ctx, 1, std_noise_pixels) before the frame";
    return SVO_ERR_STATE;
}
extern "C" int svo_get_landmarks_info(svo_ctx* ctx, int lane, svo_landmarks_info* info)
{
    if (ctx) use_device(ctx);
    if (!ctx || !info || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    int rc = landmarks_ready(ctx); if (rc) return rc;
    rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(info, ctx->d_lmk_info + lane, sizeof(*info), hipMemcpyDeviceToHost));
    return SVO_OK;
}
// One synchronisation (svo_wait), then the lane's count and min(count, cap) records.  Returns the count.
extern "C" int svo_get_landmarks(svo_ctx* ctx, int lane, svo_landmark* out, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes || cap < 0 || (cap > 0 && !out)) return SVO_ERR_ARG;
    int rc = landmarks_ready(ctx); if (rc) return rc;
    rc = svo_wait(ctx); if (rc) return rc;
    svo_landmarks_info info;
    HIPCHECK(hipMemcpy(&info, ctx->d_lmk_info + lane, sizeof(info), hipMemcpyDeviceToHost));
    const int n = info.n < 0 ? 0 : (info.n > ctx->dc.max_kps ? ctx->dc.max_kps : info.n), m = n < cap ? n : cap;
    if (m > 0) HIPCHECK(hipMemcpy(out, ctx->d_lmk + (size_t)lane * ctx->dc.max_kps, sizeof(svo_landmark) * (size_t)m, hipMemcpyDeviceToHost));
    return n;
}
// dst_info: n_lanes svo_landmarks_info (or NULL); dst_records: n_lanes x max_kps svo_landmark, lane after lane (or NULL); bytes = the
// size of the records' destination
extern "C" int svo_copy_landmarks_async(svo_ctx* ctx, void* dst_info, void* dst_records, size_t bytes)
{
    if (ctx) use_device(ctx);
    if (!ctx || (!dst_info && !dst_records)) return SVO_ERR_ARG;
    const size_t L = (size_t)ctx->cfg.n_lanes, need = sizeof(svo_landmark) * L * (size_t)ctx->dc.max_kps;
    if (dst_records && bytes < need) return SVO_ERR_ARG;
    { const int rc = landmarks_ready(ctx); if (rc) return rc; }
    note_stream(ctx);
    if (dst_info) HIPCHECK(hipMemcpyAsync(dst_info, ctx->d_lmk_info, sizeof(svo_landmarks_info) * L, hipMemcpyDeviceToDevice, ctx->stream));
    if (dst_records) HIPCHECK(hipMemcpyAsync(dst_records, ctx->d_lmk, need, hipMemcpyDeviceToDevice, ctx->stream));
    mark_stream(ctx);
    return SVO_OK;
}

// dmFASTER's dynamic threshold (stage2_detect.cpp:522-550; svo_hip.h at svo_set_dyn_fast_threshold).  The thresholds are device data: no
// host copy exists, a frame never synchronises for them, and a captured graph stays valid while they move.
// A fresh m_threshold of one lane (-1: every lane): initial_FAST_threshold on every octave, empty statistics.  Waits for the enqueued work.
static int dyn_fast_init(svo_ctx* ctx, int lane)
{
    HIPCHECK(sync_all(ctx));
    svo_faster_stats fresh; memset(&fresh, 0, sizeof(fresh));
    for (int o = 0; o < SVO_MAX_OCTAVES; o++) fresh.next[o] = ctx->params.initial_FAST_threshold;
    for (int l = 0; l < ctx->cfg.n_lanes; l++)
        if (lane < 0 || lane == l) HIPCHECK(hipMemcpy(ctx->d_fstats + l, &fresh, sizeof(fresh), hipMemcpyHostToDevice));
    return SVO_OK;
}
extern "C" int svo_set_dyn_fast_threshold(svo_ctx* ctx, int enable, double target_feats_per_pixel)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    SVO_REFUSE(check_dyn_fast_target(target_feats_per_pixel, why));
    const bool on = enable != 0;
    if (on == ctx->dyn_fast && target_feats_per_pixel == ctx->dyn_target) return SVO_OK;
    drop_graphs(ctx);                                        // the launches of a detect call and one of their arguments change
    if (on && !ctx->dyn_fast) {                              // allocated here, not at the first frame: before any capture (as d_cov)
        if (!ctx->d_fstats) HIPCHECK(dev_alloc(ctx, &ctx->d_fstats, (size_t)ctx->cfg.n_lanes));
        const int rc = dyn_fast_init(ctx, -1); if (rc) return rc;
    }
    ctx->dyn_fast = on; ctx->dyn_target = target_feats_per_pixel;
    return SVO_OK;
}
extern "C" int svo_get_dyn_fast_threshold(const svo_ctx* ctx, int* enable, double* target_feats_per_pixel)
{
    if (!ctx) return SVO_ERR_ARG;
    if (enable) *enable = ctx->dyn_fast ? 1 : 0;
    if (target_feats_per_pixel) *target_feats_per_pixel = ctx->dyn_target;
    return SVO_OK;
}
extern "C" size_t svo_faster_stats_size(void) { return sizeof(svo_faster_stats); }
extern "C" int svo_get_faster_stats(svo_ctx* ctx, int lane, svo_faster_stats* out)
{
    if (ctx) use_device(ctx);
    if (!ctx || !out || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    if (!ctx->dyn_fast) { ctx->last_error = "the dynamic FAST threshold is off: svo_set_dyn_fast_threshold(ctx, 1, target) first"; return SVO_ERR_STATE; }
    const int rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(out, ctx->d_fstats + lane, sizeof(*out), hipMemcpyDeviceToHost));
    return SVO_OK;
}
// (svo_faster_threshold_step, the rule as a host function, is in frame_call.cpp: it needs no device)

// The adaptive NMS under dmFASTER (stage2_detect.cpp:599-606 behind S2:519-576; svo_hip.h at svo_set_faster_adaptive_nms): an opt-in of
// the context.  While it is off a call that selects the combination is refused as it always was (frame_call.cpp).
extern "C" int svo_set_faster_adaptive_nms(svo_ctx* ctx, int enable)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    const bool on = enable != 0;
    if (on == ctx->faster_anms) return SVO_OK;
    if (on) {
        if (std::max(1024, ctx->cfg.max_cand) > faster_anms_max_candidates()) {
            char msg[160]; snprintf(msg, sizeof(msg), "max_cand %d: the adaptive NMS under dmFASTER ranks at most %d candidates per image", ctx->cfg.max_cand, faster_anms_max_candidates());
            ctx->last_error = msg; return SVO_ERR_UNSUPPORTED;
        }
        // allocated here, not at the first frame: before any capture (as d_fstats), and so that a context that cannot afford it learns so now
        if (!ctx->d_fanms) HIPCHECK(dev_alloc(ctx, &ctx->d_fanms, faster_anms_scratch_words(2 * ctx->cfg.n_lanes, ctx->cand_total_alloc)));
        HIPCHECK(configure_faster_anms(ctx->dc.max_kps));
    }
    drop_graphs(ctx);                                        // the launches of a detect call under dmFASTER + nmsmAdaptive change
    ctx->faster_anms = on;
    return SVO_OK;
}
extern "C" int svo_get_faster_adaptive_nms(const svo_ctx* ctx) { return ctx ? (ctx->faster_anms ? 1 : 0) : SVO_ERR_ARG; }

// m_adaptive_non_max_sup on caller arrays: the device code of k_faster_anms on one list, so that it can be held to a reference on
// hand-built inputs.  The keys are built here as k_faster publishes them; strictly ascending raster order makes position order index order.
extern "C" int svo_adaptive_nms(svo_ctx* ctx, const svo_keypoint* kps, int n, int num_out_points, int img_w, int img_h, int32_t* out_order, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    const int n_cap = std::min(std::max(1024, ctx->cfg.max_cand), faster_anms_max_candidates());
    SVO_REFUSE(check_adaptive_nms_args(kps, n, num_out_points, img_w, img_h, out_order, cap, n_cap, ctx->dc.max_kps, why));
    const int actual = std::min(num_out_points, n);                               // S2:151
    if (actual <= 0) return 0;                                                   // S2:152
    if (!ctx->d_anms_list) {
        HIPCHECK(dev_alloc(ctx, &ctx->d_anms_list, (size_t)n_cap + faster_anms_scratch_words(1, n_cap)));
        HIPCHECK(dev_alloc(ctx, &ctx->d_anms_pos, (size_t)ctx->dc.max_kps));
    }
    HIPCHECK(configure_faster_anms(ctx->dc.max_kps));
    std::vector<unsigned long long> keys((size_t)n);
    std::vector<uint32_t> pos_of((size_t)n);
    for (int i = 0; i < n; i++) {
        uint32_t u; memcpy(&u, &kps[i].response, 4);
        const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);         // ord32 (svo_device.h)
        pos_of[(size_t)i] = (uint32_t)((int)kps[i].y * img_w + (int)kps[i].x);
        keys[(size_t)i] = ((unsigned long long)ord << 32) | (unsigned long long)(0xFFFFFFFFu - pos_of[(size_t)i]);
    }
    const hipStream_t st = ctx->stream;
    HIPCHECK(hipMemcpyAsync(ctx->d_anms_list, keys.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    launch_anms_list(ctx->d_anms_list, n, img_w, img_h, actual, ctx->dc.max_kps, ctx->d_anms_list + n_cap, n_cap, ctx->d_anms_pos, st);
    std::vector<uint32_t> out((size_t)actual);
    HIPCHECK(hipMemcpyAsync(out.data(), ctx->d_anms_pos, (size_t)actual * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipGetLastError());
    for (int o = 0; o < actual && o < cap; o++)
        out_order[o] = (int32_t)(std::lower_bound(pos_of.begin(), pos_of.end(), out[(size_t)o]) - pos_of.begin());
    return actual;
}

extern "C" int svo_set_stream(svo_ctx* ctx, void* stream)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (stream) ctx->stream = (hipStream_t)stream;
    else ctx->stream = ctx->stream0;
    return SVO_OK;
}

extern "C" int svo_get_device(const svo_ctx* ctx) { return ctx ? ctx->cfg.device : SVO_ERR_ARG; }
extern "C" int svo_get_stream(svo_ctx* ctx, void** stream) { if (!ctx || !stream) return SVO_ERR_ARG; *stream = (void*)ctx->stream; return SVO_OK; }

extern "C" int svo_set_camera(svo_ctx* ctx, int lane, const svo_stereo_camera* cam)
{
    if (ctx) use_device(ctx);
    if (!ctx || !cam || lane < -1 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    HIPCHECK(sync_all(ctx));
    for (int l = 0; l < ctx->cfg.n_lanes; l++)
        if (lane < 0 || lane == l) HIPCHECK(hipMemcpy(ctx->dc.cams + l, cam, sizeof(*cam), hipMemcpyHostToDevice));
    return SVO_OK;
}

extern "C" int svo_set_rectify_map(svo_ctx* ctx, int lane, int side, const float* map_x, const float* map_y, int w, int h)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < -1 || lane >= ctx->cfg.n_lanes || side < 0 || side > 1 || ((map_x == nullptr) != (map_y == nullptr))) return SVO_ERR_ARG;
    const int NI = 2 * ctx->cfg.n_lanes;
    if (map_x && (w <= 0 || h <= 0 || w > ctx->cfg.max_w || h > ctx->cfg.max_h || (ctx->n_maps > 0 && (w != ctx->map_w || h != ctx->map_h)))) return SVO_ERR_ARG;
    HIPCHECK(sync_all(ctx));
    if (ctx->map_ptrs.empty()) {
        ctx->map_ptrs.assign(NI, nullptr); ctx->map_bufs.assign(NI, nullptr);
        HIPCHECK(dev_alloc(ctx, (uint2***)&ctx->d_map_ptrs, (size_t)NI));
        HIPCHECK(hipMemset(ctx->d_map_ptrs, 0, sizeof(uint2*) * NI));
    }
    std::vector<uint2> fixed;
    if (map_x) {
        // cv::remap's fixed point (oracle: svo_oracle_map_fixed): cvRound(32 x) -> integer part + 5-bit fraction
        fixed.resize((size_t)w * h);
        for (size_t i = 0; i < fixed.size(); i++) {
            const float mx = map_x[i], my = map_y[i];
            uint2 e; e.x = 0xFFFFFFFFu; e.y = 0;
            if (mx > -4.0f && mx < (float)(w + 4) && my > -4.0f && my < (float)(h + 4)) {
                const long ix = lrintf(mx * 32.0f), iy = lrintf(my * 32.0f);
                const int x = (int)(ix >> 5), y = (int)(iy >> 5);
                if (x >= -1 && x < w && y >= -1 && y < h) { e.x = (uint32_t)(x + 1) | ((uint32_t)(y + 1) << 16); e.y = (uint32_t)(ix & 31) | ((uint32_t)(iy & 31) << 8); }
            }
            fixed[i] = e;
        }
    }
    for (int l = 0; l < ctx->cfg.n_lanes; l++) {
        if (lane >= 0 && lane != l) continue;
        uint2*& mp = ctx->map_ptrs[2 * l + side];
        if (map_x) {
            if (mp != ctx->map_bufs[2 * l + side] || !mp) {   // a cleared camera's buffer is reused, not allocated again; a lane that shared a calibration's table gets its own
                uint2*& buf = ctx->map_bufs[2 * l + side];
                if (!buf) HIPCHECK(dev_alloc(ctx, &buf, (size_t)ctx->cfg.max_w * ctx->cfg.max_h));
                if (!mp) ctx->n_maps++;
                mp = buf;
            }
            HIPCHECK(hipMemcpy(mp, fixed.data(), fixed.size() * sizeof(uint2), hipMemcpyHostToDevice));
            ctx->map_w = w; ctx->map_h = h;
        } else if (mp) { mp = nullptr; ctx->n_maps--; }     // the buffer stays in map_bufs for the next set
    }
    HIPCHECK(hipMemcpy(ctx->d_map_ptrs, ctx->map_ptrs.data(), sizeof(uint2*) * NI, hipMemcpyHostToDevice));
    return SVO_OK;
}

// ---- maps from a calibration (svo_hip.h at svo_stereo_rectify; setFromCamParams, stage1_rectify.cpp:66-68) -----------------------
// What the two setters below share: the argument rules of svo_set_rectify_map, then ONE k_rectify_map launch for the n (1 or 2)
// cameras in sides[] / models[], into the lane's own buffers or, with lane = -1, into the context's shared table of each side.
static int rectify_map_args(svo_ctx* ctx, int lane, int w, int h)
{
    if (lane < -1 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    if (w <= 0 || h <= 0 || w > ctx->cfg.max_w || h > ctx->cfg.max_h || (ctx->n_maps > 0 && (w != ctx->map_w || h != ctx->map_h))) {
        char msg[200];
        if (ctx->n_maps > 0) snprintf(msg, sizeof(msg), "map size %d x %d: the context holds maps of %d x %d (all maps of a context share one size, within max_w x max_h = %d x %d)", w, h, ctx->map_w, ctx->map_h, ctx->cfg.max_w, ctx->cfg.max_h);
        else snprintf(msg, sizeof(msg), "map size %d x %d: 1 x 1 .. max_w x max_h = %d x %d is expected", w, h, ctx->cfg.max_w, ctx->cfg.max_h);
        ctx->last_error = msg; return SVO_ERR_ARG;
    }
    return SVO_OK;
}
static bool model_finite(const RectifyModel& m)
{
    const double* v = m.ir;                              // ir, k, fx fy cx cy: 21 doubles in a row
    static_assert(sizeof(RectifyModel) == 21 * sizeof(double), "RectifyModel is 21 doubles");
    for (int i = 0; i < 21; i++) if (!(fabs(v[i]) <= 1.7976931348623157e308)) return false;
    return true;
}
static RectifyModel make_model(const svo_camera_model& cam, const double* R, const double* P)
{
    RectifyModel m;
    rectify_inverse(P, R, m.ir);
    for (int i = 0; i < 8; i++) m.k[i] = cam.dist[i];
    m.fx = cam.fx; m.fy = cam.fy; m.cx = cam.cx; m.cy = cam.cy;
    return m;
}
static int build_rectify_maps(svo_ctx* ctx, int lane, int n, const int* sides, const RectifyModel* models, int w, int h)
{
    const int NI = 2 * ctx->cfg.n_lanes;
    HIPCHECK(sync_all(ctx));
    if (ctx->map_ptrs.empty()) {
        ctx->map_ptrs.assign(NI, nullptr); ctx->map_bufs.assign(NI, nullptr);
        HIPCHECK(dev_alloc(ctx, (uint2***)&ctx->d_map_ptrs, (size_t)NI));
        HIPCHECK(hipMemset(ctx->d_map_ptrs, 0, sizeof(uint2*) * NI));
    }
    if (!ctx->d_rect_models) HIPCHECK(dev_alloc(ctx, &ctx->d_rect_models, (size_t)2));
    RectifyImage im[2];
    for (int k = 0; k < n; k++) {
        uint2*& buf = lane < 0 ? ctx->map_shared[sides[k]] : ctx->map_bufs[2 * lane + sides[k]];
        if (!buf) HIPCHECK(dev_alloc(ctx, &buf, (size_t)ctx->cfg.max_w * ctx->cfg.max_h));
        im[k].m = models[k]; im[k].dst = buf;
    }
    HIPCHECK(hipMemcpy(ctx->d_rect_models, im, sizeof(RectifyImage) * n, hipMemcpyHostToDevice));
    launch_rectify_map(ctx->d_rect_models, n, w, h, ctx->stream);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++)
        for (int l = 0; l < ctx->cfg.n_lanes; l++) {
            if (lane >= 0 && lane != l) continue;
            uint2*& mp = ctx->map_ptrs[2 * l + sides[k]];
            if (!mp) ctx->n_maps++;
            mp = im[k].dst;
        }
    ctx->map_w = w; ctx->map_h = h;
    HIPCHECK(hipMemcpy(ctx->d_map_ptrs, ctx->map_ptrs.data(), sizeof(uint2*) * NI, hipMemcpyHostToDevice));
    return SVO_OK;
}

extern "C" int svo_set_undistort_rectify(svo_ctx* ctx, int lane, int side, const svo_camera_model* cam, const double* R, const double* P, int w, int h)
{
    if (ctx) use_device(ctx);
    if (!ctx || !cam || !R || !P || side < 0 || side > 1) return SVO_ERR_ARG;
    { const int rc = rectify_map_args(ctx, lane, w, h); if (rc) return rc; }
    const RectifyModel m = make_model(*cam, R, P);
    if (!model_finite(m)) { ctx->last_error = "svo_set_undistort_rectify: a value of the model or of (A R)^-1 is not finite"; return SVO_ERR_ARG; }
    return build_rectify_maps(ctx, lane, 1, &side, &m, w, h);
}

extern "C" int svo_set_stereo_calibration(svo_ctx* ctx, int lane, const svo_stereo_calibration* calib, int set_camera, svo_stereo_rectification* out)
{
    if (ctx) use_device(ctx);
    if (!ctx || !calib || lane < -1 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    svo_stereo_rectification rect;
    char why[320];
    { const int rc = svo_stereo_rectify(calib, &rect, why, sizeof(why)); if (rc) { ctx->last_error = why; return rc; } }
    { const int rc = rectify_map_args(ctx, lane, calib->w, calib->h); if (rc) return rc; }
    const RectifyModel m[2] = { make_model(calib->left, rect.R1, rect.P1), make_model(calib->right, rect.R2, rect.P2) };
    if (!model_finite(m[0]) || !model_finite(m[1])) { ctx->last_error = "svo_set_stereo_calibration: (A R)^-1 of a rectified camera is not finite"; return SVO_ERR_ARG; }
    const int sides[2] = { 0, 1 };
    { const int rc = build_rectify_maps(ctx, lane, 2, sides, m, calib->w, calib->h); if (rc) return rc; }
    if (set_camera) { const int rc = svo_set_camera(ctx, lane, &rect.cam); if (rc) return rc; }
    if (out) *out = rect;
    return SVO_OK;
}

extern "C" int svo_debug_get_rectify_map(svo_ctx* ctx, int lane, int side, uint32_t* xy, uint32_t* frac, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes || side < 0 || side > 1 || cap < 0 || (cap > 0 && (!xy || !frac))) return SVO_ERR_ARG;
    if (ctx->map_ptrs.empty() || !ctx->map_ptrs[2 * lane + side]) return 0;
    const int count = ctx->map_w * ctx->map_h, n = count < cap ? count : cap;      // max_w * max_h < 2^24 (svo_create)
    if (n > 0) {
        HIPCHECK(sync_all(ctx));
        std::vector<uint2> e((size_t)n);
        HIPCHECK(hipMemcpy(e.data(), ctx->map_ptrs[2 * lane + side], (size_t)n * sizeof(uint2), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) { xy[i] = e[(size_t)i].x; frac[i] = e[(size_t)i].y; }
    }
    return count;
}

extern "C" int svo_reset(svo_ctx* ctx, int lane)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < -1 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    HIPCHECK(sync_all(ctx));
    for (int l = 0; l < ctx->cfg.n_lanes; l++)
        if (lane < 0 || lane == l) {
            HIPCHECK(hipMemset(ctx->dc.lane + l, 0, sizeof(LaneState)));
            const int OC = ctx->dc.oct_cap;
            HIPCHECK(hipMemset(ctx->dc.n_kps + (size_t)l * OC * 4, 0, (size_t)OC * 4 * sizeof(int)));
            HIPCHECK(hipMemset(ctx->dc.n_matches + (size_t)l * OC * 2, 0, (size_t)OC * 2 * sizeof(int)));
            HIPCHECK(hipMemset(ctx->dc.n_tracked + (size_t)l * OC, 0, (size_t)OC * sizeof(int)));
            HIPCHECK(hipMemset(ctx->dc.n_ids + (size_t)l * OC * 2, 0, (size_t)OC * 2 * sizeof(int)));
            HIPCHECK(hipMemset(ctx->dc.results + l, 0, sizeof(svo_result)));
            if (ctx->pose_cov) HIPCHECK(hipMemset(ctx->d_cov + l, 0, sizeof(svo_pose_cov)));
            if (ctx->landmarks) HIPCHECK(hipMemset(ctx->d_lmk_info + l, 0, sizeof(svo_landmarks_info)));      // SVO_LMK_NONE, n = 0
            if (ctx->dyn_fast) { const int rc = dyn_fast_init(ctx, l); if (rc) return rc; }     // a fresh estimator: m_threshold is empty (S2:522-523)
            HIPCHECK(hipMemset(ctx->dc.fast_th_dyn + (size_t)2 * l * SVO_MAX_LEVELS, 0, (size_t)2 * SVO_MAX_LEVELS * sizeof(uint32_t)));   // a fresh estimator speculates nothing
            ctx->sad.cur[l] = ctx->sad.prev[l] = 1; ctx->sad.drop[l] = 0;                       // no frames: nothing a SAD stage could miss
        }
    return SVO_OK;
}

// cv::ORB per-level feature budget (oracle: orb_level_quota)
void level_quota(int nfeatures, int nlevels, int* q)
{
    const float factor = (float)(1.0 / 1.2);
    float nd = (float)nfeatures * (1.0f - factor) / (1.0f - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int l = 0; l < nlevels - 1; l++) { q[l] = (int)lrintf(nd); sum += q[l]; nd *= factor; }
    q[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;
}

// cv::resize's INTER_LINEAR tables for one axis of an 8-bit image (oracle v7: svo_oracle_resize_table, same float operations in the same
// order; this file is compiled with -ffp-contract=off): idx = first tap, w01 = weight of that tap | weight of the next << 16
static void resize_table(int src, int dst, int* idx, int* w01)
{
    const double inv_scale = (double)dst / src, scale = 1.0 / inv_scale;
    for (int d = 0; d < dst; d++) {
        float fx = (float)((d + 0.5) * scale - 0.5);
        int sx = (int)floor((double)fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.f; sx = 0; }
        if (sx >= src - 1) { fx = 0.f; sx = src - 1; }
        long a0 = lrintf((1.f - fx) * 2048.f), a1 = lrintf(fx * 2048.f);       // cvRound: half to even
        if (a0 > 32767) a0 = 32767;
        if (a1 > 32767) a1 = 32767;
        idx[d] = sx; w01[d] = (int)a0 | ((int)a1 << 16);
    }
}

static void drop_graphs(svo_ctx* ctx)
{
    if (ctx->graphs.empty()) return;
    sync_all(ctx);
    for (auto& g : ctx->graphs) hipGraphExecDestroy(g.exec);
    ctx->graphs.clear();
}

int ensure_geometry(svo_ctx* ctx, int w, int h)
{
    const svo_params& p = ctx->params;
    // dmFAST_ORB and dmFASTER both work on the x1/2 octave pyramid and keep one list per octave (S2:502-515, 519-576): same geometry,
    // except that dmFASTER's detector tiles start 3 pixels from the border
    const bool faster = p.detect_method == SVO_DM_FASTER, fast_orb = p.detect_method == SVO_DM_FAST_ORB || faster;
    const int nfe = p.non_maximal_suppression ? (int)(size_t)(1.5 * (double)(size_t)p.orb_nfeats) : p.orb_nfeats;   // stage2_detect.cpp:461-464
    // stage1_rectify.cpp:80: one octave for dmORB (cv::ORB builds its own x1/1.2 pyramid), params_rectify.nOctaves otherwise
    const int noct = fast_orb ? (p.nOctaves < 1 ? 1 : p.nOctaves) : 1;
    int nlev = fast_orb ? noct : p.orb_nlevels; if (nlev < 1) nlev = 1;
    const int nfe_key = fast_orb ? (p.non_maximal_suppression ? p.orb_nfeats : -1) : nfe;      // FAST + ORB without NMS keeps every corner: its own slot layout
    if (ctx->geom_ready && ctx->geom_w == w && ctx->geom_h == h && ctx->geom_nfe == nfe_key && ctx->geom_nlevels == nlev &&
        ctx->geom_method == p.detect_method && ctx->geom_noct == noct) return SVO_OK;
    if (w > ctx->cfg.max_w || h > ctx->cfg.max_h || w < 64 || h < 64) return SVO_ERR_CAPACITY;
    if (nlev > SVO_MAX_LEVELS) return SVO_ERR_UNSUPPORTED;
    if (noct > ctx->dc.oct_cap) return SVO_ERR_CAPACITY;       // svo_config.max_octaves
    HIPCHECK(sync_all(ctx));
    drop_graphs(ctx);
    DevCtx& d = ctx->dc;
    int lw[SVO_MAX_LEVELS], lh[SVO_MAX_LEVELS], quota[SVO_MAX_LEVELS]; float sc[SVO_MAX_LEVELS];
    d.fast_orb = fast_orb ? 1 : 0; d.n_oct = noct;
    // number of keypoints the reference's NMS may keep per octave (stage2_detect.cpp:404-407)
    {
        size_t k0 = (size_t)((double)(size_t)p.orb_nfeats * (double)(2 * noct) / (pow(2, noct) - 1));
        for (int o = 0; o < SVO_MAX_OCTAVES; o++) d.kps_to_detect[o] = o == 0 ? (int)k0 : (o < noct ? (int)(size_t)round((double)k0 / pow(2, o)) : 0);
    }
    if (fast_orb) {
        // mrpt x1/2 octaves (S1:82-83).  Slots per octave: what the NMS may keep (kps_to_detect); without NMS the reference keeps EVERY
        // FAST corner (S2:613-614: no cap at all) -- here as many as the context's lists hold, max_kps for octave 0 and half of the one
        // before for the others (a quarter of the pixels each), beyond which SVO_ST_KPS_OVERFLOW is raised
        for (int l = 0; l < nlev; l++) {
            lw[l] = l ? lw[l - 1] / 2 : w; lh[l] = l ? lh[l - 1] / 2 : h; sc[l] = 1.0f;
            quota[l] = p.non_maximal_suppression ? d.kps_to_detect[l] : std::max(64, d.max_kps >> l);
        }
    } else {
        level_sizes(w, h, nlev, lw, lh, sc);
        level_quota(nfe, nlev, quota);
    }
    for (int o = 0; o < SVO_MAX_OCTAVES; o++) { d.ow[o] = fast_orb ? (o < noct ? lw[o] : 0) : (o == 0 ? w : 0); d.oh[o] = fast_orb ? (o < noct ? lh[o] : 0) : (o == 0 ? h : 0); }
    d.W = w; d.H = h; d.n_levels = nlev;
    long long off = 0; int tile_off = 0, slot_off = 0, cand_off = 0, rt_off = 0;
    std::vector<int> rtab;
    for (int l = 0; l < nlev; l++) {
        LevelGeom& g = d.lv[l];
        g.w = lw[l]; g.h = lh[l]; g.pitch = align_up(lw[l], 64); g.scale = sc[l];
        g.offset = off; if (l >= 1) off += (long long)g.pitch * g.h;
        const int edge = faster ? 3 : SVO_EDGE, tw = faster ? SVO_FK_W : SVO_FT_W, th = faster ? SVO_FK_H : SVO_FT_H;
        const int iw = g.w - 2 * edge, ih = g.h - 2 * edge;
        const bool live = iw > 0 && ih > 0 && quota[l] > 0;
        g.tiles_x = live ? (iw + tw - 1) / tw : 0; g.tiles_y = live ? (ih + th - 1) / th : 0;
        g.tile_off = tile_off; tile_off += g.tiles_x * g.tiles_y;
        g.quota = live ? quota[l] : 0; g.slot_off = slot_off; slot_off += g.quota;
        long long cc = (long long)ctx->cfg.max_cand * ((long long)g.w * g.h) / ((long long)lw[0] * lh[0]);
        if (cc < 1024) cc = 1024;
        g.cand_cap = (int)cc; g.cand_off = cand_off; cand_off += g.cand_cap;
        g.rtab_off = rt_off;
        if (l >= 1 && !fast_orb) {
            std::vector<int> xi(g.w), xf(g.w), yi(g.h), yf(g.h);
            resize_table(lw[l - 1], g.w, xi.data(), xf.data());
            resize_table(lh[l - 1], g.h, yi.data(), yf.data());
            // what k_resize's tile shape relies on (true for every x1/1.2 step; a geometry that broke it would be refused, not mis-sampled):
            // the four adjacent pixels of a thread sample within one 8-byte window, a 128 x 32 tile's taps fit the 176 x 42 LDS window
            for (int x = 0; x + 3 < g.w; x++) if (xi[x + 3] < xi[x] || xi[x + 3] - xi[x] > 5) return SVO_ERR_UNSUPPORTED;
            for (int x = 0; x < g.w; x += 128) if (xi[std::min(x + 127, g.w - 1)] + 1 - (xi[x] & ~15) + 4 > 176) return SVO_ERR_UNSUPPORTED;
            for (int y = 0; y < g.h; y += 32) if (yi[std::min(y + 31, g.h - 1)] + 1 - yi[y] > 41) return SVO_ERR_UNSUPPORTED;
            rtab.insert(rtab.end(), xi.begin(), xi.end()); rtab.insert(rtab.end(), xf.begin(), xf.end());
            rtab.insert(rtab.end(), yi.begin(), yi.end()); rtab.insert(rtab.end(), yf.begin(), yf.end());
            rt_off += 2 * (g.w + g.h);
        }
        if (!fast_orb && 2 * g.quota > d.sel_max) return SVO_ERR_CAPACITY;         // k_select's list capacity (2048, 4096 with max_kps 8192, 8192 with max_kps 16384)
        if (fast_orb && g.quota > d.max_kps) return SVO_ERR_CAPACITY;               // one octave's list must fit max_kps
    }
    for (int l = nlev; l < SVO_MAX_LEVELS; l++) { memset(&d.lv[l], 0, sizeof(LevelGeom)); d.lv[l].tile_off = tile_off; d.lv[l].slot_off = slot_off; }
    d.pyr_bytes = ctx->pyr_bytes_alloc;
    d.raw_cap = ctx->raw_cap_alloc;
    if (off > ctx->pyr_bytes_alloc || cand_off > ctx->cand_total_alloc || (int)rtab.size() > ctx->rtab_alloc || slot_off > d.raw_cap) return SVO_ERR_CAPACITY;
    if (!fast_orb && slot_off > d.max_kps) return SVO_ERR_CAPACITY;                 // ORB mode: all levels feed one list
    d.n_tiles = tile_off; d.n_slots = slot_off; d.cand_total = ctx->cand_total_alloc;
    d.div_tiles = make_fastdiv((uint32_t)(tile_off > 0 ? tile_off : 1));
    if (!rtab.empty()) HIPCHECK(hipMemcpy(d.rtab, rtab.data(), rtab.size() * sizeof(int), hipMemcpyHostToDevice));
    {   // k_fast's / k_faster's tile table (same for every image and frame of this geometry)
        const int edge = faster ? 3 : SVO_EDGE, tw = faster ? SVO_FK_W : SVO_FT_W, th = faster ? SVO_FK_H : SVO_FT_H;
        if (tile_off > ctx->tile_tab_alloc) return SVO_ERR_CAPACITY;
        std::vector<uint4> tt((size_t)tile_off);
        for (int l = 0; l < nlev; l++) {
            const LevelGeom& g = d.lv[l];
            for (int t = 0; t < g.tiles_x * g.tiles_y; t++) {
                const int by = t / g.tiles_x, bx = t - by * g.tiles_x;
                tt[(size_t)g.tile_off + t] = make_uint4((uint32_t)(edge + bx * tw) | ((uint32_t)(edge + by * th) << 16), (uint32_t)g.w | ((uint32_t)g.h << 16),
                                                        (uint32_t)l | ((uint32_t)g.pitch << 8), (uint32_t)g.offset);
            }
        }
        if (!tt.empty()) HIPCHECK(hipMemcpy((void*)d.fast_tiles, tt.data(), tt.size() * sizeof(uint4), hipMemcpyHostToDevice));
    }
    HIPCHECK(configure_nms_rowsort(d));
    if (faster) HIPCHECK(configure_faster_nms(d));
    ctx->geom_ready = true; ctx->geom_once = true; ctx->geom_w = w; ctx->geom_h = h; ctx->geom_nfe = nfe_key; ctx->geom_nlevels = nlev;
    ctx->geom_method = p.detect_method; ctx->geom_noct = noct;
    return SVO_OK;
}

// ---- kernel timing ------------------------------------------------------------------------------------------
hipEvent_t get_event(svo_ctx* ctx)
{
    if (!ctx->free_events.empty()) { hipEvent_t e = ctx->free_events.back(); ctx->free_events.pop_back(); return e; }
    hipEvent_t e; hipEventCreate(&e); return e;
}
static void collect_spans(svo_ctx* ctx)
{
    for (auto& s : ctx->spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { ctx->kt_total[s.id] += ms; ctx->kt_calls[s.id] += 1; }
        ctx->free_events.push_back(s.a); ctx->free_events.push_back(s.b);
    }
    ctx->spans.clear();
}

extern "C" int svo_wait(svo_ctx* ctx)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    HIPCHECK(sync_all(ctx));
    collect_spans(ctx);
    return SVO_OK;
}

extern "C" int svo_kernel_times(svo_ctx* ctx, const char** names, double* total_ms, int64_t* calls, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    // which names, in which order: kernel_names.cpp (a context that has made none of the optional calls reports the list it always did)
    int ids[KT_COUNT];
    const int n = kernel_time_listing(ctx->kt_seen, ctx->pose_cov, ctx->landmarks, ids);
    for (int i = 0; i < n && i < cap; i++) {
        if (names) names[i] = kernel_names[ids[i]].name;
        if (total_ms) total_ms[i] = ctx->kt_total[ids[i]];
        if (calls) calls[i] = ctx->kt_calls[ids[i]];
    }
    return n;
}
extern "C" int svo_kernel_times_select(svo_ctx* ctx, const char* name)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (!name || !*name) { ctx->kt_mask = ~0ull; return SVO_OK; }
    const int id = kernel_time_id(name);
    if (id < 0) return SVO_ERR_ARG;
    ctx->kt_mask = 1ull << id;
    return SVO_OK;
}

extern "C" int svo_kernel_times_reset(svo_ctx* ctx)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    for (int i = 0; i < KT_COUNT; i++) { ctx->kt_total[i] = 0; ctx->kt_calls[i] = 0; }
    return SVO_OK;
}

// train-side splits of the brute-force matcher: enough workgroups for ~8 waves per SIMD (a ~2000 x 2000 problem is
// 8 query blocks x 8 train tiles; with one split per lane a 16-lane launch keeps ONE wave per SIMD busy)
static int hamming_splits(const svo_ctx* ctx)
{
    if (ctx->knobs.ham_splits > 0) return ctx->knobs.ham_splits;      // SVO_HAM_SPLITS
    int s = 1024 / (8 * ctx->cfg.n_lanes); return s < 1 ? 1 : (s > 8 ? 8 : s);     // train splits: enough workgroups to fill the GPU, few enough to amortise the query expansion (64 lanes: 2 -- 32.1 us per launch against 34.8 with 4, 38.2 with 6: profiles/r04o)
}

// ---- host-fed frames ------------------------------------------------------------------------------------------
static int ensure_upload(svo_ctx* ctx)
{
    if (ctx->up_ready) return SVO_OK;
    {   // the upload stream at the highest priority: when a caller's compute stream is a high-priority one (svo_batch's detect stream),
        // an upload queued at normal priority was scheduled behind it (host-fed batch: 21.3 k -> 16.1 k pairs/s, 52 -> 40 GB/s)
        int least = 0, greatest = 0;
        (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        HIPCHECK(hipStreamCreateWithPriority(&ctx->s_copy, hipStreamNonBlocking, ctx->knobs.copy_prio_normal ? 0 : greatest));      // SVO_COPY_PRIO=0
    }
    for (int i = 0; i < 2; i++) { HIPCHECK(hipEventCreateWithFlags(&ctx->ev_h2d[i], hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&ctx->ev_det[i], hipEventDisableTiming)); }
    ctx->slot_bytes = (size_t)2 * ctx->cfg.n_lanes * ctx->img0_pitch_internal * ctx->cfg.max_h;
    ctx->d_img0_ring[0] = ctx->d_img0;
    HIPCHECK(dev_alloc(ctx, &ctx->d_img0_ring[1], ctx->slot_bytes));
    ctx->up_ready = true;
    return SVO_OK;
}

// Enqueue the upload of one frame of every lane (8-bit grey, host memory) into the next slot of the device ring, on the
// copy stream; the compute stream `st` is made to wait for it.  No host synchronisation when the images are
// page-locked (SVO_FLAG_PINNED_IMAGES): the call returns while the copy is in flight and the caller keeps the images
// valid until svo_wait_upload / svo_wait.  Pageable images are first copied into the context's own page-locked
// staging slot (that is the cost of "borrowed for the duration of the call", P:111-120), then uploaded the same way.
// idle: lanes that sit the call out (svo_process_lanes) -- their images are neither copied nor uploaded, frames[l] is not read
static int upload_frames(svo_ctx* ctx, const svo_frame* frames, int w, int h, bool pinned, hipStream_t st, const uint8_t** ptrs, const LaneMask& idle)
{
    auto is_idle = [&](int l) { return lane_in(idle, l); };
    const bool partial = (idle.w[0] | idle.w[1]) != 0;
    int rc = ensure_upload(ctx); if (rc) return rc;
    const int L = ctx->cfg.n_lanes, ipitch = ctx->img0_pitch_internal, slot = ctx->up_slot;
    const size_t img_bytes = (size_t)ipitch * ctx->cfg.max_h;
    uint8_t* dbase = ctx->d_img0_ring[slot];
    // the slot's previous frame must be through stage 2 (the only stage that reads level 0) before it is overwritten
    if (ctx->ev_det_valid[slot]) HIPCHECK(hipStreamWaitEvent(ctx->s_copy, ctx->ev_det[slot], 0));
    const uint8_t* src0 = partial ? nullptr : frames[0].left.data;
    bool contiguous = !partial && (w == ipitch) && (h == ctx->cfg.max_h);
    for (int l = 0; l < L && contiguous; l++)
        for (int sd = 0; sd < 2; sd++) {
            const svo_image& im = sd ? frames[l].right : frames[l].left;
            if (im.stride != (int64_t)w || im.data != src0 + (size_t)(2 * l + sd) * img_bytes) contiguous = false;
        }
    if (pinned) {
        if (contiguous) HIPCHECK(hipMemcpyAsync(dbase, src0, img_bytes * 2 * L, hipMemcpyHostToDevice, ctx->s_copy));       // [lane][side][h][w] in one piece
        else for (int l = 0; l < L; l++)
            for (int sd = 0; sd < 2; sd++) {
                if (is_idle(l)) continue;
                const svo_image& im = sd ? frames[l].right : frames[l].left;
                HIPCHECK(hipMemcpy2DAsync(dbase + (size_t)(2 * l + sd) * img_bytes, ipitch, im.data, (size_t)im.stride, (size_t)w, (size_t)h, hipMemcpyHostToDevice, ctx->s_copy));
            }
    } else {
        if (!ctx->h_stage[slot]) HIPCHECK(hipHostMalloc((void**)&ctx->h_stage[slot], ctx->slot_bytes, hipHostMallocDefault));
        if (ctx->ev_h2d_valid[slot]) HIPCHECK(hipEventSynchronize(ctx->ev_h2d[slot]));          // the staging slot's last upload has left it
        for (int l = 0; l < L; l++)
            for (int sd = 0; sd < 2; sd++) {
                if (is_idle(l)) continue;
                const svo_image& im = sd ? frames[l].right : frames[l].left;
                uint8_t* hs = ctx->h_stage[slot] + (size_t)(2 * l + sd) * img_bytes;
                if (im.stride == (int64_t)ipitch && w == ipitch) memcpy(hs, im.data, (size_t)ipitch * h);
                else for (int y = 0; y < h; y++) memcpy(hs + (size_t)y * ipitch, im.data + (size_t)y * im.stride, (size_t)w);
            }
        if (h == ctx->cfg.max_h && !partial) HIPCHECK(hipMemcpyAsync(dbase, ctx->h_stage[slot], img_bytes * 2 * L, hipMemcpyHostToDevice, ctx->s_copy));
        else for (int i = 0; i < 2 * L; i++) if (!is_idle(i >> 1)) HIPCHECK(hipMemcpyAsync(dbase + (size_t)i * img_bytes, ctx->h_stage[slot] + (size_t)i * img_bytes, (size_t)ipitch * h, hipMemcpyHostToDevice, ctx->s_copy));
    }
    HIPCHECK(hipEventRecord(ctx->ev_h2d[slot], ctx->s_copy)); ctx->ev_h2d_valid[slot] = true;
    HIPCHECK(hipStreamWaitEvent(st, ctx->ev_h2d[slot], 0));
    for (int i = 0; i < 2 * L; i++) ptrs[i] = dbase + (size_t)i * img_bytes;
    ctx->det_slot = slot; ctx->up_slot = slot ^ 1;
    return SVO_OK;
}

extern "C" int svo_use_graphs(svo_ctx* ctx, int enable)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (!enable) drop_graphs(ctx);
    ctx->use_graphs = enable != 0;
    return SVO_OK;
}

extern "C" int svo_wait_upload(svo_ctx* ctx)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (ctx->up_ready) HIPCHECK(hipStreamSynchronize(ctx->s_copy));
    return SVO_OK;
}
extern "C" int svo_host_alloc(size_t bytes, void** out)
{
    if (!out || !bytes) return SVO_ERR_ARG;
    *out = nullptr;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? SVO_OK : SVO_ERR_HIP;
}
extern "C" int svo_host_free(void* p) { return (!p || hipHostFree(p) == hipSuccess) ? SVO_OK : SVO_ERR_HIP; }
extern "C" int svo_host_register(void* p, size_t bytes) { return (p && bytes && hipHostRegister(p, bytes, hipHostRegisterDefault) == hipSuccess) ? SVO_OK : SVO_ERR_HIP; }
extern "C" int svo_host_unregister(void* p) { return (p && hipHostUnregister(p) == hipSuccess) ? SVO_OK : SVO_ERR_HIP; }

// The frame intake of a call that reads images (svo_process with SVO_RUN_DETECT, svo_gather_windows): the checks of the read contract of
// svo_image.stride (svo_hip.h) -- all before anything is enqueued --, the geometry, and the way of every kind of frame to the
// level-0 addresses in ptrs[]: device frames in place, host frames through the upload ring, BGR / unrectified ones through stage 1's
// source staging (prep is then filled and *prepare_out set: the caller launches k_prepare behind the pointer table).
// lists_geometry: the images belong to lists that are already there (svo_gather_windows) -- their geometry is required, not made.
static int intake_frames(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, const LaneMask& idle, bool lists_geometry, hipStream_t st,
                         const uint8_t** ptrs, PrepArgs& prep, bool* prepare_out)
{
    DevCtx& d = ctx->dc;
    auto is_idle = [&](int l) { return lane_in(idle, l); };
    const bool partial = (idle.w[0] | idle.w[1]) != 0;
    *prepare_out = false;
    if (!frames) return SVO_ERR_ARG;                    // P:81
    int l0 = 0; while (is_idle(l0)) l0++;               // the first active lane: what the others must agree with
    const int w = frames[l0].left.w, h = frames[l0].left.h;
    for (int l = 0; l < d.n_lanes; l++) {
        if (is_idle(l)) continue;                       // (its frames[] entry is not read: it may hold NULL pointers)
        const svo_frame& f = frames[l];
        if (!f.left.data || !f.right.data || f.left.w != w || f.left.h != h || f.right.w != w || f.right.h != h) return SVO_ERR_ARG;
    }
    const int ch = (flags & SVO_FLAG_BGR_IMAGES) ? 3 : 1;
    // the read contract of svo_image.stride (svo_hip.h): rows may not overlap, and the kernels that read a device frame in place
    // address it with 32-bit byte offsets from its base.  Refused here, before anything is enqueued.
    for (int l = 0; l < d.n_lanes; l++)
        for (int s = 0; s < 2; s++) {
            if (is_idle(l)) continue;
            const svo_image& im = s ? frames[l].right : frames[l].left;
            char msg[200];
            if (w < 1 || h < 1) {
                snprintf(msg, sizeof(msg), "image size %d x %d: both must be positive", w, h);
                ctx->last_error = msg; return SVO_ERR_ARG;
            }
            if (im.stride < (int64_t)w * ch) {
                snprintf(msg, sizeof(msg), "lane %d %s image: stride %lld is smaller than a row (%d px x %d B)", l, s ? "right" : "left", (long long)im.stride, w, ch);
                ctx->last_error = msg; return SVO_ERR_ARG;
            }
            if ((flags & SVO_FLAG_DEVICE_IMAGES) && im.stride > (int64_t)INT32_MAX / h) {
                snprintf(msg, sizeof(msg), "lane %d %s image: h * stride = %d x %lld exceeds the 2^31 - 1 bytes a device frame may span", l, s ? "right" : "left", h, (long long)im.stride);
                ctx->last_error = msg; return SVO_ERR_ARG;
            }
        }
    int rc = SVO_OK;
    if (!lists_geometry) { rc = ensure_geometry(ctx, w, h); if (rc) return rc; }
    else {
        // svo_gather_windows: the geometry is the one the lists were put (or loaded) with; the images must be of that frame size
        if (!ctx->geom_ready) { ctx->last_error = "no geometry yet: put or load the lists first (svo_set_params clears the geometry of the lists before it)"; return SVO_ERR_STATE; }
        if (w != ctx->geom_w || h != ctx->geom_h) {
            char msg[160]; snprintf(msg, sizeof(msg), "frame size %d x %d, but the lists were put with %d x %d", w, h, ctx->geom_w, ctx->geom_h);
            ctx->last_error = msg; return SVO_ERR_STATE;
        }
    }
    const bool prepare = ch == 3 || ctx->n_maps > 0;
    if (ctx->n_maps > 0 && (ctx->map_w != w || ctx->map_h != h)) return SVO_ERR_ARG;
    const int ipitch = ctx->img0_pitch_internal;
    if (flags & SVO_FLAG_DEVICE_IMAGES) {
        const long long stride = frames[l0].left.stride;
        for (int l = 0; l < d.n_lanes; l++) {
            if (is_idle(l)) { ptrs[2 * l] = nullptr; ptrs[2 * l + 1] = nullptr; continue; }
            if (frames[l].left.stride != stride || frames[l].right.stride != stride) { ctx->last_error = "device frames of one call must share one stride"; return SVO_ERR_ARG; }
            ptrs[2 * l] = frames[l].left.data; ptrs[2 * l + 1] = frames[l].right.data;
        }
        d.img0_pitch = (int)stride;
        if (prepare) { for (int i = 0; i < 2 * d.n_lanes; i++) prep.src[i] = ptrs[i]; prep.src_stride = stride; }
        else if (ctx->use_graphs && !partial && !lists_geometry) {
            // a captured frame reads fixed addresses: the images go to the ring slot first (device to device, same stream)
            rc = ensure_upload(ctx); if (rc) return rc;
            const int slot = ctx->up_slot; ctx->up_slot = slot ^ 1; ctx->det_slot = slot;
            const size_t img_bytes = (size_t)ipitch * ctx->cfg.max_h;
            for (int i = 0; i < 2 * d.n_lanes; i++) {
                uint8_t* dst = ctx->d_img0_ring[slot] + (size_t)i * img_bytes;
                HIPCHECK(hipMemcpy2DAsync(dst, ipitch, ptrs[i], (size_t)stride, (size_t)w, (size_t)h, hipMemcpyDeviceToDevice, st));
                ptrs[i] = dst;
            }
            d.img0_pitch = ipitch;
        }
    } else if (!prepare) {
        rc = upload_frames(ctx, frames, w, h, (flags & SVO_FLAG_PINNED_IMAGES) != 0, st, ptrs, idle); if (rc) return rc;
        d.img0_pitch = ipitch;
    } else {
        if (!ctx->d_src) { ctx->src_pitch = align_up(3 * ctx->cfg.max_w, 64); HIPCHECK(dev_alloc(ctx, &ctx->d_src, (size_t)2 * ctx->cfg.n_lanes * ctx->src_pitch * ctx->cfg.max_h)); }
        for (int l = 0; l < d.n_lanes; l++)
            for (int s = 0; s < 2; s++) {
                if (is_idle(l)) continue;
                const svo_image& im = s ? frames[l].right : frames[l].left;
                uint8_t* dst = ctx->d_src + (size_t)(2 * l + s) * ctx->src_pitch * ctx->cfg.max_h;
                HIPCHECK(hipMemcpy2DAsync(dst, ctx->src_pitch, im.data, (size_t)im.stride, (size_t)w * ch, (size_t)h, hipMemcpyHostToDevice, st));
                prep.src[2 * l + s] = dst;
            }
        prep.src_stride = ctx->src_pitch;
    }
    if (prepare) {       // stage 1 writes the context's own level-0 buffers; detection reads those
        for (int i = 0; i < 2 * d.n_lanes; i++) ptrs[i] = ctx->d_img0 + (size_t)i * ipitch * ctx->cfg.max_h;
        d.img0_pitch = ipitch;
        prep.maps = ctx->n_maps > 0 ? (const uint2* const*)ctx->d_map_ptrs : nullptr;
        prep.dst = ctx->d_img0; prep.dst_img_stride = (long long)ipitch * ctx->cfg.max_h; prep.dst_pitch = ipitch;
        prep.channels = ch; prep.w = w; prep.h = h; prep.idle = idle;
    }
    *prepare_out = prepare;
    return SVO_OK;
}

// ---- what a call that enqueues leaves behind, whichever way it ends ---------------------------------------------------------
// Records the event armed by svo_record_after_post behind what the stream holds, and disarms it.  consumes: the call runs the detector's
// post-processing and somebody takes part (a call in which nobody takes part is no call: it leaves the event armed).  Never while the
// stream captures: inside this call's own capture the event stays armed for the launch of the graph; on the way out of a call
// (leaving, PostDisarm) it is disarmed whatever the stream is doing, so that a later, unrelated call cannot record it at the wrong point.
static hipError_t record_post_event(svo_ctx* ctx, bool consumes, bool leaving = false)
{
    if (!consumes || !ctx->post_event || ctx->capturing) return hipSuccess;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (leaving) hipStreamIsCapturing(ctx->stream, &cs);
    const hipError_t e = cs == hipStreamCaptureStatusNone ? hipEventRecord(ctx->post_event, ctx->stream) : hipSuccess;
    ctx->post_event = nullptr;
    return e;
}
// the reader of the level-0 images is through (stage 2, the window gather): the upload ring's slot may take the next frame
static hipError_t release_ring_slot(svo_ctx* ctx)
{
    if (!ctx->up_ready || ctx->det_slot < 0) return hipSuccess;
    const hipError_t e = hipEventRecord(ctx->ev_det[ctx->det_slot], ctx->stream);
    if (e == hipSuccess) ctx->ev_det_valid[ctx->det_slot] = true;
    return e;
}
// svo_record_after_post arms ONE call: the next one that runs the detector's post-processing.  Whatever way that call leaves -- an
// argument check (the mask's included), SVO_ERR_STATE, a failed launch -- the event is recorded behind what was enqueued (possibly
// nothing) and disarmed, so that a waiter is released
struct PostDisarm { svo_ctx* c; bool consumes; ~PostDisarm() { (void)record_post_event(c, consumes, true); } };
// whatever was enqueued before an error exit is still covered by the stream's event (declared before the capture guard: a capture is
// closed first)
// the idle lanes travel in DevCtx to every launch of a call; outside it the mask is all zero (the other entry points launch with it)
// a capture that an error exit leaves open is closed and thrown away
struct CaptureGuard { svo_ctx* c; ~CaptureGuard() { if (c->capturing) { hipGraph_t g = nullptr; hipStreamEndCapture(c->stream, &g); if (g) hipGraphDestroy(g); c->capturing = false; } } };

// ---- the launches of a frame, one function per stage --------------------------------------------------------------------
// kernel_times: the instantiations of a 16384-entry context are counted under their own names (kernel_names.cpp)
static int kt_select(const DevCtx& d) { return d.sel_max > 4096 ? KT_SELECT_8192 : KT_SELECT; }
static int kt_nms(const DevCtx& d) { return nms_rowsort_items(d) > 8 ? KT_NMS_16 : KT_NMS; }
static bool wide_lists(const DevCtx& d) { return d.max_kps > 8192; }

// stage 2 up to the detector's own output: pyramid, corners, the detector's selection (and, where the detector describes, description)
static void enqueue_detect(svo_ctx* ctx, const FrameCall& call, hipStream_t st)
{
    DevCtx& d = ctx->dc; const svo_params& p = ctx->params;
    if (call.faster) {      // stage2_detect.cpp:519-576: FAST-12, KLT response, grid NMS; svo_set_fast_threshold has no part in it.  The threshold is the
                            // constant initial_FAST_threshold (m_threshold never moves: processNewImagePair passes no update_dyn_thresholds) unless
                            // svo_set_dyn_fast_threshold is on: then the lane's own m_threshold[octave], moved on the device (S2:537-546)
        { Span s(ctx, KT_RESIZE); for (int l = 1; l < d.n_levels; l++) launch_half(d, l, st); }
        if (call.faster_anms) {     // svo_set_faster_adaptive_nms + nmsmAdaptive (S2:599-606 on this detector's output): the same detector launches, then
                                    // k_faster_anms where the grid NMS would go -- it commits the dynamic thresholds itself when those are on
            if (ctx->dyn_fast) { Span s(ctx, KT_FASTER); launch_faster_dyn(d, ctx->d_cand64, ctx->d_fstats, ctx->dyn_target, ctx->klt_win, st); }
            else { Span s(ctx, KT_FASTER); launch_faster(d, ctx->d_cand64, p.initial_FAST_threshold, ctx->klt_win, st); }
            { Span s(ctx, KT_FASTER_NMS); launch_faster_anms(d, ctx->d_cand64, ctx->d_fanms, ctx->dyn_fast ? ctx->d_fstats : nullptr, ctx->dyn_target, st); }
            return;
        }
        if (ctx->dyn_fast) {
            { Span s(ctx, KT_FASTER); launch_faster_dyn(d, ctx->d_cand64, ctx->d_fstats, ctx->dyn_target, ctx->klt_win, st); }      // two launches under one name
            { Span s(ctx, KT_FASTER_NMS); launch_faster_nms_dyn(d, ctx->d_cand64, p.non_maximal_suppression, p.min_distance, ctx->d_fstats, ctx->dyn_target, st); }
            return;
        }
        { Span s(ctx, KT_FASTER); launch_faster(d, ctx->d_cand64, p.initial_FAST_threshold, ctx->klt_win, st); }
        { Span s(ctx, KT_FASTER_NMS); launch_faster_nms(d, ctx->d_cand64, p.non_maximal_suppression, p.min_distance, st); }
    } else if (d.fast_orb) {       // stage2_detect.cpp:502-515 on the x1/2 octave pyramid
        { Span s(ctx, KT_RESIZE); for (int l = 1; l < d.n_levels; l++) launch_half(d, l, st); }
        { Span s(ctx, KT_FAST); launch_fast(d, st); }
        if (p.non_maximal_suppression && p.nmsMethod == SVO_NMS_ADAPTIVE) {      // S2:599-606 on the FAST detector's output
            Span s(ctx, KT_SELECT); launch_fastorb_anms(d, ctx->d_anms, st);
        } else { Span s(ctx, KT_SELECT); launch_fastorb_nms(d, p.non_maximal_suppression, p.min_distance, st); }
        { Span s(ctx, KT_DESCRIBE); launch_describe(d, ctx->knobs, 0, st); }
    } else {                // stage2_detect.cpp:458-497
        { Span s(ctx, KT_RESIZE); for (int l = 1; l < d.n_levels; l++) launch_resize(d, l, st); }
        { Span s(ctx, KT_FAST); launch_fast(d, st); }
        if (!call.select_in_post) { Span s(ctx, kt_select(d)); launch_select(d, st); }
        // debug mode 9 keeps the detector's order: describe everything, then NMS -- that is what svo_debug_get_raw_keypoints shows
        if (d.debug_mode == DBG_DESCRIBE_BEFORE_NMS) { Span s(ctx, KT_DESCRIBE); launch_describe(d, ctx->knobs, 0, st); }
    }
}
// The reference's own post-processing of the detector output: grid NMS and row sort.  The one copy: run by a detect call that does not
// leave it out (SVO_FLAG_DETECT_NO_POST) and by the SVO_RUN_DETECT_POST call that makes up for it.
static void enqueue_detect_post(svo_ctx* ctx, const FrameCall& call, hipStream_t st)
{
    DevCtx& d = ctx->dc; const svo_params& p = ctx->params;
    if (call.select_in_post && !d.fast_orb) { Span s(ctx, kt_select(d)); launch_select(d, st); }
    // The x1/2-octave detectors have run their NMS and described (0: the NMS ran above; 3: none, raster order).  dmORB: the reference's NMS
    // needs positions and responses only, so it runs BEFORE orientation + description and only its survivors are described (unless
    // debug mode 9 has described everything already)
    const bool described = d.fast_orb || d.debug_mode == DBG_DESCRIBE_BEFORE_NMS;
    { Span s(ctx, kt_nms(d)); launch_nms_rowsort(d, ctx->knobs, d.fast_orb ? call.nms_mode_oct : call.nms_mode, p.min_distance, described ? 0 : 1, st); }
    if (!described) { Span s(ctx, KT_DESCRIBE); launch_describe(d, ctx->knobs, 1, st); }
}
static void enqueue_match(svo_ctx* ctx, const FrameCall& call, hipStream_t st)
{
    DevCtx& d = ctx->dc; const svo_params& p = ctx->params;
    Section sec("_stg3"), sec2("stg3.find_pairings");                           // S3:64, 77
    // (the brute-force result words were set to all ones by k_begin_frame)
    if (p.match_method == SVO_SM_DESC_BF) {
        { Span s(ctx, wide_lists(d) ? KT_HAM_LR_WIDE : KT_HAM_LR); launch_hamming(d, ctx->knobs, 0, hamming_splits(ctx), st); }
        { Span s(ctx, KT_LR_FILTER); launch_match_lr_filter(d, p.enable_robust_1to1_match, p.max_y_diff, st); }
    } else if (p.match_method == SVO_SM_DESC_RBR) {         // smDescRbR (stage3_match_left_right.cpp:185-419)
        Span s(ctx, KT_LR_FILTER);
        launch_match_lr_rbr(d, false, p.enable_robust_1to1_match, p.max_y_diff, call.minresp, (int)(size_t)p.orb_max_distance, st);
    } else {                                                // smSAD: the same loop on the gathered windows
        Span s(ctx, KT_LR_SAD);
        launch_match_lr_rbr(d, true, p.enable_robust_1to1_match, p.max_y_diff, call.minresp, call.max_sad_match, st);
    }
}
// The chunks of the RANSAC's sample schedule (set before the tracker kernels: phase 0 of the schedule rides in them).  A handful of
// lanes (one stream on its own): chunk 0 takes chunk 1's samples and more -- a hypothesis + count launch pair is ~20 us of latency
// there, more than evaluating the samples an early bound might have saved.  SVO_RS_C0 = 32 | 160 | 320 forces a form (A/B, tests).
static void set_ransac_chunks(svo_ctx* ctx)
{
    DevCtx& d = ctx->dc;
    const int forced = ctx->knobs.rs_c0;
    d.rs_c0 = forced ? forced : (d.n_lanes * d.n_oct > 8 ? SVO_RANSAC_CHUNK0 : SVO_RANSAC_FEW);
    d.rs_c1 = d.rs_c0 > SVO_RANSAC_CHUNK1 ? d.rs_c0 : SVO_RANSAC_CHUNK1;
}
// F-matrix RANSAC: the first SVO_RANSAC_CHUNK0 hypotheses of the fixed schedule, then two more chunks, each only
// as far as the 0.99-confidence stop of the sequential algorithm can still reach given what has been counted so far
static void enqueue_ransac_chunks(svo_ctx* ctx, hipStream_t st)
{
    DevCtx& d = ctx->dc;
    { Span s(ctx, KT_RANSAC_HYP); launch_ransac_hyp(d, 0, st); }
    { Span s(ctx, KT_RANSAC_CNT); launch_ransac_count(d, ctx->knobs, 0, st); }
    if (d.rs_c0 < d.rs_c1) {
        { Span s(ctx, KT_RANSAC_HYP1); launch_ransac_hyp(d, 1, st); }
        { Span s(ctx, KT_RANSAC_CNT1); launch_ransac_count(d, ctx->knobs, 1, st); }
    }
    { Span s(ctx, KT_RANSAC_HYP2); launch_ransac_hyp(d, 2, st); }
    { Span s(ctx, KT_RANSAC_CNT2); launch_ransac_count(d, ctx->knobs, 2, st); }
}
static void enqueue_track(svo_ctx* ctx, const FrameCall& call, hipStream_t st)
{
    DevCtx& d = ctx->dc; const svo_params& p = ctx->params;
    Section sec("_stg4"), sec2("stg4.track");                                    // S4:76, 457
    const int win = p.ifm_method == SVO_IFM_DESC_WIN || p.ifm_method == SVO_IFM_SAD;
    set_ransac_chunks(ctx);
    if (!win) {
        { Span s(ctx, wide_lists(d) ? KT_HAM_TRK_WIDE : KT_HAM_TRK); launch_hamming(d, ctx->knobs, 1, hamming_splits(ctx), st); }
        { Span s(ctx, wide_lists(d) ? KT_TRK_FILTER_64 : KT_TRK_FILTER); launch_track_filter(d, st); }
    } else if (p.ifm_method == SVO_IFM_DESC_WIN) {          // ifmDescWin (stage4_match_consecutive.cpp:435-738)
        Span s(ctx, KT_TRK_FILTER); launch_track_win(d, false, p.ifm_win_w, p.ifm_win_h, 0u, st);
    } else {                                                // ifmSAD
        Span s(ctx, KT_TRK_SAD); launch_track_win(d, true, p.ifm_win_w, p.ifm_win_h, call.max_sad_track, st);
    }
    enqueue_ransac_chunks(ctx, st);
    { Span s(ctx, KT_TRK_FINAL); launch_track_finalize(d, p.bad_tracking_th, win, st); }
}
// svo_ransac_tracked, and the gate of a step under svo_klt_set_ransac: the RANSAC of stage 4 on the tracked pairs the lanes hold, for
// the lanes DevCtx.idle leaves in.  No bad-tracking gate: the precomputed-data bypass has none
void enqueue_ransac_tracked(svo_ctx* ctx, hipStream_t st)
{
    DevCtx& d = ctx->dc;
    set_ransac_chunks(ctx);
    { Span s(ctx, KT_RANSAC_FEED); launch_ransac_feed(d, st); }
    enqueue_ransac_chunks(ctx, st);
    { Span s(ctx, KT_TRK_FINAL); launch_track_finalize_ungated(d, st); }
    ctx->seen(KG_RANSAC_FEED);
}
void enqueue_optimize(svo_ctx* ctx, const FrameCall&, hipStream_t st)
{
    DevCtx& d = ctx->dc; const svo_params& p = ctx->params;
    Section sec("_stg5");                                                        // S5:398, 729
    GNParams g; memset(&g, 0, sizeof(g));
    g.use_robust_kernel = p.use_robust_kernel; g.max_iters = p.max_iters; g.initial_max_iters = p.initial_max_iters; g.max_incr_cost = p.max_incr_cost;
    g.use_previous_pose_as_initial = p.use_previous_pose_as_initial; g.use_custom_initial_pose = 0;   // processNewImagePair passes no initial estimate (P:338)
    g.min_distance = p.min_distance; g.img_w = d.W; g.img_h = d.H; g.pmax = d.max_kps; g.standalone = 0;
    g.kernel_param = p.kernel_param; g.min_mod_out_vector = p.min_mod_out_vector; g.residual_threshold = p.residual_threshold;
    if (p.use_custom_initial_pose) g.use_custom_initial_pose = 1;        // deltaPose = initial_estimation = zeros (S5:504-505, default argument H:1045)
    if (ctx->pose_cov || ctx->landmarks) g.mask_out = ctx->d_cov_mask;
    { Span s(ctx, KT_GN); launch_gauss_newton(d, ctx->knobs, g, st); }
    if (ctx->pose_cov) { Span s(ctx, KT_POSE_COV); launch_pose_covariance(d, ctx->knobs, g, ctx->d_cov, !ctx->landmarks, st); }
    if (ctx->landmarks) {                                                        // behind k_pose_covariance: cov_cur takes its cov_delta
        LmkArgs a; memset(&a, 0, sizeof(a));
        a.rec = ctx->d_lmk; a.info = ctx->d_lmk_info; a.cnt = ctx->d_lmk_cnt; a.cov = ctx->pose_cov ? ctx->d_cov : nullptr;
        a.std_px = ctx->lmk_std; a.var_px = ctx->lmk_std * ctx->lmk_std; a.ids_on = p.vo_use_matches_ids ? 1 : 0;
        Span s(ctx, KT_LANDMARKS); launch_landmarks(d, g, a, st);
    }
}

// Every lazily allocated buffer a frame may need exists BEFORE a capture begins: hipMalloc / hipMemset are refused on a capturing
// thread and would invalidate the capture.  The adaptive NMS after the FAST+ORB detector has such a buffer, dmFASTER its 64-bit keys;
// the window buffer of smSAD / ifmSAD exists from the first call made while either is selected (a context that never selects them
// allocates and launches nothing).
static int ensure_call_buffers(svo_ctx* ctx, const FrameCall& call)
{
    const DevCtx& d = ctx->dc; const svo_params& p = ctx->params;
    if ((call.flags & SVO_RUN_DETECT) && d.fast_orb && !call.faster && p.non_maximal_suppression && p.nmsMethod == SVO_NMS_ADAPTIVE && !ctx->d_anms)
        HIPCHECK(dev_alloc(ctx, &ctx->d_anms, fastorb_anms_scratch_words(d.n_img, ctx->cand_total_alloc)));
    if ((call.flags & SVO_RUN_DETECT) && call.faster && !ctx->d_cand64) HIPCHECK(dev_alloc(ctx, &ctx->d_cand64, (size_t)d.n_img * ctx->cand_total_alloc));
    return call.sad_any ? ensure_sad_buffers(ctx) : SVO_OK;
}
// what follows the last launch of a call, replayed or not: the armed event of a call that ran as a graph goes behind the whole graph
// (plain launches recorded it right behind the post-processing); stage 2 is the only reader of the level-0 images
static int finish_call(svo_ctx* ctx, const FrameCall& call)
{
    HIPCHECK(record_post_event(ctx, call.runs_post));
    if (call.flags & (SVO_RUN_DETECT | SVO_RUN_DETECT_POST)) HIPCHECK(release_ring_slot(ctx));
    return SVO_OK;
}

// ---- processNewImagePair ---------------------------------------------------------------------------------
// The body of svo_process (lanes == NULL: every lane) and svo_process_lanes (one bit per lane that takes part): what the call is
// (frame_call.hpp), then its launches, stage by stage.
static int process_lanes_body(svo_ctx* ctx, const uint64_t* lanes, bool masked, const svo_frame* frames, uint32_t flags)
{
    const svo_params& p = ctx->params;
    const FrameCall call = make_frame_call(flags, p, ctx->faster_anms);
    // the mask first, without leaving: who is active, who sits out, and whether the mask itself is acceptable
    LaneMask active, idle; std::string why;
    const bool mask_ok = parse_lane_mask(lanes, masked, ctx->cfg.n_lanes, active, idle, why);
    const bool partial = lane_any(idle), nobody = mask_ok && !lane_any(active);
    PostDisarm post_disarm{ ctx, !nobody && call.runs_post };
    if (!mask_ok) { ctx->last_error = why; return SVO_ERR_ARG; }
    if (nobody) return SVO_OK;                              // nothing is enqueued, no state moves
    // the refusals: before anything is enqueued or noted
    { const int rc = check_frame_call(call, p, active, ctx->frame_active_set ? &ctx->frame_active : nullptr, why); if (rc) { ctx->last_error = why; return rc; } }
    DevCtx& d = ctx->dc;
    Section sec_all("processNewImagePair");                                       // P:79, 377
    const hipStream_t st = ctx->stream;
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    // intake: the images of a detect call on their way to the level-0 addresses
    const uint8_t* ptrs[2 * SVO_MAX_LANES];
    PrepArgs prep; memset(&prep, 0, sizeof(prep)); bool prepare = false;
    if (flags & SVO_RUN_DETECT) {
        { const int rc_in = intake_frames(ctx, frames, flags, idle, false, st, ptrs, prep, &prepare); if (rc_in) return rc_in; }
    } else if (!ctx->geom_ready && (flags & (SVO_RUN_MATCH | SVO_RUN_OPTIMIZE))) return SVO_ERR_STATE;
    d.fast_th = ctx->fast_th; d.orb_th = ctx->orb_th;
    if (flags & SVO_RUN_DETECT) d.tl_step++;                 // (a frame of the detect-ahead schedule is a detect call and then a post call)
    { const int rc = ensure_call_buffers(ctx, call); if (rc) return rc; }
    // which frames have their windows after this call; a SAD stage on a frame whose windows were never gathered is refused here
    SadStep step = sad_window_step(ctx->sad, idle, call);
    ctx->sad = std::move(step.next);
    if (step.bad_lane >= 0) { ctx->last_error = step.why; return SVO_ERR_STATE; }
    if (!call.continuation) { ctx->frame_active = active; ctx->frame_active_set = true; }
    d.idle = idle;
    IdleGuard idle_guard{ &d };
    // svo_import_frame writes every lane; the lanes of this call that it wrote and that have had no call since (all of them or none)
    const bool imported_pending = ((ctx->imported.w[0] & active.w[0]) | (ctx->imported.w[1] & active.w[1])) != 0;
    // svo_use_graphs: the launches below are captured once into a hipGraph per (flags, ring slot, thresholds) and replayed:
    // ~30 kernel launches of a frame become one graph launch (what bounds ONE stream is launch latency, not the kernels).
    // (a call with idle lanes runs as plain launches, as one with any_drop does: the mask is a kernel argument)
    const bool graph_ok = ctx->use_graphs && !partial && !prepare && !ctx->cfg.kernel_times && !step.any_drop && (!(flags & SVO_RUN_DETECT) || ctx->det_slot >= 0);
    const uint32_t gflags = flags & ~(uint32_t)(SVO_FLAG_DEVICE_IMAGES | SVO_FLAG_PINNED_IMAGES);
    const int gslot = (flags & SVO_RUN_DETECT) ? ctx->det_slot : -1;
    if (graph_ok && !(p.vo_use_matches_ids && imported_pending)) {                  // (the IDs' first frame after an import changes one kernel argument: not replayable)
        for (auto& g : ctx->graphs)
            if (g.flags == gflags && g.slot == gslot && g.fast_th == ctx->fast_th && g.orb_th == ctx->orb_th) {
                HIPCHECK(hipGraphLaunch(g.exec, st));
                ctx->graph_replays++;
                for (int wd = 0; wd < 2; wd++) ctx->imported.w[wd] &= ~active.w[wd];
                return finish_call(ctx, call);
            }
        HIPCHECK(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal)); ctx->capturing = true;
    }
    CaptureGuard capture_guard{ ctx };
    d.det_ahead = (call.ahead && (flags & SVO_RUN_DETECT)) ? 1 : 0;
    { Span s(ctx, KT_BEGIN); launch_begin_frame(d, (flags & SVO_RUN_DETECT) ? ptrs : nullptr, flags, step.drop_prev, st); if (prepare) { Section sec("_stg1"); launch_prepare(prep, 2 * d.n_lanes, st); } }
    if (flags & SVO_RUN_DETECT) {
        Section sec("_stg2");                                                        // S2:392, 670
        enqueue_detect(ctx, call, st);
        if (!(flags & SVO_FLAG_DETECT_NO_POST)) enqueue_detect_post(ctx, call, st);
    } else if (flags & SVO_RUN_DETECT_POST) {       // the post-processing a SVO_FLAG_DETECT_NO_POST call left out
        if (!ctx->geom_ready) return SVO_ERR_STATE;
        Section sec("_stg2");
        enqueue_detect_post(ctx, call, st);
    }
    // the final keypoint lists exist: the windows of the SAD matchers, while the octave images are still this frame's
    if (call.runs_post && call.sad_any) { Span s(ctx, KT_SAD_PATCH); launch_sad_patch(d, st); }
    // the detector's per-image scratch has had its last reader: the armed event (svo_record_after_post) goes here
    HIPCHECK(record_post_event(ctx, call.runs_post));
    if (flags & SVO_RUN_MATCH) enqueue_match(ctx, call, st);
    if (flags & SVO_RUN_TRACK) enqueue_track(ctx, call, st);
    // (after svo_import_frame the lane may turn out to be at its stream's FIRST frame: the first-frame ID rule of S3:172-173
    // then applies in this call although stage 3 ran in an earlier one)
    if (p.vo_use_matches_ids && (flags & (SVO_RUN_MATCH | SVO_RUN_TRACK))) { Span s(ctx, KT_TRK_FINAL); launch_match_ids(d, flags | (imported_pending ? SVO_RUN_MATCH : 0), st); }
    for (int wd = 0; wd < 2; wd++) ctx->imported.w[wd] &= ~active.w[wd];       // (a lane that sat this call out keeps its bit for its own next call)
    if (flags & SVO_RUN_OPTIMIZE) enqueue_optimize(ctx, call, st);
    if (ctx->capturing) {
        hipGraph_t graph = nullptr;
        ctx->capturing = false;
        HIPCHECK(hipStreamEndCapture(st, &graph));
        hipGraphExec_t exec = nullptr;
        const hipError_t e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        HIPCHECK(e);
        ctx->graphs.push_back({ gflags, gslot, ctx->fast_th, ctx->orb_th, exec });
        HIPCHECK(hipGraphLaunch(exec, st));
    }
    { const int rc = finish_call(ctx, call); if (rc) return rc; }
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_process(svo_ctx* ctx, const svo_frame* frames, uint32_t flags)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    ctx->last_error.clear();                               // svo_last_error speaks of THIS call: a refusal below that sets no text must not inherit an earlier one
    return process_lanes_body(ctx, nullptr, false, frames, flags);
}

// svo_process for the lanes whose bit is set; for the others as if the call had not been made (svo_hip.h)
extern "C" int svo_process_lanes(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, const uint64_t active[2])
{
    SVO_ENTER(ctx);
    return process_lanes_body(ctx, active, true, frames, flags);
}

extern "C" int svo_record_after_post(svo_ctx* ctx, void* event)
{
    if (!ctx) return SVO_ERR_ARG;
    ctx->post_event = (hipEvent_t)event;
    return SVO_OK;
}

// ---- getters ------------------------------------------------------------------------------------------------
static int lane_state(svo_ctx* ctx, int lane, LaneState* s)
{
    int rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(s, ctx->dc.lane + lane, sizeof(LaneState), hipMemcpyDeviceToHost));
    return SVO_OK;
}
static int slot_of(const LaneState& s, int which) { return which ? s.prev_slot : 1 - s.prev_slot; }

// The lists of one lane-octave (vl = lane * oct_cap + octave) in one frame slot: the host's one address computation for every per-lane
// list array of DevCtx (the kernels have feat_base / match_base, svo_device.h)
struct ListAt {
    const DevCtx* d; int vl, slot;
    long long list() const { return (long long)vl * 2 + slot; }                       // [n_vl][2 slots]
    long long feat(int side) const { return list() * 2 + side; }                     // [n_vl][2 slots][2 sides]
    svo_keypoint* kps(int side) const { return d->kps + feat(side) * d->max_kps; }
    uint8_t* desc(int side) const { return d->desc + feat(side) * d->max_kps * 32; }
    int* n_kps(int side) const { return d->n_kps + feat(side); }
    uint8_t* windows(int side) const { return d->sad_patch + feat(side) * d->max_kps * 64; }
    uint8_t* flags(int side) const { return d->sad_flag + feat(side) * d->max_kps; }
    int* row_index(int side) const { return d->row_index + feat(side) * d->max_h; }
    svo_dmatch* matches() const { return d->matches + list() * d->max_kps; }
    int* n_matches() const { return d->n_matches + list(); }
    int* mrow_index() const { return d->mrow_index + list() * (d->max_h + 1); }
    int* ids() const { return d->ids + list() * d->max_kps; }
    int* n_ids() const { return d->n_ids + list(); }
};
static ListAt list_at(const svo_ctx* ctx, int lane, const LaneState& s, int which, int octave) { return { &ctx->dc, lane * ctx->dc.oct_cap + octave, slot_of(s, which) }; }
// the argument check of every entry point that names a list (an entry point without a side passes 0)
static bool bad_list_args(const svo_ctx* ctx, int lane, int which, int side, int octave)
{
    return !ctx || lane < 0 || lane >= ctx->cfg.n_lanes || (which | 1) != 1 || (side | 1) != 1 || octave < 0 || octave >= ctx->dc.oct_cap;
}
static bool frame_absent(const LaneState& s, int which) { return which ? !s.has_prev : !s.has_cur; }
// the tail of a getter of a counted list: the count from the device, and as many entries as the caller has room for.  Returns the
// count, or the status of a failed copy.
static int read_count(svo_ctx* ctx, const int* d_n, int cap, int* m)
{
    int n = 0;
    HIPCHECK(hipMemcpy(&n, d_n, sizeof(int), hipMemcpyDeviceToHost));
    *m = n < cap ? n : cap;
    return n;
}
template <typename T>
static int read_list(svo_ctx* ctx, T* dst, const T* d_src, int m, size_t per = 1)
{
    if (dst && m > 0) HIPCHECK(hipMemcpy(dst, d_src, sizeof(T) * per * m, hipMemcpyDeviceToHost));
    return SVO_OK;
}

extern "C" int svo_get_results(svo_ctx* ctx, svo_result* res)
{
    if (ctx) use_device(ctx);
    if (!ctx || !res) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(res, ctx->dc.results, sizeof(svo_result) * ctx->cfg.n_lanes, hipMemcpyDeviceToHost));
    return SVO_OK;
}
extern "C" int svo_copy_results_async(svo_ctx* ctx, void* dst, size_t bytes)
{
    if (ctx) use_device(ctx);
    if (!ctx || !dst || bytes < sizeof(svo_result) * (size_t)ctx->cfg.n_lanes) return SVO_ERR_ARG;
    note_stream(ctx);
    HIPCHECK(hipMemcpyAsync(dst, ctx->dc.results, sizeof(svo_result) * ctx->cfg.n_lanes, hipMemcpyDeviceToDevice, ctx->stream));
    mark_stream(ctx);
    return SVO_OK;
}
extern "C" int svo_get_result(svo_ctx* ctx, int lane, svo_result* res)
{
    if (ctx) use_device(ctx);
    if (!ctx || !res || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(res, ctx->dc.results + lane, sizeof(svo_result), hipMemcpyDeviceToHost));
    return SVO_OK;
}

extern "C" int svo_get_keypoints_oct(svo_ctx* ctx, int lane, int which, int side, int octave, svo_keypoint* kps, uint8_t* desc, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, side, octave)) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    if (frame_absent(s, which)) return 0;
    const ListAt at = list_at(ctx, lane, s, which, octave);
    int m; const int n = read_count(ctx, at.n_kps(side), cap, &m); if (n < 0) return n;
    if ((rc = read_list(ctx, kps, at.kps(side), m))) return rc;
    if ((rc = read_list(ctx, desc, at.desc(side), m, 32))) return rc;
    return n;
}
extern "C" int svo_get_keypoints(svo_ctx* ctx, int lane, int which, int side, svo_keypoint* kps, uint8_t* desc, int cap)
{
    if (ctx) use_device(ctx);
    return svo_get_keypoints_oct(ctx, lane, which, side, 0, kps, desc, cap);
}

extern "C" int svo_get_row_index(svo_ctx* ctx, int lane, int which, int side, int octave, int32_t* idx, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, side, octave) || !ctx->geom_ready) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    const int H = ctx->dc.oh[octave];
    if ((rc = read_list(ctx, idx, list_at(ctx, lane, s, which, octave).row_index(side), H < cap ? H : cap))) return rc;
    return H;
}

extern "C" int svo_get_matches_oct(svo_ctx* ctx, int lane, int which, int octave, svo_dmatch* mm, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, 0, octave)) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    if (frame_absent(s, which)) return 0;
    const ListAt at = list_at(ctx, lane, s, which, octave);
    int m; const int n = read_count(ctx, at.n_matches(), cap, &m); if (n < 0) return n;
    if ((rc = read_list(ctx, mm, at.matches(), m))) return rc;
    return n;
}
extern "C" int svo_get_matches(svo_ctx* ctx, int lane, int which, svo_dmatch* mm, int cap) { return svo_get_matches_oct(ctx, lane, which, 0, mm, cap); }

// ---- getValues in one synchronisation (H:704-724) ---------------------------------------------------------------
extern "C" int svo_get_values(svo_ctx* ctx, int lane, int which, int octave, svo_values* v)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, 0, octave) || !v || v->cap_kps < 0 || v->cap_matches < 0) return SVO_ERR_ARG;
    const ValuesRecord V{ctx->dc.max_kps};
    if (!ctx->d_vals) {
        ctx->vals_bytes = V.total();
        HIPCHECK(dev_alloc(ctx, &ctx->d_vals, ctx->vals_bytes));
        HIPCHECK(hipHostMalloc((void**)&ctx->h_vals, ctx->vals_bytes, hipHostMallocDefault));
    }
    // whatever the context still has in flight on other streams must be done; the pack + copy below then run on the
    // current stream and the single synchronisation of this call waits for them
    HIPCHECK(sync_foreign(ctx));
    note_stream(ctx);
    launch_pack_values(ctx->dc, lane, which, octave, ctx->d_vals, ctx->stream);
    HIPCHECK(hipMemcpyAsync(ctx->h_vals, ctx->d_vals, ctx->vals_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHECK(hipStreamSynchronize(ctx->stream));                                      // THE synchronisation
    collect_spans(ctx);
    const int32_t* hdr = (const int32_t*)ctx->h_vals;
    v->n_left = hdr[0]; v->n_right = hdr[1]; v->n_matches = hdr[2]; v->n_ids = hdr[3];
    const uint8_t* b = ctx->h_vals;
    const uint8_t* kl = b + V.left_kps(), *kr = b + V.right_kps(), *dl = b + V.left_desc(), *dr = b + V.right_desc(), *mm = b + V.matches(), *ii = b + V.ids();
    const int nl = v->n_left < v->cap_kps ? v->n_left : v->cap_kps, nr = v->n_right < v->cap_kps ? v->n_right : v->cap_kps;
    const int nm = v->n_matches < v->cap_matches ? v->n_matches : v->cap_matches, ni = v->n_ids < v->cap_matches ? v->n_ids : v->cap_matches;
    if (v->left_kps && nl > 0) memcpy(v->left_kps, kl, sizeof(svo_keypoint) * nl);
    if (v->right_kps && nr > 0) memcpy(v->right_kps, kr, sizeof(svo_keypoint) * nr);
    if (v->left_desc && nl > 0) memcpy(v->left_desc, dl, (size_t)32 * nl);
    if (v->right_desc && nr > 0) memcpy(v->right_desc, dr, (size_t)32 * nr);
    if (v->matches && nm > 0) memcpy(v->matches, mm, sizeof(svo_dmatch) * nm);
    if (v->match_ids && ni > 0) memcpy(v->match_ids, ii, sizeof(int32_t) * ni);
    return SVO_OK;
}

extern "C" int svo_get_matches_row_index(svo_ctx* ctx, int lane, int which, int octave, int32_t* idx, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, 0, octave) || !ctx->geom_ready) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    const int H1 = ctx->dc.oh[octave] + 1;
    if ((rc = read_list(ctx, idx, list_at(ctx, lane, s, which, octave).mrow_index(), H1 < cap ? H1 : cap))) return rc;
    return H1;
}

extern "C" int svo_get_tracked_oct(svo_ctx* ctx, int lane, int octave, svo_index_pair* t, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, 0, 0, octave)) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    const int vl = lane * ctx->dc.oct_cap + octave;                          // (one track list per lane-octave: no slot)
    int m; const int n = read_count(ctx, ctx->dc.n_tracked + vl, cap, &m); if (n < 0) return n;
    if ((rc = read_list(ctx, t, ctx->dc.tracked + (long long)vl * ctx->dc.max_kps, m))) return rc;
    return n;
}
extern "C" int svo_get_tracked(svo_ctx* ctx, int lane, svo_index_pair* t, int cap) { return svo_get_tracked_oct(ctx, lane, 0, t, cap); }

extern "C" int svo_get_match_ids(svo_ctx* ctx, int lane, int which, int octave, int32_t* ids, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, 0, octave)) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    if (frame_absent(s, which)) return 0;
    const ListAt at = list_at(ctx, lane, s, which, octave);
    int m; const int n = read_count(ctx, at.n_ids(), cap, &m); if (n < 0) return n;
    if ((rc = read_list(ctx, ids, at.ids(), m))) return rc;
    return n;
}

// resetIds (H:684): the next frame renumbers the previous IDs and becomes the key frame (P:254-267)
extern "C" int svo_reset_ids(svo_ctx* ctx, int lane)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < -1 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    for (int l = 0; l < ctx->cfg.n_lanes; l++)
        if (lane < 0 || lane == l) { LaneState s; int rc = lane_state(ctx, l, &s); if (rc) return rc; s.reset_ids = 1; HIPCHECK(hipMemcpy(ctx->dc.lane + l, &s, sizeof(s), hipMemcpyHostToDevice)); }
    return SVO_OK;
}

// setThisFrameAsKF (H:675-683): m_last_kf_max_id = max ID of the current frame's octave-0 pairings
extern "C" int svo_set_this_frame_as_kf(svo_ctx* ctx, int lane)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    if (!s.has_cur) return SVO_ERR_STATE;                 // ASSERTMSG_ "Current frame does not exist" (H:677)
    const ListAt at = list_at(ctx, lane, s, 0, 0);
    int n = 0;
    HIPCHECK(hipMemcpy(&n, at.n_ids(), sizeof(int), hipMemcpyDeviceToHost));
    if (n <= 0) return SVO_ERR_STATE;
    std::vector<int32_t> ids((size_t)n);
    HIPCHECK(hipMemcpy(ids.data(), at.ids(), sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    int mx = ids[0]; for (int i = 1; i < n; i++) if (ids[i] > mx) mx = ids[i];
    s.last_kf_max_id = mx;
    HIPCHECK(hipMemcpy(ctx->dc.lane + lane, &s, sizeof(s), hipMemcpyHostToDevice));
    return SVO_OK;
}

extern "C" int svo_get_residuals(svo_ctx* ctx, int lane, double* r, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    svo_result res; int rc = svo_get_result(ctx, lane, &res); if (rc) return rc;
    const int n = res.n_residual, m = n < cap ? n : cap;
    if (r && m > 0) HIPCHECK(hipMemcpy(r, ctx->dc.residual + (long long)lane * ctx->dc.max_kps, sizeof(double) * m, hipMemcpyDeviceToHost));
    return n;
}

extern "C" int svo_get_outliers(svo_ctx* ctx, int lane, int32_t* idx, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    svo_result res; int rc = svo_get_result(ctx, lane, &res); if (rc) return rc;
    const int n = res.n_outliers, m = n < cap ? n : cap;
    if (idx && m > 0) HIPCHECK(hipMemcpy(idx, ctx->dc.outliers + (long long)lane * ctx->dc.max_kps, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
    return n;
}

// ---- precomputed-data bypass ----------------------------------------------------------------------------------
static int mark_present(svo_ctx* ctx, int lane, int which)
{
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    if (which) s.has_prev = 1; else s.has_cur = 1;
    HIPCHECK(hipMemcpy(ctx->dc.lane + lane, &s, sizeof(s), hipMemcpyHostToDevice));
    return SVO_OK;
}

extern "C" int svo_put_features_oct(svo_ctx* ctx, int lane, int which, int side, int octave, const svo_keypoint* kps, const uint8_t* desc, int n, int img_w, int img_h)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, side, octave) || n < 0 || (n > 0 && !kps)) return SVO_ERR_ARG;
    if (n > ctx->dc.max_kps) return SVO_ERR_CAPACITY;
    int rc = ensure_geometry(ctx, img_w, img_h); if (rc) return rc;
    if (octave >= ctx->dc.n_oct) return SVO_ERR_ARG;                       // P:139: the octave count of the data must match the system's
    LaneState s; rc = lane_state(ctx, lane, &s); if (rc) return rc;
    const ListAt at = list_at(ctx, lane, s, which, octave);
    if (n > 0) HIPCHECK(hipMemcpy(at.kps(side), kps, sizeof(svo_keypoint) * n, hipMemcpyHostToDevice));
    if (n > 0 && desc) HIPCHECK(hipMemcpy(at.desc(side), desc, (size_t)32 * n, hipMemcpyHostToDevice));
    (which ? ctx->sad.prev : ctx->sad.cur)[lane] = 0;                      // caller features come without an image: no windows for smSAD / ifmSAD (until svo_gather_windows brings one)
    {   // pyr_feats_index of the list just put (m_update_indexes, S2:103-129, as k_nms_rowsort leaves it): idx[r] = #keypoints with (int)y <= r
        // for first_row <= r < last_row, 0 elsewhere.  The reference builds it in stage 2 only, which this path skips; its row-by-row stereo
        // matchers (smDescRbR, smSAD: S3:253-256) would read a table nobody built.  Every entry is <= n whatever the caller's order is.
        const int H = std::max(0, std::min(ctx->dc.oh[octave], ctx->dc.max_h));
        std::vector<int32_t> ri((size_t)H, 0);
        if (n > 0 && H > 0) {
            auto row_of = [](float y) { return y >= 0.0f ? (y < 1.0e9f ? (long long)y : 1000000000LL) : (y > -1.0e9f ? (long long)y : -1000000000LL); };     // (a NaN lands in row 0)
            std::vector<int32_t> cnt((size_t)H + 1, 0);
            for (int i = 0; i < n; i++) { const long long r = row_of(kps[i].y); cnt[(size_t)(r < 0 ? 0 : (r > H ? H : r))]++; }
            const long long first_row = row_of(kps[0].y), last_row = row_of(kps[n - 1].y);
            int acc = 0;
            for (int r = 0; r < H; r++) { acc += cnt[(size_t)r]; if (r >= first_row && r < last_row) ri[(size_t)r] = acc; }
        }
        if (H > 0) HIPCHECK(hipMemcpy(at.row_index(side), ri.data(), sizeof(int32_t) * H, hipMemcpyHostToDevice));
    }
    HIPCHECK(hipMemcpy(at.n_kps(side), &n, sizeof(int), hipMemcpyHostToDevice));
    if (which == 0) {                                                      // result.detected_feats[octave] (P:171-176)
        int32_t* cnt = side ? ctx->dc.results[lane].detected_right : ctx->dc.results[lane].detected_left;
        HIPCHECK(hipMemcpy(cnt + octave, &n, sizeof(int), hipMemcpyHostToDevice));
    }
    return mark_present(ctx, lane, which);
}
extern "C" int svo_put_features(svo_ctx* ctx, int lane, int which, int side, const svo_keypoint* kps, const uint8_t* desc, int n, int img_w, int img_h)
{
    if (ctx) use_device(ctx);
    return svo_put_features_oct(ctx, lane, which, side, 0, kps, desc, n, img_w, img_h);
}

extern "C" int svo_put_matches_oct(svo_ctx* ctx, int lane, int which, int octave, const svo_dmatch* m, int n)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, 0, octave) || n < 0 || (n > 0 && !m)) return SVO_ERR_ARG;
    if (n > ctx->dc.max_kps) return SVO_ERR_CAPACITY;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    const ListAt at = list_at(ctx, lane, s, which, octave);
    if (n > 0) HIPCHECK(hipMemcpy(at.matches(), m, sizeof(svo_dmatch) * n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(at.n_matches(), &n, sizeof(int), hipMemcpyHostToDevice));
    if (which == 0) HIPCHECK(hipMemcpy(ctx->dc.results[lane].stereo_matches + octave, &n, sizeof(int), hipMemcpyHostToDevice));   // P:274-276
    // matches_lr_row_index (S3:425-445) of the list just put.  The reference builds it in stage 3 only, which the precomputed-data path
    // (P:219-251) and the state loader skip: its windowed tracker (S4:517-530) then reads an index nobody built.  Here it is built from the
    // left keypoints put BEFORE the pairings (the oracle's sequential rule, ri[H] = n as there), so that ifmDescWin works on caller data.
    if (ctx->geom_ready && octave < ctx->dc.n_oct) {
        int nl = 0;
        HIPCHECK(hipMemcpy(&nl, at.n_kps(0), sizeof(int), hipMemcpyDeviceToHost));
        nl = std::max(0, std::min(nl, ctx->dc.max_kps));
        bool ok = true;
        for (int i = 0; i < n && ok; i++) ok = m[i].queryIdx >= 0 && m[i].queryIdx < nl;
        if (ok) {
            std::vector<svo_keypoint> kl((size_t)nl);
            if (nl > 0) HIPCHECK(hipMemcpy(kl.data(), at.kps(0), sizeof(svo_keypoint) * nl, hipMemcpyDeviceToHost));
            const int H = std::max(0, std::min(ctx->dc.oh[octave], ctx->dc.max_h));
            std::vector<int32_t> ri((size_t)H + 1);
            int idx = 0;
            for (int y = 0; y < H; y++) {
                ri[y] = idx;
                while (idx < n && kl[m[idx].queryIdx].y <= (float)y) idx++;               // S3:441
            }
            ri[H] = n;
            HIPCHECK(hipMemcpy(at.mrow_index(), ri.data(), sizeof(int32_t) * (H + 1), hipMemcpyHostToDevice));
        }
    }
    return mark_present(ctx, lane, which);
}
extern "C" int svo_put_matches(svo_ctx* ctx, int lane, int which, const svo_dmatch* m, int n) { return svo_put_matches_oct(ctx, lane, which, 0, m, n); }

extern "C" int svo_put_match_ids_oct(svo_ctx* ctx, int lane, int which, int octave, const int32_t* ids, int n)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, 0, octave) || n < 0 || (n > 0 && !ids)) return SVO_ERR_ARG;
    if (n > ctx->dc.max_kps) return SVO_ERR_CAPACITY;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    const ListAt at = list_at(ctx, lane, s, which, octave);
    if (n > 0) HIPCHECK(hipMemcpy(at.ids(), ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(at.n_ids(), &n, sizeof(int), hipMemcpyHostToDevice));
    int mx = octave == 0 ? 0 : s.last_match_id;                                                    // P:236: m_last_match_ID = 0, then the maximum over the octaves (P:243)
    for (int i = 0; i < n; i++) if (ids[i] > mx) mx = ids[i];
    s.last_match_id = mx;
    HIPCHECK(hipMemcpy(ctx->dc.lane + lane, &s, sizeof(s), hipMemcpyHostToDevice));
    return SVO_OK;
}
extern "C" int svo_put_match_ids(svo_ctx* ctx, int lane, int which, const int32_t* ids, int n) { return svo_put_match_ids_oct(ctx, lane, which, 0, ids, n); }

extern "C" int svo_put_tracked(svo_ctx* ctx, int lane, const svo_index_pair* t, int n)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes || n < 0 || (n > 0 && !t)) return SVO_ERR_ARG;
    if (n > ctx->dc.max_kps) return SVO_ERR_CAPACITY;
    int rc = svo_wait(ctx); if (rc) return rc;
    const int vl = lane * ctx->dc.oct_cap;                                   // octave 0; the other octaves of the lane are emptied
    HIPCHECK(hipMemset(ctx->dc.n_tracked + vl, 0, sizeof(int) * ctx->dc.oct_cap));
    if (n > 0) HIPCHECK(hipMemcpy(ctx->dc.tracked + (long long)vl * ctx->dc.max_kps, t, sizeof(svo_index_pair) * n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->dc.n_tracked + vl, &n, sizeof(int), hipMemcpyHostToDevice));
    return SVO_OK;
}
// the tracked pairs of ONE octave; the other octaves of the lane keep theirs (svo_put_tracked is octave 0 and empties the rest)
extern "C" int svo_put_tracked_oct(svo_ctx* ctx, int lane, int octave, const svo_index_pair* t, int n)
{
    if (ctx) use_device(ctx);
    if (!ctx || lane < 0 || lane >= ctx->cfg.n_lanes || octave < 0 || octave >= ctx->dc.oct_cap || n < 0 || (n > 0 && !t)) return SVO_ERR_ARG;
    if (n > ctx->dc.max_kps) return SVO_ERR_CAPACITY;
    int rc = svo_wait(ctx); if (rc) return rc;
    const int vl = lane * ctx->dc.oct_cap + octave;
    if (n > 0) HIPCHECK(hipMemcpy(ctx->dc.tracked + (long long)vl * ctx->dc.max_kps, t, sizeof(svo_index_pair) * n, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(ctx->dc.n_tracked + vl, &n, sizeof(int), hipMemcpyHostToDevice));
    return SVO_OK;
}

// ---- windows for frames the library did not detect --------------------------------------------------------------------
// svo_gather_windows (svo_hip.h): the images of put / loaded lists arrive here, the x1/2 octave images are built from them as a detect
// call builds them, and ONE launch gathers the 8 x 8 window and border flag of every keypoint of slot `which` of the active lanes.
// Plain launches; nothing of the lane state, the records, the lists or the status words is written -- k_begin_frame would do all of
// that, hence k_publish_img0 for the level-0 pointer table.
extern "C" int svo_gather_windows(svo_ctx* ctx, const svo_frame* frames, uint32_t flags, int which, const uint64_t lanes[2])
{
    SVO_ENTER(ctx);
    char msg[200];
    if (which != 0 && which != 1) { snprintf(msg, sizeof(msg), "which = %d: 0 (current frame) or 1 (previous frame)", which); ctx->last_error = msg; return SVO_ERR_ARG; }
    if (flags & ~(uint32_t)(SVO_FLAG_DEVICE_IMAGES | SVO_FLAG_PINNED_IMAGES | SVO_FLAG_BGR_IMAGES)) {
        snprintf(msg, sizeof(msg), "flags %#x: svo_gather_windows takes SVO_FLAG_DEVICE_IMAGES, SVO_FLAG_PINNED_IMAGES and SVO_FLAG_BGR_IMAGES only", flags);
        ctx->last_error = msg; return SVO_ERR_ARG;
    }
    if (!frames) { ctx->last_error = "frames == NULL"; return SVO_ERR_ARG; }
    LaneMask active, idle; std::string why;
    if (!parse_lane_mask(lanes, false, ctx->cfg.n_lanes, active, idle, why)) { ctx->last_error = why; return SVO_ERR_ARG; }      // (NULL: every lane)
    if (!lane_any(active)) return SVO_OK;                  // nobody takes part: nothing is enqueued
    if (!ctx->geom_ready) { ctx->last_error = "no geometry yet: put or load the lists first (svo_set_params clears the geometry of the lists before it)"; return SVO_ERR_STATE; }
    DevCtx& d = ctx->dc;
    const hipStream_t st = ctx->stream;
    const uint8_t* ptrs[2 * SVO_MAX_LANES];
    PrepArgs prep; memset(&prep, 0, sizeof(prep)); bool prepare = false;
    // (the buffers before the intake: a failed allocation must not leave an upload behind)
    { const int rc = ensure_sad_buffers(ctx); if (rc) return rc; }
    note_stream(ctx);
    MarkGuard mark_guard{ ctx };
    { const int rc = intake_frames(ctx, frames, flags, idle, true, st, ptrs, prep, &prepare); if (rc) return rc; }
    d.idle = idle;
    IdleGuard idle_guard{ &d };
    launch_publish_img0(d, ptrs, st);
    if (prepare) { Section sec("_stg1"); launch_prepare(prep, 2 * d.n_lanes, st); }
    if (d.fast_orb) { Span s(ctx, KT_RESIZE); for (int l = 1; l < d.n_levels; l++) launch_half(d, l, st); }       // S1:82-83: the octave images ifmSAD reads its windows from (S4:572, 576)
    { Span s(ctx, KT_GATHER_WIN); launch_sad_patch_slot(d, which, st); }
    for (int l = 0; l < d.n_lanes; l++) if (lane_in(active, l)) (which ? ctx->sad.prev : ctx->sad.cur)[l] = 1;
    // the ring slot's reader is through once the gather is: the slot may take the next upload
    HIPCHECK(release_ring_slot(ctx));
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

extern "C" int svo_get_windows_oct(svo_ctx* ctx, int lane, int which, int side, int octave, uint8_t* win, uint8_t* flag, int cap)
{
    if (ctx) use_device(ctx);
    if (bad_list_args(ctx, lane, which, side, octave)) return SVO_ERR_ARG;
    LaneState s; int rc = lane_state(ctx, lane, &s); if (rc) return rc;
    if (frame_absent(s, which)) return 0;
    if (!ctx->dc.sad_patch || !(which ? ctx->sad.prev : ctx->sad.cur)[lane]) {
        char msg[160]; snprintf(msg, sizeof(msg), "lane %d: the 8 x 8 windows of its %s frame were never gathered", lane, which ? "previous" : "current");
        ctx->last_error = msg; return SVO_ERR_STATE;
    }
    const ListAt at = list_at(ctx, lane, s, which, octave);
    int m; const int n = read_count(ctx, at.n_kps(side), cap, &m); if (n < 0) return n;
    if ((rc = read_list(ctx, win, at.windows(side), m, 64))) return rc;
    if ((rc = read_list(ctx, flag, at.flags(side), m))) return rc;
    return n;
}

// ---- getProjectedCoords (common.cpp:415-466) --------------------------------------------------------------------
// delta = [rotation vector, translation] of the inverse of change_pose (C:456-461); same operations as
// svo_oracle_pose_to_delta (log map through the unit quaternion)
static void pose_to_delta(const double* pose, double* dp)
{
    const double cy = cos(pose[3]), sy = sin(pose[3]), cp = cos(pose[4]), sp = sin(pose[4]), cr = cos(pose[5]), sr = sin(pose[5]);
    const double R[9] = { cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
                          sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
                          -sp, cp * sr, cp * cr };
    const double Ri[9] = { R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8] };
    dp[3] = -(Ri[0] * pose[0] + Ri[1] * pose[1] + Ri[2] * pose[2]);
    dp[4] = -(Ri[3] * pose[0] + Ri[4] * pose[1] + Ri[5] * pose[2]);
    dp[5] = -(Ri[6] * pose[0] + Ri[7] * pose[1] + Ri[8] * pose[2]);
    double q0, q1, q2, q3;
    const double tr = Ri[0] + Ri[4] + Ri[8];
    if (tr > 0.0) { const double s = sqrt(tr + 1.0) * 2.0; q0 = 0.25 * s; q1 = (Ri[7] - Ri[5]) / s; q2 = (Ri[2] - Ri[6]) / s; q3 = (Ri[3] - Ri[1]) / s; }
    else if (Ri[0] > Ri[4] && Ri[0] > Ri[8]) { const double s = sqrt(1.0 + Ri[0] - Ri[4] - Ri[8]) * 2.0; q0 = (Ri[7] - Ri[5]) / s; q1 = 0.25 * s; q2 = (Ri[1] + Ri[3]) / s; q3 = (Ri[2] + Ri[6]) / s; }
    else if (Ri[4] > Ri[8]) { const double s = sqrt(1.0 + Ri[4] - Ri[0] - Ri[8]) * 2.0; q0 = (Ri[2] - Ri[6]) / s; q1 = (Ri[1] + Ri[3]) / s; q2 = 0.25 * s; q3 = (Ri[5] + Ri[7]) / s; }
    else { const double s = sqrt(1.0 + Ri[8] - Ri[0] - Ri[4]) * 2.0; q0 = (Ri[3] - Ri[1]) / s; q1 = (Ri[2] + Ri[6]) / s; q2 = (Ri[5] + Ri[7]) / s; q3 = 0.25 * s; }
    if (q0 < 0.0) { q0 = -q0; q1 = -q1; q2 = -q2; q3 = -q3; }
    const double vn = sqrt(q1 * q1 + q2 * q2 + q3 * q3);
    if (vn < 1e-12) { dp[0] = 2.0 * q1; dp[1] = 2.0 * q2; dp[2] = 2.0 * q3; }
    else { const double k = 2.0 * atan2(vn, q0) / vn; dp[0] = k * q1; dp[1] = k * q2; dp[2] = k * q3; }
}

extern "C" int svo_projected_coords(svo_ctx* ctx, const svo_dmatch* pre_matches, int n_pre, const svo_keypoint* pre_left, int n_left,
                                    const svo_keypoint* pre_right, int n_right, const int32_t* tracked_first,
                                    const svo_stereo_camera* cam, const double* change_pose6, float* pix, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx || n_pre < 0 || (n_pre > 0 && (!pre_matches || !pre_left || !pre_right || !tracked_first)) || !cam || !change_pose6) return SVO_ERR_ARG;
    std::vector<float> uvu;
    for (int m = 0; m < n_pre; m++) {
        if (tracked_first[m] != -1) continue;                                   // C:430-431
        const int l = pre_matches[m].queryIdx, r = pre_matches[m].trainIdx;
        if (l < 0 || l >= n_left || r < 0 || r >= n_right) return SVO_ERR_ARG;
        uvu.push_back(pre_left[l].x); uvu.push_back(pre_left[l].y); uvu.push_back(pre_right[r].x);
    }
    const int nb = (int)(uvu.size() / 3);
    if (!pix || cap < nb || nb == 0) return nb;                                 // size query / nothing to do
    double dp[6]; pose_to_delta(change_pose6, dp);
    float* d_in = nullptr, *d_out = nullptr;
    HIPCHECK(hipMalloc((void**)&d_in, uvu.size() * sizeof(float)));
    hipError_t e = hipMalloc((void**)&d_out, (size_t)nb * 4 * sizeof(float));
    if (e != hipSuccess) { hipFree(d_in); HIPCHECK(e); }
    const hipStream_t st = ctx->stream;
    e = hipMemcpyAsync(d_in, uvu.data(), uvu.size() * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) { launch_project_points(d_in, nb, *cam, dp, d_out, st); e = hipMemcpyAsync(pix, d_out, (size_t)nb * 4 * sizeof(float), hipMemcpyDeviceToHost, st); }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    hipFree(d_in); hipFree(d_out);
    HIPCHECK(e);
    return nb;
}

// ---- frame hand-over between contexts (k_handover.hip) ----------------------------------------------------------
extern "C" size_t svo_handover_bytes(const svo_ctx* ctx)
{
    return ctx ? handover_record_bytes(ctx->dc) * (size_t)ctx->dc.n_lanes * (size_t)ctx->dc.oct_cap : 0;
}
// the window buffers of the SAD matchers, from the first call that may need them (never while a stream captures: hipMalloc is refused there)
static int ensure_sad_buffers(svo_ctx* ctx)
{
    DevCtx& d = ctx->dc;
    if (d.sad_patch) return SVO_OK;
    const size_t nk = (size_t)d.n_lanes * d.oct_cap * 4 * d.max_kps;
    HIPCHECK(dev_alloc(ctx, &d.sad_flag, nk));
    HIPCHECK(dev_alloc(ctx, &d.sad_patch, nk * 64));
    return SVO_OK;
}
extern "C" int svo_export_frame(svo_ctx* ctx, void* dev_blob, size_t bytes)
{
    if (ctx) use_device(ctx);
    if (!ctx || !dev_blob || bytes < svo_handover_bytes(ctx)) return SVO_ERR_ARG;
    if (ctx->dc.carry_win && ((uintptr_t)dev_blob & 15)) { ctx->last_error = "a hand-over record with windows is copied in 16-byte pieces: the buffer must be 16-byte aligned"; return SVO_ERR_ARG; }
    if (!ctx->geom_once) return SVO_ERR_STATE;            // (new parameters since the last frame do not unmake its lists: svo_fpstream_set_params exports again in mid-stream)
    note_stream(ctx);
    LaneMask win_cur, win_prev; memset(&win_cur, 0, sizeof(win_cur)); memset(&win_prev, 0, sizeof(win_prev));
    for (int l = 0; l < ctx->cfg.n_lanes; l++) {
        if (ctx->sad.cur[l]) win_cur.w[l >> 6] |= 1ull << (l & 63);
        if (ctx->sad.prev[l] && !ctx->sad.drop[l]) win_prev.w[l >> 6] |= 1ull << (l & 63);
    }
    { Span s(ctx, ctx->dc.carry_win ? KT_EXPORT_WIN : KT_EXPORT); launch_export_frame(ctx->dc, (uint8_t*)dev_blob, win_cur, win_prev, ctx->stream); }
    mark_stream(ctx);
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}
extern "C" int svo_import_frame(svo_ctx* ctx, const void* dev_blob, size_t bytes)
{
    if (ctx) use_device(ctx);
    // (a context that carries windows also takes the shorter records of one that does not: the kernel is told the buffer's size)
    if (!ctx || !dev_blob || bytes < handover_record_bytes(ctx->dc, false) * (size_t)ctx->dc.n_lanes * (size_t)ctx->dc.oct_cap) return SVO_ERR_ARG;
    if (!ctx->dc.carry_win && bytes < svo_handover_bytes(ctx)) return SVO_ERR_ARG;
    if (ctx->dc.carry_win && ((uintptr_t)dev_blob & 15)) { ctx->last_error = "a hand-over record with windows is copied in 16-byte pieces: the buffer must be 16-byte aligned"; return SVO_ERR_ARG; }
    if (!ctx->geom_ready) return SVO_ERR_STATE;
    if (ctx->dc.carry_win) { const int rc = ensure_sad_buffers(ctx); if (rc) return rc; }
    note_stream(ctx);
    const int need_windows = ctx->params.ifm_method == SVO_IFM_SAD ? 1 : 0;
    { Span s(ctx, ctx->dc.carry_win ? KT_IMPORT_WIN : KT_IMPORT); launch_import_frame(ctx->dc, (const uint8_t*)dev_blob, bytes, need_windows, ctx->stream); }
    for (int l = 0; l < ctx->cfg.n_lanes; l++) ctx->imported.w[l >> 6] |= 1ull << (l & 63);
    // a record without windows leaves none behind; one with them brings them, and where it does not (an older kind of record, a frame
    // whose windows were never gathered) the device has already made the lane start afresh if the tracker in force is ifmSAD
    for (int l = 0; l < ctx->cfg.n_lanes; l++) { ctx->sad.prev[l] = ctx->dc.carry_win ? 1 : 0; if (ctx->dc.carry_win) ctx->sad.drop[l] = 0; }
    mark_stream(ctx);
    HIPCHECK(hipGetLastError());
    return SVO_OK;
}

// ---- saveStateToFile / loadStateFromFile (common.cpp:475-543, 261-350; helpers :88-255) --------------------------
// The bytes are state_format.cpp's business (host only, exercised under sanitizers by tools/state_format_fuzz.cpp); here the lists
// move between the device and a svo_state::State.
// the octave count the parameters in force give a frame (ensure_geometry)
static int params_n_oct(const svo_params& p)
{
    const bool fast_orb = p.detect_method == SVO_DM_FAST_ORB || p.detect_method == SVO_DM_FASTER;
    return fast_orb ? (p.nOctaves < 1 ? 1 : p.nOctaves) : 1;
}

extern "C" int svo_save_state(svo_ctx* ctx, int lane, const char* path)
{
    if (ctx) use_device(ctx);
    if (!ctx || !path || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    LaneState s; rc = lane_state(ctx, lane, &s); if (rc) return rc;
    const int n_oct = ctx->dc.n_oct;
    svo_state::State S;                                                                    // frame[0] = PRE (which 1), frame[1] = CUR (which 0)
    for (int f = 0; f < 2; f++) {
        const int which = 1 - f;
        S.frame[f].resize((size_t)n_oct);
        for (int o = 0; o < n_oct; o++) {
            svo_state::Group& G = S.frame[f][(size_t)o];
            for (int side = 0; side < 2; side++) {
                svo_state::List& L = side ? G.right : G.left;
                const int n = svo_get_keypoints_oct(ctx, lane, which, side, o, nullptr, nullptr, 0); if (n < 0) return n;
                L.kps.resize((size_t)n); L.desc.resize((size_t)n * 32);
                if (n) { rc = svo_get_keypoints_oct(ctx, lane, which, side, o, L.kps.data(), L.desc.data(), n); if (rc < 0) return rc; }
            }
            int n = svo_get_matches_oct(ctx, lane, which, o, nullptr, 0); if (n < 0) return n;
            G.matches.resize((size_t)n); if (n) { rc = svo_get_matches_oct(ctx, lane, which, o, G.matches.data(), n); if (rc < 0) return rc; }
            n = svo_get_match_ids(ctx, lane, which, o, nullptr, 0); if (n < 0) return n;
            G.ids.resize((size_t)n); if (n) { rc = svo_get_match_ids(ctx, lane, which, o, G.ids.data(), n); if (rc < 0) return rc; }
        }
        // the frame's windows travel when it exists and they were gathered ("true" on the host also stands for "no such frame yet")
        const bool present = which ? s.has_prev != 0 : s.has_cur != 0;
        S.has_win[f] = (present && ctx->dc.sad_patch && (which ? ctx->sad.prev : ctx->sad.cur)[lane]) ? 1 : 0;
        if (!S.has_win[f]) continue;
        S.win[f].resize((size_t)2 * n_oct);
        for (int o = 0; o < n_oct; o++)
            for (int side = 0; side < 2; side++) {
                svo_state::Windows& Wn = S.win[f][(size_t)o * 2 + side];
                const int n = svo_get_windows_oct(ctx, lane, which, side, o, nullptr, nullptr, 0); if (n < 0) return n;
                Wn.flag.resize((size_t)n); Wn.win.resize((size_t)n * 64);
                if (n) { rc = svo_get_windows_oct(ctx, lane, which, side, o, Wn.win.data(), Wn.flag.data(), n); if (rc < 0) return rc; }
                // (a flagged keypoint has no window: whatever the buffer held there does not belong in a file)
                for (int i = 0; i < n; i++) if (Wn.flag[(size_t)i]) memset(Wn.win.data() + (size_t)i * 64, 0, 64);
            }
    }
    svo_result res; HIPCHECK(hipMemcpy(&res, ctx->dc.results + lane, sizeof(res), hipMemcpyDeviceToHost));
    S.npyr = (uint64_t)n_oct;                                                              // C:488-489
    S.m_reset = s.reset_ids ? 1 : 0;
    S.tail[0] = 0 /* m_lastID: legacy, never used */; S.tail[1] = (uint64_t)s.num_tracked_last_kf; S.tail[2] = (uint64_t)res.tracked_feats_from_last_frame;
    S.tail[3] = (uint64_t)s.last_match_id; S.tail[4] = (uint64_t)s.last_kf_max_id;
    // the extension block: only where the reference's layout cannot hold the state (more octaves than one, or windows)
    S.has_ext = n_oct > 1 || S.has_win[0] || S.has_win[1];
    S.n_oct = (uint32_t)n_oct; S.w = (uint32_t)ctx->dc.W; S.h = (uint32_t)ctx->dc.H;
    std::vector<uint8_t> bytes;
    if (!svo_state::write(S, bytes)) { ctx->last_error = "internal: inconsistent state record"; return SVO_ERR_STATE; }
    FILE* f = fopen(path, "wb");
    if (!f) { ctx->last_error = std::string("cannot open ") + path; return SVO_ERR_ARG; }
    bool ok = fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    ok = (fclose(f) == 0) && ok;
    if (!ok) { ctx->last_error = std::string("short write to ") + path; return SVO_ERR_STATE; }
    return SVO_OK;
}

extern "C" int svo_load_state(svo_ctx* ctx, int lane, const char* path)
{
    if (ctx) use_device(ctx);
    if (!ctx || !path || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    std::vector<uint8_t> bytes;
    {
        FILE* f = fopen(path, "rb");
        if (!f) { ctx->last_error = std::string("cannot open ") + path; return SVO_ERR_ARG; }
        uint8_t chunk[1 << 16]; size_t k;
        while ((k = fread(chunk, 1, sizeof(chunk), f)) > 0) bytes.insert(bytes.end(), chunk, chunk + k);
        fclose(f);
    }
    // the whole file is validated before the lane is touched
    svo_state::State S; std::string why;
    if (!svo_state::parse(bytes.data(), bytes.size(), (size_t)ctx->dc.max_kps, S, why)) { ctx->last_error = std::string("malformed or truncated state file ") + path + ": " + why; return SVO_ERR_ARG; }
    const int ctx_oct = params_n_oct(ctx->params);
    char msg[200];
    if ((int)S.n_oct != ctx_oct) {                         // (a file of the reference's layout alone holds octave 0: n_oct = 1)
        snprintf(msg, sizeof(msg), "the state file holds n_oct = %u%s, the context's parameters give n_oct = %d", S.n_oct, S.has_ext ? "" : " (no extension block: octave 0 only)", ctx_oct);
        ctx->last_error = msg; return SVO_ERR_ARG;
    }
    if (S.has_ext && ((int)S.w > ctx->cfg.max_w || (int)S.h > ctx->cfg.max_h || S.w < 64 || S.h < 64)) {
        snprintf(msg, sizeof(msg), "the state file's image size %u x %u is outside what the context takes (64 x 64 .. %d x %d)", S.w, S.h, ctx->cfg.max_w, ctx->cfg.max_h);
        ctx->last_error = msg; return SVO_ERR_ARG;
    }
    if (S.has_ext && ctx_oct > ctx->dc.oct_cap) return SVO_ERR_CAPACITY;
    // a file without the block carries no image size: the geometry of the last frame, or the context's maximum for a fresh context
    const int gw = S.has_ext ? (int)S.w : (ctx->geom_ready ? ctx->geom_w : ctx->cfg.max_w), gh = S.has_ext ? (int)S.h : (ctx->geom_ready ? ctx->geom_h : ctx->cfg.max_h);
    const bool any_win = S.has_win[0] || S.has_win[1];
    int rc = ensure_geometry(ctx, gw, gh); if (rc) return rc;                             // (refusals of the geometry come before the lane is reset)
    if (any_win) { rc = ensure_sad_buffers(ctx); if (rc) return rc; }
    rc = svo_reset(ctx, lane); if (rc) return rc;
    const int n_oct = S.has_ext ? (int)S.n_oct : 1;
    for (int f = 0; f < 2; f++) {                                                        // PRE, then CUR
        const int which = 1 - f;
        for (int o = 0; o < n_oct; o++) {
            const svo_state::Group& G = S.frame[f][(size_t)o];
            for (int side = 0; side < 2; side++) {
                const svo_state::List& L = side ? G.right : G.left;
                rc = svo_put_features_oct(ctx, lane, which, side, o, L.kps.data(), L.desc.data(), (int)L.kps.size(), gw, gh);
                if (rc) return rc;
            }
            rc = svo_put_matches_oct(ctx, lane, which, o, G.matches.data(), (int)G.matches.size()); if (rc) return rc;
            rc = svo_put_match_ids_oct(ctx, lane, which, o, G.ids.data(), (int)G.ids.size()); if (rc) return rc;   // (last_match_id: the file's tail, below)
            if (!S.has_win[f]) continue;
            LaneState s; rc = lane_state(ctx, lane, &s); if (rc) return rc;
            const ListAt at = list_at(ctx, lane, s, which, o);
            for (int side = 0; side < 2; side++) {
                const svo_state::Windows& Wn = S.win[f][(size_t)o * 2 + side];
                if (Wn.flag.empty()) continue;
                HIPCHECK(hipMemcpy(at.flags(side), Wn.flag.data(), Wn.flag.size(), hipMemcpyHostToDevice));
                HIPCHECK(hipMemcpy(at.windows(side), Wn.win.data(), Wn.win.size(), hipMemcpyHostToDevice));
            }
        }
        (which ? ctx->sad.prev : ctx->sad.cur)[lane] = S.has_win[f];                      // (svo_put_features_oct cleared it: lists without an image)
    }
    LaneState s; rc = lane_state(ctx, lane, &s); if (rc) return rc;
    s.reset_ids = S.m_reset; s.num_tracked_last_kf = (int)S.tail[1]; s.last_match_id = (int)S.tail[3]; s.last_kf_max_id = (int)S.tail[4];
    HIPCHECK(hipMemcpy(ctx->dc.lane + lane, &s, sizeof(s), hipMemcpyHostToDevice));
    return SVO_OK;
}

// ---- getChangeInPose (common.cpp:355-413) -------------------------------------------------------------------
// The reference packs the caller's arrays into TEMPORARY TImagePairData / TTrackingData (C:362-400) and runs
// stage5_optimize on them: m_prev_imgpair / m_current_imgpair are not touched.  The only estimator members the call
// shares with the pipeline are the ones stage 5 itself reads and writes: m_last_computed_pose (S5:506-507, 720-721)
// and m_error (S5:380-386).  Same here: the Gauss-Newton kernel runs on a ONE-LANE SCRATCH VIEW of the device context
// (its own keypoint / pairing / track / residual buffers and lane record); lane 0's warm start and m_error are copied
// into it before the launch and back afterwards, nothing else of the live lanes is read or written.
static int ensure_cip(svo_ctx* ctx)
{
    if (ctx->cip_ready) return SVO_OK;
    DevCtx& s = ctx->cip;
    s = ctx->dc;
    const int MK = ctx->dc.max_kps;
    s.n_lanes = 1; s.n_img = 2; s.oct_cap = 1; s.n_oct = 1;
    HIPCHECK(dev_alloc(ctx, &s.kps, (size_t)4 * MK));
    HIPCHECK(dev_alloc(ctx, &s.n_kps, (size_t)4));
    HIPCHECK(dev_alloc(ctx, &s.matches, (size_t)2 * MK));
    HIPCHECK(dev_alloc(ctx, &s.n_matches, (size_t)2));
    HIPCHECK(dev_alloc(ctx, &s.tracked, (size_t)MK));
    HIPCHECK(dev_alloc(ctx, &s.n_tracked, (size_t)1));
    HIPCHECK(dev_alloc(ctx, &s.trk_kq, (size_t)MK));
    HIPCHECK(dev_alloc(ctx, &s.gn_lmk, (size_t)MK * 3));
    HIPCHECK(dev_alloc(ctx, &s.gn_obs, (size_t)MK * 8));
    HIPCHECK(dev_alloc(ctx, &s.residual, (size_t)MK));
    HIPCHECK(dev_alloc(ctx, &s.outliers, (size_t)MK));
    HIPCHECK(dev_alloc(ctx, &s.cams, (size_t)1));
    HIPCHECK(dev_alloc(ctx, &s.lane, (size_t)1));
    HIPCHECK(dev_alloc(ctx, &s.results, (size_t)1));
    HIPCHECK(dev_alloc(ctx, &s.status, (size_t)1));
    ctx->cip_ready = true;
    return SVO_OK;
}

extern "C" int svo_change_in_pose(svo_ctx* ctx, const svo_index_pair* tracked, int n_tracked,
                                  const svo_dmatch* pre_matches, int n_pre, const svo_dmatch* cur_matches, int n_cur,
                                  const svo_keypoint* pre_left, int n_pl, const svo_keypoint* pre_right, int n_pr,
                                  const svo_keypoint* cur_left, int n_cl, const svo_keypoint* cur_right, int n_cr,
                                  const svo_stereo_camera* cam, const double* init6,
                                  svo_result* res, double* residual, int32_t* outliers)
{
    if (ctx) use_device(ctx);
    if (!ctx || !cam || !res || n_tracked < 0 || n_pre < 0 || n_cur < 0 || n_pl < 0 || n_pr < 0 || n_cl < 0 || n_cr < 0) return SVO_ERR_ARG;
    if ((n_tracked > 0 && !tracked) || (n_pre > 0 && !pre_matches) || (n_cur > 0 && !cur_matches) || (n_pl > 0 && !pre_left) ||
        (n_pr > 0 && !pre_right) || (n_cl > 0 && !cur_left) || (n_cr > 0 && !cur_right)) return SVO_ERR_ARG;
    if (cam->ncols < 1 || cam->nrows < 1) return SVO_ERR_ARG;
    const svo_params& p = ctx->params;
    const int MK = ctx->dc.max_kps;
    if (n_tracked > MK || n_pre > MK || n_cur > MK || n_pl > MK || n_pr > MK || n_cl > MK || n_cr > MK) return SVO_ERR_CAPACITY;
    int rc = svo_wait(ctx); if (rc) return rc;
    if ((rc = ensure_cip(ctx))) return rc;
    DevCtx& s = ctx->cip;
    s.debug_mode = ctx->dc.debug_mode;
    s.W = cam->ncols; s.H = cam->nrows; s.ow[0] = cam->ncols; s.oh[0] = cam->nrows;      // common.cpp:402-403
    // lane record of the scratch lane: slot 0 = previous, slot 1 = current, both present; warm start and m_error of lane 0
    LaneState live; HIPCHECK(hipMemcpy(&live, ctx->dc.lane, sizeof(live), hipMemcpyDeviceToHost));
    LaneState ls = live; ls.prev_slot = 0; ls.has_prev = 1; ls.has_cur = 1;
    HIPCHECK(hipMemcpy(s.lane, &ls, sizeof(ls), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(s.cams, cam, sizeof(*cam), hipMemcpyHostToDevice));
    const svo_keypoint* kp[4] = { pre_left, pre_right, cur_left, cur_right };        // (slot 0: prev | slot 1: cur) x (left, right)
    const int nk[4] = { n_pl, n_pr, n_cl, n_cr };
    for (int i = 0; i < 4; i++) if (nk[i] > 0) HIPCHECK(hipMemcpy(s.kps + (size_t)i * MK, kp[i], sizeof(svo_keypoint) * nk[i], hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(s.n_kps, nk, sizeof(nk), hipMemcpyHostToDevice));
    if (n_pre > 0) HIPCHECK(hipMemcpy(s.matches, pre_matches, sizeof(svo_dmatch) * n_pre, hipMemcpyHostToDevice));
    if (n_cur > 0) HIPCHECK(hipMemcpy(s.matches + MK, cur_matches, sizeof(svo_dmatch) * n_cur, hipMemcpyHostToDevice));
    const int nm[2] = { n_pre, n_cur };
    HIPCHECK(hipMemcpy(s.n_matches, nm, sizeof(nm), hipMemcpyHostToDevice));
    if (n_tracked > 0) HIPCHECK(hipMemcpy(s.tracked, tracked, sizeof(svo_index_pair) * n_tracked, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(s.n_tracked, &n_tracked, sizeof(int), hipMemcpyHostToDevice));
    svo_result r0; memset(&r0, 0, sizeof(r0)); r0.n_octaves = 1;                         // what k_begin_frame leaves in a result record
    HIPCHECK(hipMemcpy(s.results, &r0, sizeof(r0), hipMemcpyHostToDevice));
    HIPCHECK(hipMemset(s.status, 0, sizeof(uint32_t)));
    GNParams g; memset(&g, 0, sizeof(g));
    g.use_robust_kernel = p.use_robust_kernel; g.max_iters = p.max_iters; g.initial_max_iters = p.initial_max_iters; g.max_incr_cost = p.max_incr_cost;
    g.use_previous_pose_as_initial = p.use_previous_pose_as_initial; g.use_custom_initial_pose = p.use_custom_initial_pose;
    g.min_distance = p.min_distance; g.img_w = cam->ncols; g.img_h = cam->nrows;      // common.cpp:402-403
    g.pmax = MK; g.standalone = 1;
    g.kernel_param = p.kernel_param; g.min_mod_out_vector = p.min_mod_out_vector; g.residual_threshold = p.residual_threshold;
    for (int k = 0; k < 6; k++) g.init[k] = init6 ? init6[k] : 0.0;
    note_stream(ctx);
    // (the scratch lane's record of the covariance is lane 0's, and its mask goes through lane 0's part of the mask array: svo_wait above)
    if (ctx->pose_cov) g.mask_out = ctx->d_cov_mask;
    { Span sp(ctx, KT_GN); launch_gauss_newton(s, ctx->knobs, g, ctx->stream); }
    // (svo_set_landmarks does not reach this entry point: no records are written here, and this launch consumes the mask itself)
    if (ctx->pose_cov) { Span sp(ctx, KT_POSE_COV); launch_pose_covariance(s, ctx->knobs, g, ctx->d_cov, true, ctx->stream); }
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(ctx->stream));
    HIPCHECK(hipMemcpy(res, s.results, sizeof(*res), hipMemcpyDeviceToHost));
    if (residual && res->n_residual > 0) HIPCHECK(hipMemcpy(residual, s.residual, sizeof(double) * res->n_residual, hipMemcpyDeviceToHost));
    if (outliers && res->n_outliers > 0) HIPCHECK(hipMemcpy(outliers, s.outliers, sizeof(int32_t) * res->n_outliers, hipMemcpyDeviceToHost));
    // m_last_computed_pose and m_error are the estimator's own members: hand them back to lane 0
    HIPCHECK(hipMemcpy(&ls, s.lane, sizeof(ls), hipMemcpyDeviceToHost));
    for (int k = 0; k < 6; k++) live.last_pose[k] = ls.last_pose[k];
    live.m_error = ls.m_error;
    HIPCHECK(hipMemcpy(ctx->dc.lane, &live, sizeof(live), hipMemcpyHostToDevice));
    return res->valid;
}

// ---- standalone brute-force matcher -------------------------------------------------------------------------
extern "C" int svo_hamming_match(svo_ctx* ctx, const uint8_t* query, int nq, const uint8_t* train, int nt, int32_t* idx, int32_t* dist)
{
    if (ctx) use_device(ctx);
    if (!ctx || nq < 0 || nt < 0 || (nq > 0 && (!query || !idx || !dist)) || (nt > 0 && !train)) return SVO_ERR_ARG;
    if (nt > 65535) return SVO_ERR_UNSUPPORTED;            // train index packs into 16 bits
    if (nq == 0) return SVO_OK;
    if (nt == 0) { for (int i = 0; i < nq; i++) { idx[i] = -1; dist[i] = 0; } return SVO_OK; }
    if (nq > ctx->ham_cap_q) {
        if (ctx->d_ham_q) hipFree(ctx->d_ham_q); if (ctx->d_ham_out) hipFree(ctx->d_ham_out);
        ctx->d_ham_q = nullptr; ctx->d_ham_out = nullptr; ctx->ham_cap_q = 0;
        HIPCHECK(hipMalloc((void**)&ctx->d_ham_q, (size_t)nq * 32)); HIPCHECK(hipMalloc((void**)&ctx->d_ham_out, (size_t)nq * 4)); ctx->ham_cap_q = nq;
    }
    if (nt > ctx->ham_cap_t) {
        if (ctx->d_ham_t) hipFree(ctx->d_ham_t);
        ctx->d_ham_t = nullptr; ctx->ham_cap_t = 0;
        HIPCHECK(hipMalloc((void**)&ctx->d_ham_t, (size_t)nt * 32)); ctx->ham_cap_t = nt;
    }
    const hipStream_t st = ctx->stream;
    HIPCHECK(hipMemcpyAsync(ctx->d_ham_q, query, (size_t)nq * 32, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemcpyAsync(ctx->d_ham_t, train, (size_t)nt * 32, hipMemcpyHostToDevice, st));
    HIPCHECK(hipMemsetAsync(ctx->d_ham_out, 0xFF, (size_t)nq * 4, st));
    const int tiles = (nt + 255) / 256;
    int nsplit = 1; while (nsplit < 16 && nsplit * 2 <= tiles && ((nq + 255) / 256) * nsplit < 1024) nsplit *= 2;
    launch_hamming_plain(ctx->d_ham_q, nq, ctx->d_ham_t, nt, ctx->d_ham_out, nsplit, st);
    std::vector<unsigned> out((size_t)nq);
    HIPCHECK(hipMemcpyAsync(out.data(), ctx->d_ham_out, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHECK(hipStreamSynchronize(st));
    for (int i = 0; i < nq; i++) { idx[i] = (int)(out[i] & 0xFFFFu); dist[i] = (int)(out[i] >> 16); }
    return SVO_OK;
}

// ---- probes ------------------------------------------------------------------------------------------------
extern "C" int svo_debug_get_level(svo_ctx* ctx, int lane, int side, int level, uint8_t* out, int cap, int* w, int* h)
{
    if (ctx) use_device(ctx);
    if (!ctx || !ctx->geom_ready || lane < 0 || lane >= ctx->cfg.n_lanes || level < 0 || level >= ctx->dc.n_levels) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    const LevelGeom& g = ctx->dc.lv[level];
    if (w) *w = g.w; if (h) *h = g.h;
    if (!out) return g.w * g.h;
    if (cap < g.w * g.h) return SVO_ERR_CAPACITY;
    const int img = lane * 2 + side;
    const uint8_t* src; int pitch;
    if (level == 0) { const uint8_t* p0 = nullptr; HIPCHECK(hipMemcpy(&p0, ctx->dc.img0 + img, sizeof(p0), hipMemcpyDeviceToHost)); src = p0; pitch = ctx->dc.img0_pitch; if (!src) return SVO_ERR_STATE; }
    else { src = ctx->dc.pyr + (long long)img * ctx->dc.pyr_bytes + g.offset; pitch = g.pitch; }
    HIPCHECK(hipMemcpy2D(out, (size_t)g.w, src, (size_t)pitch, (size_t)g.w, (size_t)g.h, hipMemcpyDeviceToHost));
    return g.w * g.h;
}

extern "C" int svo_debug_get_raw_keypoints(svo_ctx* ctx, int lane, int side, svo_keypoint* kps, uint8_t* desc, int cap)
{
    if (ctx) use_device(ctx);
    if (!ctx || !ctx->geom_ready || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    const DevCtx& d = ctx->dc;
    const int img = lane * 2 + side;
    int ln[SVO_MAX_LEVELS];
    HIPCHECK(hipMemcpy(ln, d.lvl_n + img * SVO_MAX_LEVELS, sizeof(ln), hipMemcpyDeviceToHost));
    int n = 0;
    for (int l = 0; l < d.n_levels; l++) {
        for (int i = 0; i < ln[l]; i++, n++) {
            if (n >= cap) continue;
            const long long o = (long long)img * d.raw_cap + d.lv[l].slot_off + i;
            if (kps) HIPCHECK(hipMemcpy(kps + n, d.raw_kps + o, sizeof(svo_keypoint), hipMemcpyDeviceToHost));
            if (desc) HIPCHECK(hipMemcpy(desc + (size_t)n * 32, d.raw_desc + o * 32, 32, hipMemcpyDeviceToHost));
        }
    }
    return n;
}

extern "C" int svo_debug_get_redo_count(svo_ctx* ctx, uint32_t* pairs, int reset)
{
    if (ctx) use_device(ctx);
    if (!ctx || !pairs) return SVO_ERR_ARG;
    HIPCHECK(sync_all(ctx));
    HIPCHECK(hipMemcpy(pairs, ctx->dc.redo_n + 1, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (reset) HIPCHECK(hipMemset(ctx->dc.redo_n + 1, 0, sizeof(uint32_t)));
    return SVO_OK;
}

// SVO_TIMELINE=1: the launch hulls of the last SVO_TL_STEPS frames, 4096 records of (t0, t1) in 10 ns ticks of the device-wide wall clock
// (t0 = ~0: no such launch); record index = (frame % 16) * 256 + kind * 8 + aux (svo_device.h).  Each is the min / max over the launch's
// stamping waves.  Returns the frame counter; reset = 1 clears the table.  0 when the context was created without SVO_TIMELINE=1.
// Waits for the enqueued work.
extern "C" int svo_debug_timeline(svo_ctx* ctx, uint64_t* out, int cap_records, int reset)
{
    if (ctx) use_device(ctx);
    if (!ctx) return SVO_ERR_ARG;
    if (!ctx->dc.tl) return 0;
    const int n = SVO_TL_STEPS * 256;
    int rc = svo_wait(ctx); if (rc) return rc;
    std::vector<TlRec> all((size_t)n * SVO_TL_SUB);
    if (out) {
        if (cap_records < n) return SVO_ERR_ARG;
        HIPCHECK(hipMemcpy(all.data(), ctx->dc.tl, all.size() * sizeof(TlRec), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++) {
            uint64_t t0 = ~0ull, t1 = 0;
            for (int j = 0; j < SVO_TL_SUB; j++) { const TlRec& r = all[(size_t)i * SVO_TL_SUB + j]; if (r.t0 != ~0ull) { if (r.t0 < t0) t0 = r.t0; if (r.t1 > t1) t1 = r.t1; } }
            out[2 * i] = t0; out[2 * i + 1] = t1;
        }
    }
    if (reset) {
        for (auto& r : all) { r.t0 = ~0ull; r.t1 = 0; }
        HIPCHECK(hipMemcpy(ctx->dc.tl, all.data(), all.size() * sizeof(TlRec), hipMemcpyHostToDevice));
    }
    return ctx->dc.tl_step;
}

extern "C" int svo_debug_get_graph_count(svo_ctx* ctx, uint32_t* captured, uint32_t* replayed)
{
    if (!ctx) return SVO_ERR_ARG;
    if (captured) *captured = (uint32_t)ctx->graphs.size();
    if (replayed) *replayed = ctx->graph_replays;
    return SVO_OK;
}

extern "C" int svo_debug_get_status_word(svo_ctx* ctx, int lane, uint32_t* w)
{
    if (ctx) use_device(ctx);
    if (!ctx || !w || lane < 0 || lane >= ctx->cfg.n_lanes) return SVO_ERR_ARG;
    int rc = svo_wait(ctx); if (rc) return rc;
    HIPCHECK(hipMemcpy(w, ctx->dc.status + lane, sizeof(uint32_t), hipMemcpyDeviceToHost));
    return SVO_OK;
}
