// klt_call.cpp -- the decisions of the resident KLT front end that need no device (klt_call.hpp).  Host only, built with g++.
#include "klt_call.hpp"
#include "gftt_call.hpp"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

static_assert(sizeof(svo_klt_params) == 40, "svo_klt_params: svo_lk_params (24 bytes), cap and three floats");
static_assert(sizeof(svo_klt_topup_params) == 28, "svo_klt_topup_params: svo_gftt_params (16 bytes), two counts and a float");

namespace svo_klt {

svo_klt_params klt_resolve_params(const svo_klt_params* p, int max_kps)
{
    svo_klt_params r;
    if (p) return *p;
    svo_klt_default_params(&r);
    if (r.cap > max_kps) r.cap = max_kps;
    return r;
}

int check_klt_params(const svo_klt_params& p, const Caps& caps, std::string& why)
{
    char msg[200]; msg[0] = 0;
    if (const int rc = svo_lk::check_lk_params(p.lk, why)) return rc;
    why.clear();
    int rc = SVO_ERR_ARG;
    if (p.cap < 1) snprintf(msg, sizeof(msg), "cap %d: 1 .. max_kps = %d tracks per lane are expected", p.cap, caps.max_kps);
    else if (p.cap > caps.max_kps) { snprintf(msg, sizeof(msg), "cap %d: svo_config.max_kps is %d", p.cap, caps.max_kps); rc = SVO_ERR_CAPACITY; }
    else if (!(p.max_dy >= 0.0f)) snprintf(msg, sizeof(msg), "max_dy %g: a value >= 0 is expected", (double)p.max_dy);
    else if (p.min_disp != p.min_disp || p.max_disp != p.max_disp || p.min_disp > p.max_disp)
        snprintf(msg, sizeof(msg), "min_disp %g, max_disp %g: min_disp <= max_disp is expected, neither a NaN", (double)p.min_disp, (double)p.max_disp);
    if (!msg[0]) return SVO_OK;
    why = msg; return rc;
}

int check_klt_enable(const svo_klt_params& p, const Caps& caps, bool enabled, const svo_klt_params& in_force, bool tables_empty, bool frame_parallel, bool& realloc, std::string& why)
{
    realloc = false;
    if (frame_parallel) { why = "svo_klt_enable: the context is a member of a frame-parallel stream: its frames travel between contexts, the track table does not"; return SVO_ERR_STATE; }
    if (const int rc = check_klt_params(p, caps, why)) return rc;
    if (!enabled) { realloc = true; return SVO_OK; }
    if (memcmp(&p, &in_force, sizeof(p)) == 0) return SVO_OK;
    if (!tables_empty) { why = "the front end is enabled with other parameters and a lane's table holds tracks: svo_klt_reset every lane first"; return SVO_ERR_STATE; }
    realloc = true;
    return SVO_OK;
}

int check_klt_ready(const State& s, const char* entry, std::string& why)
{
    char msg[200];
    why.clear();
    if (!s.enabled) { snprintf(msg, sizeof(msg), "%s: the KLT front end is not enabled (svo_klt_enable)", entry); why = msg; return SVO_ERR_STATE; }
    if (!s.params_set) { snprintf(msg, sizeof(msg), "%s: no svo_set_params yet: stage 5 and the lists need the parameters", entry); why = msg; return SVO_ERR_STATE; }
    if (s.frame_parallel) { snprintf(msg, sizeof(msg), "%s: the context is a member of a frame-parallel stream: its frames travel between contexts, the track table does not", entry); why = msg; return SVO_ERR_STATE; }
    if (s.capturing) { snprintf(msg, sizeof(msg), "%s: the context's stream is capturing a graph: the call cannot run inside one", entry); why = msg; return SVO_ERR_STATE; }
    return SVO_OK;
}

int check_klt_step(const svo_frame* frames, uint32_t flags, const uint64_t* lanes, const Caps& caps, const State& s,
                   LaneMask& active, LaneMask& idle, int& w, int& h, std::string& why)
{
    char msg[256]; msg[0] = 0;
    w = h = 0;
    memset(&active, 0, sizeof(active)); memset(&idle, 0, sizeof(idle));
    if (const int rc = check_klt_ready(s, "svo_klt_step", why)) return rc;
    const uint32_t img = SVO_FLAG_PINNED_IMAGES | SVO_FLAG_DEVICE_IMAGES;
    if (flags & SVO_FLAG_BGR_IMAGES) { why = "SVO_FLAG_BGR_IMAGES: the front end tracks on grey images"; return SVO_ERR_ARG; }
    if ((flags & ~(img | (uint32_t)SVO_RUN_OPTIMIZE)) || (flags & img) == img) {
        snprintf(msg, sizeof(msg), "flags %#x: SVO_RUN_OPTIMIZE and one of SVO_FLAG_PINNED_IMAGES / SVO_FLAG_DEVICE_IMAGES are what svo_klt_step takes", flags);
        why = msg; return SVO_ERR_ARG;
    }
    if (!frames) { why = "frames == NULL"; return SVO_ERR_ARG; }
    if (!svo_call::parse_lane_mask(lanes, false, caps.n_lanes, active, idle, why)) return SVO_ERR_ARG;
    if (!lane_any(active)) return SVO_OK;
    int l0 = 0; while (!lane_in(active, l0)) l0++;
    w = frames[l0].left.w; h = frames[l0].left.h;
    for (int l = 0; l < caps.n_lanes && !msg[0]; l++) {
        if (!lane_in(active, l)) continue;
        for (int sd = 0; sd < 2 && !msg[0]; sd++) {
            const svo_image& im = sd ? frames[l].right : frames[l].left;
            const char* side = sd ? "right" : "left";
            if (!im.data) snprintf(msg, sizeof(msg), "lane %d %s image: data == NULL", l, side);
            else if (im.w != w || im.h != h) snprintf(msg, sizeof(msg), "lane %d %s image: %d x %d, lane %d left is %d x %d: one size is expected", l, side, im.w, im.h, l0, w, h);
            else if (w > caps.max_w || h > caps.max_h || w < 64 || h < 64) {
                snprintf(msg, sizeof(msg), "images of %d x %d: the context takes 64 x 64 .. %d x %d", w, h, caps.max_w, caps.max_h);
                why = msg; return SVO_ERR_CAPACITY;
            }
            else if (im.stride < (int64_t)w) snprintf(msg, sizeof(msg), "lane %d %s image: stride %lld is smaller than a row (%d px)", l, side, (long long)im.stride, w);
            else if ((flags & SVO_FLAG_DEVICE_IMAGES) && im.stride > (int64_t)INT32_MAX / h)
                snprintf(msg, sizeof(msg), "lane %d %s image: h * stride = %d x %lld exceeds the 2^31 - 1 bytes a device image may span", l, side, h, (long long)im.stride);
        }
    }
    if (!msg[0]) return SVO_OK;
    why = msg; return SVO_ERR_ARG;
}

int check_klt_lane_call(const State& s, const char* entry, int lane, int n, bool arrays_ok, const Caps& caps, std::string& why)
{
    char msg[200];
    if (const int rc = check_klt_ready(s, entry, why)) return rc;
    if (lane < 0 || lane >= caps.n_lanes) { snprintf(msg, sizeof(msg), "%s: lane %d of %d", entry, lane, caps.n_lanes); why = msg; return SVO_ERR_ARG; }
    if (n < 0 || !arrays_ok) { snprintf(msg, sizeof(msg), "%s: %d entries at %s", entry, n, arrays_ok ? "an address" : "NULL"); why = msg; return SVO_ERR_ARG; }
    return SVO_OK;
}

// ---- the RANSAC gate ----
int check_ransac_tracked(bool params_set, bool geom_ready, bool capturing, const uint64_t* lanes, int n_lanes, LaneMask& active, LaneMask& idle, std::string& why)
{
    memset(&active, 0, sizeof(active)); memset(&idle, 0, sizeof(idle));
    why.clear();
    if (!params_set) { why = "svo_ransac_tracked: no svo_set_params yet: the octaves of the lists are not known"; return SVO_ERR_STATE; }
    if (!geom_ready) { why = "svo_ransac_tracked: no geometry yet: put or load the lists first (svo_set_params clears the geometry of the lists before it)"; return SVO_ERR_STATE; }
    if (capturing) { why = "svo_ransac_tracked: the context's stream is capturing a graph: the call cannot run inside one"; return SVO_ERR_STATE; }
    if (!svo_call::parse_lane_mask(lanes, false, n_lanes, active, idle, why)) return SVO_ERR_ARG;
    return SVO_OK;
}

int check_klt_set_ransac(const State& s, int mode, std::string& why)
{
    char msg[200];
    why.clear();
    if (!s.enabled) { why = "svo_klt_set_ransac: the KLT front end is not enabled (svo_klt_enable)"; return SVO_ERR_STATE; }
    if (s.capturing) { why = "svo_klt_set_ransac: the context's stream is capturing a graph: the call cannot run inside one"; return SVO_ERR_STATE; }
    if (mode < KLT_RANSAC_OFF || mode > KLT_RANSAC_PRUNE) {
        snprintf(msg, sizeof(msg), "svo_klt_set_ransac: mode %d: 0 (off), 1 (filter the tracked pairs) or 2 (and drop the rejected tracks) is expected", mode);
        why = msg; return SVO_ERR_ARG;
    }
    return SVO_OK;
}

// ---- the pose prediction ----
int check_klt_set_prediction(const State& s, int mode, bool have_buffer, bool& alloc, std::string& why)
{
    char msg[200];
    alloc = false;
    why.clear();
    if (!s.enabled) { why = "svo_klt_set_prediction: the KLT front end is not enabled (svo_klt_enable)"; return SVO_ERR_STATE; }
    if (s.capturing) { why = "svo_klt_set_prediction: the context's stream is capturing a graph: the call cannot run inside one"; return SVO_ERR_STATE; }
    if (mode < KLT_PREDICT_OFF || mode > KLT_PREDICT_POSE) {
        snprintf(msg, sizeof(msg), "svo_klt_set_prediction: mode %d: 0 (off) or 1 (constant-velocity pose prediction) is expected", mode);
        why = msg; return SVO_ERR_ARG;
    }
    alloc = mode == KLT_PREDICT_POSE && !have_buffer;
    return SVO_OK;
}

int check_klt_predict_call(const State& s, const char* entry, int mode, int lane, int cap, bool delta_ok, const Caps& caps, std::string& why)
{
    char msg[200];
    if (const int rc = check_klt_ready(s, entry, why)) return rc;
    if (mode != KLT_PREDICT_POSE) { snprintf(msg, sizeof(msg), "%s: the prediction is off (svo_klt_set_prediction)", entry); why = msg; return SVO_ERR_STATE; }
    if (lane < 0 || lane >= caps.n_lanes) { snprintf(msg, sizeof(msg), "%s: lane %d of %d", entry, lane, caps.n_lanes); why = msg; return SVO_ERR_ARG; }
    if (cap < 0) { snprintf(msg, sizeof(msg), "%s: room for %d entries", entry, cap); why = msg; return SVO_ERR_ARG; }
    if (!delta_ok) { snprintf(msg, sizeof(msg), "%s: delta6 == NULL", entry); why = msg; return SVO_ERR_ARG; }
    return SVO_OK;
}

PredictPlan plan_predict(const svo_klt_params& p, const Caps& caps)
{
    PredictPlan pl;
    pl.n_guess = (long long)caps.n_lanes * 2 * p.cap;
    pl.n_used = (long long)caps.n_lanes * p.cap;
    pl.blocks_x = (p.cap + 255) / 256;
    return pl;
}

// ---- the stereo re-association ----
int check_klt_set_stereo(const State& s, int mode, bool have_buffers, bool& alloc, std::string& why)
{
    char msg[200];
    alloc = false;
    why.clear();
    if (!s.enabled) { why = "svo_klt_set_stereo: the KLT front end is not enabled (svo_klt_enable)"; return SVO_ERR_STATE; }
    if (s.capturing) { why = "svo_klt_set_stereo: the context's stream is capturing a graph: the call cannot run inside one"; return SVO_ERR_STATE; }
    if (mode < KLT_STEREO_TEMPORAL || mode > KLT_STEREO_ROW) {
        snprintf(msg, sizeof(msg), "svo_klt_set_stereo: mode %d: 0 (the right list through time) or 1 (the right partner along the row of the new pair) is expected", mode);
        why = msg; return SVO_ERR_ARG;
    }
    alloc = mode == KLT_STEREO_ROW && !have_buffers;
    return SVO_OK;
}

StereoPlan plan_stereo(const svo_klt_params& p, const Caps& caps)
{
    StereoPlan pl;
    pl.n_jobs = caps.n_lanes;
    pl.n_guess = (long long)caps.n_lanes * 2 * p.cap;
    pl.n_pts = (2ll * caps.n_lanes - 1) * p.cap;
    return pl;
}

svo_lk::Geometry klt_geometry(const svo_klt_params& p, int w, int h) { return svo_lk::lk_geometry(w, h, p.lk.win, p.lk.max_level, true); }

Plan plan_klt(const svo_klt_params& p, const Caps& caps)
{
    Plan pl;
    // (level sizes and the level count grow with the image: the largest image has the largest block)
    const svo_lk::Geometry g = klt_geometry(p, caps.max_w, caps.max_h);
    pl.img_stride = (g.bytes + 255) / 256 * 256;
    pl.pyr_bytes = 2ll * caps.n_lanes * 2ll * pl.img_stride;
    pl.n_slots = (long long)caps.n_lanes * 2 * p.cap;
    pl.meta_ints = (long long)caps.n_lanes * 4 * p.cap;
    pl.n_pyr_jobs = caps.n_lanes; pl.n_trk_jobs = 2 * caps.n_lanes;
    pl.select_lds_bytes = 3ll * (caps.max_h + 1) * (long long)sizeof(int32_t);
    return pl;
}

// ---- the resident top-up ----
svo_klt_topup_params topup_default_params(int cap)
{
    svo_klt_topup_params r;
    svo_gftt_default_params(&r.gftt);
    r.below = (cap + 1) / 2; r.target = cap; r.init_disp = 0.0f;
    return r;
}

int check_topup_params(const svo_klt_topup_params& p, const Caps& caps, const TopupCaps& tc, std::string& why)
{
    char msg[200]; msg[0] = 0;
    if (const int rc = svo_gftt::check_gftt_params(p.gftt, why)) return rc;
    why.clear();
    int rc = SVO_ERR_ARG;
    if (p.gftt.max_corners > caps.max_kps) { snprintf(msg, sizeof(msg), "max_corners %d, svo_config.max_kps is %d", p.gftt.max_corners, caps.max_kps); rc = SVO_ERR_CAPACITY; }
    else if (p.below < 1 || p.below > tc.cap) snprintf(msg, sizeof(msg), "below %d: 1 .. cap = %d is expected", p.below, tc.cap);
    else if (p.target < 1 || p.target > tc.cap) snprintf(msg, sizeof(msg), "target %d: 1 .. cap = %d is expected", p.target, tc.cap);
    else if (!isfinite(p.init_disp)) snprintf(msg, sizeof(msg), "init_disp %g: a finite value is expected", (double)p.init_disp);
    else if (tc.max_cand > svo_gftt::GFTT_MAX_CAND_CAP) {
        snprintf(msg, sizeof(msg), "svo_config.max_cand %d: the detector sorts at most %d candidates per lane", tc.max_cand, (int)svo_gftt::GFTT_MAX_CAND_CAP);
        rc = SVO_ERR_CAPACITY;
    }
    if (!msg[0]) return SVO_OK;
    why = msg; return rc;
}

int check_topup_enable(const svo_klt_topup_params& p, const Caps& caps, const TopupCaps& tc, const State& s, bool topup_enabled,
                       const svo_klt_topup_params& in_force, bool has_run, bool tables_empty, bool& realloc, bool& adopt, std::string& why)
{
    realloc = adopt = false;
    why.clear();
    if (!s.enabled) { why = "svo_klt_topup_enable: the KLT front end is not enabled (svo_klt_enable)"; return SVO_ERR_STATE; }
    if (s.capturing) { why = "svo_klt_topup_enable: the context's stream is capturing a graph: the call cannot run inside one"; return SVO_ERR_STATE; }
    if (const int rc = check_topup_params(p, caps, tc, why)) return rc;
    if (!topup_enabled) { realloc = true; return SVO_OK; }
    if (memcmp(&p, &in_force, sizeof(p)) == 0) return SVO_OK;
    if (has_run && !tables_empty) { why = "the top-up has run with other parameters and a lane's table holds tracks: svo_klt_reset every lane first"; return SVO_ERR_STATE; }
    adopt = true;                                 // (no buffer is sized by these parameters)
    return SVO_OK;
}

int check_topup_ready(const State& s, bool topup_enabled, const char* entry, std::string& why)
{
    char msg[200];
    why.clear();
    if (!s.enabled) { snprintf(msg, sizeof(msg), "%s: the KLT front end is not enabled (svo_klt_enable)", entry); why = msg; return SVO_ERR_STATE; }
    if (!topup_enabled) { snprintf(msg, sizeof(msg), "%s: the top-up is not enabled (svo_klt_topup_enable)", entry); why = msg; return SVO_ERR_STATE; }
    if (s.capturing) { snprintf(msg, sizeof(msg), "%s: the context's stream is capturing a graph: the call cannot run inside one", entry); why = msg; return SVO_ERR_STATE; }
    return SVO_OK;
}

int check_topup_call(const State& s, bool topup_enabled, const uint64_t* lanes, const Caps& caps, LaneMask& active, std::string& why)
{
    LaneMask idle;
    memset(&active, 0, sizeof(active));
    if (const int rc = check_topup_ready(s, topup_enabled, "svo_klt_topup", why)) return rc;
    if (!svo_call::parse_lane_mask(lanes, false, caps.n_lanes, active, idle, why)) return SVO_ERR_ARG;
    return SVO_OK;
}

int check_topup_lane_call(const State& s, bool topup_enabled, const char* entry, int lane, int n, bool arrays_ok, const Caps& caps, const TopupCaps& tc, std::string& why)
{
    char msg[200];
    if (const int rc = check_topup_ready(s, topup_enabled, entry, why)) return rc;
    if (lane < 0 || lane >= caps.n_lanes) { snprintf(msg, sizeof(msg), "%s: lane %d of %d", entry, lane, caps.n_lanes); why = msg; return SVO_ERR_ARG; }
    if (n < 0 || !arrays_ok) { snprintf(msg, sizeof(msg), "%s: %d entries at %s", entry, n, arrays_ok ? "an address" : "NULL"); why = msg; return SVO_ERR_ARG; }
    if (n > tc.cap) { snprintf(msg, sizeof(msg), "%s: %d entries, a lane's table holds cap = %d", entry, n, tc.cap); why = msg; return SVO_ERR_ARG; }
    return SVO_OK;
}

TopupPlan plan_topup(const svo_klt_params& kp, const Caps& caps, const TopupCaps& tc)
{
    TopupPlan pl;
    pl.map_stride = ((long long)caps.max_w * caps.max_h + 63) / 64 * 64;
    pl.map_floats = pl.map_stride * caps.n_lanes;
    pl.cand_cap = svo_gftt::gftt_cand_cap(tc.max_cand); pl.key_stride = svo_gftt::gftt_key_stride(pl.cand_cap);
    pl.items_stride = (5ll * pl.cand_cap + 2ll * kp.cap + 3) / 4 * 4;
    pl.n_keys = (long long)caps.n_lanes * pl.key_stride; pl.n_items = (long long)caps.n_lanes * pl.items_stride;
    pl.n_state = (long long)caps.n_lanes * pl.cand_cap;
    pl.n_pts = (long long)caps.n_lanes * kp.cap;
    pl.n_jobs = caps.n_lanes;
    return pl;
}

}

extern "C" void svo_klt_default_params(svo_klt_params* p)
{
    if (!p) return;
    svo_lk_default_params(&p->lk);
    p->cap = 1024; p->max_dy = 1.5f; p->min_disp = 0.5f; p->max_disp = INFINITY;
}
