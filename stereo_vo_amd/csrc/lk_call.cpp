// lk_call.cpp -- the per-call decisions of svo_lk_track that need no device (lk_call.hpp).  Host only, built with g++.
#include "lk_call.hpp"
#include <limits.h>
#include <stdio.h>

static_assert(sizeof(svo_lk_params) == 24, "svo_lk_params is six 4-byte fields");
static_assert(sizeof(svo_image) == 24 && sizeof(svo_lk_job) == 96, "svo_lk_job: two images, five pointers and a count on the LP64 ABI");

namespace svo_lk {

Geometry lk_geometry(int w, int h, int win, int max_level, bool with_level0)
{
    Geometry g;
    g.nl = 1; g.bytes = 0;
    for (int k = 0; k < LK_MAX_LEVELS; k++) { g.w[k] = g.h[k] = 0; g.off[k] = -1; }
    g.w[0] = w; g.h[0] = h;
    if (with_level0) { g.off[0] = 0; g.bytes = (long long)w * h; }
    while (g.nl <= max_level && g.nl < LK_MAX_LEVELS) {
        const int nw = (g.w[g.nl - 1] + 1) / 2, nh = (g.h[g.nl - 1] + 1) / 2;
        if (nw < win + 4 || nh < win + 4) break;
        g.w[g.nl] = nw; g.h[g.nl] = nh; g.off[g.nl] = g.bytes;
        g.bytes += (long long)nw * nh;
        g.nl++;
    }
    return g;
}

int check_lk_params(const svo_lk_params& p, std::string& why)
{
    char msg[160]; msg[0] = 0;
    why.clear();
    if (p.win < 5 || p.win > 31 || !(p.win & 1)) snprintf(msg, sizeof(msg), "win %d: an odd window of 5 .. 31 pixels is expected", p.win);
    else if (p.max_level < 0 || p.max_level > LK_MAX_LEVELS - 1) snprintf(msg, sizeof(msg), "max_level %d: 0 .. %d is expected", p.max_level, LK_MAX_LEVELS - 1);
    else if (p.max_iters < 1 || p.max_iters > 100) snprintf(msg, sizeof(msg), "max_iters %d: 1 .. 100 is expected", p.max_iters);
    if (!msg[0]) return SVO_OK;
    why = msg; return SVO_ERR_ARG;
}

int check_lk_call(const svo_lk_job* jobs, int n_jobs, const svo_lk_params& p, uint32_t flags, const Caps& caps, std::string& why)
{
    char msg[256]; msg[0] = 0;
    why.clear();
    const uint32_t known = SVO_FLAG_PINNED_IMAGES | SVO_FLAG_DEVICE_IMAGES;
    if ((flags & ~known) || (flags & known) == known) {
        snprintf(msg, sizeof(msg), "flags %#x: 0, SVO_FLAG_PINNED_IMAGES or SVO_FLAG_DEVICE_IMAGES is expected", flags);
        why = msg; return SVO_ERR_ARG;
    }
    if (const int rc = check_lk_params(p, why)) return rc;
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) { snprintf(msg, sizeof(msg), "%d jobs at %s", n_jobs, jobs ? "an address" : "NULL"); why = msg; return SVO_ERR_ARG; }
    if (n_jobs > caps.max_jobs) {
        snprintf(msg, sizeof(msg), "%d jobs: a call takes at most 4 x n_lanes x max_octaves = %d", n_jobs, caps.max_jobs);
        why = msg; return SVO_ERR_CAPACITY;
    }
    for (int j = 0; j < n_jobs; j++) {
        const svo_lk_job& b = jobs[j];
        int rc = SVO_ERR_ARG;
        if (b.n < 0) snprintf(msg, sizeof(msg), "job %d: n = %d", j, b.n);
        else if (b.n > caps.max_kps) { snprintf(msg, sizeof(msg), "job %d: %d points, svo_config.max_kps is %d", j, b.n, caps.max_kps); rc = SVO_ERR_CAPACITY; }
        else if (b.n > 0 && (!b.pts || !b.next_pts || !b.status))
            snprintf(msg, sizeof(msg), "job %d: %s == NULL with n = %d", j, !b.pts ? "pts" : (!b.next_pts ? "next_pts" : "status"), b.n);
        else if (!b.prev.data || !b.next.data) snprintf(msg, sizeof(msg), "job %d: %s.data == NULL", j, !b.prev.data ? "prev" : "next");
        else if (b.prev.w < 1 || b.prev.h < 1) snprintf(msg, sizeof(msg), "job %d: prev is %d x %d", j, b.prev.w, b.prev.h);
        else if (b.prev.w != b.next.w || b.prev.h != b.next.h)
            snprintf(msg, sizeof(msg), "job %d: prev is %d x %d, next %d x %d: one size is expected", j, b.prev.w, b.prev.h, b.next.w, b.next.h);
        else if (b.prev.w > caps.max_w || b.prev.h > caps.max_h) {
            snprintf(msg, sizeof(msg), "job %d: images of %d x %d, the context was created for %d x %d", j, b.prev.w, b.prev.h, caps.max_w, caps.max_h);
            rc = SVO_ERR_CAPACITY;
        }
        else if ((long long)b.prev.w * b.prev.h > (long long)INT32_MAX) snprintf(msg, sizeof(msg), "job %d: %d x %d pixels exceed 2^31 - 1", j, b.prev.w, b.prev.h);
        else for (int s = 0; s < 2 && !msg[0]; s++) {
            const svo_image& im = s ? b.next : b.prev;
            if (im.stride < (int64_t)im.w)
                snprintf(msg, sizeof(msg), "job %d %s image: stride %lld is smaller than a row (%d px)", j, s ? "next" : "prev", (long long)im.stride, im.w);
            else if ((flags & SVO_FLAG_DEVICE_IMAGES) && im.stride > (int64_t)INT32_MAX / im.h)
                snprintf(msg, sizeof(msg), "job %d %s image: h * stride = %d x %lld exceeds the 2^31 - 1 bytes a device image may span", j, s ? "next" : "prev", im.h, (long long)im.stride);
        }
        if (msg[0]) { why = msg; return rc; }
    }
    return SVO_OK;
}

Plan plan_lk_call(const svo_lk_job* jobs, int n_jobs, const svo_lk_params& p, bool device_images)
{
    Plan pl;
    pl.pyr_bytes = 0; pl.n_pts = 0; pl.max_nl = 0; pl.any_init = false;
    pl.geom.reserve((size_t)(n_jobs > 0 ? n_jobs : 0)); pl.pt0.reserve(pl.geom.capacity()); pl.img_off.reserve(2 * pl.geom.capacity());
    for (int j = 0; j < n_jobs; j++) {
        const Geometry g = lk_geometry(jobs[j].prev.w, jobs[j].prev.h, p.win, p.max_level, !device_images);
        pl.geom.push_back(g);
        for (int s = 0; s < 2; s++) { pl.img_off.push_back(pl.pyr_bytes); pl.pyr_bytes += (g.bytes + 255) / 256 * 256; }
        pl.pt0.push_back(pl.n_pts);
        pl.n_pts += jobs[j].n;
        if (g.nl > pl.max_nl) pl.max_nl = g.nl;
        if (jobs[j].n > 0 && jobs[j].init) pl.any_init = true;
    }
    return pl;
}

int check_lk_set_photometric(int mode, bool capturing, std::string& why)
{
    why.clear();
    if (capturing) { why = "svo_lk_set_photometric: the context's stream is capturing a graph: the call cannot run inside one"; return SVO_ERR_STATE; }
    if (mode != LK_PHOTO_RAW && mode != LK_PHOTO_GAIN_BIAS) {
        char msg[192];
        snprintf(msg, sizeof(msg), "svo_lk_set_photometric: mode %d: 0 (raw differences) or 1 (gain and bias removed per window) is expected", mode);
        why = msg; return SVO_ERR_ARG;
    }
    return SVO_OK;
}

int lk_pixels_per_lane(int win)
{
    const int n = (win * win + 63) / 64;
    return n <= 2 ? 2 : (n <= 7 ? 7 : 16);
}

}

extern "C" void svo_lk_default_params(svo_lk_params* p)
{
    if (!p) return;
    p->win = 21; p->max_level = 3; p->max_iters = 30;
    p->eps = 0.01f; p->min_eig = 1e-4f; p->fb_max = 0.0f;
}
