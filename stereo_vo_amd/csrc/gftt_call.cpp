// gftt_call.cpp -- the per-call decisions of svo_gftt_detect that need no device (gftt_call.hpp).  Host only, built with g++.
#include "gftt_call.hpp"
#include <limits.h>
#include <math.h>
#include <stddef.h>
#include <stdio.h>

static_assert(sizeof(svo_gftt_params) == 16, "svo_gftt_params is four 4-byte fields");
static_assert(sizeof(svo_image) == 24 && sizeof(svo_gftt_job) == 64, "svo_gftt_job: an image, four pointers and two counts on the LP64 ABI");
static_assert(offsetof(svo_gftt_job, seeds) == 24 && offsetof(svo_gftt_job, n_seeds) == 32 && offsetof(svo_gftt_job, cap) == 36 &&
              offsetof(svo_gftt_job, pts) == 40 && offsetof(svo_gftt_job, response) == 48 && offsetof(svo_gftt_job, info) == 56, "svo_gftt_job field offsets");

namespace svo_gftt {

int check_gftt_params(const svo_gftt_params& p, std::string& why)
{
    char msg[160]; msg[0] = 0;
    why.clear();
    if (p.max_corners < 0) snprintf(msg, sizeof(msg), "max_corners %d: 0 (as many as cap holds) or a positive count is expected", p.max_corners);
    else if (p.block != 3 && p.block != 5 && p.block != 7) snprintf(msg, sizeof(msg), "block %d: 3, 5 or 7 is expected", p.block);
    else if (p.min_distance < 0 || p.min_distance > 255) snprintf(msg, sizeof(msg), "min_distance %d: 0 .. 255 is expected", p.min_distance);
    else if (!isfinite(p.quality) || !(p.quality > 0.0f) || p.quality > 1.0f) snprintf(msg, sizeof(msg), "quality %g: a finite value in (0, 1] is expected", (double)p.quality);
    if (!msg[0]) return SVO_OK;
    why = msg; return SVO_ERR_ARG;
}

int check_gftt_call(const svo_gftt_job* jobs, int n_jobs, const svo_gftt_params& p, uint32_t flags, const Caps& caps, std::string& why)
{
    char msg[256]; msg[0] = 0;
    why.clear();
    const uint32_t known = SVO_FLAG_PINNED_IMAGES | SVO_FLAG_DEVICE_IMAGES;
    if ((flags & ~known) || (flags & known) == known) {
        snprintf(msg, sizeof(msg), "flags %#x: 0, SVO_FLAG_PINNED_IMAGES or SVO_FLAG_DEVICE_IMAGES is expected", flags);
        why = msg; return SVO_ERR_ARG;
    }
    if (const int rc = check_gftt_params(p, why)) return rc;
    if (p.max_corners > caps.max_kps) {
        snprintf(msg, sizeof(msg), "max_corners %d, svo_config.max_kps is %d", p.max_corners, caps.max_kps);
        why = msg; return SVO_ERR_CAPACITY;
    }
    if (caps.max_cand > GFTT_MAX_CAND_CAP) {
        snprintf(msg, sizeof(msg), "svo_config.max_cand %d: svo_gftt_detect sorts at most %d candidates per job", caps.max_cand, (int)GFTT_MAX_CAND_CAP);
        why = msg; return SVO_ERR_CAPACITY;
    }
    if (n_jobs < 0 || (n_jobs > 0 && !jobs)) { snprintf(msg, sizeof(msg), "%d jobs at %s", n_jobs, jobs ? "an address" : "NULL"); why = msg; return SVO_ERR_ARG; }
    if (n_jobs > caps.max_jobs) {
        snprintf(msg, sizeof(msg), "%d jobs: a call takes at most 4 x n_lanes x max_octaves = %d", n_jobs, caps.max_jobs);
        why = msg; return SVO_ERR_CAPACITY;
    }
    for (int j = 0; j < n_jobs; j++) {
        const svo_gftt_job& b = jobs[j];
        const svo_image& im = b.img;
        int rc = SVO_ERR_ARG;
        if (b.cap < 0 || b.n_seeds < 0) snprintf(msg, sizeof(msg), "job %d: cap = %d, n_seeds = %d", j, b.cap, b.n_seeds);
        else if (b.cap > caps.max_kps) { snprintf(msg, sizeof(msg), "job %d: cap %d, svo_config.max_kps is %d", j, b.cap, caps.max_kps); rc = SVO_ERR_CAPACITY; }
        else if (b.n_seeds > caps.max_kps) { snprintf(msg, sizeof(msg), "job %d: %d seeds, svo_config.max_kps is %d", j, b.n_seeds, caps.max_kps); rc = SVO_ERR_CAPACITY; }
        else if (!b.info) snprintf(msg, sizeof(msg), "job %d: info == NULL", j);
        else if (b.cap > 0 && !b.pts) snprintf(msg, sizeof(msg), "job %d: pts == NULL with cap = %d", j, b.cap);
        else if (b.n_seeds > 0 && !b.seeds) snprintf(msg, sizeof(msg), "job %d: seeds == NULL with n_seeds = %d", j, b.n_seeds);
        else if (!im.data) snprintf(msg, sizeof(msg), "job %d: img.data == NULL", j);
        else if (im.w < 8 || im.h < 8) snprintf(msg, sizeof(msg), "job %d: the image is %d x %d, both sides must be at least 8", j, im.w, im.h);
        else if (im.w > caps.max_w || im.h > caps.max_h) {
            snprintf(msg, sizeof(msg), "job %d: an image of %d x %d, the context was created for %d x %d", j, im.w, im.h, caps.max_w, caps.max_h);
            rc = SVO_ERR_CAPACITY;
        }
        else if ((long long)im.w * im.h > (long long)INT32_MAX) snprintf(msg, sizeof(msg), "job %d: %d x %d pixels exceed 2^31 - 1", j, im.w, im.h);
        else if (im.stride < (int64_t)im.w) snprintf(msg, sizeof(msg), "job %d: stride %lld is smaller than a row (%d px)", j, (long long)im.stride, im.w);
        else if ((flags & SVO_FLAG_DEVICE_IMAGES) && im.stride > (int64_t)INT32_MAX / im.h)
            snprintf(msg, sizeof(msg), "job %d: h * stride = %d x %lld exceeds the 2^31 - 1 bytes a device image may span", j, im.h, (long long)im.stride);
        if (msg[0]) { why = msg; return rc; }
    }
    return SVO_OK;
}

int gftt_cand_cap(int max_cand) { return max_cand > GFTT_MIN_CAND_CAP ? max_cand : (int)GFTT_MIN_CAND_CAP; }

int gftt_key_stride(int cand_cap)
{
    int s = 2;                                    // cand_cap <= 2^24 (check_gftt_call)
    while (s < cand_cap && s < (1 << 30)) s <<= 1;
    return s;
}

Cells gftt_cells(int w, int h, int min_distance)
{
    Cells c;
    const int side = w > h ? w : h;
    c.cell = (side + GFTT_MAX_CELLS_SIDE - 1) / GFTT_MAX_CELLS_SIDE;
    if (c.cell < min_distance) c.cell = min_distance;
    if (c.cell < 1) c.cell = 1;
    c.gw = (w + c.cell - 1) / c.cell; c.gh = (h + c.cell - 1) / c.cell;
    return c;
}

Plan plan_gftt_call(const svo_gftt_job* jobs, int n_jobs, const svo_gftt_params& p, bool device_images)
{
    Plan pl;
    pl.map_floats = 0; pl.img_bytes = 0; pl.n_seeds = 0; pl.n_pts = 0; pl.max_w = 0; pl.max_h = 0;
    for (int j = 0; j < n_jobs; j++) {
        const svo_image& im = jobs[j].img;
        const long long px = (long long)im.w * im.h;
        pl.map_off.push_back(pl.map_floats); pl.map_floats += (px + 63) / 64 * 64;
        pl.img_off.push_back(device_images ? -1 : pl.img_bytes);
        if (!device_images) pl.img_bytes += (px + 255) / 256 * 256;
        pl.seed0.push_back(pl.n_seeds); pl.n_seeds += jobs[j].n_seeds;
        pl.pts0.push_back(pl.n_pts); pl.n_pts += jobs[j].cap;
        pl.cells.push_back(gftt_cells(im.w, im.h, p.min_distance));
        if (im.w > pl.max_w) pl.max_w = im.w;
        if (im.h > pl.max_h) pl.max_h = im.h;
    }
    return pl;
}

}

extern "C" void svo_gftt_default_params(svo_gftt_params* p)
{
    if (!p) return;
    p->max_corners = 0; p->block = 3; p->min_distance = 20; p->quality = 0.01f;
}
