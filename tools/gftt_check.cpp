// gftt_check.cpp -- holds the host-side decisions of svo_gftt_detect (stereo_vo_amd/csrc/gftt_call.hpp) to the contract of svo_hip.h:
// every refusal with its status and a text, the capacity arithmetic, the cell grid of the distance rule and the layout of a call's
// buffers.  Host only; built with the address and undefined-behaviour sanitizers by `make hostcheck` in stereo_vo_amd/csrc and run on
// the CPU.
#include "gftt_call.hpp"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

using namespace svo_gftt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint8_t pix[64 * 48];
static float seeds[8], pts[16], resp[8];
static int32_t info[3];

static svo_gftt_job good_job()
{
    svo_gftt_job j;
    memset(&j, 0, sizeof(j));
    j.img.data = pix; j.img.w = 64; j.img.h = 48; j.img.stride = 64;
    j.seeds = seeds; j.n_seeds = 4; j.cap = 8; j.pts = pts; j.response = resp; j.info = info;
    return j;
}

static int call(const svo_gftt_job* jobs, int n, const svo_gftt_params& p, uint32_t flags, std::string& why, Caps caps = Caps{ 64, 8, 1280, 960, 256 })
{
    return check_gftt_call(jobs, n, p, flags, caps, why);
}

int main()
{
    svo_gftt_params def;
    svo_gftt_default_params(&def);
    CHECK(def.max_corners == 0 && def.block == 3 && def.min_distance == 20 && def.quality == 0.01f);
    svo_gftt_default_params(nullptr);
    std::string why;

    // accepted calls
    svo_gftt_job j = good_job();
    CHECK(call(&j, 1, def, 0, why) == SVO_OK && why.empty());
    CHECK(call(&j, 1, def, SVO_FLAG_PINNED_IMAGES, why) == SVO_OK);
    CHECK(call(&j, 1, def, SVO_FLAG_DEVICE_IMAGES, why) == SVO_OK);
    CHECK(call(nullptr, 0, def, 0, why) == SVO_OK);
    { svo_gftt_job e = good_job(); e.cap = 0; e.pts = nullptr; e.response = nullptr; e.n_seeds = 0; e.seeds = nullptr; CHECK(call(&e, 1, def, 0, why) == SVO_OK); }
    { svo_gftt_job e = good_job(); e.response = nullptr; e.n_seeds = 0; e.img.stride = 100; CHECK(call(&e, 1, def, 0, why) == SVO_OK); }   // n_seeds = 0 with a pointer
    { svo_gftt_job e = good_job(); e.img.w = e.img.h = 8; e.img.stride = 8; CHECK(call(&e, 1, def, 0, why) == SVO_OK); }

    // flags
    CHECK(call(&j, 1, def, SVO_FLAG_BGR_IMAGES, why) == SVO_ERR_ARG && !why.empty());
    CHECK(call(&j, 1, def, SVO_RUN_DETECT, why) == SVO_ERR_ARG && !why.empty());
    CHECK(call(&j, 1, def, SVO_FLAG_PINNED_IMAGES | SVO_FLAG_DEVICE_IMAGES, why) == SVO_ERR_ARG && !why.empty());
    // parameters
    for (int b : { 0, 1, 2, 4, 6, 8, 9, -3 }) { svo_gftt_params p = def; p.block = b; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); CHECK(check_gftt_params(p, why) == SVO_ERR_ARG); }
    for (int b : { 3, 5, 7 }) { svo_gftt_params p = def; p.block = b; CHECK(check_gftt_params(p, why) == SVO_OK && why.empty()); }
    for (int d : { -1, 256 }) { svo_gftt_params p = def; p.min_distance = d; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); }
    for (int d : { 0, 1, 255 }) { svo_gftt_params p = def; p.min_distance = d; CHECK(call(&j, 1, p, 0, why) == SVO_OK); }
    for (float q : { 0.0f, -0.5f, 1.5f, (float)NAN, (float)INFINITY }) { svo_gftt_params p = def; p.quality = q; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_gftt_params p = def; p.quality = 1.0f; CHECK(call(&j, 1, p, 0, why) == SVO_OK); }
    { svo_gftt_params p = def; p.max_corners = -1; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_gftt_params p = def; p.max_corners = 65; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_CAPACITY && why.find("65") != std::string::npos && why.find("64") != std::string::npos);
      p.max_corners = 64; CHECK(call(&j, 1, p, 0, why) == SVO_OK); }
    // a context with room for more than 2^24 candidates per job
    CHECK(call(&j, 1, def, 0, why, Caps{ 64, 8, 1280, 960, (1 << 24) + 1 }) == SVO_ERR_CAPACITY && why.find("max_cand") != std::string::npos);
    CHECK(call(&j, 1, def, 0, why, Caps{ 64, 8, 1280, 960, 1 << 24 }) == SVO_OK && gftt_key_stride(1 << 24) == (1 << 24));
    // job list
    CHECK(call(nullptr, 1, def, 0, why) == SVO_ERR_ARG && !why.empty());
    CHECK(call(&j, -1, def, 0, why) == SVO_ERR_ARG && !why.empty());
    { svo_gftt_job many[9]; for (auto& m : many) m = good_job(); CHECK(call(many, 9, def, 0, why) == SVO_ERR_CAPACITY && why.find("9") != std::string::npos && why.find("8") != std::string::npos); CHECK(call(many, 8, def, 0, why) == SVO_OK); }
    // per job
    { svo_gftt_job b = good_job(); b.cap = -1; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_gftt_job b = good_job(); b.n_seeds = -1; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_gftt_job b = good_job(); b.cap = 65; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_CAPACITY && why.find("65") != std::string::npos && why.find("64") != std::string::npos); b.cap = 64; CHECK(call(&b, 1, def, 0, why) == SVO_OK); }
    { svo_gftt_job b = good_job(); b.n_seeds = 65; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_CAPACITY && why.find("65") != std::string::npos); b.n_seeds = 64; CHECK(call(&b, 1, def, 0, why) == SVO_OK); }
    { svo_gftt_job b = good_job(); b.info = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("info") != std::string::npos); }
    { svo_gftt_job b = good_job(); b.pts = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("pts") != std::string::npos); }
    { svo_gftt_job b = good_job(); b.seeds = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("seeds") != std::string::npos); }
    { svo_gftt_job b = good_job(); b.img.data = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("img") != std::string::npos); }
    { svo_gftt_job b = good_job(); b.img.w = 7; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("8") != std::string::npos); }
    { svo_gftt_job b = good_job(); b.img.h = 7; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_gftt_job b = good_job(); b.img.w = 0; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_gftt_job b = good_job(); b.img.stride = 63; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("stride") != std::string::npos); }
    { svo_gftt_job b = good_job(); b.img.stride = -64; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("stride") != std::string::npos); }
    { svo_gftt_job b = good_job(); CHECK(call(&b, 1, def, 0, why, Caps{ 64, 8, 63, 960, 256 }) == SVO_ERR_CAPACITY && why.find("63") != std::string::npos); CHECK(call(&b, 1, def, 0, why, Caps{ 64, 8, 1280, 47, 256 }) == SVO_ERR_CAPACITY); }
    // the span of a device image: h * stride <= 2^31 - 1 (a host image is copied row by row and may have any stride)
    { svo_gftt_job b = good_job(); b.img.stride = (int64_t)INT32_MAX / 48 + 1; CHECK(call(&b, 1, def, SVO_FLAG_DEVICE_IMAGES, why) == SVO_ERR_ARG && why.find("2^31") != std::string::npos); CHECK(call(&b, 1, def, 0, why) == SVO_OK);
      b.img.stride = (int64_t)INT32_MAX / 48; CHECK(call(&b, 1, def, SVO_FLAG_DEVICE_IMAGES, why) == SVO_OK); }
    // the second job's fault is found, and named
    { svo_gftt_job two[2] = { good_job(), good_job() }; two[1].info = nullptr; CHECK(call(two, 2, def, 0, why) == SVO_ERR_ARG && why.find("job 1") != std::string::npos); }

    // capacities: max(1024, max_cand) candidates, the key row a power of two that holds them
    CHECK(gftt_cand_cap(256) == 1024 && gftt_cand_cap(1024) == 1024 && gftt_cand_cap(1025) == 1025 && gftt_cand_cap(1 << 17) == (1 << 17) && gftt_cand_cap(-5) == 1024);
    CHECK(gftt_key_stride(1024) == 1024 && gftt_key_stride(1025) == 2048 && gftt_key_stride(3000) == 4096 && gftt_key_stride(1 << 17) == (1 << 17));
    // the cell grid: side >= max(min_distance, 1), at most 64 x 64 cells, every pixel in a cell
    for (int w : { 8, 9, 63, 64, 65, 321, 1280, 4096, 5000 }) for (int h : { 8, 243, 960, 4097 }) for (int md : { 0, 1, 2, 19, 20, 255 }) {
        const Cells c = gftt_cells(w, h, md);
        CHECK(c.cell >= 1 && c.cell >= md && c.gw >= 1 && c.gh >= 1 && c.gw <= 64 && c.gh <= 64);
        CHECK((w - 1) / c.cell == c.gw - 1 && (h - 1) / c.cell == c.gh - 1);
    }
    { const Cells c = gftt_cells(321, 243, 20); CHECK(c.cell == 20 && c.gw == 17 && c.gh == 13); }
    { const Cells c = gftt_cells(1280, 960, 0); CHECK(c.cell == 20 && c.gw == 64 && c.gh == 48); }
    { const Cells c = gftt_cells(8, 8, 255); CHECK(c.cell == 255 && c.gw == 1 && c.gh == 1); }

    // the layout of a call: maps in job order, 64-float aligned; image copies 256-byte aligned (host images only); seeds and results flat
    { svo_gftt_job three[3] = { good_job(), good_job(), good_job() };
      three[1].img.w = 9; three[1].img.h = 8; three[1].img.stride = 16; three[1].n_seeds = 0; three[1].cap = 0; three[2].cap = 5;
      const Plan h = plan_gftt_call(three, 3, def, false);
      CHECK(h.map_off.size() == 3 && h.img_off.size() == 3 && h.seed0.size() == 3 && h.pts0.size() == 3 && h.cells.size() == 3);
      CHECK(h.map_off[0] == 0 && h.map_off[1] == 64 * 48 && h.map_off[2] == 64 * 48 + 128 && h.map_floats == 2 * 64 * 48 + 128);
      CHECK(h.img_off[0] == 0 && h.img_off[1] == 64 * 48 && h.img_off[2] == 64 * 48 + 256 && h.img_bytes == 2 * 64 * 48 + 256);
      CHECK(h.seed0[0] == 0 && h.seed0[1] == 4 && h.seed0[2] == 4 && h.n_seeds == 8);
      CHECK(h.pts0[0] == 0 && h.pts0[1] == 8 && h.pts0[2] == 8 && h.n_pts == 13);
      CHECK(h.max_w == 64 && h.max_h == 48 && h.cells[1].gw == 1 && h.cells[0].cell == 20);
      const Plan d = plan_gftt_call(three, 2, def, true);
      CHECK(d.img_bytes == 0 && d.img_off[0] == -1 && d.img_off[1] == -1 && d.map_floats == 64 * 48 + 128 && d.n_pts == 8); }
    { const Plan e = plan_gftt_call(nullptr, 0, def, false); CHECK(e.map_off.empty() && e.map_floats == 0 && e.n_seeds == 0 && e.n_pts == 0 && e.max_w == 0); }

    if (failures) { printf("gftt_check: %d check(s) failed\n", failures); return 1; }
    printf("gftt_check: ok\n");
    return 0;
}
