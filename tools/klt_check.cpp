// klt_check.cpp -- holds the host-side decisions of the resident KLT front end (stereo_vo_amd/csrc/klt_call.hpp) to the contract of
// svo_hip.h: the parameter ranges, every refusal of every entry point in order with its status and a text, and the buffer plan.
// Host only; built with the address and undefined-behaviour sanitizers by `make hostcheck` in stereo_vo_amd/csrc and run on the CPU.
#include "klt_call.hpp"
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace svo_klt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint8_t pix[160 * 120];

static svo_frame good_frame(int w = 160, int h = 120)
{
    svo_frame f;
    memset(&f, 0, sizeof(f));
    f.left.data = pix; f.left.w = w; f.left.h = h; f.left.stride = w;
    f.right = f.left;
    return f;
}

int main()
{
    const Caps caps{ 3, 512, 320, 240 };
    const State ready{ true, true, false, false };
    std::string why;

    // the defaults, and what NULL parameters resolve to
    svo_klt_params def; svo_lk_params lk;
    svo_klt_default_params(&def); svo_lk_default_params(&lk);
    svo_klt_default_params(nullptr);
    CHECK(memcmp(&def.lk, &lk, sizeof(lk)) == 0 && def.cap == 1024 && def.max_dy == 1.5f && def.min_disp == 0.5f && isinf(def.max_disp) && def.max_disp > 0);
    CHECK(klt_resolve_params(nullptr, 512).cap == 512 && klt_resolve_params(nullptr, 4096).cap == 1024);
    { svo_klt_params p = def; p.cap = 7; CHECK(klt_resolve_params(&p, 512).cap == 7); }

    // the ranges
    svo_klt_params ok = klt_resolve_params(nullptr, caps.max_kps);
    CHECK(check_klt_params(ok, caps, why) == SVO_OK && why.empty());
    { svo_klt_params p = ok; p.cap = 0; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_klt_params p = ok; p.cap = 513; CHECK(check_klt_params(p, caps, why) == SVO_ERR_CAPACITY && why.find("512") != std::string::npos); }
    { svo_klt_params p = ok; p.cap = 1; CHECK(check_klt_params(p, caps, why) == SVO_OK); }
    { svo_klt_params p = ok; p.lk.win = 4; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG && why.find("win") != std::string::npos); }
    { svo_klt_params p = ok; p.lk.max_level = 6; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG); }
    { svo_klt_params p = ok; p.lk.fb_max = 0.5f; CHECK(check_klt_params(p, caps, why) == SVO_OK); }
    { svo_klt_params p = ok; p.max_dy = -0.5f; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG); }
    { svo_klt_params p = ok; p.max_dy = NAN; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG); }
    { svo_klt_params p = ok; p.min_disp = NAN; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG); }
    { svo_klt_params p = ok; p.min_disp = 3.0f; p.max_disp = 2.0f; CHECK(check_klt_params(p, caps, why) == SVO_ERR_ARG); }
    { svo_klt_params p = ok; p.min_disp = -INFINITY; p.max_disp = INFINITY; CHECK(check_klt_params(p, caps, why) == SVO_OK); }

    // svo_klt_enable
    bool re = false;
    CHECK(check_klt_enable(ok, caps, false, ok, true, false, re, why) == SVO_OK && re);
    CHECK(check_klt_enable(ok, caps, true, ok, false, false, re, why) == SVO_OK && !re);             // the parameters in force: nothing to do
    { svo_klt_params p = ok; p.cap = 64;
      CHECK(check_klt_enable(p, caps, true, ok, false, false, re, why) == SVO_ERR_STATE && !re && !why.empty());
      CHECK(check_klt_enable(p, caps, true, ok, true, false, re, why) == SVO_OK && re);
      p.cap = 0; CHECK(check_klt_enable(p, caps, true, ok, true, false, re, why) == SVO_ERR_ARG && !re); }   // the ranges come first

    CHECK(check_klt_enable(ok, caps, false, ok, true, true, re, why) == SVO_ERR_STATE && !re && why.find("frame-parallel") != std::string::npos);

    // what every other entry point asks first
    CHECK(check_klt_ready(State{ true, true, false, true }, "svo_klt_step", why) == SVO_ERR_STATE && why.find("frame-parallel") != std::string::npos);
    CHECK(check_klt_ready(ready, "svo_klt_step", why) == SVO_OK && why.empty());
    CHECK(check_klt_ready(State{ false, true, false, false }, "svo_klt_step", why) == SVO_ERR_STATE && why.find("not enabled") != std::string::npos);
    CHECK(check_klt_ready(State{ true, false, false, false }, "svo_klt_step", why) == SVO_ERR_STATE && why.find("svo_set_params") != std::string::npos);
    CHECK(check_klt_ready(State{ true, true, true, false }, "svo_klt_step", why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos);
    CHECK(check_klt_ready(State{ false, false, true, false }, "svo_klt_reset", why) == SVO_ERR_STATE && why.find("not enabled") != std::string::npos);

    // svo_klt_step
    LaneMask act, idle; int w = 0, h = 0;
    std::vector<svo_frame> fr(3, good_frame());
    auto step = [&](const svo_frame* f, uint32_t flags, const uint64_t* lanes, const State& s = State{ true, true, false, false }) { return check_klt_step(f, flags, lanes, caps, s, act, idle, w, h, why); };
    CHECK(step(fr.data(), SVO_RUN_OPTIMIZE, nullptr) == SVO_OK && w == 160 && h == 120 && act.w[0] == 7 && idle.w[0] == 0);
    CHECK(step(fr.data(), 0, nullptr) == SVO_OK);
    CHECK(step(fr.data(), SVO_RUN_OPTIMIZE | SVO_FLAG_DEVICE_IMAGES, nullptr) == SVO_OK && step(fr.data(), SVO_FLAG_PINNED_IMAGES, nullptr) == SVO_OK);
    CHECK(step(fr.data(), SVO_RUN_OPTIMIZE, nullptr, State{ false, true, false, false }) == SVO_ERR_STATE);          // before the flags
    CHECK(step(fr.data(), SVO_FLAG_BGR_IMAGES, nullptr) == SVO_ERR_ARG && why.find("BGR") != std::string::npos);
    for (uint32_t bad : { (uint32_t)SVO_RUN_DETECT, (uint32_t)SVO_RUN_MATCH, (uint32_t)SVO_RUN_TRACK, (uint32_t)SVO_FLAG_NO_SHIFT, (uint32_t)SVO_FLAG_REPEAT, (uint32_t)SVO_RUN_DETECT_POST, 1u << 20 })
        CHECK(step(fr.data(), SVO_RUN_OPTIMIZE | bad, nullptr) == SVO_ERR_ARG);
    CHECK(step(fr.data(), SVO_FLAG_DEVICE_IMAGES | SVO_FLAG_PINNED_IMAGES, nullptr) == SVO_ERR_ARG);
    CHECK(step(nullptr, SVO_RUN_OPTIMIZE, nullptr) == SVO_ERR_ARG && why.find("frames") != std::string::npos);
    { const uint64_t m[2] = { 8, 0 }; CHECK(step(fr.data(), 0, m) == SVO_ERR_ARG && why.find("n_lanes") != std::string::npos); }
    { const uint64_t m[2] = { 0, 1 }; CHECK(step(fr.data(), 0, m) == SVO_ERR_ARG); }
    { const uint64_t m[2] = { 0, 0 }; CHECK(step(fr.data(), 0, m) == SVO_OK && w == 0 && h == 0 && act.w[0] == 0); }       // nobody: nothing to check
    {   // an idle lane's entry is not read
        std::vector<svo_frame> g = fr; memset(&g[1], 0, sizeof(g[1]));
        const uint64_t m[2] = { 5, 0 };
        CHECK(step(g.data(), 0, m) == SVO_OK && act.w[0] == 5 && idle.w[0] == 2);
        CHECK(step(g.data(), 0, nullptr) == SVO_ERR_ARG && why.find("NULL") != std::string::npos);
    }
    { std::vector<svo_frame> g = fr; g[2].right.w = 159; CHECK(step(g.data(), 0, nullptr) == SVO_ERR_ARG && why.find("one size") != std::string::npos); }
    { std::vector<svo_frame> g = fr; g[1] = good_frame(128, 120); CHECK(step(g.data(), 0, nullptr) == SVO_ERR_ARG); }
    { std::vector<svo_frame> g(3, good_frame(63, 120)); CHECK(step(g.data(), 0, nullptr) == SVO_ERR_CAPACITY && why.find("64 x 64") != std::string::npos); }
    { std::vector<svo_frame> g(3, good_frame(160, 60)); CHECK(step(g.data(), 0, nullptr) == SVO_ERR_CAPACITY); }
    { std::vector<svo_frame> g(3, good_frame(321, 240)); CHECK(step(g.data(), 0, nullptr) == SVO_ERR_CAPACITY); }
    { std::vector<svo_frame> g(3, good_frame(320, 240)); CHECK(step(g.data(), 0, nullptr) == SVO_OK && w == 320 && h == 240); }
    { std::vector<svo_frame> g = fr; g[0].left.stride = 159; CHECK(step(g.data(), 0, nullptr) == SVO_ERR_ARG && why.find("stride") != std::string::npos); }
    { std::vector<svo_frame> g = fr; g[0].left.stride = (int64_t)INT32_MAX / 120 + 1;
      CHECK(step(g.data(), 0, nullptr) == SVO_OK);                                                // a host image may have any stride
      CHECK(step(g.data(), SVO_FLAG_DEVICE_IMAGES, nullptr) == SVO_ERR_ARG && why.find("2^31") != std::string::npos); }

    // the lane calls
    CHECK(check_klt_lane_call(ready, "svo_klt_add_points", 0, 5, true, caps, why) == SVO_OK);
    CHECK(check_klt_lane_call(ready, "svo_klt_add_points", 2, 0, true, caps, why) == SVO_OK);
    CHECK(check_klt_lane_call(ready, "svo_klt_add_points", 3, 5, true, caps, why) == SVO_ERR_ARG && why.find("lane") != std::string::npos);
    CHECK(check_klt_lane_call(ready, "svo_klt_add_points", -1, 5, true, caps, why) == SVO_ERR_ARG);
    CHECK(check_klt_lane_call(ready, "svo_klt_add_points", 0, -1, true, caps, why) == SVO_ERR_ARG);
    CHECK(check_klt_lane_call(ready, "svo_klt_add_points", 0, 5, false, caps, why) == SVO_ERR_ARG && why.find("NULL") != std::string::npos);
    CHECK(check_klt_lane_call(State{ false, true, false, false }, "svo_klt_get_tracks", 9, -1, false, caps, why) == SVO_ERR_STATE);       // the state first

    // the plan: blocks that hold the largest image's pyramid, two parities, two table halves
    for (int win : { 5, 11, 21, 31 })
        for (int ml : { 0, 2, 5 }) {
            svo_klt_params p = ok; p.lk.win = win; p.lk.max_level = ml; p.cap = 300;
            const Plan pl = plan_klt(p, caps);
            const svo_lk::Geometry big = klt_geometry(p, caps.max_w, caps.max_h);
            CHECK(pl.img_stride >= big.bytes && pl.img_stride % 256 == 0 && pl.pyr_bytes == 2 * 3 * 2 * pl.img_stride);
            CHECK(pl.n_slots == 3 * 2 * 300 && pl.meta_ints == 3 * 4 * 300 && pl.n_pyr_jobs == 3 && pl.n_trk_jobs == 6);
            CHECK(pl.select_lds_bytes == 3 * 241 * 4);
            for (int ww = 64; ww <= caps.max_w; ww += 37)
                for (int hh = 64; hh <= caps.max_h; hh += 29) {
                    const svo_lk::Geometry g = klt_geometry(p, ww, hh);
                    CHECK(g.bytes <= pl.img_stride && g.nl >= 1 && g.nl <= big.nl && g.off[0] == 0);
                    for (int l = 0; l < g.nl; l++) CHECK(g.off[l] + (long long)g.w[l] * g.h[l] <= g.bytes);
                }
        }

    if (failures) { printf("klt_check: %d FAILED\n", failures); return 1; }
    printf("klt_check: ok\n");
    return 0;
}
