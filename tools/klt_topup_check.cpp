// klt_topup_check.cpp -- holds the host-side decisions of the resident top-up of the KLT front end (stereo_vo_amd/csrc/klt_call.hpp) to
// the contract of svo_hip.h: the defaults, the parameter ranges, every refusal of svo_klt_topup_enable / svo_klt_topup /
// svo_klt_topup_info / svo_debug_klt_topup_append in order with its status and a text, and the buffer plan.
// Host only; built with the address and undefined-behaviour sanitizers by `make hostcheck` in stereo_vo_amd/csrc and run on the CPU.
#include "klt_call.hpp"
#include "gftt_call.hpp"
#include <math.h>
#include <stdio.h>
#include <string.h>

using namespace svo_klt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main()
{
    const Caps caps{ 5, 512, 320, 240 };
    const TopupCaps tc{ 300, 1 << 15 };
    const State ready{ true, true, false, false };
    std::string why;

    // the defaults follow cap
    svo_gftt_params gd; svo_gftt_default_params(&gd);
    const svo_klt_topup_params def = topup_default_params(300);
    CHECK(memcmp(&def.gftt, &gd, sizeof(gd)) == 0 && def.below == 150 && def.target == 300 && def.init_disp == 0.0f);
    CHECK(topup_default_params(301).below == 151 && topup_default_params(1).below == 1 && topup_default_params(1).target == 1);

    // the ranges
    CHECK(check_topup_params(def, caps, tc, why) == SVO_OK && why.empty());
    { svo_klt_topup_params p = def; p.below = 0; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG && why.find("below") != std::string::npos); }
    { svo_klt_topup_params p = def; p.below = 301; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG); }
    { svo_klt_topup_params p = def; p.below = 1; CHECK(check_topup_params(p, caps, tc, why) == SVO_OK); }
    { svo_klt_topup_params p = def; p.below = 300; CHECK(check_topup_params(p, caps, tc, why) == SVO_OK); }
    { svo_klt_topup_params p = def; p.target = 0; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG && why.find("target") != std::string::npos); }
    { svo_klt_topup_params p = def; p.target = 301; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG); }
    { svo_klt_topup_params p = def; p.target = 1; p.below = 300; CHECK(check_topup_params(p, caps, tc, why) == SVO_OK); }      // target below `below` is a choice, not an error
    { svo_klt_topup_params p = def; p.init_disp = NAN; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG && why.find("init_disp") != std::string::npos); }
    { svo_klt_topup_params p = def; p.init_disp = INFINITY; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG); }
    { svo_klt_topup_params p = def; p.init_disp = -3.5f; CHECK(check_topup_params(p, caps, tc, why) == SVO_OK); }
    { svo_klt_topup_params p = def; p.gftt.block = 4; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG && why.find("block") != std::string::npos); }
    { svo_klt_topup_params p = def; p.gftt.min_distance = 256; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG); }
    { svo_klt_topup_params p = def; p.gftt.quality = 0.0f; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG); }
    { svo_klt_topup_params p = def; p.gftt.max_corners = -1; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_ARG); }
    { svo_klt_topup_params p = def; p.gftt.max_corners = 513; CHECK(check_topup_params(p, caps, tc, why) == SVO_ERR_CAPACITY && why.find("512") != std::string::npos); }
    { const TopupCaps big{ 300, (1 << 24) + 1 }; CHECK(check_topup_params(def, caps, big, why) == SVO_ERR_CAPACITY && why.find("max_cand") != std::string::npos); }
    { const TopupCaps edge{ 300, 1 << 24 }; CHECK(check_topup_params(def, caps, edge, why) == SVO_OK); }

    // svo_klt_topup_enable, in order
    bool re = false, adopt = false;
    { State s = ready; s.enabled = false; CHECK(check_topup_enable(def, caps, tc, s, false, def, false, true, re, adopt, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos && !re && !adopt); }
    { State s = ready; s.capturing = true; CHECK(check_topup_enable(def, caps, tc, s, false, def, false, true, re, adopt, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos); }
    { State s = ready; s.params_set = false; CHECK(check_topup_enable(def, caps, tc, s, false, def, false, true, re, adopt, why) == SVO_OK && re); }   // the top-up needs no svo_set_params
    { svo_klt_topup_params p = def; p.below = 0; State s = ready; s.enabled = false; CHECK(check_topup_enable(p, caps, tc, s, false, def, false, true, re, adopt, why) == SVO_ERR_STATE); }   // the state comes first
    { svo_klt_topup_params p = def; p.below = 0; CHECK(check_topup_enable(p, caps, tc, ready, false, def, false, true, re, adopt, why) == SVO_ERR_ARG && !re); }
    CHECK(check_topup_enable(def, caps, tc, ready, false, def, false, true, re, adopt, why) == SVO_OK && re && !adopt);
    CHECK(check_topup_enable(def, caps, tc, ready, true, def, true, false, re, adopt, why) == SVO_OK && !re && !adopt);          // the parameters in force: nothing to do
    {
        svo_klt_topup_params p = def; p.target = 200;
        CHECK(check_topup_enable(p, caps, tc, ready, true, def, false, false, re, adopt, why) == SVO_OK && !re && adopt);       // no top-up has run yet
        CHECK(check_topup_enable(p, caps, tc, ready, true, def, true, true, re, adopt, why) == SVO_OK && !re && adopt);         // one has, but every table is empty
        CHECK(check_topup_enable(p, caps, tc, ready, true, def, true, false, re, adopt, why) == SVO_ERR_STATE && why.find("svo_klt_reset") != std::string::npos && !re && !adopt);
    }

    // svo_klt_topup
    LaneMask active;
    CHECK(check_topup_call(ready, true, nullptr, caps, active, why) == SVO_OK && active.w[0] == 0x1full && active.w[1] == 0);
    { const uint64_t m[2] = { 0x5, 0 }; CHECK(check_topup_call(ready, true, m, caps, active, why) == SVO_OK && active.w[0] == 0x5ull); }
    { const uint64_t m[2] = { 0, 0 }; CHECK(check_topup_call(ready, true, m, caps, active, why) == SVO_OK && !lane_any(active)); }
    { const uint64_t m[2] = { 1ull << 5, 0 }; CHECK(check_topup_call(ready, true, m, caps, active, why) == SVO_ERR_ARG && !why.empty()); }
    { const uint64_t m[2] = { 1, 1 }; CHECK(check_topup_call(ready, true, m, caps, active, why) == SVO_ERR_ARG); }
    CHECK(check_topup_call(ready, false, nullptr, caps, active, why) == SVO_ERR_STATE && why.find("svo_klt_topup_enable") != std::string::npos && !lane_any(active));
    { State s = ready; s.enabled = false; CHECK(check_topup_call(s, false, nullptr, caps, active, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos); }
    { State s = ready; s.capturing = true; CHECK(check_topup_call(s, true, nullptr, caps, active, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos); }
    { State s = ready; s.params_set = false; CHECK(check_topup_call(s, true, nullptr, caps, active, why) == SVO_OK); }

    // svo_klt_topup_info / svo_debug_klt_topup_append
    CHECK(check_topup_lane_call(ready, true, "svo_klt_topup_info", 0, 0, true, caps, tc, why) == SVO_OK);
    CHECK(check_topup_lane_call(ready, true, "svo_klt_topup_info", 5, 0, true, caps, tc, why) == SVO_ERR_ARG && why.find("svo_klt_topup_info") == 0);
    CHECK(check_topup_lane_call(ready, true, "svo_klt_topup_info", -1, 0, true, caps, tc, why) == SVO_ERR_ARG);
    CHECK(check_topup_lane_call(ready, true, "svo_klt_topup_info", 0, 0, false, caps, tc, why) == SVO_ERR_ARG && why.find("NULL") != std::string::npos);
    CHECK(check_topup_lane_call(ready, false, "svo_klt_topup_info", 0, 0, true, caps, tc, why) == SVO_ERR_STATE);
    CHECK(check_topup_lane_call(ready, true, "svo_debug_klt_topup_append", 4, 300, true, caps, tc, why) == SVO_OK);
    CHECK(check_topup_lane_call(ready, true, "svo_debug_klt_topup_append", 4, 301, true, caps, tc, why) == SVO_ERR_ARG && why.find("300") != std::string::npos);
    CHECK(check_topup_lane_call(ready, true, "svo_debug_klt_topup_append", 4, -1, true, caps, tc, why) == SVO_ERR_ARG);
    CHECK(check_topup_lane_call(ready, true, "svo_debug_klt_topup_append", 4, 0, true, caps, tc, why) == SVO_OK);

    // the plan: everything a lane's kernels index lies inside its share
    for (int max_cand : { 0, 1000, 1024, 1025, 1 << 15, 1 << 24 })
        for (int cap : { 1, 64, 300, 512 }) {
            svo_klt_params kp = klt_resolve_params(nullptr, caps.max_kps); kp.cap = cap;
            const TopupCaps t{ cap, max_cand };
            const TopupPlan pl = plan_topup(kp, caps, t);
            CHECK(pl.map_stride >= 320ll * 240 && pl.map_stride % 64 == 0 && pl.map_floats == 5 * pl.map_stride);
            CHECK(pl.cand_cap == svo_gftt::gftt_cand_cap(max_cand) && pl.cand_cap >= 1024 && pl.cand_cap >= max_cand);
            CHECK(pl.key_stride >= pl.cand_cap && (pl.key_stride & (pl.key_stride - 1)) == 0);
            // per lane: (x, y, cell x, cell y) of every candidate, the candidates by cell, the seeds by cell, every seed's cell
            CHECK(pl.items_stride >= 4ll * pl.cand_cap + pl.cand_cap + 2ll * cap && pl.items_stride % 4 == 0);
            CHECK(pl.n_keys == 5ll * pl.key_stride && pl.n_items == 5 * pl.items_stride && pl.n_state == 5ll * pl.cand_cap);
            CHECK(pl.n_pts == 5ll * cap && pl.n_jobs == 5);
        }

    if (failures) { printf("klt_topup_check: %d FAILED\n", failures); return 1; }
    printf("klt_topup_check: ok\n");
    return 0;
}
