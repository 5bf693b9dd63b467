// klt_ransac_check.cpp -- holds the host-side decisions of the RANSAC gate (stereo_vo_amd/csrc/klt_call.hpp) to the contract of
// svo_hip.h: every refusal of svo_ransac_tracked in order with its status and a text, its mask, and the mode range and states of
// svo_klt_set_ransac.  svo_klt_params stays at 40 bytes: the mode travels through a setter.
// Host only; built with the address and undefined-behaviour sanitizers by `make hostcheck` in stereo_vo_amd/csrc and run on the CPU.
#include "klt_call.hpp"
#include <stdio.h>
#include <string.h>

using namespace svo_klt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main()
{
    std::string why;
    LaneMask active, idle;
    static_assert(sizeof(svo_klt_params) == 40, "svo_klt_params is pinned: the gate's mode is a setter");
    static_assert(KLT_RANSAC_OFF == 0 && KLT_RANSAC_FILTER == 1 && KLT_RANSAC_PRUNE == 2, "the modes of svo_klt_set_ransac");

    // svo_ransac_tracked: parameters, geometry, capture, then the mask
    CHECK(check_ransac_tracked(true, true, false, nullptr, 5, active, idle, why) == SVO_OK && why.empty() && active.w[0] == 0x1full && active.w[1] == 0 && !lane_any(idle));
    CHECK(check_ransac_tracked(false, true, false, nullptr, 5, active, idle, why) == SVO_ERR_STATE && why.find("svo_set_params") != std::string::npos && !lane_any(active));
    CHECK(check_ransac_tracked(true, false, false, nullptr, 5, active, idle, why) == SVO_ERR_STATE && why.find("geometry") != std::string::npos && !lane_any(active));
    CHECK(check_ransac_tracked(true, true, true, nullptr, 5, active, idle, why) == SVO_ERR_STATE && why.find("capturing a graph: the call cannot run inside one") != std::string::npos);
    CHECK(check_ransac_tracked(false, false, true, nullptr, 5, active, idle, why) == SVO_ERR_STATE && why.find("svo_set_params") != std::string::npos);       // the parameters come first
    CHECK(check_ransac_tracked(true, false, true, nullptr, 5, active, idle, why) == SVO_ERR_STATE && why.find("geometry") != std::string::npos);              // then the geometry
    { const uint64_t m[2] = { 1ull << 5, 0 }; CHECK(check_ransac_tracked(false, true, false, m, 5, active, idle, why) == SVO_ERR_STATE); }                        // the states before the mask
    { const uint64_t m[2] = { 0x5, 0 }; CHECK(check_ransac_tracked(true, true, false, m, 5, active, idle, why) == SVO_OK && active.w[0] == 0x5ull && idle.w[0] == 0x1aull); }
    { const uint64_t m[2] = { 0, 0 }; CHECK(check_ransac_tracked(true, true, false, m, 5, active, idle, why) == SVO_OK && !lane_any(active) && idle.w[0] == 0x1full); }
    { const uint64_t m[2] = { 1ull << 5, 0 }; CHECK(check_ransac_tracked(true, true, false, m, 5, active, idle, why) == SVO_ERR_ARG && !why.empty()); }
    { const uint64_t m[2] = { 1, 1 }; CHECK(check_ransac_tracked(true, true, false, m, 5, active, idle, why) == SVO_ERR_ARG); }
    { const uint64_t m[2] = { ~0ull, ~0ull }; CHECK(check_ransac_tracked(true, true, false, m, 128, active, idle, why) == SVO_OK && active.w[0] == ~0ull && active.w[1] == ~0ull); }
    { const uint64_t m[2] = { 0, 1ull << 63 }; CHECK(check_ransac_tracked(true, true, false, m, 127, active, idle, why) == SVO_ERR_ARG); }
    { const uint64_t m[2] = { 0, 1ull << 35 }; CHECK(check_ransac_tracked(true, true, false, m, 100, active, idle, why) == SVO_OK && lane_in(active, 99) && !lane_in(active, 98)); }

    // svo_klt_set_ransac: enabled, no capture, then the mode
    const State ready{ true, true, false, false };
    for (int mode = 0; mode <= 2; mode++) CHECK(check_klt_set_ransac(ready, mode, why) == SVO_OK && why.empty());
    CHECK(check_klt_set_ransac(ready, -1, why) == SVO_ERR_ARG && why.find("mode -1") != std::string::npos);
    CHECK(check_klt_set_ransac(ready, 3, why) == SVO_ERR_ARG && why.find("mode 3") != std::string::npos);
    { State s = ready; s.enabled = false; CHECK(check_klt_set_ransac(s, 1, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos); }
    { State s = ready; s.enabled = false; CHECK(check_klt_set_ransac(s, 7, why) == SVO_ERR_STATE); }                          // the state comes first
    { State s = ready; s.capturing = true; CHECK(check_klt_set_ransac(s, 1, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos); }
    { State s = ready; s.params_set = false; CHECK(check_klt_set_ransac(s, 2, why) == SVO_OK); }                              // the setter needs no svo_set_params: the step asks for them

    if (failures) { printf("klt_ransac_check: %d FAILED\n", failures); return 1; }
    printf("klt_ransac_check: ok\n");
    return 0;
}
