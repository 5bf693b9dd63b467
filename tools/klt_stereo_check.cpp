// klt_stereo_check.cpp -- holds the host-side decisions of the stereo re-association of the resident KLT front end
// (stereo_vo_amd/csrc/klt_call.hpp) and of svo_lk_track_rows (lk_call.hpp) to the contract of svo_hip.h: the mode range and states of
// svo_klt_set_stereo and when it makes the buffers, the buffer plan of mode 1 with the point range a row launch covers, and the
// refusals of the row entry point, which are svo_lk_track's (check_lk_call) in their order.  svo_klt_params stays at 40 bytes.
// Host only; built with the address and undefined-behaviour sanitizers by `make hostcheck` in stereo_vo_amd/csrc and run on the CPU.
#include "klt_call.hpp"
#include "lk_call.hpp"
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace svo_klt;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

int main()
{
    std::string why;
    bool alloc = false;
    static_assert(sizeof(svo_klt_params) == 40, "svo_klt_params is pinned: the stereo mode is a setter");
    static_assert(KLT_STEREO_TEMPORAL == 0 && KLT_STEREO_ROW == 1, "the modes of svo_klt_set_stereo");
    const State ready{ true, true, false, false };
    const Caps caps{ 5, 512, 160, 120 };

    // svo_klt_set_stereo: enabled, no capture, then the mode; the buffers are made by the first mode 1 only
    CHECK(check_klt_set_stereo(ready, 0, false, alloc, why) == SVO_OK && why.empty() && !alloc);
    CHECK(check_klt_set_stereo(ready, 1, false, alloc, why) == SVO_OK && why.empty() && alloc);
    CHECK(check_klt_set_stereo(ready, 1, true, alloc, why) == SVO_OK && !alloc);
    CHECK(check_klt_set_stereo(ready, 0, true, alloc, why) == SVO_OK && !alloc);                                               // mode 0 keeps the buffers and makes none
    CHECK(check_klt_set_stereo(ready, -1, false, alloc, why) == SVO_ERR_ARG && why.find("mode -1") != std::string::npos && !alloc);
    CHECK(check_klt_set_stereo(ready, 2, false, alloc, why) == SVO_ERR_ARG && why.find("mode 2") != std::string::npos && !alloc);
    { State s = ready; s.enabled = false; CHECK(check_klt_set_stereo(s, 1, false, alloc, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos && !alloc); }
    { State s = ready; s.enabled = false; CHECK(check_klt_set_stereo(s, 7, false, alloc, why) == SVO_ERR_STATE); }             // the state comes first
    { State s = ready; s.capturing = true; CHECK(check_klt_set_stereo(s, 1, false, alloc, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos && !alloc); }
    { State s = ready; s.capturing = true; CHECK(check_klt_set_stereo(s, 9, false, alloc, why) == SVO_ERR_STATE); }
    { State s = ready; s.enabled = false; s.capturing = true; CHECK(check_klt_set_stereo(s, 1, false, alloc, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos); }
    { State s = ready; s.params_set = false; CHECK(check_klt_set_stereo(s, 1, false, alloc, why) == SVO_OK && alloc); }        // the setter needs no svo_set_params: the step asks for them

    // the buffer plan: a record per lane, the layout of the tracker's results; the last index a row launch covers plus cap (where its
    // result goes) is the last slot of the results
    svo_klt_params p; svo_klt_default_params(&p);
    for (const int cap : { 1, 255, 256, 257, 300, 512 }) {
        p.cap = cap;
        const StereoPlan pl = plan_stereo(p, caps);
        const Plan kp = plan_klt(p, caps);
        CHECK(pl.n_jobs == 5 && pl.n_guess == kp.n_slots && pl.n_pts == 9ll * cap);
        CHECK(pl.n_pts - 1 + cap == kp.n_slots - 1 && pl.n_pts <= pl.n_guess);
        CHECK(2ll * (caps.n_lanes - 1) * cap + cap == pl.n_pts);                                                               // the last lane's points end the range
    }
    { const Caps big{ 128, 16384, 1280, 960 }; p.cap = 16384; const StereoPlan pl = plan_stereo(p, big); CHECK(pl.n_jobs == 128 && pl.n_guess == 128ll * 2 * 16384 && pl.n_pts == 255ll * 16384 && pl.n_pts < (1ll << 31)); }
    { const Caps one{ 1, 64, 160, 120 }; p.cap = 64; const StereoPlan pl = plan_stereo(p, one); CHECK(pl.n_jobs == 1 && pl.n_pts == 64 && pl.n_guess == 128); }

    // svo_lk_track_rows asks what svo_lk_track asks, in its order: flags, parameters, the job count, then job by job
    {
        const svo_lk::Caps lc{ 512, 20, 160, 120 };
        svo_lk_params lp; svo_lk_default_params(&lp);
        std::vector<uint8_t> img(160 * 120, 0), st(4);
        std::vector<float> pts(8, 30.0f), out(8);
        svo_lk_job j; memset(&j, 0, sizeof(j));
        j.prev.data = img.data(); j.prev.w = 160; j.prev.h = 120; j.prev.stride = 160; j.next = j.prev;
        j.pts = pts.data(); j.n = 4; j.next_pts = out.data(); j.status = st.data();
        CHECK(svo_lk::check_lk_call(&j, 1, lp, 0, lc, why) == SVO_OK && why.empty());
        CHECK(svo_lk::check_lk_call(&j, 1, lp, SVO_FLAG_PINNED_IMAGES | SVO_FLAG_DEVICE_IMAGES, lc, why) == SVO_ERR_ARG && why.find("flags") != std::string::npos);
        { svo_lk_params q = lp; q.win = 4; CHECK(svo_lk::check_lk_call(&j, 1, q, 0x4000, lc, why) == SVO_ERR_ARG && why.find("flags") != std::string::npos); }      // flags before parameters
        { svo_lk_params q = lp; q.win = 4; CHECK(svo_lk::check_lk_call(&j, -1, q, 0, lc, why) == SVO_ERR_ARG && why.find("win 4") != std::string::npos); }        // parameters before the count
        CHECK(svo_lk::check_lk_call(&j, 21, lp, 0, lc, why) == SVO_ERR_CAPACITY);
        { svo_lk_job k = j; k.n = 513; CHECK(svo_lk::check_lk_call(&k, 1, lp, 0, lc, why) == SVO_ERR_CAPACITY && why.find("513 points") != std::string::npos); }
        { svo_lk_job k = j; k.status = nullptr; CHECK(svo_lk::check_lk_call(&k, 1, lp, 0, lc, why) == SVO_ERR_ARG && why.find("status") != std::string::npos); }
        { svo_lk_job k = j; k.next.w = 159; CHECK(svo_lk::check_lk_call(&k, 1, lp, 0, lc, why) == SVO_ERR_ARG && why.find("one size") != std::string::npos); }
        { svo_lk_job k = j; k.next.stride = 100; CHECK(svo_lk::check_lk_call(&k, 1, lp, 0, lc, why) == SVO_ERR_ARG && why.find("stride") != std::string::npos); }
        // the instantiation a window runs is the tracker's: 2, 7 or 16 pixels per lane
        CHECK(svo_lk::lk_pixels_per_lane(5) == 2 && svo_lk::lk_pixels_per_lane(21) == 7 && svo_lk::lk_pixels_per_lane(31) == 16);
    }

    if (failures) { printf("klt_stereo_check: %d FAILED\n", failures); return 1; }
    printf("klt_stereo_check: ok\n");
    return 0;
}
