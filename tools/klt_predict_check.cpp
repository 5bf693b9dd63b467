// klt_predict_check.cpp -- holds the host-side decisions of the pose prediction of the resident KLT front end
// (stereo_vo_amd/csrc/klt_call.hpp) to the contract of svo_hip.h: the mode range and states of svo_klt_set_prediction and when it makes
// the buffer, every refusal of svo_klt_predicted / svo_debug_klt_predict in order with its status and a text, and the buffer plan.
// svo_klt_params stays at 40 bytes: the mode travels through a setter.
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
    bool alloc = false;
    static_assert(sizeof(svo_klt_params) == 40, "svo_klt_params is pinned: the prediction's mode is a setter");
    static_assert(KLT_PREDICT_OFF == 0 && KLT_PREDICT_POSE == 1, "the modes of svo_klt_set_prediction");
    const State ready{ true, true, false, false };
    const Caps caps{ 5, 512, 160, 120 };

    // svo_klt_set_prediction: enabled, no capture, then the mode; the buffer is made by the first mode 1 only
    CHECK(check_klt_set_prediction(ready, 0, false, alloc, why) == SVO_OK && why.empty() && !alloc);
    CHECK(check_klt_set_prediction(ready, 1, false, alloc, why) == SVO_OK && why.empty() && alloc);
    CHECK(check_klt_set_prediction(ready, 1, true, alloc, why) == SVO_OK && !alloc);
    CHECK(check_klt_set_prediction(ready, 0, true, alloc, why) == SVO_OK && !alloc);                                           // mode 0 keeps the buffer and makes none
    CHECK(check_klt_set_prediction(ready, -1, false, alloc, why) == SVO_ERR_ARG && why.find("mode -1") != std::string::npos && !alloc);
    CHECK(check_klt_set_prediction(ready, 2, false, alloc, why) == SVO_ERR_ARG && why.find("mode 2") != std::string::npos && !alloc);
    { State s = ready; s.enabled = false; CHECK(check_klt_set_prediction(s, 1, false, alloc, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos && !alloc); }
    { State s = ready; s.enabled = false; CHECK(check_klt_set_prediction(s, 7, false, alloc, why) == SVO_ERR_STATE); }         // the state comes first
    { State s = ready; s.capturing = true; CHECK(check_klt_set_prediction(s, 1, false, alloc, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos && !alloc); }
    { State s = ready; s.capturing = true; CHECK(check_klt_set_prediction(s, 9, false, alloc, why) == SVO_ERR_STATE); }
    { State s = ready; s.enabled = false; s.capturing = true; CHECK(check_klt_set_prediction(s, 1, false, alloc, why) == SVO_ERR_STATE && why.find("svo_klt_enable") != std::string::npos); }
    { State s = ready; s.params_set = false; CHECK(check_klt_set_prediction(s, 1, false, alloc, why) == SVO_OK && alloc); }    // the setter needs no svo_set_params: the step asks for them

    // svo_klt_predicted / svo_debug_klt_predict: ready, the prediction on, the lane, the count, delta6
    for (const char* entry : { "svo_klt_predicted", "svo_debug_klt_predict" }) {
        CHECK(check_klt_predict_call(ready, entry, 1, 0, 0, true, caps, why) == SVO_OK && why.empty());
        CHECK(check_klt_predict_call(ready, entry, 1, 4, 300, true, caps, why) == SVO_OK);
        { State s = ready; s.enabled = false; CHECK(check_klt_predict_call(s, entry, 1, 0, 0, true, caps, why) == SVO_ERR_STATE && why.find("not enabled") != std::string::npos && why.find(entry) == 0); }
        { State s = ready; s.params_set = false; CHECK(check_klt_predict_call(s, entry, 1, 0, 0, true, caps, why) == SVO_ERR_STATE && why.find("svo_set_params") != std::string::npos); }
        { State s = ready; s.frame_parallel = true; CHECK(check_klt_predict_call(s, entry, 1, 0, 0, true, caps, why) == SVO_ERR_STATE && why.find("frame-parallel") != std::string::npos); }
        { State s = ready; s.capturing = true; CHECK(check_klt_predict_call(s, entry, 1, 0, 0, true, caps, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos); }
        CHECK(check_klt_predict_call(ready, entry, 0, 0, 0, true, caps, why) == SVO_ERR_STATE && why.find("svo_klt_set_prediction") != std::string::npos);
        CHECK(check_klt_predict_call(ready, entry, 0, 9, -1, false, caps, why) == SVO_ERR_STATE);                              // the mode before the arguments
        { State s = ready; s.capturing = true; CHECK(check_klt_predict_call(s, entry, 0, 0, 0, true, caps, why) == SVO_ERR_STATE && why.find("capturing") != std::string::npos); }   // the states before the mode
        CHECK(check_klt_predict_call(ready, entry, 1, -1, 0, true, caps, why) == SVO_ERR_ARG && why.find("lane -1 of 5") != std::string::npos);
        CHECK(check_klt_predict_call(ready, entry, 1, 5, 0, true, caps, why) == SVO_ERR_ARG && why.find("lane 5 of 5") != std::string::npos);
        CHECK(check_klt_predict_call(ready, entry, 1, 5, -1, false, caps, why) == SVO_ERR_ARG && why.find("lane") != std::string::npos);      // the lane before the count
        CHECK(check_klt_predict_call(ready, entry, 1, 0, -1, false, caps, why) == SVO_ERR_ARG && why.find("-1 entries") != std::string::npos); // the count before delta6
        CHECK(check_klt_predict_call(ready, entry, 1, 0, 0, false, caps, why) == SVO_ERR_ARG && why.find("delta6") != std::string::npos);
    }

    // the buffer plan: the layout of the tracker's results, a byte per slot, one thread per slot in blocks of 256
    svo_klt_params p; svo_klt_default_params(&p);
    for (const int cap : { 1, 255, 256, 257, 300, 512 }) {
        p.cap = cap;
        const PredictPlan pl = plan_predict(p, caps);
        const Plan kp = plan_klt(p, caps);
        CHECK(pl.n_guess == kp.n_slots && pl.n_guess == 5ll * 2 * cap && pl.n_used == 5ll * cap);
        CHECK(pl.blocks_x >= 1 && (long long)pl.blocks_x * 256 >= cap && (long long)(pl.blocks_x - 1) * 256 < cap);
    }
    { const Caps big{ 128, 16384, 1280, 960 }; p.cap = 16384; const PredictPlan pl = plan_predict(p, big); CHECK(pl.n_guess == 128ll * 2 * 16384 && pl.n_used == 128ll * 16384 && pl.blocks_x == 64); }

    if (failures) { printf("klt_predict_check: %d FAILED\n", failures); return 1; }
    printf("klt_predict_check: ok\n");
    return 0;
}
