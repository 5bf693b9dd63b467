// faster_dyn_check.cpp -- the rule that moves dmFASTER's threshold (stereo_vo_amd/csrc/faster_dyn.hpp, the header the kernels compile; exported
// as svo_faster_threshold_step) held to stage2_detect.cpp:540-545 on its boundaries, and the decisions of svo_set_dyn_fast_threshold that
// need no device (frame_call.cpp), under the address and undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc hostcheck && tools/faster_dyn_check
//
// The expectation is written here a second time, from the reference's text, with every intermediate forced into a double in memory.
// Exit status 0 and a last line "ok" when everything held.
#include "faster_dyn.hpp"
#include "frame_call.hpp"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <limits>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s   [", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "]\n"); failures++; } } while (0)

// S2:540-545, one IEEE double operation per statement
static int rule(int T, unsigned n, int w, int h, double target)
{
    volatile double wh = (double)(w * h);
    volatile double density = (double)n / wh;
    volatile double lo = 0.8 * target, hi = 1.2 * target;
    if (density < lo) return T - 1 > 1 ? T - 1 : 1;
    if (density > hi) return T + 1;
    return T;
}

static void same(int T, unsigned n, int w, int h, double target)
{
    const int want = rule(T, n, w, h, target);
    const int a = faster_dyn_step(T, n, w, h, target), b = svo_faster_threshold_step(T, (int)n, w, h, target);
    CHECK(a == want && b == want, "T %d n %u %d x %d target %.17g: header %d, export %d, rule %d", T, n, w, h, target, a, b, want);
}

int main()
{
    const int Ts[] = { 0, 1, 2, 20, 254, 255 };
    // ---- the plain cases: below, inside, above the band; n = 0; target = 0 ---------------------------------------------------
    CHECK(faster_dyn_step(20, 0, 160, 120, 0.01) == 19 && faster_dyn_step(20, 192, 160, 120, 0.01) == 20 && faster_dyn_step(20, 1000, 160, 120, 0.01) == 21, "band");
    CHECK(faster_dyn_step(1, 0, 160, 120, 0.01) == 1 && faster_dyn_step(0, 0, 160, 120, 0.01) == 1 && faster_dyn_step(2, 0, 160, 120, 0.01) == 1, "the floor is 1, from 0 too");
    CHECK(faster_dyn_step(255, 0, 160, 120, 0.01) == 254 && faster_dyn_step(254, 19200, 160, 120, 0.01) == 255, "254 <-> 255");
    // target = 0: both bounds are 0; no corners is ON them (stay), any corner is above (rise)
    for (int T : Ts) {
        CHECK(faster_dyn_step(T, 0, 160, 120, 0.0) == T, "target 0, n 0, T %d", T);
        CHECK(faster_dyn_step(T, 1, 160, 120, 0.0) == T + 1, "target 0, n 1, T %d", T);
    }
    // ---- a sweep against the second writing of the rule ------------------------------------------------------------------------
    const double targets[] = { 0.0, 1e-9, 1e-4, 0.01, 0.05, 0.085, 0.1, 0.25, 1.0, 1.25, 1e300 };
    const int sizes[][2] = { { 160, 120 }, { 80, 60 }, { 40, 30 }, { 251, 187 }, { 1280, 960 }, { 7, 7 }, { 1, 1 } };
    for (double target : targets)
        for (auto& s : sizes) {
            const unsigned wh = (unsigned)(s[0] * s[1]);
            for (int T : Ts)
                for (unsigned n : { 0u, 1u, wh / 100, wh / 10, wh / 2, wh - 1, wh, 2 * wh, 0x7FFFFFFFu, 0xFFFFFFFFu }) same(T, n, s[0], s[1], target);
        }
    // ---- the boundaries: (n, wh, target) with n / wh EXACTLY on 0.8 target or on 1.2 target, found by search -----------------
    // On a bound neither strict comparison holds: the threshold stays.  One corner fewer than the lower bound falls, one more than the
    // upper bound rises.  (Triples that are on the bound in the rationals but not in doubles are counted, and held to the rule as computed.)
    int on_lo = 0, on_hi = 0, off_lo = 0, off_hi = 0;
    const double search_targets[] = { 0.01, 0.05, 0.1, 0.125, 0.25, 0.5, 1.0 / 64, 5.0 / 1024, 0.3 };
    for (double target : search_targets)
        for (int w = 8; w <= 96; w += 8)
            for (int h = 5; h <= 40; h += 5) {
                const unsigned wh = (unsigned)(w * h);
                for (unsigned n = 1; n < wh; n++) {
                    volatile double d = (double)n / (double)wh, lo = 0.8 * target, hi = 1.2 * target;
                    const bool rat_lo = fabs((double)n * 10.0 - 8.0 * target * wh) < 1e-9 * wh, rat_hi = fabs((double)n * 10.0 - 12.0 * target * wh) < 1e-9 * wh;
                    if (d == lo) {
                        on_lo++;
                        for (int T : Ts) {
                            CHECK(faster_dyn_step(T, n, w, h, target) == T, "on 0.8 target: n %u wh %u target %.17g T %d", n, wh, target, T);
                            CHECK(faster_dyn_step(T, n - 1, w, h, target) == (T - 1 > 1 ? T - 1 : 1), "one below 0.8 target: n %u wh %u target %.17g T %d", n - 1, wh, target, T);
                            same(T, n + 1, w, h, target);
                        }
                    } else if (rat_lo) { off_lo++; for (int T : Ts) same(T, n, w, h, target); }
                    if (d == hi) {
                        on_hi++;
                        for (int T : Ts) {
                            CHECK(faster_dyn_step(T, n, w, h, target) == T, "on 1.2 target: n %u wh %u target %.17g T %d", n, wh, target, T);
                            CHECK(faster_dyn_step(T, n + 1, w, h, target) == T + 1, "one above 1.2 target: n %u wh %u target %.17g T %d", n + 1, wh, target, T);
                            same(T, n - 1, w, h, target);
                        }
                    } else if (rat_hi) { off_hi++; for (int T : Ts) same(T, n, w, h, target); }
                }
            }
    CHECK(on_lo >= 50 && on_hi >= 50, "the search found %d / %d triples exactly on the bounds", on_lo, on_hi);
    printf("boundary search: %d triples exactly on 0.8 target, %d on 1.2 target; %d / %d on a bound in the rationals only\n", on_lo, on_hi, off_lo, off_hi);
    // ---- the refusals of svo_set_dyn_fast_threshold and the re-initialisation rule of svo_set_params ---------------------------
    {
        using namespace svo_call;
        std::string why;
        for (double ok : { 0.0, 1e-300, 0.01, 1.0, 1e300 }) CHECK(check_dyn_fast_target(ok, why) == SVO_OK && why.empty(), "%g", ok);
        const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
        for (double bad : { -1e-300, -1.0, inf, -inf, nan }) CHECK(check_dyn_fast_target(bad, why) == SVO_ERR_ARG && why.find("target_feats_per_pixel") != std::string::npos, "%g", bad);
        svo_params a; memset(&a, 0, sizeof(a)); a.nOctaves = 3; a.initial_FAST_threshold = 20;
        svo_params b = a;
        CHECK(!dyn_fast_octaves_changed(a, b), "same record");
        b.initial_FAST_threshold = 7; b.detect_method = 1; b.orb_nfeats = 99;
        CHECK(!dyn_fast_octaves_changed(a, b), "initial_FAST_threshold alone does not re-initialise");
        b.nOctaves = 2; CHECK(dyn_fast_octaves_changed(a, b) && dyn_fast_octaves_changed(b, a), "3 -> 2 octaves");
        a.nOctaves = 0; b.nOctaves = 1; CHECK(!dyn_fast_octaves_changed(a, b), "nOctaves below 1 counts as 1");
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
