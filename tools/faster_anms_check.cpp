// faster_anms_check.cpp -- the decisions around the adaptive NMS under dmFASTER that need no device (stereo_vo_amd/csrc/frame_call.cpp): the
// new branch of check_frame_call behind svo_set_faster_adaptive_nms, and the argument rules of svo_adaptive_nms, under the address and
// undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc hostcheck && tools/faster_anms_check
//
// Exit status 0 and a last line "ok" when everything held.
#include "frame_call.hpp"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>

using namespace svo_call;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s   [", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "]\n"); failures++; } } while (0)

static const char* OLD_TEXT = "the adaptive NMS is not built for dmFASTER: use nmsMethod = nmsmStandard";

static svo_params faster_params(int nms, int method)
{
    svo_params p; memset(&p, 0, sizeof(p));
    p.detect_method = SVO_DM_FASTER; p.match_method = SVO_SM_SAD; p.ifm_method = SVO_IFM_SAD;
    p.non_maximal_suppression = nms; p.nmsMethod = method; p.min_distance = 3; p.initial_FAST_threshold = 20; p.nOctaves = 3;
    return p;
}

static int check(uint32_t flags, const svo_params& p, bool opt_in, std::string& why)
{
    LaneMask all; memset(&all, 0, sizeof(all)); all.w[0] = 1;
    return check_frame_call(make_frame_call(flags, p, opt_in), p, all, nullptr, why);
}

static std::vector<svo_keypoint> lattice(int nx, int ny, int pitch)
{
    std::vector<svo_keypoint> k;
    for (int y = 0; y < ny; y++)
        for (int x = 0; x < nx; x++) {
            svo_keypoint e; memset(&e, 0, sizeof(e));
            e.x = (float)(x * pitch); e.y = (float)(y * pitch); e.angle = -1.0f; e.response = (float)((x * 7 + y * 3) % 11); e.class_id = -1;
            k.push_back(e);
        }
    return k;
}

int main()
{
    std::string why;
    const uint32_t ALL = SVO_RUN_DETECT | SVO_RUN_MATCH | SVO_RUN_TRACK | SVO_RUN_OPTIMIZE;
    const uint32_t detect_calls[] = { ALL, SVO_RUN_DETECT, SVO_RUN_DETECT | SVO_FLAG_DETECT_NO_POST, SVO_RUN_DETECT_POST | SVO_FLAG_NO_SHIFT };
    // ---- the opt-in: off -> the old status and the old text exactly; on -> accepted ------------------------------------------------
    const svo_params adaptive = faster_params(1, SVO_NMS_ADAPTIVE), standard = faster_params(1, SVO_NMS_STANDARD), none = faster_params(0, SVO_NMS_ADAPTIVE);
    for (uint32_t flags : detect_calls) {
        CHECK(check(flags, adaptive, false, why) == SVO_ERR_UNSUPPORTED && why == OLD_TEXT, "off, flags %x: %s", flags, why.c_str());
        CHECK(check(flags, adaptive, true, why) == SVO_OK && why.empty(), "on, flags %x: %s", flags, why.c_str());
        for (bool on : { false, true }) {
            CHECK(check(flags, standard, on, why) == SVO_OK, "nmsmStandard, opt-in %d, flags %x", (int)on, flags);
            CHECK(check(flags, none, on, why) == SVO_OK, "no NMS, opt-in %d, flags %x", (int)on, flags);
        }
    }
    // the default argument is "off": what every existing caller of make_frame_call gets
    {
        LaneMask all; memset(&all, 0, sizeof(all)); all.w[0] = 1;
        const FrameCall c = make_frame_call(ALL, adaptive);
        CHECK(!c.faster_anms_on && !c.faster_anms && check_frame_call(c, adaptive, all, nullptr, why) == SVO_ERR_UNSUPPORTED && why == OLD_TEXT, "default argument");
    }
    // a call that runs neither the detector nor its post-processing was never refused for it
    CHECK(check(SVO_RUN_MATCH | SVO_FLAG_NO_SHIFT, adaptive, false, why) == SVO_OK, "stage 3 alone");
    // ---- the fact itself: set only for dmFASTER + NMS + nmsmAdaptive on a context that opted in ---------------------------------
    CHECK(make_frame_call(ALL, adaptive, true).faster_anms && make_frame_call(ALL, adaptive, true).faster_anms_on, "selected");
    CHECK(!make_frame_call(ALL, standard, true).faster_anms && !make_frame_call(ALL, none, true).faster_anms && !make_frame_call(ALL, adaptive, false).faster_anms, "not selected");
    for (int dm : { (int)SVO_DM_ORB, (int)SVO_DM_FAST_ORB }) {
        svo_params p = adaptive; p.detect_method = dm; p.match_method = 0; p.ifm_method = 0;
        const FrameCall on = make_frame_call(ALL, p, true), off = make_frame_call(ALL, p, false);
        CHECK(!on.faster_anms && !on.faster && on.nms_mode == off.nms_mode && on.nms_mode_oct == off.nms_mode_oct, "inert under detector %d", dm);
        CHECK(check(ALL, p, true, why) == SVO_OK && check(ALL, p, false, why) == SVO_OK, "detector %d accepted either way", dm);
    }
    // the other dmFASTER rules hold with the opt-in on
    {
        svo_params p = adaptive; p.match_method = 0;
        CHECK(check(ALL, p, true, why) == SVO_ERR_STATE && why.find("smSAD") != std::string::npos, "descriptors: %s", why.c_str());
        p = adaptive; p.initial_FAST_threshold = 256;
        CHECK(check(ALL, p, true, why) == SVO_ERR_ARG && why.find("initial_FAST_threshold") != std::string::npos, "threshold: %s", why.c_str());
    }
    // ---- dmKLT and optical flow stay refused either way ----------------------------------------------------------------------
    for (bool on : { false, true }) {
        svo_params p = adaptive; p.detect_method = SVO_DM_KLT;
        CHECK(check(ALL, p, on, why) == SVO_ERR_UNSUPPORTED, "dmKLT, opt-in %d", (int)on);
        p = adaptive; p.ifm_method = SVO_IFM_OPTICAL_FLOW;
        CHECK(check(ALL, p, on, why) == SVO_ERR_UNSUPPORTED, "optical flow, opt-in %d", (int)on);
        p = adaptive; p.nmsMethod = 2;
        CHECK(check(ALL, p, on, why) == SVO_ERR_ARG, "nmsMethod 2, opt-in %d", (int)on);
    }
    // ---- svo_adaptive_nms: the argument rules ------------------------------------------------------------------------------------
    std::vector<svo_keypoint> k = lattice(16, 12, 4);
    std::vector<int32_t> out(k.size());
    const int n = (int)k.size();
    auto args = [&](const std::vector<svo_keypoint>& v, int cnt, int num_out, int w, int h, const int32_t* o, int cap, int cand_cap, int max_kps) {
        return check_adaptive_nms_args(v.empty() ? nullptr : v.data(), cnt, num_out, w, h, o, cap, cand_cap, max_kps, why);
    };
    CHECK(args(k, n, 50, 64, 48, out.data(), n, 1024, 1024) == SVO_OK && why.empty(), "a valid list: %s", why.c_str());
    CHECK(args(k, 0, 50, 64, 48, nullptr, 0, 1024, 1024) == SVO_OK, "an empty list");
    CHECK(check_adaptive_nms_args(nullptr, 0, 0, 64, 48, nullptr, 0, 1024, 1024, why) == SVO_OK, "NULL with n = 0");
    CHECK(args(k, n, -3, 64, 48, out.data(), n, 1024, 1024) == SVO_OK, "num_out_points < 0 keeps nothing");
    CHECK(args(k, n, n + 5, 64, 48, out.data(), 1, 1024, 1024) == SVO_OK, "cap below the count");
#define REFUSED(call, text) CHECK((call) == SVO_ERR_ARG && why.find(text) != std::string::npos, "%s", why.c_str())
    REFUSED(check_adaptive_nms_args(nullptr, 3, 1, 64, 48, out.data(), n, 1024, 1024, why), "kps");
    REFUSED(args(k, -1, 1, 64, 48, out.data(), n, 1024, 1024), "kps");
    REFUSED(args(k, n, 1, 64, 48, nullptr, 5, 1024, 1024), "out_order");
    REFUSED(args(k, n, 1, 64, 48, out.data(), -1, 1024, 1024), "out_order");
    REFUSED(args(k, n, 1, 4096, 4096, out.data(), n, 1024, 1024), "2^24");
    REFUSED(args(k, n, 1, 70000, 4, out.data(), n, 1024, 1024), "2^24");
    REFUSED(args(k, n, 1, 0, 48, out.data(), n, 1024, 1024), "2^24");
    REFUSED(args(k, n, 1, 64, 48, out.data(), n, n - 1, 1024), "candidate capacity");
    REFUSED(args(k, n, 100, 64, 48, out.data(), n, 1024, 99), "max_kps");
    CHECK(args(k, n, 100, 64, 48, out.data(), n, n, 100) == SVO_OK, "exactly at both capacities");
    REFUSED(args(k, n, 1, 60, 48, out.data(), n, 1024, 1024), "integer coordinates");          // x = 60 is outside a 60-wide image
    REFUSED(args(k, n, 1, 64, 44, out.data(), n, 1024, 1024), "integer coordinates");
    {
        std::vector<svo_keypoint> v = k; v[7].x += 0.5f;
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "integer coordinates");
        v = k; v[7].y = -1.0f;
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "integer coordinates");
        v = k; v[7].x = NAN;
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "integer coordinates");
        v = k; v[7].x = INFINITY;
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "integer coordinates");
        v = k; v[n - 1].response = NAN;
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "NaN");
        v = k; v[3].response = -INFINITY; v[4].response = INFINITY; v[5].response = -0.0f;
        CHECK(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024) == SVO_OK, "infinite and signed-zero responses are ordered: accepted");
        v = k; std::swap(v[3], v[4]);
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "raster order");
        v = k; v[4] = v[3];
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "raster order");
        v = k; std::swap(v[0], v[16]);                            // rows exchanged
        REFUSED(args(v, n, 1, 64, 48, out.data(), n, 1024, 1024), "raster order");
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
