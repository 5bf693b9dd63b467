// lk_check.cpp -- holds the host-side decisions of svo_lk_track (stereo_vo_amd/csrc/lk_call.hpp) to the contract of svo_hip.h: every
// refusal with its status and a text, the capacity arithmetic, the pyramid geometry and the layout of a call's buffers.  Host only;
// built with the address and undefined-behaviour sanitizers by `make hostcheck` in stereo_vo_amd/csrc and run on the CPU.
#include "lk_call.hpp"
#include <limits.h>
#include <stdio.h>
#include <string.h>

using namespace svo_lk;

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } } while (0)

static uint8_t pix[64 * 48];
static float pts[8], outp[8], errs[4];
static uint8_t stat[4];

static svo_lk_job good_job()
{
    svo_lk_job j;
    memset(&j, 0, sizeof(j));
    j.prev.data = pix; j.prev.w = 64; j.prev.h = 48; j.prev.stride = 64;
    j.next = j.prev;
    j.pts = pts; j.init = nullptr; j.n = 4; j.next_pts = outp; j.status = stat; j.err = errs;
    return j;
}

static int call(const svo_lk_job* jobs, int n, const svo_lk_params& p, uint32_t flags, std::string& why, Caps caps = Caps{ 64, 8, 1280, 960 })
{
    return check_lk_call(jobs, n, p, flags, caps, why);
}

int main()
{
    svo_lk_params def;
    svo_lk_default_params(&def);
    CHECK(def.win == 21 && def.max_level == 3 && def.max_iters == 30 && def.eps == 0.01f && def.min_eig == 1e-4f && def.fb_max == 0.0f);
    svo_lk_default_params(nullptr);
    std::string why;

    // accepted calls
    svo_lk_job j = good_job();
    CHECK(call(&j, 1, def, 0, why) == SVO_OK && why.empty());
    CHECK(call(&j, 1, def, SVO_FLAG_PINNED_IMAGES, why) == SVO_OK);
    CHECK(call(&j, 1, def, SVO_FLAG_DEVICE_IMAGES, why) == SVO_OK);
    CHECK(call(nullptr, 0, def, 0, why) == SVO_OK);
    { svo_lk_job e = good_job(); e.n = 0; e.pts = nullptr; e.next_pts = nullptr; e.status = nullptr; e.err = nullptr; CHECK(call(&e, 1, def, 0, why) == SVO_OK); }
    { svo_lk_job e = good_job(); e.err = nullptr; e.next.stride = 100; CHECK(call(&e, 1, def, 0, why) == SVO_OK); }

    // flags
    CHECK(call(&j, 1, def, SVO_FLAG_BGR_IMAGES, why) == SVO_ERR_ARG && !why.empty());
    CHECK(call(&j, 1, def, SVO_RUN_DETECT, why) == SVO_ERR_ARG && !why.empty());
    CHECK(call(&j, 1, def, SVO_FLAG_PINNED_IMAGES | SVO_FLAG_DEVICE_IMAGES, why) == SVO_ERR_ARG && !why.empty());
    // parameters
    for (int win : { 4, 6, 20, 33, -1, 3 }) { svo_lk_params p = def; p.win = win; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); CHECK(check_lk_params(p, why) == SVO_ERR_ARG); }
    for (int win : { 5, 7, 21, 31 }) { svo_lk_params p = def; p.win = win; CHECK(check_lk_params(p, why) == SVO_OK && why.empty()); }
    for (int ml : { -1, 6 }) { svo_lk_params p = def; p.max_level = ml; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); }
    for (int it : { 0, 101, -5 }) { svo_lk_params p = def; p.max_iters = it; CHECK(call(&j, 1, p, 0, why) == SVO_ERR_ARG && !why.empty()); }
    // job list
    CHECK(call(nullptr, 1, def, 0, why) == SVO_ERR_ARG && !why.empty());
    CHECK(call(&j, -1, def, 0, why) == SVO_ERR_ARG && !why.empty());
    { svo_lk_job many[9]; for (auto& m : many) m = good_job(); CHECK(call(many, 9, def, 0, why) == SVO_ERR_CAPACITY && why.find("9") != std::string::npos && why.find("8") != std::string::npos); CHECK(call(many, 8, def, 0, why) == SVO_OK); }
    // per job
    { svo_lk_job b = good_job(); b.n = -1; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_lk_job b = good_job(); b.n = 65; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_CAPACITY && why.find("65") != std::string::npos && why.find("64") != std::string::npos); b.n = 64; CHECK(call(&b, 1, def, 0, why) == SVO_OK); }
    { svo_lk_job b = good_job(); b.pts = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("pts") != std::string::npos); }
    { svo_lk_job b = good_job(); b.next_pts = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("next_pts") != std::string::npos); }
    { svo_lk_job b = good_job(); b.status = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("status") != std::string::npos); }
    { svo_lk_job b = good_job(); b.prev.data = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("prev") != std::string::npos); }
    { svo_lk_job b = good_job(); b.next.data = nullptr; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("next") != std::string::npos); }
    { svo_lk_job b = good_job(); b.next.w = 63; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_lk_job b = good_job(); b.next.h = 47; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_lk_job b = good_job(); b.prev.w = b.next.w = 0; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && !why.empty()); }
    { svo_lk_job b = good_job(); b.prev.stride = 63; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("stride") != std::string::npos); }
    { svo_lk_job b = good_job(); b.next.stride = -64; CHECK(call(&b, 1, def, 0, why) == SVO_ERR_ARG && why.find("stride") != std::string::npos); }
    { svo_lk_job b = good_job(); CHECK(call(&b, 1, def, 0, why, Caps{ 64, 8, 63, 960 }) == SVO_ERR_CAPACITY && why.find("63") != std::string::npos); CHECK(call(&b, 1, def, 0, why, Caps{ 64, 8, 1280, 47 }) == SVO_ERR_CAPACITY); }
    // the span of a device image: h * stride <= 2^31 - 1 (a host image is copied row by row and may have any stride)
    { svo_lk_job b = good_job(); b.next.stride = (int64_t)INT32_MAX / 48 + 1; CHECK(call(&b, 1, def, SVO_FLAG_DEVICE_IMAGES, why) == SVO_ERR_ARG && why.find("2^31") != std::string::npos); CHECK(call(&b, 1, def, 0, why) == SVO_OK);
      b.next.stride = (int64_t)INT32_MAX / 48; CHECK(call(&b, 1, def, SVO_FLAG_DEVICE_IMAGES, why) == SVO_OK); }
    // the second job's fault is found, and named
    { svo_lk_job two[2] = { good_job(), good_job() }; two[1].status = nullptr; CHECK(call(two, 2, def, 0, why) == SVO_ERR_ARG && why.find("job 1") != std::string::npos); }

    // geometry: ((w + 1) / 2, (h + 1) / 2) per level, while both sides stay >= win + 4
    { const Geometry g = lk_geometry(321, 243, 21, 3, true);
      CHECK(g.nl == 4 && g.w[1] == 161 && g.h[1] == 122 && g.w[2] == 81 && g.h[2] == 61 && g.w[3] == 41 && g.h[3] == 31);
      CHECK(g.off[0] == 0 && g.off[1] == 321 * 243 && g.off[2] == g.off[1] + 161 * 122 && g.off[3] == g.off[2] + 81 * 61 && g.bytes == g.off[3] + 41 * 31); }
    { const Geometry g = lk_geometry(321, 243, 21, 5, false); CHECK(g.nl == 4 && g.off[0] == -1 && g.off[1] == 0 && g.bytes == 161 * 122 + 81 * 61 + 41 * 31); }
    { const Geometry g = lk_geometry(96, 80, 21, 5, true); CHECK(g.nl == 2 && g.w[1] == 48 && g.h[1] == 40); }       // 24 x 20 is below 25
    { const Geometry g = lk_geometry(96, 80, 5, 5, true); CHECK(g.nl == 4 && g.w[3] == 12 && g.h[3] == 10); }        // 6 x 5 is below 9
    { const Geometry g = lk_geometry(96, 80, 21, 0, true); CHECK(g.nl == 1 && g.bytes == 96 * 80); }
    { const Geometry g = lk_geometry(1, 1, 5, 5, true); CHECK(g.nl == 1 && g.bytes == 1); }
    { const Geometry g = lk_geometry(50, 49, 21, 5, true); CHECK(g.nl == 2 && g.w[1] == 25 && g.h[1] == 25); }      // exactly win + 4
    { const Geometry g = lk_geometry(50, 48, 21, 5, true); CHECK(g.nl == 1); }

    // the layout of a call: blocks in job order, prev before next, 256-byte aligned; points flat in job order
    { svo_lk_job three[3] = { good_job(), good_job(), good_job() };
      three[1].n = 0; three[2].init = pts; three[2].n = 3;
      const Plan h = plan_lk_call(three, 3, def, false);
      const long long blk = (64 * 48 + 255) / 256 * 256;
      CHECK(h.geom.size() == 3 && h.img_off.size() == 6 && h.pt0.size() == 3 && h.n_pts == 7 && h.max_nl == 1 && h.any_init);
      CHECK(h.pt0[0] == 0 && h.pt0[1] == 4 && h.pt0[2] == 4);
      for (int i = 0; i < 6; i++) CHECK(h.img_off[(size_t)i] == i * blk);
      CHECK(h.pyr_bytes == 6 * blk);
      const Plan d = plan_lk_call(three, 2, def, true);
      CHECK(d.pyr_bytes == 0 && d.n_pts == 4 && !d.any_init && d.geom[0].off[0] == -1); }
    { const Plan e = plan_lk_call(nullptr, 0, def, false); CHECK(e.geom.empty() && e.pyr_bytes == 0 && e.n_pts == 0 && e.max_nl == 0); }

    // the kernel instantiation of every window: enough pixels per lane for win^2 on 64 lanes
    for (int win = 5; win <= 31; win += 2) { const int n = lk_pixels_per_lane(win); CHECK((n == 2 || n == 7 || n == 16) && n * 64 >= win * win); }
    CHECK(lk_pixels_per_lane(5) == 2 && lk_pixels_per_lane(11) == 2 && lk_pixels_per_lane(13) == 7 && lk_pixels_per_lane(21) == 7 && lk_pixels_per_lane(23) == 16 && lk_pixels_per_lane(31) == 16);
    // the kernels divide a tile index by the tile side with a multiplication: exact for every side and index they use
    for (int T = 5; T <= 34; T++) { const unsigned M = (65536u + (unsigned)T - 1u) / (unsigned)T; for (int t = 0; t < T * T; t++) CHECK((int)(((unsigned)t * M) >> 16) == t / T); }

    // svo_lk_set_photometric: modes 0 and 1, anything else SVO_ERR_ARG with the mode in the text; a capturing stream comes first
    { static_assert(LK_PHOTO_RAW == 0 && LK_PHOTO_GAIN_BIAS == 1, "the modes of svo_lk_set_photometric");
      std::string t;
      CHECK(check_lk_set_photometric(0, false, t) == SVO_OK && t.empty());
      CHECK(check_lk_set_photometric(1, false, t) == SVO_OK && t.empty());
      CHECK(check_lk_set_photometric(2, false, t) == SVO_ERR_ARG && t.find("mode 2") != std::string::npos);
      CHECK(check_lk_set_photometric(-1, false, t) == SVO_ERR_ARG && t.find("mode -1") != std::string::npos);
      CHECK(check_lk_set_photometric(INT32_MIN, false, t) == SVO_ERR_ARG && check_lk_set_photometric(INT32_MAX, false, t) == SVO_ERR_ARG);
      CHECK(check_lk_set_photometric(1, true, t) == SVO_ERR_STATE && t.find("capturing") != std::string::npos);
      CHECK(check_lk_set_photometric(7, true, t) == SVO_ERR_STATE); }
    // the photometric sums of k_lk.hip: a lane's 16 pixels of I I or d I stay inside a signed 32-bit partial sum, the centred moments
    // times n inside the 2^53 a double holds exactly
    { const long long lane = 16ll * 8160 * 8160, n = 31 * 31;
      CHECK(lane == 1065369600ll && lane < (1ll << 30));
      CHECK(n * (n * 8160 * 8160) < (1ll << 53) && 16ll * (n * 8160 + n * 8160) < (1ll << 28)); }

    if (failures) { printf("lk_check: %d check(s) failed\n", failures); return 1; }
    printf("lk_check: ok\n");
    return 0;
}
