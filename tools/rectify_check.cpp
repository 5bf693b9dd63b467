// rectify_check.cpp -- svo_stereo_rectify (stereo_vo_amd/csrc/rectify_host.cpp) and the map model the kernel compiles
// (csrc/rectify_model.hpp) under the address and undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc hostcheck && tools/rectify_check
//
// Held here: every refusal with its status and a text, and nothing written to `out`; the identity rig (R1 = R2 = I, P = K, every
// entry of the table is its own pixel with fraction 0); the epipolar property of an accepted rig (space points project to one row in
// both rectified cameras); the sentinel of a sample outside the image and of a non-finite one.
// Exit status 0 and a last line "ok" when everything held.
#include "rectify_model.hpp"
#include "svo_hip.h"
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <limits>

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s   [", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "]\n"); failures++; } } while (0)

static void rodrigues(const double om[3], double R[9])
{
    const double th = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double c = cos(th), s = sin(th), x = om[0] / th, y = om[1] / th, z = om[2] / th;
    const double K[9] = { 0, -z, y, z, 0, -x, -y, x, 0 }, rrt[9] = { x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z };
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? c : 0.0) + (1.0 - c) * rrt[i] + s * K[i];
}

static svo_stereo_calibration rig(int w, int h, double f, int zero_disparity)
{
    svo_stereo_calibration c; memset(&c, 0, sizeof(c));
    const double dl[8] = { -0.28, 0.09, 0.001, -0.0007, -0.01, 0, 0, 0 }, dr[8] = { 0.12, -0.05, -0.0008, 0.0005, 0, 0.01, 0.002, 0 };
    c.left.fx = f; c.left.fy = 1.01 * f; c.left.cx = w / 2 + 0.8; c.left.cy = h / 2 - 1.3; memcpy(c.left.dist, dl, sizeof(dl));
    c.right.fx = 0.99 * f; c.right.fy = f; c.right.cx = w / 2 - 2.6; c.right.cy = h / 2 + 0.6; memcpy(c.right.dist, dr, sizeof(dr));
    const double om[3] = { 0.01, -0.02, 0.005 };
    rodrigues(om, c.R);
    c.T[0] = -0.12; c.T[1] = 0.002; c.T[2] = -0.001;
    c.w = w; c.h = h; c.zero_disparity = zero_disparity; c.alpha = -1.0;
    return c;
}

static void refused(const char* what, const svo_stereo_calibration& c, int status)
{
    svo_stereo_rectification out; memset(&out, 0x5A, sizeof(out));
    svo_stereo_rectification untouched; memset(&untouched, 0x5A, sizeof(untouched));
    char why[256]; memset(why, 'x', sizeof(why)); why[255] = 0;
    const int rc = svo_stereo_rectify(&c, &out, why, sizeof(why));
    CHECK(rc == status, "%s: status %d, expected %d (%s)", what, rc, status, why);
    CHECK(rc != SVO_OK && why[0] != 0 && strlen(why) < sizeof(why), "%s: no text", what);
    CHECK(memcmp(&out, &untouched, sizeof(out)) == 0, "%s: out was written", what);
    // a text longer than the caller's room is cut, never overrun; no room at all is accepted
    char tiny[8]; memset(tiny, 'x', sizeof(tiny));
    CHECK(svo_stereo_rectify(&c, &out, tiny, 4) == status && tiny[3] == 0 && tiny[4] == 'x', "%s: a 4-byte text", what);
    CHECK(svo_stereo_rectify(&c, &out, nullptr, 0) == status && svo_stereo_rectify(&c, &out, tiny, 0) == status, "%s: no room for a text", what);
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // ---- the refusals ---------------------------------------------------------------------------------------------------------
    {
        const svo_stereo_calibration good = rig(96, 64, 80.0, 0);
        svo_stereo_rectification out;
        char why[256];
        CHECK(svo_stereo_rectify(&good, &out, why, sizeof(why)) == SVO_OK && why[0] == 0, "the rig itself: %s", why);
        CHECK(svo_stereo_rectify(nullptr, &out, why, sizeof(why)) == SVO_ERR_ARG && why[0], "calib NULL");
        CHECK(svo_stereo_rectify(&good, nullptr, why, sizeof(why)) == SVO_ERR_ARG && why[0], "out NULL");
        svo_stereo_calibration c = good;
        c.alpha = 0.0; refused("alpha 0", c, SVO_ERR_UNSUPPORTED);
        c.alpha = 1.0; refused("alpha 1", c, SVO_ERR_UNSUPPORTED);
        c = good; c.alpha = nan; refused("alpha NaN", c, SVO_ERR_ARG);
        c = good; c.T[0] = 0.002; c.T[1] = -0.12; refused("vertical rig", c, SVO_ERR_UNSUPPORTED);
        c = good; c.T[0] = 0.12; refused("right camera on the left", c, SVO_ERR_ARG);
        c = good; c.T[0] = c.T[1] = c.T[2] = 0.0; refused("T = 0", c, SVO_ERR_ARG);
        c = good; c.left.dist[1] = inf; refused("dist inf", c, SVO_ERR_ARG);
        c = good; c.right.cx = nan; refused("cx NaN", c, SVO_ERR_ARG);
        c = good; c.R[4] = nan; refused("R NaN", c, SVO_ERR_ARG);
        c = good; c.T[2] = -inf; refused("T inf", c, SVO_ERR_ARG);
        c = good; c.R[1] += 1e-5; refused("R not orthonormal", c, SVO_ERR_ARG);
        c = good; for (int i = 0; i < 3; i++) c.R[i] = -c.R[i]; refused("R a reflection", c, SVO_ERR_ARG);
        c = good; { const double half[9] = { -1, 0, 0, 0, -1, 0, 0, 0, 1 }; memcpy(c.R, half, sizeof(half)); } refused("R a half turn", c, SVO_ERR_UNSUPPORTED);
        c = good; c.R[1] += 5e-7; CHECK(svo_stereo_rectify(&c, &out, why, sizeof(why)) == SVO_OK, "5e-7 off orthonormal is accepted: %s", why);
        c = good; c.w = 0; refused("w 0", c, SVO_ERR_ARG);
        c = good; c.h = -3; refused("h negative", c, SVO_ERR_ARG);
    }
    // ---- the identity rig -------------------------------------------------------------------------------------------------------
    for (int zd = 0; zd < 2; zd++) {
        svo_stereo_calibration c; memset(&c, 0, sizeof(c));
        const int w = 97, h = 61;
        c.left.fx = c.left.fy = c.right.fx = c.right.fy = 83.25; c.left.cx = c.right.cx = 47.3; c.left.cy = c.right.cy = 29.9;
        c.R[0] = c.R[4] = c.R[8] = 1.0; c.T[0] = -0.25; c.w = w; c.h = h; c.zero_disparity = zd; c.alpha = -1.0;
        svo_stereo_rectification r; char why[256];
        CHECK(svo_stereo_rectify(&c, &r, why, sizeof(why)) == SVO_OK, "identity rig: %s", why);
        for (int i = 0; i < 9; i++) CHECK(r.R1[i] == (i % 4 == 0 ? 1.0 : 0.0) && r.R2[i] == r.R1[i], "R%d", i);
        const double K[4] = { 83.25, 83.25, 47.3, 29.9 };
        for (int i = 0; i < 4; i++) CHECK(fabs(r.P1[i] - K[i]) <= 1e-12 * K[i] && fabs(r.P2[i] - K[i]) <= 1e-12 * K[i], "P[%d] = %.17g / %.17g", i, r.P1[i], r.P2[i]);
        CHECK(r.tx == -0.25 && r.cam.baseline == 0.25 && r.cam.ncols == w && r.cam.nrows == h && r.cam.l_fx == r.P1[0] && r.cam.r_cx == r.P2[2], "tx and cam");
        RectifyModel m; memset(&m, 0, sizeof(m));
        rectify_inverse(r.P1, r.R1, m.ir);
        m.fx = c.left.fx; m.fy = c.left.fy; m.cx = c.left.cx; m.cy = c.left.cy;
        int bad = 0;
        for (int i = 0; i < h; i++)
            for (int j = 0; j < w; j++) {
                double u, v; rectify_source(m, j, i, &u, &v);
                const RectifyEntry e = rectify_fixed(u, v, w, h);
                if (e.x != ((uint32_t)(j + 1) | ((uint32_t)(i + 1) << 16)) || e.y != 0) bad++;
            }
        CHECK(bad == 0, "%d entries of the identity map are not their own pixel", bad);
    }
    // ---- the epipolar property: a space point lands on one row of both rectified cameras --------------------------------------
    for (int zd = 0; zd < 2; zd++) {
        const svo_stereo_calibration c = rig(333, 127, 260.0, zd);
        svo_stereo_rectification r; char why[256];
        CHECK(svo_stereo_rectify(&c, &r, why, sizeof(why)) == SVO_OK, "%s", why);
        double worst = 0.0;
        unsigned long long s = 88172645463325252ull;
        auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (double)(s >> 11) / 9007199254740992.0; };
        for (int n = 0; n < 50; n++) {
            const double X[3] = { 4.0 * rnd() - 2.0, 3.0 * rnd() - 1.5, 2.0 + 8.0 * rnd() };
            double Xr[3], a[3], b[3];
            for (int i = 0; i < 3; i++) Xr[i] = c.R[3 * i] * X[0] + c.R[3 * i + 1] * X[1] + c.R[3 * i + 2] * X[2] + c.T[i];
            for (int i = 0; i < 3; i++) { a[i] = r.R1[3 * i] * X[0] + r.R1[3 * i + 1] * X[1] + r.R1[3 * i + 2] * X[2]; b[i] = r.R2[3 * i] * Xr[0] + r.R2[3 * i + 1] * Xr[1] + r.R2[3 * i + 2] * Xr[2]; }
            const double va = r.P1[1] * a[1] / a[2] + r.P1[3], vb = r.P2[1] * b[1] / b[2] + r.P2[3];
            worst = fmax(worst, fabs(va - vb));
            CHECK(fabs(a[2] - b[2]) < 1e-12 && fabs((a[0] - b[0]) + r.tx) < 1e-12, "the rectified cameras differ by (tx, 0, 0) alone");
        }
        CHECK(worst < 1e-9, "rows differ by %.3g px", worst);
        CHECK(r.P1[0] == r.P2[0] && r.P1[1] == r.P2[1] && r.P1[0] == r.P1[1] && r.P1[3] == r.P2[3] && (zd ? r.P1[2] == r.P2[2] : r.P1[2] != r.P2[2]), "the shape of P");
        CHECK(r.tx < 0 && r.cam.baseline == -r.tx, "tx %g", r.tx);
    }
    // ---- the fixed point's edges ----------------------------------------------------------------------------------------------
    {
        const int w = 33, h = 17;
        CHECK(rectify_fixed(nan, 3.0, w, h).x == 0xFFFFFFFFu && rectify_fixed(3.0, inf, w, h).x == 0xFFFFFFFFu && rectify_fixed(-inf, 3.0, w, h).x == 0xFFFFFFFFu, "non-finite");
        CHECK(rectify_fixed(1e300, 3.0, w, h).x == 0xFFFFFFFFu && rectify_fixed(3.0, -1e300, w, h).x == 0xFFFFFFFFu, "far outside (inf as a float)");
        CHECK(rectify_fixed(-1.5, 3.0, w, h).x == 0xFFFFFFFFu && rectify_fixed(33.0, 3.0, w, h).x == 0xFFFFFFFFu, "one tap column outside");
        const RectifyEntry a = rectify_fixed(-0.5, 16.25, w, h);
        CHECK(a.x == (0u | (17u << 16)) && a.y == (16u | (8u << 8)), "the -1 column and the last row: %08x %08x", a.x, a.y);
        RectifyModel m; memset(&m, 0, sizeof(m));                      // W = 0 everywhere
        double u, v; rectify_source(m, 3, 4, &u, &v);
        CHECK(rectify_fixed(u, v, w, h).x == 0xFFFFFFFFu, "W = 0");
    }
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
