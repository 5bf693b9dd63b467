// rectify_host.cpp -- svo_stereo_rectify: Bouguet's rectification of a calibrated rig as cv::stereoRectify does it for alpha = -1 (what
// mrpt::vision::CStereoRectifyMap::setFromCamParams runs, stage1_rectify.cpp:66-68).  Host only, built with g++, no HIP: the maps
// themselves are rectify_model.hpp's.  IEEE double, one operation per operator, left to right as written (-ffp-contract=off);
// tests/rectify_ref.py walks the same operations in the same order.
//
// From memory of the algorithm, not of a source text (DESIGN.md section 4 lists what is recollection): the undistortion of the image
// corners is the fixed-point iteration run FIVE times; the corners are carried in double, not in float.
#include "../../include/svo_hip.h"
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

namespace {

int refuse(char* why, size_t cap, int status, const char* fmt, ...)
{
    if (why && cap > 0) { va_list ap; va_start(ap, fmt); vsnprintf(why, cap, fmt, ap); va_end(ap); }
    return status;
}

// rotation vector -> matrix: R = c I + (1 - c) r r^T + s [r]x, r = om / |om|
void rodrigues_matrix(const double om[3], double R[9])
{
    const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
    if (theta < DBL_EPSILON) { for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0; return; }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
    const double rx = om[0] * it, ry = om[1] * it, rz = om[2] * it;
    R[0] = c + (c1 * rx) * rx;      R[1] = (c1 * rx) * ry - s * rz; R[2] = (c1 * rx) * rz + s * ry;
    R[3] = (c1 * rx) * ry + s * rz; R[4] = c + (c1 * ry) * ry;      R[5] = (c1 * ry) * rz - s * rx;
    R[6] = (c1 * rx) * rz - s * ry; R[7] = (c1 * ry) * rz + s * rx; R[8] = c + (c1 * rz) * rz;
}

// matrix -> rotation vector; false for a half turn (the axis is not in the antisymmetric part)
bool rodrigues_vector(const double R[9], double om[3])
{
    const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
    const double s = sqrt(((rx * rx + ry * ry) + rz * rz) * 0.25);
    double c = (((R[0] + R[4]) + R[8]) - 1.0) * 0.5;
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double theta = acos(c);
    if (s < 1e-5) {
        if (!(c > 0.0)) return false;
        om[0] = om[1] = om[2] = 0.0;
        return true;
    }
    const double vth = (1.0 / (2.0 * s)) * theta;
    om[0] = rx * vth; om[1] = ry * vth; om[2] = rz * vth;
    return true;
}

void mat_vec(const double A[9], const double x[3], double y[3])
{
    for (int i = 0; i < 3; i++) y[i] = (A[3 * i] * x[0] + A[3 * i + 1] * x[1]) + A[3 * i + 2] * x[2];
}
// C = A B (bt = false) or A B^T (bt = true)
void mat_mul(const double A[9], const double B[9], bool bt, double C[9])
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double b0 = bt ? B[3 * j] : B[j], b1 = bt ? B[3 * j + 1] : B[3 + j], b2 = bt ? B[3 * j + 2] : B[6 + j];
            C[3 * i + j] = (A[3 * i] * b0 + A[3 * i + 1] * b1) + A[3 * i + 2] * b2;
        }
}

bool finite_all(const double* v, int n) { for (int i = 0; i < n; i++) if (!(fabs(v[i]) <= DBL_MAX)) return false; return true; }

// the principal point that centres the four undistorted, rotated image corners at focal length f
void centre_corners(const svo_camera_model& cam, const double Rk[9], double f, int w, int h, double cc[2])
{
    const double* k = cam.dist;
    double sx = 0.0, sy = 0.0;
    for (int i = 0; i < 4; i++) {
        const double px = (double)((i % 2) * (w - 1)), py = (double)((i / 2) * (h - 1));
        const double x0 = (px - cam.cx) / cam.fx, y0 = (py - cam.cy) / cam.fy;
        double x = x0, y = y0;
        for (int it = 0; it < 5; it++) {
            const double r2 = x * x + y * y;
            const double icdist = (1.0 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1.0 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2);
            const double dx = ((2.0 * k[2]) * x) * y + k[3] * (r2 + (2.0 * x) * x);
            const double dy = k[2] * (r2 + (2.0 * y) * y) + ((2.0 * k[3]) * x) * y;
            x = (x0 - dx) * icdist; y = (y0 - dy) * icdist;
        }
        const double X = (Rk[0] * x + Rk[1] * y) + Rk[2], Y = (Rk[3] * x + Rk[4] * y) + Rk[5], Z = (Rk[6] * x + Rk[7] * y) + Rk[8];
        sx = sx + f * (X / Z); sy = sy + f * (Y / Z);
    }
    cc[0] = (double)(w - 1) * 0.5 - sx * 0.25;
    cc[1] = (double)(h - 1) * 0.5 - sy * 0.25;
}

}

extern "C" int svo_stereo_rectify(const svo_stereo_calibration* calib, svo_stereo_rectification* out, char* why, size_t why_cap)
{
    if (why && why_cap > 0) why[0] = 0;
    if (!calib || !out) return refuse(why, why_cap, SVO_ERR_ARG, "%s == NULL", calib ? "out" : "calib");
    const svo_stereo_calibration& c = *calib;
    if (c.w <= 0 || c.h <= 0) return refuse(why, why_cap, SVO_ERR_ARG, "image size %d x %d: both must be positive", c.w, c.h);
    if (!finite_all(&c.left.fx, 12) || !finite_all(&c.right.fx, 12) || !finite_all(c.R, 9) || !finite_all(c.T, 3) || !finite_all(&c.alpha, 1))
        return refuse(why, why_cap, SVO_ERR_ARG, "the calibration holds a value that is not finite");
    if (c.alpha >= 0.0)
        return refuse(why, why_cap, SVO_ERR_UNSUPPORTED, "alpha = %g: the scaling to the inner / outer rectangle is not built, pass a negative alpha (cv::stereoRectify's -1)", c.alpha);
    double worst = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double d = fabs(((c.R[i] * c.R[j] + c.R[3 + i] * c.R[3 + j]) + c.R[6 + i] * c.R[6 + j]) - (i == j ? 1.0 : 0.0));
            worst = d > worst ? d : worst;
        }
    const double det = (c.R[0] * (c.R[4] * c.R[8] - c.R[5] * c.R[7]) - c.R[1] * (c.R[3] * c.R[8] - c.R[5] * c.R[6])) + c.R[2] * (c.R[3] * c.R[7] - c.R[4] * c.R[6]);
    if (worst > 1e-6 || !(det > 0.0))
        return refuse(why, why_cap, SVO_ERR_ARG, "R is no rotation: max |R^T R - I| = %g (at most 1e-6 is accepted), det = %g", worst, det);

    // 1. half of the rotation to each camera
    double om[3], rr[9], t[3];
    if (!rodrigues_vector(c.R, om)) return refuse(why, why_cap, SVO_ERR_UNSUPPORTED, "R turns the right camera by half a turn: not a stereo rig this rectification handles");
    om[0] = om[0] * -0.5; om[1] = om[1] * -0.5; om[2] = om[2] * -0.5;
    rodrigues_matrix(om, rr);
    mat_vec(rr, c.T, t);
    // 2. the half-rotated baseline onto +-x
    const double nt = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
    if (!(nt > 0.0)) return refuse(why, why_cap, SVO_ERR_ARG, "T = 0: the cameras have no baseline");
    if (!(fabs(t[0]) > fabs(t[1])))
        return refuse(why, why_cap, SVO_ERR_UNSUPPORTED, "the half-rotated baseline (%g, %g, %g) is more vertical than horizontal: vertical rigs are not built", t[0], t[1], t[2]);
    const double cb = t[0], ux = cb > 0.0 ? 1.0 : -1.0;
    double ww[3] = { 0.0, t[2] * ux, -(t[1] * ux) };                 // t x (ux, 0, 0)
    const double nw = sqrt((ww[0] * ww[0] + ww[1] * ww[1]) + ww[2] * ww[2]);
    if (nw > 0.0) { const double sc = acos(fabs(cb) / nt) / nw; ww[0] = ww[0] * sc; ww[1] = ww[1] * sc; ww[2] = ww[2] * sc; }
    double wR[9], R1[9], R2[9], t2[3];
    rodrigues_matrix(ww, wR);
    mat_mul(wR, rr, true, R1);
    mat_mul(wR, rr, false, R2);
    mat_vec(R2, c.T, t2);
    const double tx = t2[0];
    if (!(-tx > 0.0))
        return refuse(why, why_cap, SVO_ERR_ARG, "tx = %g: the right camera is not to the right of the left one (x_right = R x_left + T has T[0] < 0 there)", tx);
    // 3. the common focal length
    const double nn = (double)c.w * (double)c.w + (double)c.h * (double)c.h;
    double f = DBL_MAX;
    for (int k = 0; k < 2; k++) {
        const svo_camera_model& cam = k ? c.right : c.left;
        double fc = cam.fy;
        if (cam.dist[0] < 0.0) fc = fc * (1.0 + (cam.dist[0] * nn) / ((4.0 * fc) * fc));
        f = fc < f ? fc : f;
    }
    // 4., 5. the principal points
    double cc0[2], cc1[2];
    centre_corners(c.left, R1, f, c.w, c.h, cc0);
    centre_corners(c.right, R2, f, c.w, c.h, cc1);
    const double my = (cc0[1] + cc1[1]) * 0.5;
    cc0[1] = cc1[1] = my;
    if (c.zero_disparity) { const double mx = (cc0[0] + cc1[0]) * 0.5; cc0[0] = cc1[0] = mx; }
    if (!finite_all(&f, 1) || !finite_all(cc0, 2) || !finite_all(cc1, 2) || !(f > 0.0))
        return refuse(why, why_cap, SVO_ERR_ARG, "the rectified intrinsics are not finite and positive (f' = %g): check the intrinsics and distortion", f);

    for (int i = 0; i < 9; i++) { out->R1[i] = R1[i]; out->R2[i] = R2[i]; }
    out->P1[0] = out->P1[1] = f; out->P1[2] = cc0[0]; out->P1[3] = cc0[1];
    out->P2[0] = out->P2[1] = f; out->P2[2] = cc1[0]; out->P2[3] = cc1[1];
    out->tx = tx;
    svo_stereo_camera& sc = out->cam;
    sc.l_fx = sc.l_fy = f; sc.l_cx = cc0[0]; sc.l_cy = cc0[1];
    sc.r_fx = sc.r_fy = f; sc.r_cx = cc1[0]; sc.r_cy = cc1[1];
    sc.baseline = -tx; sc.ncols = c.w; sc.nrows = c.h;
    return SVO_OK;
}
