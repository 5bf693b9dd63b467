// rectify_model.hpp -- the rectification map of one camera from its calibration (what mrpt::vision::CStereoRectifyMap::setFromCamParams
// precomputes through cv::initUndistortRectifyMap, stage1_rectify.cpp:66-68), once, for k_rectify_map and for host code.
//
// All arithmetic is IEEE double with one operation per operator, evaluated left to right as written (every unit that includes this
// header is compiled without contraction and without fast-math); tests/rectify_ref.py walks the same operations in the same order.
//
//   rectify_inverse(P, R, ir): ir = (A R)^-1, A = [[fx' 0 cx'], [0 fy' cy'], [0 0 1]], P = fx' fy' cx' cy', R row-major.
//       m0 = fx'*R0 + cx'*R6   m1 = fx'*R1 + cx'*R7   m2 = fx'*R2 + cx'*R8
//       m3 = fy'*R3 + cy'*R6   m4 = fy'*R4 + cy'*R7   m5 = fy'*R5 + cy'*R8
//       m6 = R6                m7 = R7                m8 = R8
//       c0 = m4*m8 - m5*m7     c1 = m5*m6 - m3*m8     c2 = m3*m7 - m4*m6          (cofactors of the first row)
//       det = (m0*c0 + m1*c1) + m2*c2          id = 1 / det
//       ir0 = c0*id            ir1 = (m2*m7 - m1*m8)*id    ir2 = (m1*m5 - m2*m4)*id
//       ir3 = c1*id            ir4 = (m0*m8 - m2*m6)*id    ir5 = (m2*m3 - m0*m5)*id
//       ir6 = c2*id            ir7 = (m1*m6 - m0*m7)*id    ir8 = (m0*m4 - m1*m3)*id
//
//   rectify_source(m, j, i, &u, &v): the source coordinates of output pixel (column j, row i) -- the CLOSED FORM of every pixel, not
//   OpenCV's running sums along a row (a deliberate deviation of ~1e-13 px).  k = k1 k2 p1 p2 k3 k4 k5 k6 (OpenCV's order).
//       X = (j*ir0 + i*ir1) + ir2     Y = (j*ir3 + i*ir4) + ir5     W = (j*ir6 + i*ir7) + ir8
//       x = X/W   y = Y/W   x2 = x*x   y2 = y*y   r2 = x2 + y2   _2xy = (2*x)*y
//       kr = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2)
//       u = fx*((x*kr + p1*_2xy) + p2*(r2 + 2*x2)) + cx
//       v = fy*((y*kr + p1*(r2 + 2*y2)) + p2*_2xy) + cy
//
//   rectify_fixed(u, v, w, h): mx = (float)u, my = (float)v, then the lines of svo_set_rectify_map (cv::remap's 1/32-pixel fixed
//   point): the window -4 < m < size + 4, lrintf(m * 32.0f), integer part >> 5 and fraction & 31, the -1 .. size - 1 test, and the
//   sentinel 0xFFFFFFFF for a sample wholly outside.  A non-finite u or v (W = 0) fails the window and never reaches lrintf.
//       .x = (sx + 1) | (sy + 1) << 16        .y = fx | fy << 8
#ifndef SVO_RECTIFY_MODEL_HPP
#define SVO_RECTIFY_MODEL_HPP
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define SVO_RM_FN __host__ __device__ inline
#else
#define SVO_RM_FN inline
#endif

struct RectifyModel {
    double ir[9];            // (A R)^-1 of the rectified camera, row-major
    double k[8];             // k1 k2 p1 p2 k3 k4 k5 k6 of the source camera
    double fx, fy, cx, cy;   // intrinsics of the source camera
};
struct RectifyEntry { uint32_t x, y; };

SVO_RM_FN void rectify_inverse(const double P[4], const double R[9], double ir[9])
{
    const double fx = P[0], fy = P[1], cx = P[2], cy = P[3];
    const double m0 = fx * R[0] + cx * R[6], m1 = fx * R[1] + cx * R[7], m2 = fx * R[2] + cx * R[8];
    const double m3 = fy * R[3] + cy * R[6], m4 = fy * R[4] + cy * R[7], m5 = fy * R[5] + cy * R[8];
    const double m6 = R[6], m7 = R[7], m8 = R[8];
    const double c0 = m4 * m8 - m5 * m7, c1 = m5 * m6 - m3 * m8, c2 = m3 * m7 - m4 * m6;
    const double det = (m0 * c0 + m1 * c1) + m2 * c2;
    const double id = 1.0 / det;
    ir[0] = c0 * id; ir[1] = (m2 * m7 - m1 * m8) * id; ir[2] = (m1 * m5 - m2 * m4) * id;
    ir[3] = c1 * id; ir[4] = (m0 * m8 - m2 * m6) * id; ir[5] = (m2 * m3 - m0 * m5) * id;
    ir[6] = c2 * id; ir[7] = (m1 * m6 - m0 * m7) * id; ir[8] = (m0 * m4 - m1 * m3) * id;
}

SVO_RM_FN void rectify_source(const RectifyModel& m, int col, int row, double* u, double* v)
{
    const double j = (double)col, i = (double)row;
    const double X = (j * m.ir[0] + i * m.ir[1]) + m.ir[2], Y = (j * m.ir[3] + i * m.ir[4]) + m.ir[5], W = (j * m.ir[6] + i * m.ir[7]) + m.ir[8];
    const double x = X / W, y = Y / W, x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = (2.0 * x) * y;
    const double kr = (1.0 + ((m.k[4] * r2 + m.k[1]) * r2 + m.k[0]) * r2) / (1.0 + ((m.k[7] * r2 + m.k[6]) * r2 + m.k[5]) * r2);
    *u = m.fx * ((x * kr + m.k[2] * _2xy) + m.k[3] * (r2 + 2.0 * x2)) + m.cx;
    *v = m.fy * ((y * kr + m.k[2] * (r2 + 2.0 * y2)) + m.k[3] * _2xy) + m.cy;
}

SVO_RM_FN RectifyEntry rectify_fixed(double u, double v, int w, int h)
{
    const float mx = (float)u, my = (float)v;
    RectifyEntry e; e.x = 0xFFFFFFFFu; e.y = 0;
    if (mx > -4.0f && mx < (float)(w + 4) && my > -4.0f && my < (float)(h + 4)) {
        const long ix = lrintf(mx * 32.0f), iy = lrintf(my * 32.0f);
        const int x = (int)(ix >> 5), y = (int)(iy >> 5);
        if (x >= -1 && x < w && y >= -1 && y < h) { e.x = (uint32_t)(x + 1) | ((uint32_t)(y + 1) << 16); e.y = (uint32_t)(ix & 31) | ((uint32_t)(iy & 31) << 8); }
    }
    return e;
}

#undef SVO_RM_FN
#endif
