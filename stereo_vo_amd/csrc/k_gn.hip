// k_gn.hip -- stage 5 on the device: one persistent 384-thread workgroup per lane (256 / 512 by SVO_GN_NT) runs the whole optimiser
// (gather, grid-NMS mask, triangulation, both Gauss-Newton phases, residual gating, pose inverse) in ONE launch
// with no host round trip.
//
// Replaces stage5_optimize (libstereo-odometry/src/stage5_optimization.cpp:392-736), m_evalRGN (:275-390) and
// m_pinhole_stereo_projection (:35-257).  Double precision throughout, like the reference.  The 28 sums of one
// iteration (21 of J^T J, 6 of J^T r, cost) are reduced inside each wave on the permlane-swap / DPP network and across the
// waves through 28 doubles of LDS each (gn_wave_sums): the Jacobian block is 4T x 6 with a 6x6 output, far too thin for an
// MFMA tile.  LDS per block: 33 KB (lists of up to 1024 tracked pairs; longer ones use DevCtx::gn_scratch).
// The reduction order differs from the reference's sequential loop, so results agree with the oracle to rounding, not bit for
// bit.  What "to rounding" means is held per evaluation: from a given start, ONE m_evalRGN returns the float residuals of an
// extended-precision reference exactly (squared and summed within 4 * 2^-52) and a step within
// K * kappa_2(H) * 2^-52 * ||step|| of it, K = 16 times what the oracle itself reaches
// (tests/test_gpu_stage5.py::test_single_evaluation_against_the_reference, reference in tests/stage5_ref.py).
#include <mutex>
#include <map>
#include <utility>
#include <type_traits>
#include "svo_device.h"
#include "svo_kernels.h"
#include <float.h>
#include <stdlib.h>

// Reciprocal, reciprocal square root, sine and cosine for the ONE thread that solves the normal equations and rebuilds the rotation
// between two barriers of every Gauss-Newton iteration (4.5 of the 8.3 us of an iteration were that thread: tests/dev/gn_breakdown.py).
// An IEEE f64 division is ~10 dependent instructions and the device library's sin / cos ~100 each with their range reduction;
// v_rcp_f64 / v_rsq_f64 plus two Newton steps are 5, and below 0.5 rad the Taylor series to x^17 / x^16 is exact to 1e-19.
// Stage 5 is held to rounding, not bit for bit (the single-evaluation bound in the file header: a step within
// K * kappa_2(H) * 2^-52 of the extended-precision one, tests/test_gpu_stage5.py::test_single_evaluation_against_the_reference, whose
// K allows for exactly this): these agree with the correctly rounded results to an ulp or two.
__device__ __forceinline__ double gn_rcp(double a)
{
    double r = __builtin_amdgcn_rcp(a);
    r = __builtin_fma(r, __builtin_fma(-a, r, 1.0), r);
    return __builtin_fma(r, __builtin_fma(-a, r, 1.0), r);
}
__device__ __forceinline__ double gn_rsqrt(double a)
{
    double y = __builtin_amdgcn_rsq(a);
    y = y * __builtin_fma(-0.5 * a * y, y, 1.5);
    return y * __builtin_fma(-0.5 * a * y, y, 1.5);
}
__device__ __forceinline__ void gn_sincos(double x, double& sn, double& cs)
{
    if (__builtin_expect(!(fabs(x) < 0.5), 0)) { sn = sin(x); cs = cos(x); return; }
    const double z = x * x;
    double ps = -2.8114572543455206e-15;                  // -1/17!
    ps = __builtin_fma(ps, z, 7.6471637318198164e-13);    //  1/15!
    ps = __builtin_fma(ps, z, -1.6059043836821613e-10);   // -1/13!
    ps = __builtin_fma(ps, z, 2.5052108385441720e-08);    //  1/11!
    ps = __builtin_fma(ps, z, -2.7557319223985893e-06);   // -1/9!
    ps = __builtin_fma(ps, z, 1.9841269841269841e-04);    //  1/7!
    ps = __builtin_fma(ps, z, -8.3333333333333332e-03);   // -1/5!
    ps = __builtin_fma(ps, z, 1.6666666666666666e-01);    //  1/3!
    sn = __builtin_fma(-x * z, ps, x);
    double pc = 4.7794773323873853e-14;                   //  1/16!
    pc = __builtin_fma(pc, z, -1.1470745597729725e-11);   // -1/14!
    pc = __builtin_fma(pc, z, 2.0876756987868100e-09);    //  1/12!
    pc = __builtin_fma(pc, z, -2.7557319223985888e-07);   // -1/10!
    pc = __builtin_fma(pc, z, 2.4801587301587302e-05);    //  1/8!
    pc = __builtin_fma(pc, z, -1.3888888888888889e-03);   // -1/6!
    pc = __builtin_fma(pc, z, 4.1666666666666664e-02);    //  1/4!
    pc = __builtin_fma(pc, z, -0.5);
    cs = __builtin_fma(pc, z, 1.0);
}

struct Rot { double r[9]; double dr[3][9]; int small_angle; };

// S5:45-163 (formulas kept as written, including the (w2^2+w3^2) factor of dr22dw3 at S5:162)
template <bool FAST = true>
__device__ void rodrigues_with_derivs(const double* dp, Rot& R)
{
    const double w1 = dp[0], w2 = dp[1], w3 = dp[2];
    const double w12 = w1 * w1, w22 = w2 * w2, w32 = w3 * w3;
    const double ss = w1 * w1 + w2 * w2 + w3 * w3;
    // FAST: inside the Gauss-Newton iteration (tolerance-checked); otherwise the correctly rounded library forms, as the oracle's
    // (getProjectedCoords is compared bit for bit)
    double itt_, tt, sin_tt, cos_tt;
    if (FAST) { itt_ = ss > 0.0 ? gn_rsqrt(ss) : 0.0; tt = ss * itt_; gn_sincos(tt, sin_tt, cos_tt); }
    else { tt = sqrt(ss); itt_ = 1.0 / tt; sin_tt = sin(tt); cos_tt = cos(tt); }
    const double tt2 = tt * tt, tt3 = tt2 * tt, tt4 = tt3 * tt;
    double* r = R.r;
    for (int i = 0; i < 9; i++) { R.dr[0][i] = 0; R.dr[1][i] = 0; R.dr[2][i] = 0; }
    if (tt < 1e-5) {
        R.small_angle = 1;
        r[0] = 1; r[1] = -w3; r[2] = w2; r[3] = w3; r[4] = 1; r[5] = -w1; r[6] = -w2; r[7] = w1; r[8] = 1;
        return;
    }
    R.small_angle = 0;
    // same expressions as S5:102-110 with the divisions by tt, tt2, tt3, tt4 folded into one reciprocal (an f64 divide
    // is a ~15-instruction sequence and this runs on one thread, on the critical path of every iteration)
    const double itt = itt_, itt2 = itt * itt, itt3 = itt2 * itt, itt4 = itt2 * itt2;
    const double u = (cos_tt - 1) * itt2;
    const double dudw1 = ((-sin_tt * w1 * itt) * tt2 - (cos_tt - 1) * 2 * w1) * itt4;
    const double dudw2 = ((-sin_tt * w2 * itt) * tt2 - (cos_tt - 1) * 2 * w2) * itt4;
    const double dudw3 = ((-sin_tt * w3 * itt) * tt2 - (cos_tt - 1) * 2 * w3) * itt4;
    const double v = sin_tt * itt;
    const double dvdw1 = w1 * (tt * cos_tt - sin_tt) * itt3;
    const double dvdw2 = w2 * (tt * cos_tt - sin_tt) * itt3;
    const double dvdw3 = w3 * (tt * cos_tt - sin_tt) * itt3;
    (void)tt3; (void)tt4;
    r[0] = (w22 + w32) * u + 1; r[1] = -w3 * v - w1 * w2 * u; r[2] = w2 * v - w1 * w3 * u;
    r[3] = w3 * v - w1 * w2 * u; r[4] = (w12 + w32) * u + 1; r[5] = -w1 * v - w2 * w3 * u;
    r[6] = -w2 * v - w1 * w3 * u; r[7] = w1 * v - w2 * w3 * u; r[8] = (w12 + w22) * u + 1;
    double (*d)[9] = R.dr;
    d[0][0] = (w22 + w32) * dudw1; d[1][0] = 2 * w2 * u + (w22 + w32) * dudw2; d[2][0] = 2 * w3 * u + (w22 + w32) * dudw3;
    d[0][1] = -w3 * dvdw1 - (w2 * u + w1 * w2 * dudw1); d[1][1] = -w3 * dvdw2 - (w1 * u + w1 * w2 * dudw2); d[2][1] = -(v + w3 * dvdw3) - w1 * w2 * dudw3;
    d[0][2] = w2 * dvdw1 - (w3 * u + w1 * w3 * dudw1); d[1][2] = (v + w2 * dvdw2) - w1 * w3 * dudw2; d[2][2] = w2 * dvdw3 - (w1 * u + w1 * w3 * dudw3);
    d[0][3] = w3 * dvdw1 - (w2 * u + w1 * w2 * dudw1); d[1][3] = w3 * dvdw2 - (w1 * u + w1 * w2 * dudw2); d[2][3] = (v + w3 * dvdw3) - w1 * w2 * dudw3;
    d[0][4] = 2 * w1 * u + (w12 + w32) * dudw1; d[1][4] = (w12 + w32) * dudw2; d[2][4] = 2 * w3 * u + (w12 + w32) * dudw3;
    d[0][5] = -(v + w1 * dvdw1) - w2 * w3 * dudw1; d[1][5] = -w1 * dvdw2 - (w3 * u + w2 * w3 * dudw2); d[2][5] = -w1 * dvdw3 - (w2 * u + w2 * w3 * dudw3);
    d[0][6] = -w2 * dvdw1 - (w3 * u + w1 * w3 * dudw1); d[1][6] = -(v + w2 * dvdw2) - w1 * w3 * dudw2; d[2][6] = -w2 * dvdw3 - (w1 * u + w1 * w3 * dudw3);
    d[0][7] = (v + w1 * dvdw1) - w2 * w3 * dudw1; d[1][7] = w1 * dvdw2 - (w3 * u + w2 * w3 * dudw2); d[2][7] = w1 * dvdw3 - (w2 * u + w2 * w3 * dudw3);
    d[0][8] = 2 * w1 * u + (w12 + w22) * dudw1; d[1][8] = 2 * w2 * u + (w12 + w22) * dudw2; d[2][8] = (w22 + w32) * dudw3;
}

// 6x6 symmetric solve (Eigen::JacobiSVD(H).solve(g) stand-in, S5:375-388).  Well-conditioned systems go through
// a Cholesky factorisation; anything else falls back to the oracle's Jacobi pseudo-inverse with Eigen's rank
// threshold.  Returns 0 when the condition number would be NaN (voecBadCondNumber).
__device__ int solve_sym6(const double* H, const double* g, double* x)
{
    double dmax = 0; bool bad = false;
    for (int i = 0; i < 36; i++) if (isnan(H[i]) || isinf(H[i])) bad = true;
    for (int i = 0; i < 6; i++) { if (isnan(g[i])) bad = true; dmax = fmax(dmax, fabs(H[i * 7])); }
    if (bad) return 0;
    double L[36];
    bool spd = dmax > 0;
    if (spd) {
        double amp = 4.0 * DBL_EPSILON;                                      // the growth bound of chol6's pivot test (see there)
        for (int j = 0; j < 6 && spd; j++) {
            double s = H[j * 6 + j];
            for (int k = 0; k < j; k++) s -= L[j * 6 + k] * L[j * 6 + k];
            if (!(s > 1e-13 * dmax) || !(s > amp * H[j * 6 + j])) { spd = false; break; }
            amp *= H[j * 6 + j] / s;
            const double ljj = sqrt(s);
            L[j * 6 + j] = ljj;
            for (int i = j + 1; i < 6; i++) {
                double t = H[i * 6 + j];
                for (int k = 0; k < j; k++) t -= L[i * 6 + k] * L[j * 6 + k];
                L[i * 6 + j] = t / ljj;
            }
        }
    }
    if (spd) {
        double y[6];
        for (int i = 0; i < 6; i++) { double t = g[i]; for (int k = 0; k < i; k++) t -= L[i * 6 + k] * y[k]; y[i] = t / L[i * 6 + i]; }
        for (int i = 5; i >= 0; i--) { double t = y[i]; for (int k = i + 1; k < 6; k++) t -= L[k * 6 + i] * x[k]; x[i] = t / L[i * 6 + i]; }
        return 1;
    }
    // rank-deficient or indefinite: cyclic Jacobi eigen-decomposition + pseudo-inverse (oracle's solve_sym6)
    double A[36], V[36];
    for (int i = 0; i < 36; i++) { A[i] = H[i]; V[i] = (i % 7 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; sweep++) {
        double off = 0, dg = 0;
        for (int p = 0; p < 6; p++) { dg += A[p * 7] * A[p * 7]; for (int q = p + 1; q < 6; q++) off += A[p * 6 + q] * A[p * 6 + q]; }
        if (!(off > 1e-32 * dg)) break;
        for (int p = 0; p < 5; p++)
            for (int q = p + 1; q < 6; q++) {
                const double apq = A[p * 6 + q];
                if (apq == 0.0) continue;
                const double theta = (A[q * 6 + q] - A[p * 6 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 6; k++) { const double akp = A[k * 6 + p], akq = A[k * 6 + q]; A[k * 6 + p] = cs * akp - sn * akq; A[k * 6 + q] = sn * akp + cs * akq; }
                for (int k = 0; k < 6; k++) { const double apk = A[p * 6 + k], aqk = A[q * 6 + k]; A[p * 6 + k] = cs * apk - sn * aqk; A[q * 6 + k] = sn * apk + cs * aqk; }
                for (int k = 0; k < 6; k++) { const double vkp = V[k * 6 + p], vkq = V[k * 6 + q]; V[k * 6 + p] = cs * vkp - sn * vkq; V[k * 6 + q] = sn * vkp + cs * vkq; }
            }
    }
    double smax = 0, smin = DBL_MAX;
    for (int i = 0; i < 6; i++) { const double s = fabs(A[i * 7]); if (s > smax) smax = s; if (s < smin) smin = s; }
    const double cond = smax / smin;
    if (isnan(cond)) return 0;
    const double thr = 6.0 * DBL_EPSILON * smax;
    for (int i = 0; i < 6; i++) x[i] = 0;
    for (int i = 0; i < 6; i++) {
        const double lam = A[i * 7];
        if (!(fabs(lam) > thr)) continue;
        double dot = 0;
        for (int k = 0; k < 6; k++) dot += V[k * 6 + i] * g[k];
        const double coef = dot / lam;
        for (int k = 0; k < 6; k++) x[k] += coef * V[k * 6 + i];
    }
    return 1;
}

// The general path out of line, fed from the 28 block sums in LDS and answering into LDS: rarely taken, and kept away from the
// iteration body so that neither its code nor a memory copy of H (an array whose address escapes lives in scratch) sits in it.
__device__ __attribute__((noinline)) int solve_sym6_from_sums(const double* tot, double* x_out)
{
    double H[36], g[6], x[6] = { 0, 0, 0, 0, 0, 0 };
    int h = 0;
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) { const double v = tot[h++]; H[a * 6 + b] = v; H[b * 6 + a] = v; }
    for (int a = 0; a < 6; a++) g[a] = tot[21 + a];
    const int ok = solve_sym6(H, g, x);
    for (int a = 0; a < 6; a++) x_out[a] = x[a];
    return ok;
}

// CPose3D(CPose3DRotVec(delta).getInverse()) -> x y z yaw pitch roll (S5:717-718; oracle's svo_oracle_delta_to_pose)
__device__ void delta_to_pose(const double* dp, double* pose)
{
    const double w1 = dp[0], w2 = dp[1], w3 = dp[2];
    const double th = sqrt(w1 * w1 + w2 * w2 + w3 * w3);
    double R[9];
    if (th < 1e-10) { R[0] = 1; R[1] = -w3; R[2] = w2; R[3] = w3; R[4] = 1; R[5] = -w1; R[6] = -w2; R[7] = w1; R[8] = 1; }
    else {
        const double a = sin(th) / th, b = (1.0 - cos(th)) / (th * th);
        R[0] = 1 - b * (w2 * w2 + w3 * w3); R[1] = -a * w3 + b * w1 * w2; R[2] = a * w2 + b * w1 * w3;
        R[3] = a * w3 + b * w1 * w2; R[4] = 1 - b * (w1 * w1 + w3 * w3); R[5] = -a * w1 + b * w2 * w3;
        R[6] = -a * w2 + b * w1 * w3; R[7] = a * w1 + b * w2 * w3; R[8] = 1 - b * (w1 * w1 + w2 * w2);
    }
    const double Ri[9] = { R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8] };
    pose[0] = -(Ri[0] * dp[3] + Ri[1] * dp[4] + Ri[2] * dp[5]);
    pose[1] = -(Ri[3] * dp[3] + Ri[4] * dp[4] + Ri[5] * dp[5]);
    pose[2] = -(Ri[6] * dp[3] + Ri[7] * dp[4] + Ri[8] * dp[5]);
    const double pitch = atan2(-Ri[6], hypot(Ri[0], Ri[3]));
    double yaw, roll;
    if (fabs(Ri[7]) + fabs(Ri[8]) < 10 * DBL_EPSILON) { roll = 0.0; yaw = pitch > 0 ? atan2(Ri[5], Ri[2]) : atan2(-Ri[5], -Ri[2]); }
    else { roll = atan2(Ri[7], Ri[8]); yaw = atan2(Ri[3], Ri[0]); }
    pose[3] = yaw; pose[4] = pitch; pose[5] = roll;
}

#define GN_NSUM 28
#define GN_NT_MAX 512        // the kernel is built for 256, 384 and 512 threads per lane (template parameter NT): SVO_GN_NT picks, see launch_gauss_newton
// Lists of up to GN_LCAP tracked pairs keep the sort / hash arrays of the stage-5 NMS mask and the two byte arrays in LDS
// (30 bytes per entry); longer lists use the lane's region of DevCtx::gn_scratch in global memory.  The LDS a block asks for
// therefore depends on what a frame of the workload tracks (a few hundred pairs), not on the capacity of the context's lists:
// 33 KB instead of 123 KB at max_kps 4096, so that a lane's block finds room on a CU beside the detector's tiles (round 5).
#define GN_LCAP 1024
struct GnShared {
    double part[GN_NT_MAX / 64][GN_NSUM];      // the 28 sums of every wave (reduced inside the wave on the DPP / permlane network)
    double tot[GN_NSUM];
    double step[6];
    double delta[6];
    double cost;
    Rot R;
    int ok;
    int n_non_masked;
};

// Dynamic LDS and scratch of k_gauss_newton<NT>: ONE description (the form of k_match.hip's layouts).  The per-entry arrays keys |
// hkey, hval | cellxy | state | mask hold n entries each: n = lc() in LDS, n = pmax in the lane's region of DevCtx::gn_scratch.  In
// LDS scan[] and one GnShared follow them.  No static LDS.
#define LDS_FN __host__ __device__ constexpr int
struct LdsGaussNewton {
    int pmax;
    static constexpr int PER_ENTRY = 8 + 2 * 2 * 4 + 4 + 1 + 1;
    LDS_FN lc() const { return pmax < GN_LCAP ? pmax : GN_LCAP; }
    static LDS_FN n_keys(int n) { return n; }              // u64
    static LDS_FN n_hash(int n) { return 2 * n; }          // uint32_t, twice: hkey, hval
    static LDS_FN n_cellxy(int n) { return n; }            // uint32_t
    static LDS_FN n_state(int n) { return n; }             // unsigned char
    static LDS_FN n_mask(int n) { return n; }              // unsigned char
    static __host__ __device__ constexpr size_t entry_bytes(int n) { return (size_t)n * PER_ENTRY; }
    LDS_FN n_scan() const { return 40; }                   // int
    LDS_FN n_spare() const { return 16; }                  // bytes behind the GnShared: nothing is carved from them; the total has always asked for them
    LDS_FN total() const { return (int)entry_bytes(lc()) + 4 * n_scan() + (int)sizeof(GnShared) + n_spare(); }
    __host__ __device__ constexpr size_t scratch_bytes_per_lane() const { return entry_bytes(pmax); }
};
#undef LDS_FN
static_assert(8 * LdsGaussNewton::n_keys(64) + 4 * (2 * LdsGaussNewton::n_hash(64) + LdsGaussNewton::n_cellxy(64)) + LdsGaussNewton::n_state(64) + LdsGaussNewton::n_mask(64) == 30 * 64, "the per-entry arrays fill entry_bytes()");
static_assert(sizeof(GnShared) == 2424 && LdsGaussNewton{64}.total() == 4520 && LdsGaussNewton{1024}.total() == 33320 && LdsGaussNewton{16384}.total() == 33320, "k_gauss_newton LDS totals: 30 * min(pmax, 1024) + 160 + 2424 + 16");
static_assert(LdsGaussNewton{64}.scratch_bytes_per_lane() == 30 * 64 && LdsGaussNewton{16384}.scratch_bytes_per_lane() == 30 * 16384, "k_gauss_newton scratch");
static_assert(LdsGaussNewton{16384}.total() <= 160 * 1024, "gfx950: 160 KB of LDS per CU");
// What k_gauss_newton leaves per lane in GNParams::mask_out for k_pose_covariance and k_landmarks (svo_set_pose_covariance or
// svo_set_landmarks allocates it, whichever comes first): {int ended_valid, int T, pad to HEAD} | mask[pmax].  ended_valid is cleared
// ("consumed") by the LAST kernel that reads the record: k_landmarks when it runs, else k_pose_covariance.
struct GnMaskRecord {
    int pmax;
    static constexpr int HEAD = 16;
    __host__ __device__ constexpr size_t bytes() const { return (size_t)pmax + HEAD; }
};
static_assert(GnMaskRecord{64}.bytes() == 64 + 16 && GnMaskRecord{16384}.bytes() == 16384 + 16, "mask-out record");

// ---- the 28 sums of a wave without LDS ----------------------------------------------------------------------------------
// v_permlane16_swap / v_permlane32_swap (gfx950) exchange the odd rows of one register with the even rows of another (the upper
// half with the lower half): for a PAIR of sums (a, b) one swap per dword and one add leave "a over both rows" in one row and "b
// over both rows" in the other -- each step halves the number of live values instead of doubling the work: 28 -> 14 -> 7 values,
// then four DPP steps inside the rows of 16.  147 instructions per wave and iteration; a butterfly per sum would be 504.
template <bool ROW16>
__device__ __forceinline__ double gn_fold(double a, double b)
{
    const uint32_t a0 = (uint32_t)__double2loint(a), a1 = (uint32_t)__double2hiint(a), b0 = (uint32_t)__double2loint(b), b1 = (uint32_t)__double2hiint(b);
    if (ROW16) {
        const auto r0 = __builtin_amdgcn_permlane16_swap(a0, b0, false, false), r1 = __builtin_amdgcn_permlane16_swap(a1, b1, false, false);
        return __hiloint2double((int)r1[0], (int)r0[0]) + __hiloint2double((int)r1[1], (int)r0[1]);
    }
    const auto r0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false), r1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
    return __hiloint2double((int)r1[0], (int)r0[0]) + __hiloint2double((int)r1[1], (int)r0[1]);
}
template <int CTRL>
__device__ __forceinline__ double gn_dpp_add(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false), hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return v + __hiloint2double(hi, lo);
}
// acc[28] of every lane -> out[28] = the wave's sums (written by one lane per row of 16: 7 sums each)
__device__ __forceinline__ void gn_wave_sums(const double* acc, double* out)
{
    double n[14], m[7];
#pragma unroll
    for (int j = 0; j < 14; j++) n[j] = gn_fold<true>(acc[j], acc[j + 14]);       // rows 0, 2: sum j over two rows; rows 1, 3: sum j + 14
#pragma unroll
    for (int j = 0; j < 7; j++) m[j] = gn_fold<false>(n[j], n[j + 7]);            // lanes 0..31: n[j] over both halves; lanes 32..63: n[j + 7]
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double v = m[j];
        v = gn_dpp_add<0xB1>(v);       // quad_perm [1,0,3,2]
        v = gn_dpp_add<0x4E>(v);       // quad_perm [2,3,0,1]
        v = gn_dpp_add<0x141>(v);      // row_half_mirror
        v = gn_dpp_add<0x140>(v);      // row_mirror
        m[j] = v;
    }
    const int lane = threadIdx.x & 63;
    if ((lane & 15) == 0) {
        const int row = lane >> 4, base = (row & 1) * 14 + (row >> 1) * 7;       // row 0: sums 0..6, row 1: 14..20, row 2: 7..13, row 3: 21..27
#pragma unroll
        for (int j = 0; j < 7; j++) out[base + j] = m[j];
    }
}

// Solve of the 6x6 normal equations by the square-root-free Cholesky form H = L D L^T (unit lower L), every index static
// (registers, no scratch).  This runs on ONE thread between two barriers of every iteration, so what counts is the length of
// its dependent chain: one division per column, where L L^T needs a square root and a division (~30 dependent instructions more
// per column).  Same pivots as the L L^T form (d_j = l_jj^2), same positivity test; the solution agrees to rounding, which is
// what stage 5's tolerance is stated in.  Returns false when a pivot is not safely positive; the caller then takes the general
// path (solve_sym6).
// "Safely" has two parts.  s > 1e-13 * dmax alone is not enough: a pivot d_k far below its diagonal entry H_kk is the difference of
// two nearly equal numbers, its rounding error is of the order DBL_EPSILON * H_kk, and every later pivot inherits that error
// multiplied by up to H_kk / d_k.  On a rank-deficient H (collinear landmarks) a genuine fifth pivot of 8.7e-9 * H_55 left a sixth
// "pivot" of +-1e-10 * dmax that was nothing but that noise, positive or negative with the summation order, and a positive one
// passed the first test: the step then had a component of ~2000 times its norm along the direction the pseudo-inverse cuts
// (tests/test_gpu_stage5.py, collinear-eps0).  So a pivot must also exceed 4 * DBL_EPSILON * H_jj * prod_{k<j} H_kk / d_k, the noise
// the columns before it can have put into it; the product is 1 ... 1e4 on ordinary frames.
// (Split in two so that k_pose_covariance can factor once and solve six times; chol6 below is the pair, as the iteration uses it.)
__device__ __forceinline__ bool chol6_factor(const double* H, double dmax, double (&L)[6][6], double (&inv)[6])
{
    double d[6];
    bool ok = true;
    double amp = 4.0 * DBL_EPSILON;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double w[6];                                                        // w[k] = L[j][k] * d[k]
        double s = H[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) { w[k] = L[j][k] * d[k]; s = __builtin_fma(-L[j][k], w[k], s); }
        ok = ok && (s > 1e-13 * dmax) && (s > amp * H[j * 6 + j]);
        d[j] = s;
        inv[j] = gn_rcp(s);
        amp *= H[j * 6 + j] * inv[j];
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double t = H[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) t = __builtin_fma(-L[i][k], w[k], t);
            L[i][j] = t * inv[j];
        }
    }
    return ok;
}
__device__ __forceinline__ void chol6_solve(const double (&L)[6][6], const double (&inv)[6], const double* g, double* x)
{
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { double t = g[i];
#pragma unroll
        for (int k = 0; k < i; k++) t = __builtin_fma(-L[i][k], y[k], t);
        y[i] = t; }
#pragma unroll
    for (int i = 5; i >= 0; i--) { double t = y[i] * inv[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) t = __builtin_fma(-L[k][i], x[k], t);
        x[i] = t; }
}
__device__ __forceinline__ bool chol6(const double* H, const double* g, double dmax, double* x)
{
    double L[6][6], inv[6];
    const bool ok = chol6_factor(H, dmax, L, inv);
    chol6_solve(L, inv, g, x);
    return ok;
}

// One landmark of m_evalRGN: the projection through R, t (S5:180-195), its 4 x 6 Jacobian (S5:197-257) and, when that is finite
// (S5:322), the four float-minus-float residuals (S5:335-338).  Shared by eval_rgn and k_pose_covariance: one copy of the formulas.
__device__ __forceinline__ bool gn_point(const svo_stereo_camera& cam, const Rot& R, bool small_angle, double t1, double t2, double t3,
                                         const double* lmk, const float* obs, int m, double (&J)[4][6], double (&ri)[4])
{
#pragma clang fp contract(fast)
    const double X1p = lmk[3 * m], Y1p = lmk[3 * m + 1], Z1p = lmk[3 * m + 2];
    const double* r = R.r;
    const double X1c = r[0] * X1p + r[1] * Y1p + r[2] * Z1p + t1;
    const double Y1c = r[3] * X1p + r[4] * Y1p + r[5] * Z1p + t2;
    const double Z1c = r[6] * X1p + r[7] * Y1p + r[8] * Z1p + t3;
    const double X2c = X1c - cam.baseline;
    // S5:189-193 and 251-254 with the 28 divisions by Z1c / Z1c^2 folded into two reciprocals
    const double iz = gn_rcp(Z1c), iz2 = iz * iz;
    const float pl_x = (float)(cam.l_fx * X1c * iz + cam.l_cx), pl_y = (float)(cam.l_fy * Y1c * iz + cam.l_cy);
    const float pr_x = (float)(cam.r_fx * X2c * iz + cam.r_cx), pr_y = (float)(cam.r_fy * Y1c * iz + cam.r_cy);
    bool good = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double X1cd, Y1cd, Z1cd;
        if (j < 3) {
            if (small_angle) {
                if (j == 0) { X1cd = 0; Y1cd = -Z1p; Z1cd = Y1p; }
                else if (j == 1) { X1cd = Z1p; Y1cd = 0; Z1cd = -X1p; }
                else { X1cd = -Y1p; Y1cd = X1p; Z1cd = 0; }
            } else {
                const double* d = R.dr[j];
                X1cd = d[0] * X1p + d[1] * Y1p + d[2] * Z1p;
                Y1cd = d[3] * X1p + d[4] * Y1p + d[5] * Z1p;
                Z1cd = d[6] * X1p + d[7] * Y1p + d[8] * Z1p;
            }
        } else { X1cd = j == 3; Y1cd = j == 4; Z1cd = j == 5; }
        const double ju = (X1cd * Z1c - X1c * Z1cd) * iz2, jv = (Y1cd * Z1c - Y1c * Z1cd) * iz2, jur = (X1cd * Z1c - X2c * Z1cd) * iz2;
        J[0][j] = cam.l_fx * ju; J[1][j] = cam.l_fy * jv; J[2][j] = cam.r_fx * jur; J[3][j] = cam.r_fy * jv;
        if (isnan(ju) || isinf(ju) || isnan(jv) || isinf(jv) || isnan(jur) || isinf(jur)) good = false;
    }
    if (!good) return false;                                               // S5:322
    const float* o = obs + 8 * (long long)m;
    ri[0] = (double)(o[4] - pl_x); ri[1] = (double)(o[5] - pl_y); ri[2] = (double)(o[6] - pr_x); ri[3] = (double)(o[7] - pr_y);   // float subtraction, S5:335-338
    return true;
}

// One landmark of stage 5's triangulation (S5:529-544) from the previous frame's ul, vl, ur: xyz = baseline / den * (fr (ul - cul),
// fr (vl - cvl), fl fr).  Returns den = fl (cur - ur) + fr (ul - cul).  Shared by k_gauss_newton and k_landmarks: one copy of the formula.
__device__ __forceinline__ double gn_triangulate(double baseline, double fl, double fr, double cul, double cvl, double cur_,
                                                 double ul, double vl, double ur, double* xyz)
{
    const double den = fl * (cur_ - ur) + fr * (ul - cul);
    const double b_d = baseline / den;
    xyz[0] = b_d * fr * (ul - cul); xyz[1] = b_d * fr * (vl - cvl); xyz[2] = b_d * fl * fr;
    return den;
}

// Block reduction of the 28 sums: inside every wave on the permlane / DPP network (no LDS), then GN_NT / 64 x 28 doubles through
// LDS (1.3 KB; rounds 1-4 staged all 28 x GN_NT values there: 86 KB, and one more barrier).  Wave 0 adds the wave sums into tot; its
// first thread may go on to read them: LDS operations of one wave are ordered, so no block barrier in between.
template <int GN_NT>
__device__ __forceinline__ void gn_block_sums(const double* acc, double (*part)[GN_NSUM], double* tot)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    gn_wave_sums(acc, part[wid]);
    __syncthreads();
    if (wid == 0) {
        if (lane < GN_NSUM) {
            double sum = part[0][lane];
#pragma unroll
            for (int w = 1; w < GN_NT / 64; w++) sum += part[w][lane];
            tot[lane] = sum;
        }
        wave_lds_sync();
    }
}

// one m_evalRGN (S5:275-390) with the rotation taken from sh.R / sh.delta (prepared by thread 0).  On return every
// thread sees sh.ok, sh.cost, sh.step, and sh.delta / sh.R already advanced by the step (S5:576-577).
template <int GN_NT>
__device__ void eval_rgn(const GNParams& P, const svo_stereo_camera& cam, int T, const unsigned char* mask,
                         const double* lmk, const float* obs, double* residual, GnShared& sh, int dbg = 0)
{
    // Contraction ON inside the iteration (the file is compiled with -ffp-contract=off for the kernels that are compared bit for
    // bit): stage 5 is held to the oracle by a tolerance, and a lone wave pays ~5 cycles per instruction whatever it is, so
    // a * b + c as one v_fma_f64 instead of two instructions is a third of this function's arithmetic.
#pragma clang fp contract(fast)
    const int tid = threadIdx.x;
    const double b2 = P.use_robust_kernel ? P.kernel_param * P.kernel_param : 0;
    const double b2_1 = P.use_robust_kernel ? 1. / b2 : 0;
    const double t1 = sh.delta[3], t2 = sh.delta[4], t3 = sh.delta[5];
    const bool small_angle = sh.R.small_angle != 0;
    double acc[GN_NSUM];
#pragma unroll
    for (int i = 0; i < GN_NSUM; i++) acc[i] = 0;
    for (int m = tid; m < T; m += blockDim.x) {
        if (!mask[m] || dbg == DBG_GN_NO_TRACK_LOOP) continue;
        double J[4][6], ri[4];
        if (!gn_point(cam, sh.R, small_angle, t1, t2, t3, lmk, obs, m, J, ri)) continue;          // S5:322
        const double s = ri[0] * ri[0] + ri[1] * ri[1] + ri[2] * ri[2] + ri[3] * ri[3];
        residual[m] = s;                                                        // S5:345
        double rho_p = 1, fi;
        if (P.use_robust_kernel) { const double q = 1 + (s * b2_1); rho_p = gn_rsqrt(q); const double nn = q * rho_p; fi = b2 * (nn - 1); }
        else fi = 0.5 * s;
        acc[27] += fi;
        int h = 0;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            const double jr = J[0][a] * ri[0] + J[1][a] * ri[1] + J[2][a] * ri[2] + J[3][a] * ri[3];
            acc[21 + a] += rho_p * jr;                                          // gradient weighted ...
#pragma unroll
            for (int b = a; b < 6; b++) { acc[h] += J[0][a] * J[0][b] + J[1][a] * J[1][b] + J[2][a] * J[2][b] + J[3][a] * J[3][b]; h++; }   // ... Hessian NOT (S5:364-369)
        }
    }
    gn_block_sums<GN_NT>(acc, sh.part, sh.tot);
    if (tid == 0) {
        double H[36], g[6], x[6] = { 0, 0, 0, 0, 0, 0 };
        {
            int h = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int b = a; b < 6; b++) { const double v = sh.tot[h]; H[a * 6 + b] = v; H[b * 6 + a] = v; h++; }
            }
        }
        double dmax = 0; bool bad = false;
#pragma unroll
        for (int a = 0; a < 6; a++) { g[a] = sh.tot[21 + a]; bad = bad || isnan(g[a]); dmax = fmax(dmax, fabs(H[a * 7])); }
#pragma unroll
        for (int i = 0; i < 36; i++) bad = bad || isnan(H[i]) || isinf(H[i]);
        int ok;
        if (bad) ok = 0;
        else if (dbg == DBG_GN_NO_SOLVE || dbg == DBG_GN_NO_SOLVE_NO_ROT) ok = 1;
        else if (dmax > 0 && chol6(H, g, dmax, x)) ok = 1;
        else { ok = solve_sym6_from_sums(sh.tot, sh.step);                      // rank-deficient: pseudo-inverse path (out of line)
#pragma unroll
            for (int a = 0; a < 6; a++) x[a] = sh.step[a]; }
        sh.ok = ok;
        sh.cost = sh.tot[27];
#pragma unroll
        for (int a = 0; a < 6; a++) { sh.step[a] = x[a]; sh.delta[a] += x[a]; }
        if (ok && dbg != DBG_GN_NO_ROT_UPDATE && dbg != DBG_GN_NO_SOLVE_NO_ROT) { double d6[6]; for (int a = 0; a < 6; a++) d6[a] = sh.delta[a]; rodrigues_with_derivs(d6, sh.R); }
    }
    __syncthreads();
}

template <int GN_NT>
__global__ void __launch_bounds__(GN_NT) k_gauss_newton(DevCtx c, GNParams P, uint8_t* scratch)
{
    SVO_TL_SCOPE(c, TL_GN, 0);
    SVO_LATENCY_CHAIN(c);
    // dynamic LDS: LdsGaussNewton{pmax}.  A lane that tracks more than LC pairs (`big`) keeps the per-entry arrays, sized pmax, in its region of c.gn_scratch.
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const LdsGaussNewton L{P.pmax};
    const int PM = P.pmax, LC = L.lc();
    const int lane_id = blockIdx.x, tid = threadIdx.x;
    if (lane_idle(c, lane_id)) return;
    int* scan = (int*)(smem + L.entry_bytes(LC));
    GnShared& sh = *(GnShared*)(scan + L.n_scan());
    LaneState& ls = c.lane[lane_id];
    svo_result& res = c.results[lane_id];
    if (!P.standalone && (!ls.has_prev || ls.m_error == SVO_VOEC_BAD_TRACKING)) return;      // P:305, P:332
    const svo_stereo_camera cam = c.cams[lane_id];
    // tracked pairs of all octaves, concatenated octave by octave (S5:419-461); toff[o] = first flat index of octave o
    const int cur = 1 - ls.prev_slot, prev = ls.prev_slot;
    int toff[SVO_MAX_OCTAVES + 1];
    toff[0] = 0;
    for (int o = 0; o < SVO_MAX_OCTAVES; o++) toff[o + 1] = toff[o] + (o < c.n_oct ? c.n_tracked[lane_id * c.oct_cap + o] : 0);
    int T = toff[SVO_MAX_OCTAVES];
    if (T > P.pmax) { T = P.pmax; if (tid == 0) { atomicOr(&c.status[lane_id], SVO_ST_KPS_OVERFLOW); atomicOr(&res.status, (int)SVO_ST_KPS_OVERFLOW); } }
    auto oct_of = [&](int i) { int o = 0; for (int q = 1; q < SVO_MAX_OCTAVES; q++) if (i >= toff[q] && q < c.n_oct) o = q; return o; };
    float* obs = c.gn_obs + (long long)lane_id * c.max_kps * 8;
    double* lmk = c.gn_lmk + (long long)lane_id * c.max_kps * 3;
    double* residual = c.residual + (long long)lane_id * c.max_kps;
    int* outl = c.outliers + (long long)lane_id * c.max_kps;
    int* cur_idx = c.trk_kq + (long long)lane_id * c.oct_cap * c.max_kps;      // tracked[..].second per point (the kept list of stage 4 is dead by now)

    const bool big = T > LC;                                                     // block-uniform
    const int AN = big ? PM : LC;
    unsigned char* abase = big ? scratch + (size_t)lane_id * L.scratch_bytes_per_lane() : smem;
    unsigned long long* keys = (unsigned long long*)abase;
    uint32_t* hkey = (uint32_t*)(keys + L.n_keys(AN));
    uint32_t* hval = hkey + L.n_hash(AN);
    uint32_t* cellxy = hval + L.n_hash(AN);
    unsigned char* state = (unsigned char*)(cellxy + L.n_cellxy(AN));
    unsigned char* mask = state + L.n_state(AN);
    int Pn = 64; while (Pn < T) Pn <<= 1;
    // ---- gather the four keypoint lists (S5:419-461, single octave) and the NMS sort keys ----
    for (int i = tid; i < Pn; i += blockDim.x) keys[i] = 0;
    for (int i = tid; i < T; i += blockDim.x) mask[i] = 0;
    __syncthreads();
    for (int i = tid; i < T; i += blockDim.x) {
        const int o = oct_of(i), vl = lane_id * c.oct_cap + o;
        const svo_index_pair tp = c.tracked[(long long)vl * c.max_kps + (i - toff[o])];
        const svo_dmatch a = c.matches[match_base(c, vl, prev) + tp.first], b = c.matches[match_base(c, vl, cur) + tp.second];
        const svo_keypoint l1 = c.kps[feat_base(c, vl, prev, 0) + a.queryIdx], r1 = c.kps[feat_base(c, vl, prev, 1) + a.trainIdx];
        const svo_keypoint l2 = c.kps[feat_base(c, vl, cur, 0) + b.queryIdx], r2 = c.kps[feat_base(c, vl, cur, 1) + b.trainIdx];
        const float sn = (float)(size_t)(c.n_oct > 1 ? (1 << o) : 1);            // scale_norm, S5:422 (applied only when nOctaves > 1)
        float* ob = obs + 8 * (long long)i;
        if (c.n_oct > 1) { ob[0] = l1.x * sn; ob[1] = l1.y * sn; ob[2] = r1.x * sn; ob[3] = r1.y * sn; ob[4] = l2.x * sn; ob[5] = l2.y * sn; ob[6] = r2.x * sn; ob[7] = r2.y * sn; }
        else { ob[0] = l1.x; ob[1] = l1.y; ob[2] = r1.x; ob[3] = r1.y; ob[4] = l2.x; ob[5] = l2.y; ob[6] = r2.x; ob[7] = r2.y; }
        cur_idx[i] = tp.second;
        keys[i] = ((unsigned long long)ord32(l1.response) << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)i);
    }
    __threadfence_block();
    if (c.debug_mode == DBG_GN_STOP_GATHER) return;                                            // timing probes 64-67: the set-up, phase by phase (tests/dev/gn_breakdown.py)
    // ---- m_non_max_sup mask overload on the previous-left coordinates (S5:465-474 -> S2:225-283); cap = T ----
    if (!big) {
        // at most GN_LCAP keys, a few hundred as a rule: every key counts the keys above it (the keys are unique, so the counts are the descending ranks).
        // All lanes read the same LDS word at a time (a broadcast): T reads per key and two barriers, where the bitonic network
        // needs 45 compare-exchange stages at 512 keys (~10 us of the ~25 us this kernel spends before its first iteration).
        unsigned long long* sorted = (unsigned long long*)hkey;             // 2 PM u32 = PM u64, free until the NMS builds its hash
        __syncthreads();
        // (round 6: this loop was 26 of the kernel's ~44 us of set-up at 380 tracks -- one dependent ds_read_b64 per key, ~70 cycles each.
        // Four keys per step through two 16-byte reads, four steps unrolled: sixteen keys in flight.  The pad keys[T .. Pn) is 0: never above.)
        for (int i = tid; i < T; i += blockDim.x) {
            const unsigned long long k = keys[i];
            int above = 0;
            const ulonglong2* k2 = (const ulonglong2*)keys;
#pragma unroll 4
            for (int j = 0; j < (T + 3) / 4; j++) {
                const ulonglong2 a = k2[2 * j], b = k2[2 * j + 1];
                above += (a.x > k ? 1 : 0) + (a.y > k ? 1 : 0) + (b.x > k ? 1 : 0) + (b.y > k ? 1 : 0);
            }
            sorted[above] = k;
        }
        __syncthreads();
        for (int i = tid; i < T; i += blockDim.x) keys[i] = sorted[i];
        __syncthreads();
    } else bitonic_sort_lds<true>(keys, Pn);
    if (c.debug_mode == DBG_GN_STOP_SORT) return;
    {
        const unsigned cell = (unsigned)((double)P.min_distance / 2.0);
        const float inv = 1.0f / (float)cell;
        const unsigned glx = (unsigned)(1 + (float)P.img_w * inv), gly = (unsigned)(1 + (float)P.img_h * inv);
        for (int i = tid; i < T; i += blockDim.x) {
            const int m = (int)(0xFFFFFFFFu - (uint32_t)(keys[i] & 0xFFFFFFFFull));
            const size_t ux = (size_t)(obs[8 * (long long)m] * inv), uy = (size_t)(obs[8 * (long long)m + 1] * inv);
            cellxy[i] = (ux < glx && uy < gly) ? (((uint32_t)ux << 16) | (uint32_t)uy) : 0xFFFFFFFFu;
        }
        __syncthreads();
        int hsz = 128; while (hsz < 2 * T) hsz <<= 1;
        grid_nms_block<0>(T, gly, cellxy, hkey, hval, hsz, state, scan + 32);
        int cnt = 0;
        for (int i = tid; i < T; i += blockDim.x) if (state[i] == 1) { mask[(int)(0xFFFFFFFFu - (uint32_t)(keys[i] & 0xFFFFFFFFull))] = 1; cnt++; }
        int tot; block_exclusive_scan(cnt, scan, &tot);
        if (tid == 0) sh.n_non_masked = tot;
        __syncthreads();
    }
    int n_non_masked = sh.n_non_masked;
    if (c.debug_mode == DBG_GN_STOP_MASK) return;
    if (n_non_masked < 8) { if (tid == 0) { res.valid = 0; res.n_residual = 0; res.n_outliers = 0; } return; }       // S5:521-526
    // ---- triangulation (S5:529-544) ----
    const double cul = cam.l_cx, cvl = cam.l_cy, fl = cam.l_fx, cur_ = cam.r_cx, fr = cam.r_fx, baseline = cam.baseline;
    auto triangulate = [&]() {
        for (int m = tid; m < T; m += blockDim.x) {
            if (!mask[m]) continue;
            const double ul = obs[8 * (long long)m], vl = obs[8 * (long long)m + 1], ur = obs[8 * (long long)m + 2];
            gn_triangulate(baseline, fl, fr, cul, cvl, cur_, ul, vl, ur, lmk + 3 * m);
        }
    };
    triangulate();
    if (c.debug_mode == DBG_GN_STOP_TRIANGULATE) return;
    if (tid == 0) {
        double d6[6] = { 0, 0, 0, 0, 0, 0 };
        if (P.use_custom_initial_pose) { for (int k = 0; k < 6; k++) d6[k] = P.init[k]; }                            // S5:504-505
        else if (P.use_previous_pose_as_initial) { for (int k = 0; k < 6; k++) d6[k] = ls.last_pose[k]; }            // S5:506-507
        for (int k = 0; k < 6; k++) sh.delta[k] = d6[k];
        rodrigues_with_derivs(d6, sh.R);
    }
    __threadfence_block();
    __syncthreads();
    if (c.debug_mode == DBG_GN_STOP_SETUP) return;
    double pCost = 0, cCost = 0; bool done = false, abort_ = false;
    unsigned timesInc = 0; int num_it = 0, num_it_final = 0, err_code = res.error_code;
    bool first = true;
    // Both phases run through ONE copy of the iteration body (a second inlined copy of eval_rgn made the kernel ~100 KB of code, more
    // than the instruction cache holds: every iteration then fetched its code again).  phase 0 = S5:549-598, phase 1 = S5:650-700;
    // timesInc, pCost, cCost carry over from one to the other.
    const bool cap1 = c.debug_mode == DBG_GN_ONE_ITER || debug_mode_gn_loop_ablation(c.debug_mode);
    int n_res = 0, n_out = 0;
    for (int phase = 0; phase < 2; phase++) {
        const int limit = phase ? P.max_iters : P.initial_max_iters;
        int it = 0;
        done = false; abort_ = false;
        while (it < limit && !done && !abort_ && !(cap1 && it >= 1)) {
            pCost = cCost;
            if (first) { for (int m = tid; m < T; m += blockDim.x) residual[m] = DBL_MAX; first = false; }            // S5:296
            eval_rgn<GN_NT>(P, cam, T, mask, lmk, obs, residual, sh, c.debug_mode);
            if (phase == 0) err_code = SVO_VOEC_NONE;                                                                // S5:299
            cCost = sh.cost;
            if (!sh.ok) {
                if (tid == 0) {
                    ls.m_error = SVO_VOEC_BAD_COND_NUMBER; res.valid = 0; res.num_it = phase ? num_it : it;
                    if (phase == 0) { res.error_code = SVO_VOEC_BAD_COND_NUMBER; res.n_residual = 0; res.n_outliers = 0; }      // S5:380-386, 569-573
                    else { res.num_it_final = it; res.error_code = err_code; res.n_residual = T; res.n_outliers = n_out; }      // S5:670-675 (result.error_code untouched)
                }
                return;
            }
            double m2 = 0;
            for (int k = 0; k < 6; k++) m2 += sh.step[k] * sh.step[k];
            if (it > 0) {
                done = sqrt(m2) < P.min_mod_out_vector;
                if (pCost < cCost) { if (++timesInc > (unsigned)P.max_incr_cost) { err_code = phase ? SVO_VOEC_INCR_FUNC_COST_STG2 : SVO_VOEC_INCR_FUNC_COST_STG1; abort_ = true; } }
            }
            it++;
            // no barrier here: eval_rgn ends with one, and thread 0 rewrites sh.* only behind the next call's two barriers
        }
        if (phase) { num_it_final = it; break; }
        num_it = it;
        // ---- keep only the inliers (S5:601-611); "outliers" receives the INLIER cur-match indices ----
        n_res = first ? 0 : T;
        for (int base = 0; base < n_res; base += blockDim.x) {
            const int i = base + tid;
            int keep = 0;
            if (i < n_res) { if (residual[i] > P.residual_threshold) mask[i] = 0; else keep = 1; }
            int tot;
            const int off = block_exclusive_scan(keep, scan, &tot);
            if (keep) outl[n_out + off] = cur_idx[i];
            n_out += tot;
            __syncthreads();
        }
        {
            int cnt = 0;
            for (int m = tid; m < T; m += blockDim.x) cnt += mask[m];
            int tot; block_exclusive_scan(cnt, scan, &tot);
            n_non_masked = tot;
            __syncthreads();
        }
        if (n_non_masked < 8) {                                                                                      // S5:616-621
            if (tid == 0) { res.valid = 0; res.num_it = num_it; res.error_code = err_code; res.n_residual = n_res; res.n_outliers = n_out; }
            return;
        }
        triangulate();                                                                                               // S5:623-638
        __threadfence_block();
        __syncthreads();
    }
    if (tid == 0) {
        double pose[6], delta[6];
        for (int k = 0; k < 6; k++) delta[k] = sh.delta[k];
        delta_to_pose(delta, pose);                                                                                  // S5:717-718
        for (int k = 0; k < 6; k++) { res.outPose[k] = pose[k]; res.delta[k] = delta[k]; }
        if (!P.use_custom_initial_pose && P.use_previous_pose_as_initial) for (int k = 0; k < 6; k++) ls.last_pose[k] = delta[k];   // S5:720-721
        res.tracked_feats_from_last_frame = T;                                                                       // S5:724
        res.tracked_feats_from_last_KF = ls.num_tracked_last_kf;                                                     // S5:725
        res.num_it = num_it; res.num_it_final = num_it_final; res.error_code = err_code;
        res.n_residual = n_res > T ? n_res : T; res.n_outliers = n_out;
        res.valid = !abort_;                                                                                         // S5:727
    }
    // svo_set_pose_covariance / svo_set_landmarks: the final mask, T and whether this run ended valid, for k_pose_covariance and k_landmarks (GnMaskRecord)
    if (P.mask_out) {
        uint8_t* mo = P.mask_out + (size_t)lane_id * GnMaskRecord{PM}.bytes();
        for (int m = tid; m < T; m += blockDim.x) mo[GnMaskRecord::HEAD + m] = mask[m];
        if (tid == 0) { ((int*)mo)[0] = !abort_; ((int*)mo)[1] = T; }
    }
}

size_t gn_scratch_bytes_per_lane(int pmax) { return LdsGaussNewton{pmax}.scratch_bytes_per_lane(); }

hipError_t svo_raise_dyn_smem(const void* kernel, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void*>, size_t> cur;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    size_t& have = cur[std::make_pair(dev, kernel)];
    if (bytes <= have) return hipSuccess;
    e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) have = bytes;
    return e;
}

// Every instantiation gets the limit.  A plain list and not gn_for_threads below: the three are first named here, ascending, and the
// order of first naming is the order in which the compiler emits them into the code object (the ladder would name them descending).
hipError_t configure_gauss_newton(int pmax)
{
    for (const void* fn : { (const void*)k_gauss_newton<256>, (const void*)k_gauss_newton<384>, (const void*)k_gauss_newton<512> }) {
        const hipError_t e = svo_raise_dyn_smem(fn, LdsGaussNewton{pmax}.total());
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// threads per lane: one pass of the per-track loop covers that many tracks per iteration (config 2 tracks ~290: 256 threads walk
// the loop twice); SVO_GN_NT = 256 / 384 / 512 overrides the default for an A/B (Knobs.gn_nt).  The one ladder over the three
// instantiations of k_gauss_newton and k_pose_covariance: f(std::integral_constant<int, nt>)
template <class F> static void gn_for_threads(int nt, F f)
{
    if (nt == 512) f(std::integral_constant<int, 512>());
    else if (nt == 384) f(std::integral_constant<int, 384>());
    else f(std::integral_constant<int, 256>());
}

void launch_gauss_newton(const DevCtx& c, const Knobs& k, const GNParams& P, hipStream_t st)
{
    gn_for_threads(k.gn_nt, [&](auto n) { constexpr int NT = decltype(n)::value; hipLaunchKernelGGL(k_gauss_newton<NT>, dim3(c.n_lanes), dim3(NT), (size_t)LdsGaussNewton{P.pmax}.total(), st, c, P, c.gn_scratch); });
}

// ------------------------------------------------------------------------------------------------------------
// The covariance of the pose increment (svo_set_pose_covariance, contract at svo_pose_cov in svo_types.h): no reference
// counterpart.  One more evaluation at the delta stage 5 returned, over the mask k_gauss_newton ended with (its mask-out array:
// one GnMaskRecord per lane) and the landmarks as it last triangulated them.
// A kernel of its own and not a tail of k_gauss_newton: the tail would add its 6 x 6 algebra to a kernel whose iteration body is
// sized to the instruction cache (see there), and to every context that never asks for a covariance.
// ------------------------------------------------------------------------------------------------------------
size_t gn_mask_bytes_per_lane(int pmax) { return GnMaskRecord{pmax}.bytes(); }

struct CovShared {
    double part[GN_NT_MAX / 64][GN_NSUM];
    double tot[GN_NSUM];          // 0..20 the upper triangle of A, 21 the weighted sum of squares, 22 the number of points
    double delta[6];
    Rot R;
    double A[36], C[36], G[36], M[36];
    double Rm[9], dR[27];         // the exact Rodrigues rotation of delta and its derivatives, for G
    int ended_valid, T;
};

// R = I + a K + b K^2 of the rotation vector w (delta_to_pose's matrix) and dR/dw_k, k = 0..2, for G.  Not Rot::dr: that holds the
// reference's S5:162 entry and is empty below 1e-5 rad, where m_evalRGN switches to the generators -- right for the Jacobian the
// iteration uses, wrong by 1e-5 for a derivative of outPose.  a = sin t / t, b = (1 - cos t) / t^2 and the factors of their
// derivatives, alpha = (cos t - a) / t^2 and beta = (a - 2 b) / t^2, by their series below 0.5 rad (the closed forms cancel).
__device__ void cov_rotation_derivs(const double* w, double* Rm, double* dR)
{
    const double z = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
    double a, b, al, be;
    if (z < 0.25) {
        double t = 1.0, p = 1.0 / 6.0;             // t_n = (-z)^n / (2n+1)!,  p_n = (-z)^n / (2n+3)!
        a = 0; b = 0; al = 0; be = 0;
        for (int n = 0; n < 12; n++) {
            a += t; b += t / (double)(2 * n + 2);
            al -= (double)(2 * n + 2) * p; be -= (double)(2 * n + 2) * p / (double)(2 * n + 4);
            t = -t * z / (double)((2 * n + 2) * (2 * n + 3));
            p = -p * z / (double)((2 * n + 4) * (2 * n + 5));
        }
    } else {
        const double th = sqrt(z), sn = sin(th), cs = cos(th);
        a = sn / th; b = (1.0 - cs) / z; al = (cs - a) / z; be = (a - 2.0 * b) / z;
    }
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            // K_ij = sg * w[3 - i - j] off the diagonal, sg = -1 where j follows i cyclically
            const double sg = i == j ? 0.0 : (((j - i + 3) % 3 == 1) ? -1.0 : 1.0);
            const int kk = i == j ? 0 : 3 - i - j;
            const double Kij = sg * w[kk], dij = i == j ? 1.0 : 0.0;
            Rm[i * 3 + j] = dij * (1.0 - b * z) + a * Kij + b * w[i] * w[j];
            for (int k = 0; k < 3; k++) {
                const double gk = (i != j && k == kk) ? sg : 0.0;
                dR[k * 9 + i * 3 + j] = al * w[k] * Kij + a * gk + be * w[k] * (w[i] * w[j] - z * dij)
                                        + b * ((i == k ? w[j] : 0.0) + (j == k ? w[i] : 0.0) - 2.0 * w[k] * dij);
            }
        }
}

template <int NT>
__global__ void __launch_bounds__(NT) k_pose_covariance(DevCtx c, GNParams P, svo_pose_cov* out, int consume)
{
    SVO_TL_SCOPE(c, TL_GN, 1);
    SVO_LATENCY_CHAIN(c);
    __shared__ CovShared sh;
    const int lane_id = blockIdx.x, tid = threadIdx.x;
    if (lane_idle(c, lane_id)) return;                                       // an idle lane keeps its record
    uint8_t* mo = P.mask_out + (size_t)lane_id * GnMaskRecord{P.pmax}.bytes();
    svo_pose_cov& o = out[lane_id];
    if (tid == 0) {
        sh.ended_valid = ((const int*)mo)[0]; sh.T = ((const int*)mo)[1];
        if (consume) ((int*)mo)[0] = 0;                                      // consumed: a later call whose stage 5 returns early finds no mask (k_landmarks does it when it follows)
        double d6[6];
        for (int k = 0; k < 6; k++) { d6[k] = c.results[lane_id].delta[k]; sh.delta[k] = d6[k]; }
        rodrigues_with_derivs(d6, sh.R);
    }
    {   // SVO_COV_NONE until proven otherwise: all zero
        double* w = (double*)&o;
        for (int i = tid; i < (int)(sizeof(svo_pose_cov) / sizeof(double)); i += NT) w[i] = 0.0;
    }
    __syncthreads();
    if (!sh.ended_valid) return;
    const int T = sh.T < P.pmax ? sh.T : P.pmax;
    const unsigned char* mask = mo + GnMaskRecord::HEAD;
    const svo_stereo_camera cam = c.cams[lane_id];
    const float* obs = c.gn_obs + (long long)lane_id * c.max_kps * 8;
    const double* lmk = c.gn_lmk + (long long)lane_id * c.max_kps * 3;
    double acc[GN_NSUM];
#pragma unroll
    for (int i = 0; i < GN_NSUM; i++) acc[i] = 0;
    {
#pragma clang fp contract(fast)
        const double b2_1 = P.use_robust_kernel ? 1. / (P.kernel_param * P.kernel_param) : 0;
        const double t1 = sh.delta[3], t2 = sh.delta[4], t3 = sh.delta[5];
        const bool small_angle = sh.R.small_angle != 0;
        for (int m = tid; m < T; m += NT) {
            if (!mask[m]) continue;
            double J[4][6], ri[4];
            if (!gn_point(cam, sh.R, small_angle, t1, t2, t3, lmk, obs, m, J, ri)) continue;
            const double s = ri[0] * ri[0] + ri[1] * ri[1] + ri[2] * ri[2] + ri[3] * ri[3];
            const double wt = P.use_robust_kernel ? gn_rsqrt(1 + (s * b2_1)) : 1.0;
            acc[21] += wt * s;
            acc[22] += 1.0;
            int h = 0;
#pragma unroll
            for (int a = 0; a < 6; a++) {
#pragma unroll
                for (int b = a; b < 6; b++) { acc[h] += wt * (J[0][a] * J[0][b] + J[1][a] * J[1][b] + J[2][a] * J[2][b] + J[3][a] * J[3][b]); h++; }
            }
        }
    }
    gn_block_sums<NT>(acc, sh.part, sh.tot);
    if (tid != 0) return;
    // ---- one thread: A, sigma2, A^-1, G and the two products.  Every value that has a mirror image is written to both places ----
    {
        int h = 0;
        for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) { const double v = sh.tot[h++]; sh.A[a * 6 + b] = v; sh.A[b * 6 + a] = v; }
    }
    for (int i = 0; i < 36; i++) o.info[i] = sh.A[i];
    const int n_used = (int)sh.tot[22], dof = 4 * n_used - 6;
    o.n_used = n_used; o.dof = dof;
    if (dof <= 0) { o.state = SVO_COV_NO_DOF; return; }
    const double sigma2 = sh.tot[21] / (double)dof;
    o.sigma2 = sigma2;
    double dmax = 0;
    for (int a = 0; a < 6; a++) dmax = fmax(dmax, fabs(sh.A[a * 7]));
    double L[6][6], inv[6];
    if (!(dmax > 0) || !chol6_factor(sh.A, dmax, L, inv)) { o.state = SVO_COV_RANK_DEFICIENT; return; }    // chol6's own pivot rule (NaN fails it too)
#pragma unroll 1
    for (int k = 0; k < 6; k++) {                                            // column k of A^-1
        double g[6], x[6];
#pragma unroll
        for (int i = 0; i < 6; i++) g[i] = i == k ? 1.0 : 0.0;
        chol6_solve(L, inv, g, x);
#pragma unroll
        for (int i = 0; i < 6; i++) sh.M[i * 6 + k] = x[i];
    }
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) {
        const double v = sigma2 * sh.M[a * 6 + b];
        sh.C[a * 6 + b] = v; sh.C[b * 6 + a] = v; o.cov_delta[a * 6 + b] = v; o.cov_delta[b * 6 + a] = v;
    }
    // G = d outPose / d delta (rows x y z yaw pitch roll, columns w1 w2 w3 t1 t2 t3) with M = R^T the pose's rotation:
    // xyz = -R^T t;  yaw = atan2(M10, M00), pitch = atan2(-M20, hypot(M00, M10)), roll = atan2(M21, M22)  (delta_to_pose)
    cov_rotation_derivs(sh.delta, sh.Rm, sh.dR);
    const double m00 = sh.Rm[0], m10 = sh.Rm[1], m20 = sh.Rm[2], m21 = sh.Rm[5], m22 = sh.Rm[8];
    const double c2 = m00 * m00 + m10 * m10;                                 // cos^2(pitch)
    if (c2 < 1e-12) { o.state = SVO_COV_DELTA_ONLY; return; }                // yaw and roll are not separable there: G is singular
    const double hy = sqrt(c2), r2 = m21 * m21 + m22 * m22, n2 = m20 * m20 + c2;
    for (int i = 0; i < 36; i++) sh.G[i] = 0;
    for (int k = 0; k < 3; k++) {
        const double* d = sh.dR + 9 * k;
        for (int i = 0; i < 3; i++) {
            sh.G[i * 6 + k] = -(d[0 * 3 + i] * sh.delta[3] + d[1 * 3 + i] * sh.delta[4] + d[2 * 3 + i] * sh.delta[5]);
            sh.G[i * 6 + 3 + k] = -sh.Rm[k * 3 + i];
        }
        const double d00 = d[0], d10 = d[1], d20 = d[2], d21 = d[5], d22 = d[8];
        sh.G[3 * 6 + k] = (m00 * d10 - m10 * d00) / c2;
        sh.G[4 * 6 + k] = (-hy * d20 + m20 * (m00 * d00 + m10 * d10) / hy) / n2;
        sh.G[5 * 6 + k] = (m22 * d21 - m21 * d22) / r2;
    }
    for (int a = 0; a < 6; a++) for (int b = 0; b < 6; b++) {
        double v = 0;
        for (int k = 0; k < 6; k++) v += sh.G[a * 6 + k] * sh.C[k * 6 + b];
        sh.M[a * 6 + b] = v;                                                 // G C
    }
    for (int a = 0; a < 6; a++) for (int b = a; b < 6; b++) {
        double v = 0;
        for (int k = 0; k < 6; k++) v += sh.M[a * 6 + k] * sh.G[b * 6 + k];
        o.cov_pose[a * 6 + b] = v; o.cov_pose[b * 6 + a] = v;
    }
    o.state = SVO_COV_OK;
}

void launch_pose_covariance(const DevCtx& c, const Knobs& k, const GNParams& P, svo_pose_cov* out, bool consume, hipStream_t st)
{
    gn_for_threads(k.gn_nt, [&](auto n) { constexpr int NT = decltype(n)::value; hipLaunchKernelGGL(k_pose_covariance<NT>, dim3(c.n_lanes), dim3(NT), 0, st, c, P, out, consume ? 1 : 0); });
}

// ------------------------------------------------------------------------------------------------------------
// The landmarks of a frame (svo_set_landmarks, contract at svo_landmark in svo_types.h): no reference counterpart -- the reference
// triangulates them (S5:529-544) and keeps them to itself.  One record per tracked pairing in stage 5's order: the point in the
// previous and in the current left camera's frame, each with its covariance, the residual of the one more evaluation at the
// returned delta (the evaluation of svo_pose_cov, through gn_point), the indices and the match ID.
// Launched behind k_gauss_newton, and behind k_pose_covariance when that runs (its cov_delta enters cov_cur).  One thread per
// pairing, a grid of (max_kps / 256, n_lanes) blocks of which those past a lane's T leave at once.  The kernel gathers from the
// lists itself and does not read gn_obs / gn_lmk: k_gauss_newton returns before its gather on a lane with bad tracking, which
// would leave them stale, and it triangulates only what its mask holds.  The final mask is k_gauss_newton's GnMaskRecord.
// The lane's counts are summed over its blocks through three words of LmkArgs::cnt (zero between launches); the block that takes
// the last ticket writes svo_landmarks_info, clears the words and consumes the mask record.
// ------------------------------------------------------------------------------------------------------------
#define LMK_NT 256
// Static LDS of k_landmarks: ONE description.  The records of the block are staged here (a thread's 176-byte record would leave its
// registers as stride-176 stores) and leave as contiguous 16-byte stores; delta, both rotations and cov_delta are read once per block.
struct LmkShared {
    svo_landmark stage[LMK_NT];   // 44 KB
    double delta[6];
    Rot R;                        // rodrigues_with_derivs: what gn_point evaluates with
    double Rm[9], dR[27];         // cov_rotation_derivs: the exact rotation, for xyz_cur, cov_cur and D
    double C[36];                 // cov_delta of the lane's svo_pose_cov (read only under pose_term)
    int ended_valid, pose_term, n_finite, n_inliers;
};
static_assert(sizeof(svo_landmark) % 16 == 0 && offsetof(LmkShared, stage) == 0, "the staged records leave as uint4");
static_assert(sizeof(LmkShared) == LMK_NT * 176 + 8 * (6 + 9 + 27 + 36) + sizeof(Rot) + 16 && sizeof(LmkShared) <= 64 * 1024, "k_landmarks LDS: 45 056 + 624 + 296 + 16");

__global__ void __launch_bounds__(LMK_NT) k_landmarks(DevCtx c, GNParams P, LmkArgs A)
{
    SVO_TL_SCOPE(c, TL_GN, 2);
    SVO_LATENCY_CHAIN(c);
    __shared__ __attribute__((aligned(16))) LmkShared sh;
    const int lane_id = blockIdx.y, tid = threadIdx.x, first = blockIdx.x * LMK_NT;
    if (lane_idle(c, lane_id)) return;                                       // an idle lane keeps its records and its info
    const LaneState& ls = c.lane[lane_id];
    const int has_prev = ls.has_prev;
    // tracked pairs of all octaves, concatenated octave by octave and cut at pmax, as k_gauss_newton does (S5:419-461)
    const int cur = 1 - ls.prev_slot, prev = ls.prev_slot;
    int toff[SVO_MAX_OCTAVES + 1];
    toff[0] = 0;
    for (int o = 0; o < SVO_MAX_OCTAVES; o++) toff[o + 1] = toff[o] + (o < c.n_oct ? c.n_tracked[lane_id * c.oct_cap + o] : 0);
    int T = has_prev ? toff[SVO_MAX_OCTAVES] : 0;
    const int cap = P.pmax < c.max_kps ? P.pmax : c.max_kps;                 // (the record array holds max_kps per lane)
    if (T > cap) T = cap;
    if (first >= T && blockIdx.x != 0) return;                               // block 0 stays: it writes the lane's info when T = 0
    const int nblk = T > 0 ? (T + LMK_NT - 1) / LMK_NT : 1;                  // the blocks of this lane that take a ticket
    uint8_t* mo = P.mask_out + (size_t)lane_id * GnMaskRecord{P.pmax}.bytes();
    if (tid == 0) {
        const int ev = has_prev && ((const int*)mo)[0] != 0 && ((const int*)mo)[1] == T;
        sh.ended_valid = ev; sh.n_finite = 0; sh.n_inliers = 0;
        int pt = 0;
        if (ev) {
            double d6[6];
            for (int k = 0; k < 6; k++) { d6[k] = c.results[lane_id].delta[k]; sh.delta[k] = d6[k]; }
            rodrigues_with_derivs(d6, sh.R);
            cov_rotation_derivs(sh.delta, sh.Rm, sh.dR);
            if (A.cov) { const int st = A.cov[lane_id].state; pt = st == SVO_COV_OK || st == SVO_COV_DELTA_ONLY; }
        }
        sh.pose_term = pt;
    }
    if (A.cov && tid >= 64 && tid < 64 + 36) sh.C[tid - 64] = A.cov[lane_id].cov_delta[tid - 64];
    __syncthreads();
    const int ev = sh.ended_valid, pose_term = sh.pose_term;
    const int i = first + tid;
    bool fin = false, inl = false;
    if (i < T) {
        int o = 0;
        for (int q = 1; q < SVO_MAX_OCTAVES; q++) if (i >= toff[q] && q < c.n_oct) o = q;
        const int vl = lane_id * c.oct_cap + o;
        const svo_index_pair tp = c.tracked[(long long)vl * c.max_kps + (i - toff[o])];
        const svo_dmatch a = c.matches[match_base(c, vl, prev) + tp.first], b = c.matches[match_base(c, vl, cur) + tp.second];
        const svo_keypoint l1 = c.kps[feat_base(c, vl, prev, 0) + a.queryIdx], r1 = c.kps[feat_base(c, vl, prev, 1) + a.trainIdx];
        const svo_keypoint l2 = c.kps[feat_base(c, vl, cur, 0) + b.queryIdx], r2 = c.kps[feat_base(c, vl, cur, 1) + b.trainIdx];
        const float sn = (float)(size_t)(c.n_oct > 1 ? (1 << o) : 1);            // scale_norm, S5:422 (applied only when nOctaves > 1)
        float ob[8];
        if (c.n_oct > 1) { ob[0] = l1.x * sn; ob[1] = l1.y * sn; ob[2] = r1.x * sn; ob[3] = r1.y * sn; ob[4] = l2.x * sn; ob[5] = l2.y * sn; ob[6] = r2.x * sn; ob[7] = r2.y * sn; }
        else { ob[0] = l1.x; ob[1] = l1.y; ob[2] = r1.x; ob[3] = r1.y; ob[4] = l2.x; ob[5] = l2.y; ob[6] = r2.x; ob[7] = r2.y; }
        const svo_stereo_camera cam = c.cams[lane_id];
        const double fl = cam.l_fx, fr = cam.r_fx;
        svo_landmark rec;
        double X[3];
        const double den = gn_triangulate(cam.baseline, fl, fr, cam.l_cx, cam.l_cy, cam.r_cx, (double)ob[0], (double)ob[1], (double)ob[2], X);
        // J = d(X, Y, Z) / d(ul, vl, ur): d den / d ul = fr, d den / d ur = -fl, and every coordinate is (a numerator) / den
        const double id = 1.0 / den, bf = (cam.baseline / den) * fr, kl = fr * id, kr = fl * id;
        const double J[3][3] = { { bf - X[0] * kl, 0.0, X[0] * kr }, { -X[1] * kl, bf, X[1] * kr }, { -X[2] * kl, 0.0, X[2] * kr } };
        double Cp[3][3];
        {
            int h = 0;
            for (int r = 0; r < 3; r++) for (int s = r; s < 3; s++) {
                const double v = A.var_px * (J[r][0] * J[s][0] + J[r][1] * J[s][1] + J[r][2] * J[s][2]);
                Cp[r][s] = v; Cp[s][r] = v; rec.cov_prev[h++] = v;
            }
        }
        fin = den != 0.0;
        for (int k = 0; k < 3; k++) { rec.xyz_prev[k] = X[k]; fin = fin && isfinite(X[k]); }
        for (int k = 0; k < 6; k++) fin = fin && isfinite(rec.cov_prev[k]);
        unsigned flags = fin ? SVO_LMK_FINITE : 0u;
        for (int k = 0; k < 3; k++) rec.xyz_cur[k] = 0.0;
        for (int k = 0; k < 6; k++) rec.cov_cur[k] = 0.0;
        rec.residual = 0.0;
        if (ev) {
            inl = mo[GnMaskRecord::HEAD + i] != 0;
            if (inl) {
                flags |= SVO_LMK_INLIER;
                double Jp[4][6], ri[4];
                if (gn_point(cam, sh.R, sh.R.small_angle != 0, sh.delta[3], sh.delta[4], sh.delta[5], X, ob, 0, Jp, ri)) {
                    flags |= SVO_LMK_USED;
                    rec.residual = ri[0] * ri[0] + ri[1] * ri[1] + ri[2] * ri[2] + ri[3] * ri[3];
                }
            }
            if (fin) {
                flags |= SVO_LMK_POSE | (pose_term ? SVO_LMK_POSE_TERM : 0u);
                const double* R = sh.Rm;
                for (int r = 0; r < 3; r++) rec.xyz_cur[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2] + sh.delta[3 + r];
                double M[3][3];                                                  // R cov_prev
                for (int r = 0; r < 3; r++) for (int s = 0; s < 3; s++) M[r][s] = R[3 * r] * Cp[0][s] + R[3 * r + 1] * Cp[1][s] + R[3 * r + 2] * Cp[2][s];
                double Dm[3][6], E[3][6];                                        // D = [d(R X)/dw | I3], E = D cov_delta
                if (pose_term) {
                    for (int k = 0; k < 3; k++) {
                        const double* d = sh.dR + 9 * k;
                        for (int r = 0; r < 3; r++) { Dm[r][k] = d[3 * r] * X[0] + d[3 * r + 1] * X[1] + d[3 * r + 2] * X[2]; Dm[r][3 + k] = r == k ? 1.0 : 0.0; }
                    }
                    for (int r = 0; r < 3; r++) for (int s = 0; s < 6; s++) {
                        double v = 0;
                        for (int k = 0; k < 6; k++) v += Dm[r][k] * sh.C[k * 6 + s];
                        E[r][s] = v;
                    }
                }
                int h = 0;
                for (int r = 0; r < 3; r++) for (int s = r; s < 3; s++) {
                    double v = M[r][0] * R[3 * s] + M[r][1] * R[3 * s + 1] + M[r][2] * R[3 * s + 2];
                    if (pose_term) { double e = 0; for (int k = 0; k < 6; k++) e += E[r][k] * Dm[s][k]; v += e; }
                    rec.cov_cur[h++] = v;
                }
            }
        }
        if (!fin) {                                                              // every double of the record is 0
            for (int k = 0; k < 3; k++) rec.xyz_prev[k] = 0.0;
            for (int k = 0; k < 6; k++) rec.cov_prev[k] = 0.0;
            rec.residual = 0.0;
        }
        const int n_ids = A.ids_on ? c.n_ids[vl * 2 + cur] : 0;
        rec.match_id = tp.second >= 0 && tp.second < n_ids ? c.ids[((long long)vl * 2 + cur) * c.max_kps + tp.second] : -1;
        rec.prev_match = tp.first; rec.cur_match = tp.second; rec.octave = o; rec.flags = flags; rec.reserved = 0;
        sh.stage[tid] = rec;
    }
    {
        const unsigned long long bfin = __ballot(fin), binl = __ballot(inl);
        if ((tid & 63) == 0) { atomicAdd(&sh.n_finite, (int)__popcll(bfin)); atomicAdd(&sh.n_inliers, (int)__popcll(binl)); }
    }
    __syncthreads();
    {   // the block's records, contiguous in the lane's array: 16 bytes per thread and pass
        const int nrec = T - first < LMK_NT ? (T - first > 0 ? T - first : 0) : LMK_NT;
        const uint4* src = (const uint4*)sh.stage;
        uint4* dst = (uint4*)(A.rec + (size_t)lane_id * c.max_kps + first);
        for (int q = tid; q < nrec * (int)(sizeof(svo_landmark) / 16); q += LMK_NT) dst[q] = src[q];
    }
    if (tid == 0) {
        int* cn = A.cnt + 4 * lane_id;
        if (sh.n_finite) atomicAdd(cn, sh.n_finite);
        if (sh.n_inliers) atomicAdd(cn + 1, sh.n_inliers);
        __threadfence();
        if (atomicAdd(cn + 2, 1) == nblk - 1) {                                  // the lane's last block
            svo_landmarks_info& info = A.info[lane_id];
            info.n = T; info.n_finite = atomicExch(cn, 0); info.n_inliers = atomicExch(cn + 1, 0);
            info.state = !has_prev ? SVO_LMK_NONE : (ev ? SVO_LMK_OK : SVO_LMK_POINTS_ONLY);
            info.std_noise_pixels = A.std_px; info.reserved[0] = 0; info.reserved[1] = 0;
            atomicExch(cn + 2, 0);
            ((int*)mo)[0] = 0;                                                   // consumed (see GnMaskRecord)
        }
    }
}

void launch_landmarks(const DevCtx& c, const GNParams& P, const LmkArgs& A, hipStream_t st)
{
    hipLaunchKernelGGL(k_landmarks, dim3((c.max_kps + LMK_NT - 1) / LMK_NT, c.n_lanes), dim3(LMK_NT), 0, st, c, P, A);
}

// ------------------------------------------------------------------------------------------------------------
// getProjectedCoords (common.cpp:415-466): landmarks of the untracked previous pairings triangulated as in stage 5
// (C:436-455) and projected after the change in pose through m_pinhole_stereo_projection (C:464, S5:180-195).
// One thread per point; same expressions, in the same order, as oracle/svo_oracle.c (svo_oracle_projected_coords).
// ------------------------------------------------------------------------------------------------------------
struct Delta6 { double v[6]; };

// One point: triangulated from (ul, vl, ur) as stage 5 does, moved by the rotation r (row-major 3 x 3) and the translation t, projected
// into both cameras.  One IEEE operation per operator, in this order: k_project_points and k_klt_predict both evaluate exactly this.
// Returns the disparity and the moved depth with the four pixels (uL vL uR vR)
struct MovedPoint { double disparity, Z1c; float pix[4]; };
__device__ __forceinline__ MovedPoint triangulate_move_project(double ul, double vl, double ur, const svo_stereo_camera& cam, const double* r, const double* t)
{
    MovedPoint m;
    const double cul = cam.l_cx, cvl = cam.l_cy, fl = cam.l_fx, cur = cam.r_cx, fr = cam.r_fx;
    const double disparity = fl * (cur - ur) + fr * (ul - cul);
    const double b_d = cam.baseline / disparity;
    const double X1p = b_d * fr * (ul - cul), Y1p = b_d * fr * (vl - cvl), Z1p = b_d * fl * fr;
    const double X1c = r[0] * X1p + r[1] * Y1p + r[2] * Z1p + t[0];
    const double Y1c = r[3] * X1p + r[4] * Y1p + r[5] * Z1p + t[1];
    const double Z1c = r[6] * X1p + r[7] * Y1p + r[8] * Z1p + t[2];
    const double X2c = X1c - cam.baseline;
    m.disparity = disparity; m.Z1c = Z1c;
    m.pix[0] = (float)(cam.l_fx * X1c / Z1c + cam.l_cx);
    m.pix[1] = (float)(cam.l_fy * Y1c / Z1c + cam.l_cy);
    m.pix[2] = (float)(cam.r_fx * X2c / Z1c + cam.r_cx);
    m.pix[3] = (float)(cam.r_fy * Y1c / Z1c + cam.r_cy);
    return m;
}

__global__ void __launch_bounds__(256) k_project_points(const float* uvu, int n, svo_stereo_camera cam, Delta6 dp, float* pix)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rot R; rodrigues_with_derivs<false>(dp.v, R);
    const double ul = (double)uvu[3 * i], vl = (double)uvu[3 * i + 1], ur = (double)uvu[3 * i + 2];
    const MovedPoint m = triangulate_move_project(ul, vl, ur, cam, R.r, dp.v + 3);
    pix[4 * i + 0] = m.pix[0];
    pix[4 * i + 1] = m.pix[1];
    pix[4 * i + 2] = m.pix[2];
    pix[4 * i + 3] = m.pix[3];
}

void launch_project_points(const float* uvu, int n, const svo_stereo_camera& cam, const double* delta6, float* pix, hipStream_t st)
{
    Delta6 d; for (int k = 0; k < 6; k++) d.v[k] = delta6[k];
    if (n > 0) hipLaunchKernelGGL(k_project_points, dim3((n + 255) / 256), dim3(256), 0, st, uvu, n, cam, d, pix);
}

// ------------------------------------------------------------------------------------------------------------
// svo_klt_set_prediction(1): the first guesses of a step of the resident KLT front end (svo_hip.h; the walk: tests/klt_predict_ref.py).
// Grid (ceil(cap / 256), n_lanes), one thread per slot.  Thread 0 of a block decides whether the lane predicts -- it is one of
// `tracks`, its record is valid, its six delta values are finite -- and builds the lane's rotation ONCE into LDS (section 7 of DESIGN.md:
// what a rotation per thread cost k_landmarks); behind the barrier every thread triangulates its slot from the live half, moves it and
// projects it with the expressions of k_project_points.  A slot whose guess cannot be used, and every slot of a lane that does not
// predict, starts at its own points; the slots behind the live count get NaN.  Reads: the live half, the lane's count, its record and
// camera.  Writes: the guesses and `used`, nothing else.
// ------------------------------------------------------------------------------------------------------------
// (the rotation is built in place in LDS: a Rot local to thread 0 leaves its two small-angle branches in scratch)
struct KltPredictLds { Rot R; double t[3]; int predicts; };
static __device__ __forceinline__ bool predict_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ void __launch_bounds__(256) k_klt_predict(const DevCtx c, const KltPredictArgs a)
{
    __shared__ KltPredictLds S;
    const int lane = a.only_lane >= 0 ? a.only_lane : (int)blockIdx.y;
    const int slot = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int cap = a.t.cap;
    if (threadIdx.x == 0) {
        int predicts = 0;
        if (lane_bit(a.tracks, lane)) {
            Delta6 d;
            int valid;
            if (a.forced) { valid = a.forced_valid; for (int k = 0; k < 6; k++) d.v[k] = a.forced_delta[k]; }
            else { const svo_result& res = c.results[lane]; valid = res.valid; for (int k = 0; k < 6; k++) d.v[k] = res.delta[k]; }
            bool finite = true;
            for (int k = 0; k < 6; k++) finite = finite && isfinite(d.v[k]);
            if (valid != 0 && finite) {
                rodrigues_with_derivs<false>(d.v, S.R);
                for (int k = 0; k < 3; k++) S.t[k] = d.v[3 + k];
                predicts = 1;
            }
        }
        S.predicts = predicts;
    }
    __syncthreads();
    if (slot >= cap) return;
    const float2* __restrict__ pts = a.t.pts[a.half] + (size_t)lane * 2 * cap;
    const int n = a.t.lane[lane].n, n_live = n < cap ? n : cap;
    float2 gl, gr;
    bool used = false;
    if (slot < n_live) {
        const float2 pl = pts[slot], pr = pts[cap + slot];
        gl = pl; gr = pr;
        if (S.predicts) {
            const svo_stereo_camera cam = c.cams[lane];
            double r[9], t[3];
            for (int k = 0; k < 9; k++) r[k] = S.R.r[k];
            for (int k = 0; k < 3; k++) t[k] = S.t[k];
            const MovedPoint m = triangulate_move_project((double)pl.x, (double)pl.y, (double)pr.x, cam, r, t);
            used = m.disparity > 0.0 && m.Z1c > 0.0
                && predict_finite(m.pix[0]) && predict_finite(m.pix[1]) && predict_finite(m.pix[2]) && predict_finite(m.pix[3])
                && m.pix[0] >= 0.0f && m.pix[0] <= a.x_max && m.pix[1] >= 0.0f && m.pix[1] <= a.y_max
                && m.pix[2] >= 0.0f && m.pix[2] <= a.x_max && m.pix[3] >= 0.0f && m.pix[3] <= a.y_max;
            if (used) { gl = make_float2(m.pix[0], m.pix[1]); gr = make_float2(m.pix[2], m.pix[3]); }
        }
    } else {
        const float nan = __uint_as_float(0x7fc00000u);
        gl = make_float2(nan, nan); gr = gl;
    }
    a.guess[(size_t)(2 * lane) * cap + slot] = gl;
    a.guess[(size_t)(2 * lane + 1) * cap + slot] = gr;
    a.used[(size_t)lane * cap + slot] = used ? 1 : 0;
}

void launch_klt_predict(const DevCtx& c, const KltPredictArgs& a, hipStream_t st)
{
    if (a.t.n_lanes <= 0 || a.t.cap <= 0) return;
    const dim3 grid((unsigned)((a.t.cap + 255) / 256), (unsigned)(a.only_lane >= 0 ? 1 : a.t.n_lanes));
    hipLaunchKernelGGL(k_klt_predict, grid, dim3(256), 0, st, c, a);
}
