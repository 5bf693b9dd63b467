// k_lk.hip -- svo_lk_track on the device: the pyramid (k_lk_pyrdown) and the pyramidal Lucas-Kanade tracker (k_lk_track); behind them
// the row tracker of svo_lk_track_rows (k_lk_track_row), a kernel of its own on the same helpers.
//
// The arithmetic is the walk of tests/lk_ref.py, operation for operation: integer pyramid, integer Scharr derivatives, bilinear samples
// with 14-bit weights, exact integer sums, and the double 2 x 2 solve in the walk's order (-ffp-contract=off: one IEEE operation per
// operator).  k_lk_track gives one wave to each (job, point): the iteration loop is wave-uniform, so no lane waits on another point's
// convergence.  A lane owns up to NP window pixels, whose template I, Ix, Iy stay in registers for the level; the derivatives are
// computed on the fly from a (win + 3)^2 byte tile of the previous image staged in the wave's LDS slice, and every iteration stages the
// (win + 1)^2 tile of the next image into the same slice.  No block barrier anywhere: the four waves of a block share nothing.
#include "svo_kernels.h"

#define LK_TILE_BYTES 1168                       // (31 + 3)^2 = 1156 bytes of the largest template tile, rounded up to 16

// ---- pyramid ----------------------------------------------------------------------------------------------------------------
// level `level` of both images of every job from level - 1: [1 4 6 4 1] on both axes, BORDER_REFLECT_101, (sum + 128) >> 8.  Integer only.
// blockIdx.z = 2 * job + image; a job whose pyramid ends above `level` and the blocks beyond its size leave at once.
__global__ __launch_bounds__(256) void k_lk_pyrdown(const LkJobDev* __restrict__ jobs, int level)
{
    const LkJobDev& J = jobs[blockIdx.z >> 1];
    const int s = blockIdx.z & 1;
    if (level >= J.nl) return;
    const int ow = J.w[level], oh = J.h[level];
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= ow || y >= oh) return;
    const int sw = J.w[level - 1], sh = J.h[level - 1], sp = J.pitch[s][level - 1];
    const uint8_t* __restrict__ src = J.img[s][level - 1];
    int xi[5], yo[5];
    for (int i = 0; i < 5; i++) {                                  // the reflected indices: never outside the source
        int v = 2 * x + i - 2; v = v < 0 ? -v : v; xi[i] = v >= sw ? 2 * sw - 2 - v : v;
        int u = 2 * y + i - 2; u = u < 0 ? -u : u; yo[i] = (u >= sh ? 2 * sh - 2 - u : u) * sp;
    }
    const int k[5] = { 1, 4, 6, 4, 1 };
    int sum = 0;
    for (int j = 0; j < 5; j++) {
        const uint8_t* r = src + yo[j];
        sum += k[j] * ((int)r[xi[0]] + 4 * (int)r[xi[1]] + 6 * (int)r[xi[2]] + 4 * (int)r[xi[3]] + (int)r[xi[4]]);
    }
    uint8_t* dst = const_cast<uint8_t*>(J.img[s][level]);          // levels above 0 lie in the context's own pyramid buffer
    dst[y * J.pitch[s][level] + x] = (uint8_t)((sum + 128) >> 8);
}

void launch_lk_pyrdown(const LkJobDev* jobs, int n_jobs, int level, int max_w, int max_h, hipStream_t st)
{
    if (n_jobs <= 0 || max_w <= 0 || max_h <= 0) return;
    hipLaunchKernelGGL(k_lk_pyrdown, dim3((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)(2 * n_jobs)), dim3(64, 4, 1), 0, st, jobs, level);
}

// ---- tracker ----------------------------------------------------------------------------------------------------------------
// what one wave wrote to its LDS slice becomes visible to its other lanes: the LDS serves a wave's accesses in order, this keeps the
// compiler from moving them across
static __device__ __forceinline__ void lk_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// the sum of a 32-bit value over the wave, in the VALU: an inclusive scan inside each row of 16 lanes (row_shr 1, 2, 4, 8; a lane without
// a source adds 0), then lane 15 of a row to the rows 1 and 3 and lane 31 to the rows 2 and 3 (row_bcast); lane 63 holds the total, and
// readlane hands it on as a scalar, so the branches on what follows stay scalar.  The caller keeps |v| * 64 inside 32 bits.
static __device__ __forceinline__ int lk_wave_sum32(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    return __builtin_amdgcn_readlane(v, 63);
}
// ... and of a per-lane partial sum of up to 32 bits in 64: its low 16 bits and its (signed) high part apart, each exact in 32 bits
static __device__ __forceinline__ long long lk_wave_sum(int v)
{
    const int lo = lk_wave_sum32(v & 0xffff), hi = lk_wave_sum32(v >> 16);
    return (long long)hi * 65536 + (long long)lo;
}
// ---- photometric compensation (svo_lk_set_photometric(ctx, 1); the walk: tests/lk_photo_ref.py) --------------------------------------
// The model J ~ (1 + a) I + b per window; a and b are eliminated from exact integer window sums.  n = win^2 <= 961; over the window
// |I|, |d| <= 8160 (a byte with 5 fractional bits), |Ix|, |Iy| <= 4080.  The centred moments times n are 64-bit scalar work behind the
// reductions: n * S and S * S stay below 961 * 961 * 8160^2 < 6.2e13 < 2^53, so the conversion to double is exact as well.
// n S_ab - S_a S_b
static __device__ __forceinline__ long long lk_centred(long long n, long long Sab, long long Sa, long long Sb) { return n * Sab - Sa * Sb; }
// (C - Ca Cb / CII) / n * 2^-20 in the walk's order: the product, the quotient, the difference, / n, * 2^-20 (one IEEE operation each)
static __device__ __forceinline__ double lk_reduce(long long C, double Ca, long long Cb, double CII, double n)
{
    return ((double)C - Ca * (double)Cb / CII) / n * 0x1p-20;
}
// a wave-uniform double into scalar registers: the values a level keeps for its iterations cost no vector register there
static __device__ __forceinline__ double lk_scalar(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}
static __device__ __forceinline__ bool lk_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// the window whose corner is the float position (px, py): its integer corner and the four 14-bit weights; false when it is not inside
// the w x h level (the float compares come first: they keep NaN and huge positions out of the conversion)
static __device__ __forceinline__ bool lk_window(float px, float py, int w, int h, int win, int& ix, int& iy, int& w00, int& w01, int& w10, int& w11)
{
    if (!(px >= 1.0f && py >= 1.0f && px < (float)w && py < (float)h)) return false;
    const float fx = floorf(px), fy = floorf(py);
    ix = (int)fx; iy = (int)fy;
    if (ix < 1 || iy < 1 || ix + win + 1 > w - 1 || iy + win + 1 > h - 1) return false;
    const float a = px - fx, b = py - fy;
    w00 = __float2int_rn(((1.0f - a) * (1.0f - b)) * 16384.0f);
    w01 = __float2int_rn((a * (1.0f - b)) * 16384.0f);
    w10 = __float2int_rn(((1.0f - a) * b) * 16384.0f);
    w11 = 16384 - w00 - w01 - w10;
    return true;
}
// T x T bytes of a level at (x0, y0) into the wave's slice; t / T by a multiplication that is exact for t < 2^11, T < 2^6
static __device__ __forceinline__ void lk_stage(uint8_t* tile, const uint8_t* __restrict__ img, int pitch, int x0, int y0, int T, int lane)
{
    const unsigned M = (65536u + (unsigned)T - 1u) / (unsigned)T;
    const uint8_t* __restrict__ p = img + (y0 * pitch + x0);
#pragma unroll 2
    for (int t = lane; t < T * T; t += 64) {
        const int ty = (int)(((unsigned)t * M) >> 16), tx = t - ty * T;
        tile[t] = p[ty * pitch + tx];
    }
    lk_wave_sync();
}
static __device__ __forceinline__ int lk_sample(const uint8_t* tile, int base, int T, int w00, int w01, int w10, int w11)
{
    return ((int)tile[base] * w00 + (int)tile[base + 1] * w01 + (int)tile[base + T] * w10 + (int)tile[base + T + 1] * w11 + 256) >> 9;
}

// NP: the window pixels a lane owns at most; BACK: the forward-backward pass (LkTrackArgs::backward); PHOTO: gain and bias removed per
// window (LkTrackArgs::photo).  PHOTO == false is the tracker of tests/lk_ref.py and compiles to what it was before the mode existed.
template <int NP, bool BACK, bool PHOTO = false>
__global__ __launch_bounds__(256) void k_lk_track(const LkTrackArgs A)
{
    __shared__ uint8_t tiles[4][LK_TILE_BYTES];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int gp = (int)blockIdx.x * 4 + wave;
    if (gp >= A.n_pts) return;
    uint8_t* tile = tiles[wave];
    // the job of this point: the last one that starts at or before it (an empty job shares its start with the next)
    int lo = 0, hi = A.n_jobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (A.jobs[mid].pt0 <= gp) lo = mid; else hi = mid - 1; }
    const LkJobDev& J = A.jobs[lo];
    const int sp = BACK ? 1 : 0, sn = 1 - sp;                // which image plays prev and which next
    if (BACK && !__builtin_amdgcn_readfirstlane((int)A.status[gp])) return;      // the forward pass lost it: no round trip
    const float2 pt = A.pts[gp];
    float g0x = pt.x, g0y = pt.y;
    if (!BACK && J.has_init) { const float2 t = A.aux[gp]; g0x = t.x; g0y = t.y; }
    if (!(lk_finite(pt.x) && lk_finite(pt.y) && lk_finite(g0x) && lk_finite(g0y))) {
        if (lane == 0) { A.out[gp] = make_float2(g0x, g0y); A.status[gp] = 0; A.err[gp] = 0.0f; }
        return;
    }
    const int win = A.p.win, nwin = win * win;
    const float half = (float)((win - 1) / 2);
    // The window pixels of this lane: index k * 64 + lane, row-major.  Two registers per pixel for the level:
    //   pk   bits 0-9 the pixel's offset y * (win + 1) + x in the next image's tile, 10-14 y, 15 set for a pixel of the window (clear for
    //        the indices behind it, which sit on pixel 0 and count for nothing), 16-28 the template I (<= 8160)
    //   gxy  Ix and Iy as two int16 (|.| <= 4080)
    int pk[NP], gxy[NP];
    {
        const unsigned M = (65536u + (unsigned)win - 1u) / (unsigned)win;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int idx = k * 64 + lane;
            const int y = (int)(((unsigned)idx * M) >> 16), x = idx - y * win;
            pk[k] = idx < nwin ? ((y * (win + 1) + x) | (y << 10) | 0x8000) : 0;
            gxy[k] = 0;
        }
    }
    const int top = J.nl - 1;
    float gx = g0x * __uint_as_float((unsigned)(127 - top) << 23), gy = g0y * __uint_as_float((unsigned)(127 - top) << 23);
    bool lost = false;
    float err = 0.0f;
#pragma unroll 1
    for (int L = top; L >= 0; --L) {
        const int w = J.w[L], h = J.h[L];
        const float sc = __uint_as_float((unsigned)(127 - L) << 23);            // 1 / 2^L
        int ix, iy, w00, w01, w10, w11;
        bool ok = lk_window(pt.x * sc - half, pt.y * sc - half, w, h, win, ix, iy, w00, w01, w10, w11);
        double A11 = 0.0, A12 = 0.0, A22 = 0.0, D = 0.0;
        // PHOTO: the level's plain sums and the centred moments an iteration needs again (scalars)
        int SI = 0, Sx = 0, Sy = 0;
        double CxI = 0.0, CyI = 0.0, CII = 1.0;
        if (ok) {
            // 1. template: I with 5 fractional bits, Ix and Iy from the Scharr derivatives at the four taps
            const int T = win + 3;
            lk_stage(tile, J.img[sp][L], J.pitch[sp][L], ix - 1, iy - 1, T, lane);
            int s11 = 0, s12 = 0, s22 = 0;
            // PHOTO, per lane over its NP <= 16 pixels: sum I <= 16 * 8160 < 2^17, |sum Ix| <= 16 * 4080 < 2^16 (their wave totals stay
            // inside 32 bits: one lk_wave_sum32 each); sum I I <= 16 * 8160^2 = 1 065 369 600 < 2^30; |sum Ix I| <= 16 * 4080 * 8160 < 2^29
            int sI = 0, sII = 0, sx = 0, sy = 0, sxI = 0, syI = 0;
#pragma unroll
            for (int k = 0; k < NP; k++) {
                const int q = pk[k] & 0xffff, m = (q << 16) >> 31;                          // m: all ones for a pixel of the window
                const int base = (q & 1023) + 2 * ((q >> 10) & 31) + win + 4;              // (y + 1) * T + x + 1
                int P[4][4];
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int c = 0; c < 4; c++) P[r][c] = (int)tile[base + (r - 1) * T + (c - 1)];
                int dx[2][2], dy[2][2];
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int c = 0; c < 2; c++) {
                        dx[r][c] = 3 * (P[r][c + 2] - P[r][c]) + 10 * (P[r + 1][c + 2] - P[r + 1][c]) + 3 * (P[r + 2][c + 2] - P[r + 2][c]);
                        dy[r][c] = 3 * (P[r + 2][c] - P[r][c]) + 10 * (P[r + 2][c + 1] - P[r][c + 1]) + 3 * (P[r + 2][c + 2] - P[r][c + 2]);
                    }
                const int I = (P[1][1] * w00 + P[1][2] * w01 + P[2][1] * w10 + P[2][2] * w11 + 256) >> 9;
                const int Ix = ((dx[0][0] * w00 + dx[0][1] * w01 + dx[1][0] * w10 + dx[1][1] * w11 + 8192) >> 14) & m;
                const int Iy = ((dy[0][0] * w00 + dy[0][1] * w01 + dy[1][0] * w10 + dy[1][1] * w11 + 8192) >> 14) & m;
                pk[k] = q | (I << 16); gxy[k] = (Ix & 0xffff) | (Iy << 16);
                s11 += Ix * Ix; s12 += Ix * Iy; s22 += Iy * Iy;
            }
            lk_wave_sync();                                        // every lane has read the tile before the iterations overwrite it
            // 2. gradient matrix
            if constexpr (PHOTO) {
                const long long n = nwin;
                const long long Sxx = lk_wave_sum(s11), Sxy = lk_wave_sum(s12), Syy = lk_wave_sum(s22);
                // the six sums with I in a pass of their own over the packed registers, behind the taps: the template pass is where the
                // kernel's registers peak.  Ix, Iy are masked already; I is not: an index behind the window sits on pixel 0
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    int q = pk[k], gq = gxy[k];
                    asm volatile("" : "+v"(q), "+v"(gq));
                    const int Im = (int)((unsigned)q >> 16) & ((q << 16) >> 31), Ix = (int)(short)(gq & 0xffff), Iy = gq >> 16;
                    sI += Im; sII += Im * Im; sx += Ix; sy += Iy; sxI += Ix * Im; syI += Iy * Im;
                }
                SI = lk_wave_sum32(sI); Sx = lk_wave_sum32(sx); Sy = lk_wave_sum32(sy);
                const long long SII = lk_wave_sum(sII), SxI = lk_wave_sum(sxI), SyI = lk_wave_sum(syI);
                const long long cII = lk_centred(n, SII, SI, SI), cxI = lk_centred(n, SxI, Sx, SI), cyI = lk_centred(n, SyI, Sy, SI);
                if (cII == 0) ok = false;                          // a flat template: nothing is divided by CII
                else {
                    CII = lk_scalar((double)cII); CxI = lk_scalar((double)cxI); CyI = lk_scalar((double)cyI);
                    A11 = lk_scalar(lk_reduce(lk_centred(n, Sxx, Sx, Sx), CxI, cxI, CII, (double)nwin));
                    A12 = lk_scalar(lk_reduce(lk_centred(n, Sxy, Sx, Sy), CxI, cyI, CII, (double)nwin));
                    A22 = lk_scalar(lk_reduce(lk_centred(n, Syy, Sy, Sy), CyI, cyI, CII, (double)nwin));
                }
            } else {
            A11 = (double)lk_wave_sum(s11) * 0x1p-20;
            A12 = (double)lk_wave_sum(s12) * 0x1p-20;
            A22 = (double)lk_wave_sum(s22) * 0x1p-20;
            }
            D = A11 * A22 - A12 * A12;
            if constexpr (PHOTO) D = lk_scalar(D);
            const double min_eig = (A22 + A11 - sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / (2.0 * win * win);
            if (min_eig < (double)A.p.min_eig || D < 0x1p-23) ok = false;        // PHOTO with a flat template: A = 0, D = 0, ok stays false
        }
        if (!ok) {                                                 // the level is skipped; at level 0 the point is lost
            if (L == 0) { lost = true; break; }
            gx = gx * 2.0f; gy = gy * 2.0f;
            continue;
        }
        // 3. iterations
        const uint8_t* __restrict__ nimg = J.img[sn][L];
        const int npitch = J.pitch[sn][L], T1 = win + 1;
        float pdx = 0.0f, pdy = 0.0f;
        bool outside = false;
        int jx, jy, v00, v01, v10, v11;
#pragma unroll 1
        for (int j = 0; j < A.p.max_iters; j++) {
            if (!lk_window(gx - half, gy - half, w, h, win, jx, jy, v00, v01, v10, v11)) { outside = true; break; }
            lk_stage(tile, nimg, npitch, jx, jy, T1, lane);
            int s1 = 0, s2 = 0;
            // PHOTO, per lane: |sum d| <= 16 * 8160 < 2^17 (one lk_wave_sum32); |sum d I| <= 16 * 8160^2 = 1 065 369 600 < 2^30.  d is
            // masked for both: the difference at an index behind the window is pixel 0's and counts for nothing
            int sd = 0, sdI = 0;
#pragma unroll
            for (int k = 0; k < NP; k++) {
                int q = pk[k], gq = gxy[k];
                asm volatile("" : "+v"(q), "+v"(gq));              // unpack here, every iteration: hoisted out of the loop the fields take four registers per pixel
                const int d = lk_sample(tile, q & 1023, T1, v00, v01, v10, v11) - (int)((unsigned)q >> 16);
                s1 += d * (int)(short)(gq & 0xffff); s2 += d * (gq >> 16);
                if constexpr (PHOTO) { const int dm = d & ((q << 16) >> 31); sd += dm; sdI += dm * (int)((unsigned)q >> 16); }
            }
            lk_wave_sync();
            double b1, b2;
            if constexpr (PHOTO) {
                // four independent reductions: their DPP chains interleave, no readlane waits on another sum's
                const long long n = nwin, Sd = lk_wave_sum32(sd), SdI = lk_wave_sum(sdI), Sdx = lk_wave_sum(s1), Sdy = lk_wave_sum(s2);
                const long long cdI = lk_centred(n, SdI, SI, Sd);
                b1 = lk_reduce(lk_centred(n, Sdx, Sx, Sd), CxI, cdI, CII, (double)nwin);
                b2 = lk_reduce(lk_centred(n, Sdy, Sy, Sd), CyI, cdI, CII, (double)nwin);
            } else { b1 = (double)lk_wave_sum(s1) * 0x1p-20; b2 = (double)lk_wave_sum(s2) * 0x1p-20; }
            const float dx = (float)((A12 * b2 - A22 * b1) / D), dy = (float)((A12 * b1 - A11 * b2) / D);
            gx = gx + dx; gy = gy + dy;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= (double)A.p.eps * (double)A.p.eps) break;
            if (j > 0 && fabs((double)(dx + pdx)) < 0.01 && fabs((double)(dy + pdy)) < 0.01) { gx = gx - 0.5f * dx; gy = gy - 0.5f * dy; break; }
            pdx = dx; pdy = dy;
        }
        if (L == 0) {
            if (outside) { lost = true; break; }
            // 4. error at the final position
            if (lk_window(gx - half, gy - half, w, h, win, jx, jy, v00, v01, v10, v11)) {
                lk_stage(tile, nimg, npitch, jx, jy, T1, lane);
                int s = 0;
                if constexpr (PHOTO) {
                    // the mean absolute centred difference: Sd first, then sum |n d - Sd| over the window.  |n d|, |Sd| <= 961 * 8160 < 2^23,
                    // so a term is below 2^24 and a lane's 16 below 2^28
                    int sd = 0;
#pragma unroll
                    for (int k = 0; k < NP; k++) {
                        const int q = pk[k], d = lk_sample(tile, q & 1023, T1, v00, v01, v10, v11) - (int)((unsigned)q >> 16);
                        sd += d & ((q << 16) >> 31);
                    }
                    const int Sd = lk_wave_sum32(sd);
#pragma unroll
                    for (int k = 0; k < NP; k++) {
                        int q = pk[k];
                        asm volatile("" : "+v"(q));                // sampled again, not kept from the pass above: NP registers less
                        const int d = lk_sample(tile, q & 1023, T1, v00, v01, v10, v11) - (int)((unsigned)q >> 16);
                        const int c = nwin * d - Sd;
                        s += (c < 0 ? -c : c) & ((q << 16) >> 31);
                    }
                    err = (float)((double)lk_wave_sum(s) / (double)(32 * nwin * nwin));
                } else {
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    const int q = pk[k], d = lk_sample(tile, q & 1023, T1, v00, v01, v10, v11) - (int)((unsigned)q >> 16);
                    s += (d < 0 ? -d : d) & ((q << 16) >> 31);
                }
                err = (float)((double)lk_wave_sum(s) / (double)(32 * nwin));
                }
            }
            break;
        }
        gx = gx * 2.0f; gy = gy * 2.0f;
    }
    if (lane != 0) return;
    if (!BACK) {
        A.out[gp] = make_float2(gx, gy); A.status[gp] = lost ? 0 : 1;
        A.err[gp] = lost ? 0.0f : err;
        return;
    }
    // the round trip: lost when this pass lost it or when it ends farther than fb_max from where the point started
    const float2 o = A.aux[gp];
    const double ddx = (double)gx - (double)o.x, ddy = (double)gy - (double)o.y;
    if (lost || ddx * ddx + ddy * ddy > (double)A.p.fb_max * (double)A.p.fb_max) A.status[gp] = 0;
}

// ---- row tracker (svo_lk_track_rows, step item 3b under svo_klt_set_stereo(1)) --------------------------------------------------
// The walk of tests/lk_row_ref.py: the template from prev at pt, the partner searched in next along the row of the guess.  One unknown, so
// a pixel keeps I and Ix (pk and gi), an iteration reduces one sum, and the update is one double division.  gy never moves inside a
// level: the win + 1 rows an iteration reads are the same in all of them, and only the window's column moves.  So the wave stages a
// STRIP of those rows once per level, S = min(LK_TILE_BYTES / (win + 1), win + 17, level width) columns wide with the first window in
// its middle, and stages again only when a window leaves it (the bytes a sample reads are the image's either way: no bit depends on S).
//
// `rows` rows of S bytes of a level at (x0, y0) into the wave's slice; t / S by a multiplication that is exact for t < 1168, S <= 48
static __device__ __forceinline__ void lk_stage_strip(uint8_t* tile, const uint8_t* __restrict__ img, int pitch, int x0, int y0, int S, int rows, int lane)
{
    const unsigned M = (65536u + (unsigned)S - 1u) / (unsigned)S;
    const uint8_t* __restrict__ p = img + (y0 * pitch + x0);
#pragma unroll 2
    for (int t = lane; t < S * rows; t += 64) {
        const int ty = (int)(((unsigned)t * M) >> 16), tx = t - ty * S;
        tile[t] = p[ty * pitch + tx];
    }
    lk_wave_sync();
}

// NP, BACK, PHOTO: as k_lk_track.  BACK compares along x alone.  A point index behind its job's count leaves at once: the records of a step
// (k_klt_jobs) give lane l the slots [2 l cap, 2 l cap + cap) and leave the cap slots behind them to nobody.
template <int NP, bool BACK, bool PHOTO = false>
__global__ __launch_bounds__(256) void k_lk_track_row(const LkTrackArgs A)
{
    __shared__ uint8_t tiles[4][LK_TILE_BYTES];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int gp = (int)blockIdx.x * 4 + wave;
    if (gp >= A.n_pts) return;
    uint8_t* tile = tiles[wave];
    int lo = 0, hi = A.n_jobs - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (A.jobs[mid].pt0 <= gp) lo = mid; else hi = mid - 1; }
    const LkJobDev& J = A.jobs[lo];
    if (gp - J.pt0 >= J.n) return;
    const int sp = BACK ? 1 : 0, sn = 1 - sp;
    if (BACK && !__builtin_amdgcn_readfirstlane((int)A.status[gp])) return;
    const float2 pt = A.pts[gp];
    float g0x = pt.x, g0y = pt.y;
    if (!BACK && J.has_init) { const float2 t = A.aux[gp]; g0x = t.x; g0y = t.y; }
    if (!(lk_finite(pt.x) && lk_finite(pt.y) && lk_finite(g0x) && lk_finite(g0y))) {
        if (lane == 0) { A.out[gp] = make_float2(g0x, g0y); A.status[gp] = 0; A.err[gp] = 0.0f; }
        return;
    }
    const int win = A.p.win, nwin = win * win;
    const float half = (float)((win - 1) / 2);
    // pk as in k_lk_track (offset y * (win + 1) + x, y, the window flag, I); gi: Ix
    int pk[NP], gi[NP];
    {
        const unsigned M = (65536u + (unsigned)win - 1u) / (unsigned)win;
#pragma unroll
        for (int k = 0; k < NP; k++) {
            const int idx = k * 64 + lane;
            const int y = (int)(((unsigned)idx * M) >> 16), x = idx - y * win;
            pk[k] = idx < nwin ? ((y * (win + 1) + x) | (y << 10) | 0x8000) : 0;
            gi[k] = 0;
        }
    }
    const int top = J.nl - 1;
    float gx = g0x * __uint_as_float((unsigned)(127 - top) << 23), gy = g0y * __uint_as_float((unsigned)(127 - top) << 23);
    bool lost = false;
    float err = 0.0f;
#pragma unroll 1
    for (int L = top; L >= 0; --L) {
        const int w = J.w[L], h = J.h[L];
        const float sc = __uint_as_float((unsigned)(127 - L) << 23);
        int ix, iy, w00, w01, w10, w11;
        bool ok = lk_window(pt.x * sc - half, pt.y * sc - half, w, h, win, ix, iy, w00, w01, w10, w11);
        double A11 = 0.0;
        int SI = 0, Sx = 0;                                        // PHOTO: as in k_lk_track, one unknown
        double CxI = 0.0, CII = 1.0;
        if (ok) {
            // 1. template: I and Ix
            const int T = win + 3;
            lk_stage(tile, J.img[sp][L], J.pitch[sp][L], ix - 1, iy - 1, T, lane);
            int s11 = 0;
            int sI = 0, sII = 0, sx = 0, sxI = 0;                  // PHOTO: the bounds of k_lk_track's sums hold
#pragma unroll
            for (int k = 0; k < NP; k++) {
                const int q = pk[k] & 0xffff, m = (q << 16) >> 31;
                const int base = (q & 1023) + 2 * ((q >> 10) & 31) + win + 4;
                int P[4][4];
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int c = 0; c < 4; c++) P[r][c] = (int)tile[base + (r - 1) * T + (c - 1)];
                int dx[2][2];
#pragma unroll
                for (int r = 0; r < 2; r++)
#pragma unroll
                    for (int c = 0; c < 2; c++)
                        dx[r][c] = 3 * (P[r][c + 2] - P[r][c]) + 10 * (P[r + 1][c + 2] - P[r + 1][c]) + 3 * (P[r + 2][c + 2] - P[r + 2][c]);
                const int I = (P[1][1] * w00 + P[1][2] * w01 + P[2][1] * w10 + P[2][2] * w11 + 256) >> 9;
                const int Ix = ((dx[0][0] * w00 + dx[0][1] * w01 + dx[1][0] * w10 + dx[1][1] * w11 + 8192) >> 14) & m;
                pk[k] = q | (I << 16); gi[k] = Ix;
                s11 += Ix * Ix;
                if constexpr (PHOTO) { const int Im = I & m; sI += Im; sII += Im * Im; sx += Ix; sxI += Ix * Im; }
            }
            lk_wave_sync();                                        // every lane has read the tile before the strip overwrites it
            // 2. the gradient sum
            if constexpr (PHOTO) {
                const long long n = nwin;
                SI = lk_wave_sum32(sI); Sx = lk_wave_sum32(sx);
                const long long SII = lk_wave_sum(sII), SxI = lk_wave_sum(sxI), Sxx = lk_wave_sum(s11);
                const long long cII = lk_centred(n, SII, SI, SI), cxI = lk_centred(n, SxI, Sx, SI);
                if (cII != 0) { CII = (double)cII; CxI = (double)cxI; A11 = lk_reduce(lk_centred(n, Sxx, Sx, Sx), CxI, cxI, CII, (double)nwin); }
                else ok = false;                                   // a flat template: A11 stays 0 and fails the test below as well
            } else
            A11 = (double)lk_wave_sum(s11) * 0x1p-20;
            if (A11 / (double)nwin < (double)A.p.min_eig || A11 < 0x1p-23) ok = false;
        }
        if (!ok) {
            if (L == 0) { lost = true; break; }
            gx = gx * 2.0f; gy = gy * 2.0f;
            continue;
        }
        // 3. iterations along the row
        const uint8_t* __restrict__ nimg = J.img[sn][L];
        const int npitch = J.pitch[sn][L], T1 = win + 1;
        int S = LK_TILE_BYTES / T1;
        S = S < win + 17 ? S : win + 17; S = S < w ? S : w;                   // T1 <= S <= 48: an inside window needs w >= win + 3
        const int dS = S - T1;
        int x0 = -1;                                                          // the strip's first column; -1: the slice holds no strip
        float pdx = 0.0f;
        bool outside = false;
        int jx, jy, v00, v01, v10, v11;
        // the strip covers the window at jx: columns x0 .. x0 + S - 1 inside 0 .. w - 1, rows jy .. jy + win inside the level (lk_window)
        auto cover = [&]() {
            if (x0 >= 0 && jx >= x0 && jx + T1 <= x0 + S) return;
            x0 = jx - (dS >> 1); x0 = x0 < w - S ? x0 : w - S; x0 = x0 > 0 ? x0 : 0;
            lk_stage_strip(tile, nimg, npitch, x0, jy, S, T1, lane);
        };
#pragma unroll 1
        for (int j = 0; j < A.p.max_iters; j++) {
            if (!lk_window(gx - half, gy - half, w, h, win, jx, jy, v00, v01, v10, v11)) { outside = true; break; }
            cover();
            const int off = jx - x0;
            int s1 = 0;
            int sd = 0, sdI = 0;                                   // PHOTO: masked, bounded as in k_lk_track
#pragma unroll
            for (int k = 0; k < NP; k++) {
                int q = pk[k], g = gi[k];
                asm volatile("" : "+v"(q), "+v"(g));               // unpack here, every iteration (as k_lk_track does)
                const int base = (q & 1023) + ((q >> 10) & 31) * dS + off;
                const int d = lk_sample(tile, base, S, v00, v01, v10, v11) - (int)((unsigned)q >> 16);
                s1 += d * g;
                if constexpr (PHOTO) { const int dm = d & ((q << 16) >> 31); sd += dm; sdI += dm * (int)((unsigned)q >> 16); }
            }
            lk_wave_sync();
            const long long Sdx = lk_wave_sum(s1);
            double b1;
            if constexpr (PHOTO) {
                const long long n = nwin, Sd = lk_wave_sum32(sd), SdI = lk_wave_sum(sdI);
                b1 = lk_reduce(lk_centred(n, Sdx, Sx, Sd), CxI, lk_centred(n, SdI, SI, Sd), CII, (double)nwin);
            } else b1 = (double)Sdx * 0x1p-20;
            const float dx = (float)(-b1 / A11);
            gx = gx + dx;
            if ((double)dx * (double)dx <= (double)A.p.eps * (double)A.p.eps) break;
            if (j > 0 && fabs((double)(dx + pdx)) < 0.01) { gx = gx - 0.5f * dx; break; }
            pdx = dx;
        }
        if (L == 0) {
            if (outside) { lost = true; break; }
            // 4. error at the final position
            if (lk_window(gx - half, gy - half, w, h, win, jx, jy, v00, v01, v10, v11)) {
                cover();
                const int off = jx - x0;
                int s = 0;
                if constexpr (PHOTO) {                             // as in k_lk_track: Sd, then sum |n d - Sd|
                    int sd = 0;
#pragma unroll
                    for (int k = 0; k < NP; k++) {
                        const int q = pk[k], base = (q & 1023) + ((q >> 10) & 31) * dS + off;
                        sd += (lk_sample(tile, base, S, v00, v01, v10, v11) - (int)((unsigned)q >> 16)) & ((q << 16) >> 31);
                    }
                    const int Sd = lk_wave_sum32(sd);
#pragma unroll
                    for (int k = 0; k < NP; k++) {
                        int q = pk[k];
                        asm volatile("" : "+v"(q));                // sampled again, not kept from the pass above
                        const int base = (q & 1023) + ((q >> 10) & 31) * dS + off;
                        const int c = nwin * (lk_sample(tile, base, S, v00, v01, v10, v11) - (int)((unsigned)q >> 16)) - Sd;
                        s += (c < 0 ? -c : c) & ((q << 16) >> 31);
                    }
                    err = (float)((double)lk_wave_sum(s) / (double)(32 * nwin * nwin));
                } else {
#pragma unroll
                for (int k = 0; k < NP; k++) {
                    const int q = pk[k], base = (q & 1023) + ((q >> 10) & 31) * dS + off;
                    const int d = lk_sample(tile, base, S, v00, v01, v10, v11) - (int)((unsigned)q >> 16);
                    s += (d < 0 ? -d : d) & ((q << 16) >> 31);
                }
                err = (float)((double)lk_wave_sum(s) / (double)(32 * nwin));
                }
            }
            break;
        }
        gx = gx * 2.0f; gy = gy * 2.0f;
    }
    if (lane != 0) return;
    if (!BACK) {
        A.out[gp] = make_float2(gx, gy); A.status[gp] = lost ? 0 : 1;
        A.err[gp] = lost ? 0.0f : err;
        return;
    }
    // the round trip along the row: lost when this pass lost it or when it ends farther than fb_max in x from where the point started
    const float2 o = A.aux[gp];
    const double ddx = (double)gx - (double)o.x;
    if (lost || ddx * ddx > (double)A.p.fb_max * (double)A.p.fb_max) A.status[gp] = 0;
}

void launch_lk_track_row(const LkTrackArgs& a, int pixels_per_lane, hipStream_t st)
{
    if (a.n_pts <= 0) return;
    const dim3 grid((unsigned)((a.n_pts + 3) / 4)), block(256);
    if (a.photo) {
        if (pixels_per_lane <= 2) { if (a.backward) hipLaunchKernelGGL((k_lk_track_row<2, true, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track_row<2, false, true>), grid, block, 0, st, a); }
        else if (pixels_per_lane <= 7) { if (a.backward) hipLaunchKernelGGL((k_lk_track_row<7, true, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track_row<7, false, true>), grid, block, 0, st, a); }
        else { if (a.backward) hipLaunchKernelGGL((k_lk_track_row<16, true, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track_row<16, false, true>), grid, block, 0, st, a); }
        return;
    }
    if (pixels_per_lane <= 2) { if (a.backward) hipLaunchKernelGGL((k_lk_track_row<2, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track_row<2, false>), grid, block, 0, st, a); }
    else if (pixels_per_lane <= 7) { if (a.backward) hipLaunchKernelGGL((k_lk_track_row<7, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track_row<7, false>), grid, block, 0, st, a); }
    else { if (a.backward) hipLaunchKernelGGL((k_lk_track_row<16, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track_row<16, false>), grid, block, 0, st, a); }
}

void launch_lk_track(const LkTrackArgs& a, int pixels_per_lane, hipStream_t st)
{
    if (a.n_pts <= 0) return;
    const dim3 grid((unsigned)((a.n_pts + 3) / 4)), block(256);
    if (a.photo) {
        if (pixels_per_lane <= 2) { if (a.backward) hipLaunchKernelGGL((k_lk_track<2, true, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track<2, false, true>), grid, block, 0, st, a); }
        else if (pixels_per_lane <= 7) { if (a.backward) hipLaunchKernelGGL((k_lk_track<7, true, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track<7, false, true>), grid, block, 0, st, a); }
        else { if (a.backward) hipLaunchKernelGGL((k_lk_track<16, true, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track<16, false, true>), grid, block, 0, st, a); }
        return;
    }
    if (pixels_per_lane <= 2) { if (a.backward) hipLaunchKernelGGL((k_lk_track<2, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track<2, false>), grid, block, 0, st, a); }
    else if (pixels_per_lane <= 7) { if (a.backward) hipLaunchKernelGGL((k_lk_track<7, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track<7, false>), grid, block, 0, st, a); }
    else { if (a.backward) hipLaunchKernelGGL((k_lk_track<16, true>), grid, block, 0, st, a); else hipLaunchKernelGGL((k_lk_track<16, false>), grid, block, 0, st, a); }
}
