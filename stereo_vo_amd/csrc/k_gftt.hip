// k_gftt.hip -- svo_gftt_detect on the device: the Shi-Tomasi response map (k_gftt_response), the candidates above the threshold that
// are 3 x 3 maxima (k_gftt_candidates), and per job the walk by descending response under the minimum-distance rule (k_gftt_select).
//
// The arithmetic is the walk of tests/gftt_ref.py, operation for operation: integer Sobel derivatives, integer block sums (the
// derivative maps read at reflect-101 positions), the smaller eigenvalue in double with one IEEE operation per operator
// (-ffp-contract=off, correctly rounded sqrt), float32 from there on.  A response is a non-negative float32, so its bit pattern orders as
// an unsigned integer: the maximum, the sort keys and the ties are integer work.
//
// Every loop of k_gftt_select has a bound that follows from the candidate count: the sort is a bitonic network over the next power of
// two, the cell lists are counting sorts, and the decision rounds end after at most as many rounds as there are candidates (each round
// decides at least the strongest undecided one).  No hash table, no spinning on another block.
#include "svo_kernels.h"
#include "gftt_call.hpp"

#define GFTT_TILE svo_gftt::GFTT_TILE            // k_gftt_response: 32 x 32 output pixels per block of 256 threads, 4 rows per thread
#define GFTT_SEL_THREADS 1024
#define GFTT_MAX_CELLS (svo_gftt::GFTT_MAX_CELLS_SIDE * svo_gftt::GFTT_MAX_CELLS_SIDE)     // gftt_call.hpp: at most 64 x 64 cells
#define GFTT_LDS_KEYS 4096                       // a job with at most this many (padded) keys sorts them in LDS

static __device__ __forceinline__ int gftt_reflect(int v, int n)
{
    v = v < 0 ? -v : v;
    v = v >= n ? 2 * n - 2 - v : v;
    return v < 0 ? 0 : (v >= n ? n - 1 : v);      // only positions no output pixel reads need the clamp (a tile far beyond a small image)
}

// ---- response ---------------------------------------------------------------------------------------------------------------
// The tile's pixels with a halo of R + 1 go to LDS at reflected indices; dx, dy of the tile with a halo of R follow as int16.  The walk
// reflects the derivative MAPS, not the image: the derivative of the reflected image behind a vertical border is -dx (dy unchanged),
// behind a horizontal one -dy, so those positions are negated.  Each thread then owns one column and four rows: it sums every row of
// its strip horizontally once and adds it to the outputs whose window holds that row.
template <int BLOCK>
__global__ __launch_bounds__(256) void k_gftt_response(GfttArgs A)
{
    constexpr int R = BLOCK / 2, H = R + 1, SW = GFTT_TILE + 2 * H, DW = GFTT_TILE + 2 * R, ROWS = 4 + 2 * R;
    __shared__ uint8_t s_img[SW * SW];
    __shared__ short s_dx[DW * DW], s_dy[DW * DW];
    __shared__ unsigned s_max;
    const GfttJobDev& J = A.jobs[blockIdx.z];
    const int w = J.w, h = J.h;
    const int x0 = blockIdx.x * GFTT_TILE, y0 = blockIdx.y * GFTT_TILE;
    if (x0 >= w || y0 >= h) return;
    const int tid = threadIdx.x;
    if (tid == 0) s_max = 0u;
    const uint8_t* __restrict__ img = J.img;
    for (int i = tid; i < SW * SW; i += 256) {
        const int ly = i / SW, lx = i - ly * SW;
        s_img[i] = img[(long long)gftt_reflect(y0 - H + ly, h) * J.pitch + gftt_reflect(x0 - H + lx, w)];
    }
    __syncthreads();
    for (int i = tid; i < DW * DW; i += 256) {
        const int ly = i / DW, lx = i - ly * DW;
        const uint8_t* p = s_img + ly * SW + lx;
        int dx = ((int)p[2] + 2 * (int)p[SW + 2] + (int)p[2 * SW + 2]) - ((int)p[0] + 2 * (int)p[SW] + (int)p[2 * SW]);
        int dy = ((int)p[2 * SW] + 2 * (int)p[2 * SW + 1] + (int)p[2 * SW + 2]) - ((int)p[0] + 2 * (int)p[1] + (int)p[2]);
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        if (gx < 0 || gx >= w) dx = -dx;
        if (gy < 0 || gy >= h) dy = -dy;
        s_dx[i] = (short)dx; s_dy[i] = (short)dy;
    }
    __syncthreads();
    const int tx = tid & 31, ty = tid >> 5;
    int a[4] = { 0, 0, 0, 0 }, b[4] = { 0, 0, 0, 0 }, c[4] = { 0, 0, 0, 0 };
#pragma unroll
    for (int rr = 0; rr < ROWS; rr++) {
        const int base = (ty * 4 + rr) * DW + tx;
        int ha = 0, hb = 0, hc = 0;
#pragma unroll
        for (int k = 0; k < BLOCK; k++) { const int gx = s_dx[base + k], gy = s_dy[base + k]; ha += gx * gx; hb += gx * gy; hc += gy * gy; }
#pragma unroll
        for (int i = 0; i < 4; i++) if (rr >= i && rr <= i + 2 * R) { a[i] += ha; b[i] += hb; c[i] += hc; }
    }
    unsigned best = 0u;
    const int gx = x0 + tx;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int gy = y0 + ty * 4 + i;
        if (gx >= w || gy >= h) continue;
        const long long s = (long long)a[i] + (long long)c[i], d = (long long)a[i] - (long long)c[i];
        const long long D = d * d + 4ll * (long long)b[i] * (long long)b[i];
        const double lam = 0.5 * ((double)s - sqrt((double)D));
        const float r = (float)(lam > 0.0 ? lam : 0.0);
        J.map[(long long)gy * w + gx] = r;
        const unsigned bits = __float_as_uint(r);
        best = bits > best ? bits : best;
    }
    if (best) atomicMax(&s_max, best);
    __syncthreads();
    if (tid == 0 && s_max) atomicMax((unsigned*)&A.info[4 * blockIdx.z + 3], s_max);
}

void launch_gftt_response(const GfttArgs& a, int max_w, int max_h, hipStream_t st)
{
    if (a.n_jobs <= 0 || max_w <= 0 || max_h <= 0) return;
    const dim3 grid((unsigned)((max_w + GFTT_TILE - 1) / GFTT_TILE), (unsigned)((max_h + GFTT_TILE - 1) / GFTT_TILE), (unsigned)a.n_jobs);
    if (a.p.block == 3) hipLaunchKernelGGL(k_gftt_response<3>, grid, dim3(256), 0, st, a);
    else if (a.p.block == 5) hipLaunchKernelGGL(k_gftt_response<5>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_gftt_response<7>, grid, dim3(256), 0, st, a);
}

// ---- candidates -------------------------------------------------------------------------------------------------------------
// One thread per pixel, 64 x 4 per block.  A candidate lies off the border ring, exceeds thr = float32(quality * m) and is not below any
// of its eight neighbours.  Each wave counts its candidates with one atomic and appends their keys behind that base while there is
// room; the count goes on beyond the capacity, so that it is the true one.  The order of the list is arbitrary: the keys are distinct
// and k_gftt_select sorts them.
__global__ __launch_bounds__(256) void k_gftt_candidates(GfttArgs A)
{
    const GfttJobDev& J = A.jobs[blockIdx.z];
    const int w = J.w, h = J.h;
    if ((int)(blockIdx.x * 64) >= w || (int)(blockIdx.y * 4) >= h) return;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    int* info = A.info + 4 * blockIdx.z;
    const float m = __uint_as_float((unsigned)info[3]);
    const float thr = __fmul_rn(A.p.quality, m);
    bool cand = false;
    float v = 0.0f;
    if (x >= 1 && x <= w - 2 && y >= 1 && y <= h - 2) {
        const float* __restrict__ r = J.map + (long long)y * w + x;
        v = r[0];
        if (v > thr) {
            cand = v >= r[-w - 1] && v >= r[-w] && v >= r[-w + 1] && v >= r[-1] && v >= r[1] && v >= r[w - 1] && v >= r[w] && v >= r[w + 1];
        }
    }
    const unsigned long long mask = __ballot(cand);                  // the 64 lanes of a wave are one row of the block
    if (!mask) return;
    const int lane = threadIdx.x;
    int base = 0;
    if (lane == __ffsll((long long)mask) - 1) base = atomicAdd(&info[1], __popcll(mask));
    base = __shfl(base, __ffsll((long long)mask) - 1);
    if (cand) {
        const int idx = base + __popcll(mask & ((1ull << lane) - 1ull));
        if (idx < A.cand_cap)
            A.keys[(size_t)blockIdx.z * (size_t)A.key_stride + (size_t)idx] =
                ((unsigned long long)__float_as_uint(v) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)(y * w + x));
    }
}

void launch_gftt_candidates(const GfttArgs& a, int max_w, int max_h, hipStream_t st)
{
    if (a.n_jobs <= 0 || max_w <= 0 || max_h <= 0) return;
    hipLaunchKernelGGL(k_gftt_candidates, dim3((unsigned)((max_w + 63) / 64), (unsigned)((max_h + 3) / 4), (unsigned)a.n_jobs), dim3(64, 4, 1), 0, st, a);
}

// ---- selection --------------------------------------------------------------------------------------------------------------
// exclusive prefix sum of one value per thread over the block of 1024; *total receives the sum.  Two barriers per step, ten steps.
static __device__ __forceinline__ int gftt_block_scan(int v, int* s_scan, int* total)
{
    const int tid = threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int off = 1; off < GFTT_SEL_THREADS; off <<= 1) {
        const int add = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const int incl = s_scan[tid];
    *total = s_scan[GFTT_SEL_THREADS - 1];
    __syncthreads();
    return incl - v;
}

// s_cell[c] = number of items in cell c on entry; on exit s_cell[c] = first index of cell c in the item list (the caller's scatter
// advances it to the cell's end, which is the next cell's start)
static __device__ __forceinline__ void gftt_cell_starts(int* s_cell, int ncell, int* s_scan)
{
    const int tid = threadIdx.x;
    int v[4], sum = 0;
    for (int k = 0; k < 4; k++) { const int c = 4 * tid + k; v[k] = c < ncell ? s_cell[c] : 0; sum += v[k]; }
    int total;
    int at = gftt_block_scan(sum, s_scan, &total);
    for (int k = 0; k < 4; k++) { const int c = 4 * tid + k; if (c < ncell) s_cell[c] = at; at += v[k]; }
    __syncthreads();
}

static __device__ __forceinline__ bool gftt_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One block per job.  state of a candidate (by rank): 0 undecided, 1 accepted, 2 rejected.  A state changes once, to the decision the
// sequential walk takes, so a thread that reads another's state in the round it is written still decides as the walk does.
__global__ __launch_bounds__(GFTT_SEL_THREADS) void k_gftt_select(GfttArgs A)
{
    __shared__ unsigned long long s_keys[GFTT_LDS_KEYS];
    __shared__ int s_cell[GFTT_MAX_CELLS];
    __shared__ int s_scan[GFTT_SEL_THREADS];
    const int job = blockIdx.x, tid = threadIdx.x;
    const GfttJobDev& J = A.jobs[job];
    int* info = A.info + 4 * job;
    const int n = info[1];
    if (n > A.cand_cap) { if (tid == 0) { info[0] = 0; info[2] = 1; } return; }
    if (n <= 0) { if (tid == 0) { info[0] = 0; info[2] = 0; } return; }
    const int w = J.w, h = J.h;
    int npad = 2;
    while (npad < n) npad <<= 1;                                      // <= key_stride
    unsigned long long* gk = A.keys + (size_t)job * (size_t)A.key_stride;
    unsigned long long* k = gk;
    if (npad <= GFTT_LDS_KEYS) {
        for (int i = tid; i < npad; i += GFTT_SEL_THREADS) s_keys[i] = i < n ? gk[i] : 0ull;
        k = s_keys;
    } else {
        for (int i = n + tid; i < npad; i += GFTT_SEL_THREADS) gk[i] = 0ull;
    }
    __syncthreads();
    // bitonic network, descending; a real key is never 0 (its response exceeds thr >= 0), so the padding sorts to the end
#pragma unroll 1
    for (int size = 2; size <= npad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < (npad >> 1); t += GFTT_SEL_THREADS) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const bool desc = (i & size) == 0;
                const unsigned long long u = k[i], v = k[j];
                if ((u < v) == desc) { k[i] = v; k[j] = u; }
            }
            __syncthreads();
        }
    }
    const int md = A.p.min_distance;
    const int cell = J.cell, gw = J.gw, gh = J.gh, ncell = gw * gh;
    uint8_t* state = A.state + (size_t)job * (size_t)A.cand_cap;
    // the job's scratch: (x, y, cell x, cell y) of every candidate by rank, the candidates by cell, the seeds by cell, every seed's cell
    int4* pos = (int4*)(A.items + (size_t)job * (size_t)A.items_stride);
    int* items = (int*)(pos + A.cand_cap);
    int* seed_items = items + A.cand_cap;
    int* seed_cell = seed_items + A.seed_cap;
    for (int i = tid; i < n; i += GFTT_SEL_THREADS) {
        const unsigned raster = 0xFFFFFFFFu - (unsigned)k[i];
        const int y = (int)(raster / (unsigned)w), x = (int)(raster - (unsigned)y * (unsigned)w);
        pos[i] = make_int4(x, y, x / cell, y / cell);
    }
    __syncthreads();
    if (md > 0) {
        // the seeds that count, by cell; then every candidate against the seeds of its 3 x 3 cells
        const float2* seeds = A.seeds + J.seed0;
        const float md2 = (float)(md * md), fw = (float)w, fh = (float)h;
        for (int c = tid; c < ncell; c += GFTT_SEL_THREADS) s_cell[c] = 0;
        __syncthreads();
        for (int s = tid; s < J.n_seeds; s += GFTT_SEL_THREADS) {
            const float2 q = seeds[s];
            int c = -1;
            if (gftt_finite(q.x) && gftt_finite(q.y) && q.x >= 0.0f && q.x < fw && q.y >= 0.0f && q.y < fh) {
                c = ((int)q.y / cell) * gw + (int)q.x / cell;
                atomicAdd(&s_cell[c], 1);
            }
            seed_cell[s] = c;
        }
        __syncthreads();
        gftt_cell_starts(s_cell, ncell, s_scan);
        for (int s = tid; s < J.n_seeds; s += GFTT_SEL_THREADS) {
            const int c = seed_cell[s];
            if (c >= 0) seed_items[atomicAdd(&s_cell[c], 1)] = s;
        }
        __syncthreads();
        for (int i = tid; i < n; i += GFTT_SEL_THREADS) {
            const int4 me = pos[i];
            const float fxc = (float)me.x, fyc = (float)me.y;
            const int xa = me.z > 0 ? me.z - 1 : 0, xb = me.z + 1 < gw ? me.z + 1 : gw - 1, yb = me.w + 1 < gh ? me.w + 1 : gh - 1;
            bool hit = false;
#pragma unroll 1
            for (int yy = (me.w > 0 ? me.w - 1 : 0); yy <= yb && !hit; yy++) {
                // the cells xa .. xb of a row are neighbours in the list: one run of seeds
                const int c0 = yy * gw + xa, c1 = yy * gw + xb;
                for (int e = (c0 ? s_cell[c0 - 1] : 0); e < s_cell[c1]; e++) {
                    const float2 q = seeds[seed_items[e]];
                    const float fx = fxc - q.x, fy = fyc - q.y;
                    if (__fadd_rn(__fmul_rn(fx, fx), __fmul_rn(fy, fy)) < md2) { hit = true; break; }
                }
            }
            state[i] = hit ? 2 : 0;
        }
        __syncthreads();
        // the candidates by cell
        for (int c = tid; c < ncell; c += GFTT_SEL_THREADS) s_cell[c] = 0;
        __syncthreads();
        for (int i = tid; i < n; i += GFTT_SEL_THREADS) { const int4 me = pos[i]; atomicAdd(&s_cell[me.w * gw + me.z], 1); }
        __syncthreads();
        gftt_cell_starts(s_cell, ncell, s_scan);
        for (int i = tid; i < n; i += GFTT_SEL_THREADS) { const int4 me = pos[i]; items[atomicAdd(&s_cell[me.w * gw + me.z], 1)] = i; }
        __syncthreads();
        // the rounds: an undecided candidate is rejected by an accepted stronger one within reach, accepted when no stronger one within
        // reach is undecided.  The strongest undecided candidate has no undecided stronger one, so every round decides it: <= n rounds.
        const int md2i = md * md;
#pragma unroll 1
        for (int round = 0; round < n; round++) {
            int open = 0;
            for (int i = tid; i < n; i += GFTT_SEL_THREADS) {
                if (__atomic_load_n(&state[i], __ATOMIC_RELAXED) != 0) continue;
                const int4 me = pos[i];
                const int xa = me.z > 0 ? me.z - 1 : 0, xb = me.z + 1 < gw ? me.z + 1 : gw - 1, yb = me.w + 1 < gh ? me.w + 1 : gh - 1;
                bool rejected = false, blocked = false;
#pragma unroll 1
                for (int yy = (me.w > 0 ? me.w - 1 : 0); yy <= yb && !rejected; yy++) {
                    const int c0 = yy * gw + xa, c1 = yy * gw + xb;
                    for (int e = (c0 ? s_cell[c0 - 1] : 0); e < s_cell[c1]; e++) {
                        const int j = items[e];
                        if (j >= i) continue;                         // only the stronger ones: they come first in the walk
                        const int4 o = pos[j];
                        if ((me.x - o.x) * (me.x - o.x) + (me.y - o.y) * (me.y - o.y) >= md2i) continue;
                        const uint8_t sj = __atomic_load_n(&state[j], __ATOMIC_RELAXED);
                        if (sj == 1) { rejected = true; break; }
                        if (sj == 0) blocked = true;
                    }
                }
                if (rejected) __atomic_store_n(&state[i], (uint8_t)2, __ATOMIC_RELAXED);
                else if (!blocked) __atomic_store_n(&state[i], (uint8_t)1, __ATOMIC_RELAXED);
                else open = 1;
            }
            if (!__syncthreads_or(open)) break;
        }
    }
    // the accepted ones in walk order, cut at the limit
    int limit = J.cap;
    if (A.p.max_corners > 0 && A.p.max_corners < limit) limit = A.p.max_corners;
    const int chunk = (n + GFTT_SEL_THREADS - 1) / GFTT_SEL_THREADS;
    const int i0 = tid * chunk < n ? tid * chunk : n, i1 = i0 + chunk < n ? i0 + chunk : n;
    int mine = 0;
    for (int i = i0; i < i1; i++) mine += (md > 0 ? state[i] == 1 : 1);
    int total;
    int at = gftt_block_scan(mine, s_scan, &total);
    for (int i = i0; i < i1 && at < limit; i++) {
        if (md > 0 && state[i] != 1) continue;
        const unsigned long long key = k[i];
        const int4 me = pos[i];
        A.pts[J.pts0 + at] = make_float2((float)me.x, (float)me.y);
        A.resp[J.pts0 + at] = __uint_as_float((unsigned)(key >> 32));
        at++;
    }
    if (tid == 0) { info[0] = total < limit ? total : limit; info[2] = 0; }
}

void launch_gftt_select(const GfttArgs& a, hipStream_t st)
{
    if (a.n_jobs <= 0) return;
    hipLaunchKernelGGL(k_gftt_select, dim3((unsigned)a.n_jobs), dim3(GFTT_SEL_THREADS), 0, st, a);
}
