// k_klt.hip -- the resident KLT front end on the device (svo_hip.h: svo_klt_step): the job records of a step (k_klt_jobs), the gate and
// stable compaction that turn the tracker's results into a lane's current-frame lists (k_klt_select), the append behind
// svo_klt_add_points (k_klt_append) and the table reset (k_klt_clear).  The tracker itself is k_lk.hip's, launched as it is.
// Behind them the top-up of svo_klt_topup: the detector's records decided on the device (k_klt_topup_jobs), the tracker's records and
// first guesses (k_klt_topup_prepare), the gate and the append (k_klt_topup_append), around k_gftt.hip's and k_lk.hip's kernels.
//
// k_klt_select is the walk of tests/klt_ref.py and leaves what svo_put_features_oct / svo_put_matches_oct / svo_put_match_ids_oct /
// svo_put_tracked_oct leave for the same lists (svo_api.hip), row tables included.
#include "svo_kernels.h"

#define KLT_BLOCK 256
#define KLT_WAVES (KLT_BLOCK / 64)

// LDS of k_klt_select.  Static: the counters and the per-wave words of a chunk.  Dynamic: three row tables of H + 1 ints --
//   hl, hr   keypoints of the left / right list per row (row_of clamped to 0 .. H), for pyr_feats_index
//   hq       pairings per row at which the sequential walk of svo_put_matches_oct passes them, for matches_lr_row_index
struct KltSelectLds {
    int wsurv[KLT_WAVES], wtrk[KLT_WAVES];   // survivors / tracked pairs of each wave in the chunk
    float wmax[KLT_WAVES];                   // the largest left y among each wave's survivors in the chunk
    int first_l, last_l, first_r, last_r;    // row_of of the first and last entry of the two keypoint lists
    int max_id;
    int scan[20];                            // block_exclusive_scan's words
};
size_t klt_select_lds_bytes(int H) { return 3 * ((size_t)H + 1) * sizeof(int); }

static __device__ __forceinline__ bool klt_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// (long long)y of svo_put_features_oct's row_of, saturated where it saturates
static __device__ __forceinline__ int klt_row_of(float y) { return y >= 0.0f ? (y < 1.0e9f ? (int)y : 1000000000) : (y > -1.0e9f ? (int)y : -1000000000); }
static __device__ __forceinline__ int klt_clamp(int r, int H) { return r < 0 ? 0 : (r > H ? H : r); }

// One block per lane.  The lane's cap slots are walked in chunks of 256 in slot order; a chunk's survivors get consecutive indices
// behind the running base (ballot + popcount inside a wave, the wave totals through LDS), so the compaction is stable.  Everything a
// survivor contributes is written in that pass: both keypoints, the pairing, its ID, its tracked pair (a second compaction over the
// survivors that have a previous index), its slot of the new table (the OTHER half: nothing is compacted in place), and its counts in
// the three row tables.  The tables are then scanned, and thread 0 writes the counts, the record fields and the lane words.
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_select(const DevCtx c, const KltSelectArgs a)
{
    extern __shared__ int klt_rows[];
    __shared__ KltSelectLds S;
    const int lane = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
    const int cap = a.t.cap;
    const float2* __restrict__ in_pts = a.t.pts[a.half] + (size_t)lane * 2 * cap;
    const int* __restrict__ in_meta = a.t.meta[a.half] + (size_t)lane * KLT_META * cap;
    float2* out_pts = a.t.pts[a.half ^ 1] + (size_t)lane * 2 * cap;
    int* out_meta = a.t.meta[a.half ^ 1] + (size_t)lane * KLT_META * cap;
    if (lane_idle(c, lane)) {                  // the lane sits the step out: its table moves to the other half as it is
        for (int i = tid; i < 2 * cap; i += KLT_BLOCK) out_pts[i] = in_pts[i];
        for (int i = tid; i < KLT_META * cap; i += KLT_BLOCK) out_meta[i] = in_meta[i];
        return;
    }
    const int H = a.H;
    int* hl = klt_rows, * hr = klt_rows + (H + 1), * hq = klt_rows + 2 * (H + 1);
    for (int i = tid; i < 3 * (H + 1); i += KLT_BLOCK) klt_rows[i] = 0;
    if (tid == 0) { S.first_l = S.last_l = S.first_r = S.last_r = 0; S.max_id = 0; }
    const LaneState ls = c.lane[lane];
    const KltLaneDev kl = a.t.lane[lane];
    const int cur = 1 - ls.prev_slot, vl = lane * c.oct_cap;
    const bool shifted = ls.prev_slot != kl.seen_slot;
    const bool fresh = lane_bit(a.fresh, lane);
    const int n_live = kl.n < cap ? kl.n : cap;
    svo_keypoint* kps_l = c.kps + feat_base(c, vl, cur, 0), * kps_r = c.kps + feat_base(c, vl, cur, 1);
    svo_dmatch* mm = c.matches + match_base(c, vl, cur);
    int* ids = c.ids + match_base(c, vl, cur);
    svo_index_pair* trk = c.tracked + (long long)vl * c.max_kps;
    const float2* __restrict__ res_l = a.t.out + (size_t)(2 * lane) * cap, * __restrict__ res_r = a.t.out + (size_t)(2 * lane + 1) * cap;
    const uint8_t* __restrict__ st_l = a.t.status + (size_t)(2 * lane) * cap, * __restrict__ st_r = a.t.status + (size_t)(2 * lane + 1) * cap;
    __syncthreads();
    int n_surv = 0, n_trk = 0;                 // the running bases: block-uniform
    float run_max = -INFINITY;                 // the largest left y of the survivors so far
    for (int base = 0; base < n_live; base += KLT_BLOCK) {
        const int slot = base + tid;
        const bool in = slot < n_live;
        float2 pl = make_float2(0.0f, 0.0f), pr = pl;
        int id = 0, age = 0, p = -1;
        bool ok = false;
        if (in) {
            if (fresh) { pl = in_pts[slot]; pr = in_pts[cap + slot]; ok = true; }
            else { pl = res_l[slot]; pr = res_r[slot]; ok = st_l[slot] == 1 && st_r[slot] == 1; }
            id = in_meta[KLT_ID * cap + slot]; age = in_meta[KLT_AGE * cap + slot];
            p = shifted ? in_meta[KLT_IDX * cap + slot] : in_meta[KLT_PIDX * cap + slot];
            const float disp = pl.x - pr.x;
            ok = ok && klt_finite(pl.x) && klt_finite(pl.y) && klt_finite(pr.x) && klt_finite(pr.y)
                    && fabsf(pl.y - pr.y) <= a.max_dy && disp >= a.min_disp && disp <= a.max_disp;
        }
        const bool has_p = ok && p >= 0;
        const unsigned long long bs = __ballot(ok), bt = __ballot(has_p), below = (1ull << wl) - 1ull;
        // the largest left y up to and including this slot, inside the wave
        float pm = ok ? pl.y : -INFINITY;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const float t = __shfl_up(pm, o, 64); if (wl >= o) pm = fmaxf(pm, t); }
        if (wl == 63) { S.wsurv[wave] = __popcll(bs); S.wtrk[wave] = __popcll(bt); S.wmax[wave] = pm; }
        __syncthreads();
        int i = n_surv + __popcll(bs & below), k = n_trk + __popcll(bt & below), tot_s = 0, tot_t = 0;
        float carry = run_max, chunk_max = run_max;
#pragma unroll
        for (int w = 0; w < KLT_WAVES; w++) {
            if (w < wave) { i += S.wsurv[w]; k += S.wtrk[w]; carry = fmaxf(carry, S.wmax[w]); }
            tot_s += S.wsurv[w]; tot_t += S.wtrk[w]; chunk_max = fmaxf(chunk_max, S.wmax[w]);
        }
        if (ok) {
            pm = fmaxf(pm, carry);
            svo_keypoint kp; kp.x = pl.x; kp.y = pl.y; kp.size = a.kp_size; kp.angle = -1.0f; kp.response = 0.0f; kp.octave = 0; kp.class_id = id;
            kps_l[i] = kp;
            kp.x = pr.x; kp.y = pr.y;
            kps_r[i] = kp;
            svo_dmatch m; m.queryIdx = i; m.trainIdx = i; m.imgIdx = 0; m.distance = 0.0f;
            mm[i] = m; ids[i] = id;
            if (has_p) { svo_index_pair t; t.first = p; t.second = i; trk[k] = t; }
            out_pts[i] = pl; out_pts[cap + i] = pr;
            out_meta[KLT_ID * cap + i] = id; out_meta[KLT_AGE * cap + i] = age + 1; out_meta[KLT_IDX * cap + i] = i; out_meta[KLT_PIDX * cap + i] = p;
            const int rl = klt_row_of(pl.y), rr = klt_row_of(pr.y);
            atomicAdd(&hl[klt_clamp(rl, H)], 1); atomicAdd(&hr[klt_clamp(rr, H)], 1);
            // the walk of svo_put_matches_oct passes pairing i at the first row y >= 0 with max(y_0 .. y_i) <= (float)y
            const int q = pm <= 0.0f ? 0 : (pm > (float)H ? H : (int)ceilf(pm));
            atomicAdd(&hq[q > H ? H : q], 1);
            atomicMax(&S.max_id, id);
            if (i == 0) { S.first_l = rl; S.first_r = rr; }
            if (i == n_surv + tot_s - 1) { S.last_l = rl; S.last_r = rr; }     // (the last survivor of a later chunk overwrites it)
        }
        n_surv += tot_s; n_trk += tot_t; run_max = chunk_max;
        __syncthreads();                       // the per-wave words are free for the next chunk
    }
    // the tail of the new table
    for (int i = n_surv + tid; i < cap; i += KLT_BLOCK) {
        out_pts[i] = make_float2(NAN, NAN); out_pts[cap + i] = make_float2(NAN, NAN);
        out_meta[KLT_ID * cap + i] = -1; out_meta[KLT_AGE * cap + i] = 0; out_meta[KLT_IDX * cap + i] = -1; out_meta[KLT_PIDX * cap + i] = -1;
    }
    __syncthreads();
    // pyr_feats_index of both lists: the keypoints up to and including row r for first_row <= r < last_row, 0 elsewhere;
    // matches_lr_row_index: the pairings passed before row r, and the count in entry H
    const int first_l = S.first_l, last_l = S.last_l, first_r = S.first_r, last_r = S.last_r;
    int* ri_l = c.row_index + (((long long)vl * 2 + cur) * 2 + 0) * c.max_h, * ri_r = c.row_index + (((long long)vl * 2 + cur) * 2 + 1) * c.max_h;
    int* ri_m = c.mrow_index + ((long long)vl * 2 + cur) * (c.max_h + 1);
    int acc_l = 0, acc_r = 0, acc_q = 0;
    for (int r0 = 0; r0 < H; r0 += KLT_BLOCK) {
        const int r = r0 + tid;
        const int vl_ = r < H ? hl[r] : 0, vr_ = r < H ? hr[r] : 0, vq_ = r < H ? hq[r] : 0;
        int tl, tr, tq;
        const int el = block_exclusive_scan(vl_, S.scan, &tl);
        const int er = block_exclusive_scan(vr_, S.scan, &tr);
        const int eq = block_exclusive_scan(vq_, S.scan, &tq);
        if (r < H) {
            ri_l[r] = (n_surv > 0 && r >= first_l && r < last_l) ? acc_l + el + vl_ : 0;
            ri_r[r] = (n_surv > 0 && r >= first_r && r < last_r) ? acc_r + er + vr_ : 0;
            ri_m[r] = acc_q + eq;
        }
        acc_l += tl; acc_r += tr; acc_q += tq;
    }
    if (tid == 0) {
        ri_m[H] = n_surv;
        c.n_kps[feat_cnt_idx(vl, cur, 0)] = n_surv; c.n_kps[feat_cnt_idx(vl, cur, 1)] = n_surv;
        c.n_matches[vl * 2 + cur] = n_surv; c.n_ids[vl * 2 + cur] = n_surv;
        c.n_tracked[vl] = n_trk;
        svo_result& r = c.results[lane];
        r.detected_left[0] = n_surv; r.detected_right[0] = n_surv; r.stereo_matches[0] = n_surv;
        LaneState& s = c.lane[lane];
        s.has_cur = 1; s.last_match_id = S.max_id;
        KltLaneDev& k = a.t.lane[lane];
        k.n = n_surv; k.seen_slot = ls.prev_slot;
    }
}

void launch_klt_select(const DevCtx& c, const KltSelectArgs& a, hipStream_t st)
{
    if (a.t.n_lanes <= 0) return;
    hipLaunchKernelGGL(k_klt_select, dim3((unsigned)a.t.n_lanes), dim3(KLT_BLOCK), klt_select_lds_bytes(a.H), st, c, a);
}

// appends up to n (left, right) pairs behind the live count of one lane: fresh IDs, age 0, no indices.  One block.
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_append(const KltDev t, int half, int lane, const float2* __restrict__ left, const float2* __restrict__ right, int n)
{
    const KltLaneDev kl = t.lane[lane];
    const int cap = t.cap, n0 = kl.n < cap ? (kl.n < 0 ? 0 : kl.n) : cap;
    const int m = n < cap - n0 ? n : cap - n0;
    float2* pts = t.pts[half] + (size_t)lane * 2 * cap;
    int* meta = t.meta[half] + (size_t)lane * KLT_META * cap;
    for (int i = threadIdx.x; i < m; i += KLT_BLOCK) {
        pts[n0 + i] = left[i]; pts[cap + n0 + i] = right[i];
        meta[KLT_ID * cap + n0 + i] = kl.next_id + i; meta[KLT_AGE * cap + n0 + i] = 0;
        meta[KLT_IDX * cap + n0 + i] = -1; meta[KLT_PIDX * cap + n0 + i] = -1;
    }
    __syncthreads();                           // every thread has read the lane words
    if (threadIdx.x == 0) { t.lane[lane].n = n0 + m; t.lane[lane].next_id = kl.next_id + m; *t.appended = m; }
}

void launch_klt_append(const KltDev& t, int half, int lane, const float2* left, const float2* right, int n, hipStream_t st)
{
    hipLaunchKernelGGL(k_klt_append, dim3(1), dim3(KLT_BLOCK), 0, st, t, half, lane, left, right, n);
}

// empties the tables of the lanes of the mask: NaN points, no tracks, IDs from 0; the lane's shift is seen from here on
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_clear(const DevCtx c, const KltDev t, int half, LaneMask lanes)
{
    const int lane = blockIdx.x, cap = t.cap;
    if (!lane_bit(lanes, lane)) return;
    float2* pts = t.pts[half] + (size_t)lane * 2 * cap;
    int* meta = t.meta[half] + (size_t)lane * KLT_META * cap;
    for (int i = threadIdx.x; i < 2 * cap; i += KLT_BLOCK) pts[i] = make_float2(NAN, NAN);
    for (int i = threadIdx.x; i < cap; i += KLT_BLOCK) { meta[KLT_ID * cap + i] = -1; meta[KLT_AGE * cap + i] = 0; meta[KLT_IDX * cap + i] = -1; meta[KLT_PIDX * cap + i] = -1; }
    if (threadIdx.x == 0) {
        KltLaneDev& k = t.lane[lane];
        k.n = 0; k.next_id = 0; k.seen_slot = c.lane[lane].prev_slot; k.pad = 0;
    }
}

void launch_klt_clear(const DevCtx& c, const KltDev& t, int half, const LaneMask& lanes, hipStream_t st)
{
    if (t.n_lanes <= 0) return;
    hipLaunchKernelGGL(k_klt_clear, dim3((unsigned)t.n_lanes), dim3(KLT_BLOCK), 0, st, c, t, half, lanes);
}

// svo_klt_set_ransac(2), behind k_track_finalize: the tracks whose pair the RANSAC rejected leave the table.  One block per lane, on
// the LIVE half (the one k_klt_select has just written: slot j is list index j).  The candidates of the lane's octave 0 are still where
// k_ransac_feed put them (block 1 of bf_idx holds their current indices, trk_nk their count) and c.tracked holds the survivors: a slot is
// dropped iff it is the `second` of a candidate and of no survivor -- one bit per slot in LDS, set by the candidates, cleared by the
// survivors.  The points and the four meta rows are compacted stably IN PLACE in chunks of 256: a chunk is read, then a barrier, then
// written (a slot moves to a lower or the same index, never into a later chunk).  KLT_IDX keeps the list index -- the lists are not
// touched --, the slots behind the new count become what k_klt_select leaves behind a count, and no ID is given out again.
// A lane whose candidates all survived (no use_f, or a clean list) writes nothing; an idle lane is not touched.
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_prune(const DevCtx c, const KltDev t, int half)
{
    extern __shared__ unsigned klt_drop[];
    __shared__ int wkeep[KLT_WAVES];
    const int lane = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
    if (lane_idle(c, lane)) return;
    const int cap = t.cap, vl = lane * c.oct_cap;
    auto count = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
    const int n_cand = count(c.trk_nk[vl], c.max_kps), n_keep = count(c.n_tracked[vl], c.max_kps);
    if (n_keep >= n_cand) return;                                      // block-uniform: nothing was rejected
    const int n = count(t.lane[lane].n, cap);
    for (int i = tid; i < (cap + 31) / 32; i += KLT_BLOCK) klt_drop[i] = 0u;
    __syncthreads();
    const int* __restrict__ cand = c.bf_idx + ((long long)vl * 3 + 1) * c.max_kps;
    const svo_index_pair* __restrict__ kept = c.tracked + (long long)vl * c.max_kps;
    for (int i = tid; i < n_cand; i += KLT_BLOCK) { const int s = cand[i]; if ((unsigned)s < (unsigned)n) atomicOr(&klt_drop[s >> 5], 1u << (s & 31)); }
    __syncthreads();
    for (int i = tid; i < n_keep; i += KLT_BLOCK) { const int s = kept[i].second; if ((unsigned)s < (unsigned)n) atomicAnd(&klt_drop[s >> 5], ~(1u << (s & 31))); }
    __syncthreads();
    float2* pts = t.pts[half] + (size_t)lane * 2 * cap;
    int* meta = t.meta[half] + (size_t)lane * KLT_META * cap;
    int n_new = 0;                                                     // the running base: block-uniform
    for (int base = 0; base < n; base += KLT_BLOCK) {
        const int slot = base + tid;
        float2 pl = make_float2(0.0f, 0.0f), pr = pl;
        int m[KLT_META] = { 0, 0, 0, 0 };
        bool keep = false;
        if (slot < n) {
            pl = pts[slot]; pr = pts[cap + slot];
#pragma unroll
            for (int r = 0; r < KLT_META; r++) m[r] = meta[r * cap + slot];
            keep = !((klt_drop[slot >> 5] >> (slot & 31)) & 1u);
        }
        const unsigned long long b = __ballot(keep);
        if (wl == 63) wkeep[wave] = __popcll(b);
        __syncthreads();                       // the chunk is read: its slots may be written
        int o = n_new + __popcll(b & ((1ull << wl) - 1ull)), tot = 0;
#pragma unroll
        for (int w = 0; w < KLT_WAVES; w++) { if (w < wave) o += wkeep[w]; tot += wkeep[w]; }
        if (keep && o != slot) {
            pts[o] = pl; pts[cap + o] = pr;
#pragma unroll
            for (int r = 0; r < KLT_META; r++) meta[r * cap + o] = m[r];
        }
        n_new += tot;
        __syncthreads();                       // the per-wave words are free for the next chunk
    }
    for (int i = n_new + tid; i < n; i += KLT_BLOCK) {
        pts[i] = make_float2(NAN, NAN); pts[cap + i] = make_float2(NAN, NAN);
        meta[KLT_ID * cap + i] = -1; meta[KLT_AGE * cap + i] = 0; meta[KLT_IDX * cap + i] = -1; meta[KLT_PIDX * cap + i] = -1;
    }
    if (tid == 0) t.lane[lane].n = n_new;
}

void launch_klt_prune(const DevCtx& c, const KltDev& t, int half, hipStream_t st)
{
    if (t.n_lanes <= 0) return;
    hipLaunchKernelGGL(k_klt_prune, dim3((unsigned)t.n_lanes), dim3(KLT_BLOCK), (size_t)((t.cap + 31) / 32) * sizeof(unsigned), st, c, t, half);
}

// the job records of a step (KltJobArgs, svo_kernels.h): thread l < n_lanes writes lane l's pyramid record, thread n_lanes + j the
// tracking record of job j = 2 * lane + side.  has_init: 1 under svo_klt_set_prediction(1), where the forward launch starts from the
// guesses of k_klt_predict (k_gn.hip)
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_jobs(const KltJobArgs a, const int has_init)
{
    const int t = blockIdx.x * KLT_BLOCK + threadIdx.x;
    if (t >= (a.row_jobs ? 4 : 3) * a.n_lanes) return;
    const bool row = t >= 3 * a.n_lanes;       // (only with row_jobs) a row record: the images of a pyramid record, the points of a tracking one
    const bool pyr = t < a.n_lanes || row;
    const int lane = row ? t - 3 * a.n_lanes : pyr ? t : (t - a.n_lanes) >> 1, side = pyr ? 0 : (t - a.n_lanes) & 1;
    const int par = lane_bit(a.parity, lane) ? 1 : 0;
    LkJobDev& J = row ? a.row_jobs[lane] : pyr ? a.pyr_jobs[lane] : a.trk_jobs[2 * lane + side];      // written in place: a local record indexed by level would live in scratch
    for (int s = 0; s < 2; s++) for (int l = 0; l < 6; l++) { J.img[s][l] = nullptr; J.pitch[s][l] = 0; }
    for (int l = 0; l < 6; l++) { J.w[l] = 0; J.h[l] = 0; }
    J.pt0 = pyr ? 0 : (2 * lane + side) * a.cap; J.n = pyr ? 0 : a.cap; J.has_init = pyr ? 0 : has_init;
    if (row) { J.pt0 = 2 * lane * a.cap; J.n = lane_bit(a.idle, lane) ? 0 : a.cap; J.has_init = 1; }
    auto block = [&](int parity, int sd) { return a.pyr + ((long long)(parity * a.n_lanes + lane) * 2 + sd) * a.img_stride; };
    // a lane that builds no pyramid has no level; a lane that tracks nothing has one level of 0 x 0 pixels
    const bool none = pyr ? lane_bit(a.idle, lane) : (lane_bit(a.empty, lane) || (a.row_jobs && side == 1));
    J.nl = none ? (pyr && !row ? 0 : 1) : a.nl;
    if (none) return;
    for (int l = 0; l < a.nl; l++) {
        J.w[l] = a.w[l]; J.h[l] = a.h[l]; J.pitch[0][l] = a.w[l]; J.pitch[1][l] = a.w[l];
        J.img[0][l] = (pyr ? block(par, 0) : block(par ^ 1, side)) + a.off[l];
        J.img[1][l] = (pyr ? block(par, 1) : block(par, side)) + a.off[l];
    }
}

void launch_klt_jobs(const KltJobArgs& a, int has_init, hipStream_t st)
{
    if (a.n_lanes <= 0) return;
    hipLaunchKernelGGL(k_klt_jobs, dim3((unsigned)(((a.row_jobs ? 4 : 3) * a.n_lanes + KLT_BLOCK - 1) / KLT_BLOCK)), dim3(KLT_BLOCK), 0, st, a, has_init);
}

// the first guesses of a step's row pass (KltRowGuessArgs, svo_kernels.h): grid (ceil(cap / 256), n_lanes), one thread per slot
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_row_guess(const KltRowGuessArgs a)
{
    const int lane = blockIdx.y, s = blockIdx.x * KLT_BLOCK + threadIdx.x, cap = a.t.cap;
    if (s >= cap || !lane_bit(a.active, lane)) return;
    const size_t o = (size_t)(2 * lane) * cap + s;
    const float2 pl = a.t.pts[a.half][o], pr = a.t.pts[a.half][o + cap];
    float2 nl = pl;
    bool ok = true;
    if (lane_bit(a.fresh, lane)) { a.t.out[o] = pl; a.t.status[o] = 1; a.t.err[o] = 0.0f; }
    else { nl = a.t.out[o]; ok = a.t.status[o] == 1; }
    const float nan = __uint_as_float(0x7fc00000u);
    a.guess[o] = ok ? make_float2(nl.x - (pl.x - pr.x), nl.y) : make_float2(nan, nan);
}

void launch_klt_row_guess(const KltRowGuessArgs& a, hipStream_t st)
{
    if (a.t.n_lanes <= 0 || a.t.cap <= 0) return;
    hipLaunchKernelGGL(k_klt_row_guess, dim3((unsigned)((a.t.cap + KLT_BLOCK - 1) / KLT_BLOCK), (unsigned)a.t.n_lanes), dim3(KLT_BLOCK), 0, st, a);
}

// ---- svo_klt_topup ------------------------------------------------------------------------------------------------------------
// The detector (k_gftt.hip) and the tracker (k_lk.hip) are launched as they are, on records these kernels write: which lanes take part
// is decided here from KltLaneDev.n, never on the host.
//
// k_klt_topup_jobs: thread l writes lane l's detector record and the reason the lane sits out, if it does.  Such a lane gets a 0 x 0
// image and cap 0: its blocks of k_gftt_response and k_gftt_candidates leave on their first lines, and k_gftt_select finds no candidate
// and writes a count of 0.  The seeds are the lane's live left points where they lie in the table.
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_topup_jobs(const KltTopupArgs a)
{
    const int lane = blockIdx.x * KLT_BLOCK + threadIdx.x;
    if (lane >= a.t.n_lanes) return;
    const int cap = a.t.cap;
    int n = a.t.lane[lane].n;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const int reason = !lane_bit(a.lanes, lane) ? KLT_TOPUP_NOT_ASKED : !lane_bit(a.has_img, lane) ? KLT_TOPUP_NO_PAIR : n >= a.below ? KLT_TOPUP_ENOUGH : KLT_TOPUP_OK;
    const bool run = reason == KLT_TOPUP_OK;
    const int goal = a.target < cap ? a.target : cap, want = goal > n ? goal - n : 0;
    const int par = lane_bit(a.parity, lane) ? 1 : 0;
    GfttJobDev& J = a.gjobs[lane];
    J.img = run ? a.pyr + ((long long)(par * a.t.n_lanes + lane) * 2 + 0) * a.img_stride + a.off[0] : nullptr;
    J.map = a.map + (long long)lane * a.map_stride;
    J.pitch = run ? a.w[0] : 0; J.w = run ? a.w[0] : 0; J.h = run ? a.h[0] : 0;
    J.seed0 = lane * 2 * cap; J.n_seeds = run ? n : 0; J.pts0 = lane * cap; J.cap = run ? want : 0;
    J.cell = a.cell; J.gw = run ? a.gw : 0; J.gh = run ? a.gh : 0;
    for (int k = 0; k < 4; k++) { a.ginfo[4 * lane + k] = 0; a.tinfo[4 * lane + k] = k == 3 ? reason : 0; }
}

void launch_klt_topup_jobs(const KltTopupArgs& a, hipStream_t st)
{
    if (a.t.n_lanes <= 0) return;
    hipLaunchKernelGGL(k_klt_topup_jobs, dim3((unsigned)((a.t.n_lanes + KLT_BLOCK - 1) / KLT_BLOCK)), dim3(KLT_BLOCK), 0, st, a);
}

// k_klt_topup_prepare, behind k_gftt_select: one thread per slot writes the slot's first guess -- the corner shifted by (-init_disp, 0),
// NaN behind the detector's count, on which the tracker retires the slot before it reads a pixel --, and the thread of a lane's slot 0
// writes the lane's tracking record (left -> right of the lane's last pair), in place
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_topup_prepare(const KltTopupArgs a)
{
    const int cap = a.t.cap;
    const int g = blockIdx.x * KLT_BLOCK + threadIdx.x;
    if (g >= a.t.n_lanes * cap) return;
    const int lane = g / cap, slot = g - lane * cap;
    const bool run = a.tinfo[4 * lane + 3] == KLT_TOPUP_OK && a.ginfo[4 * lane + 2] == 0;
    const int cnt = run ? a.ginfo[4 * lane + 0] : 0;
    float2 q = make_float2(NAN, NAN);
    if (slot < cnt) { const float2 p = a.corners[g]; q = make_float2(__fsub_rn(p.x, a.init_disp), p.y); }
    a.init[g] = q;
    if (slot != 0) return;
    const int par = lane_bit(a.parity, lane) ? 1 : 0;
    LkJobDev& J = a.lk_jobs[lane];
    for (int s = 0; s < 2; s++) for (int l = 0; l < 6; l++) { J.img[s][l] = nullptr; J.pitch[s][l] = 0; }
    for (int l = 0; l < 6; l++) { J.w[l] = 0; J.h[l] = 0; }
    J.pt0 = lane * cap; J.n = cnt; J.has_init = 1;
    J.nl = cnt > 0 ? a.nl : 1;
    if (cnt <= 0) return;
    for (int l = 0; l < a.nl; l++) {
        J.w[l] = a.w[l]; J.h[l] = a.h[l]; J.pitch[0][l] = a.w[l]; J.pitch[1][l] = a.w[l];
        for (int s = 0; s < 2; s++) J.img[s][l] = a.pyr + ((long long)(par * a.t.n_lanes + lane) * 2 + s) * a.img_stride + a.off[l];
    }
}

void launch_klt_topup_prepare(const KltTopupArgs& a, hipStream_t st)
{
    const long long n = (long long)a.t.n_lanes * a.t.cap;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_klt_topup_prepare, dim3((unsigned)((n + KLT_BLOCK - 1) / KLT_BLOCK)), dim3(KLT_BLOCK), 0, st, a);
}

// k_klt_topup_append, behind the tracker: one block per lane.  The gate of k_klt_select on (corner, partner), the stable compaction of
// its scheme -- chunks of 256 in slot order, ballot + popcount inside a wave, the wave totals through LDS --, and the append of
// k_klt_append behind the live count: fresh IDs, age 0, no indices, nothing beyond cap.  Thread 0 writes the lane words and the record
// of svo_klt_topup_info.  A lane that sits out is not touched.
__global__ __launch_bounds__(KLT_BLOCK) void k_klt_topup_append(const KltTopupArgs a, int only_lane)
{
    __shared__ int wsurv[KLT_WAVES];
    const int lane = only_lane >= 0 ? only_lane : blockIdx.x, tid = threadIdx.x, wave = tid >> 6, wl = tid & 63;
    const int cap = a.t.cap;
    int* tinfo = a.tinfo + 4 * lane;
    const int* ginfo = a.ginfo + 4 * lane;
    if (tinfo[3] != KLT_TOPUP_OK) return;                              // block-uniform
    if (ginfo[2] != 0) { if (tid == 0) { tinfo[0] = 0; tinfo[1] = ginfo[1]; tinfo[2] = 0; tinfo[3] = KLT_TOPUP_OVERFLOW; } return; }
    const KltLaneDev kl = a.t.lane[lane];
    const int n0 = kl.n < cap ? (kl.n < 0 ? 0 : kl.n) : cap;
    const int cnt = ginfo[0] < cap ? ginfo[0] : cap;
    float2* pts = a.t.pts[a.half] + (size_t)lane * 2 * cap;
    int* meta = a.t.meta[a.half] + (size_t)lane * KLT_META * cap;
    const float2* __restrict__ cl = a.corners + (size_t)lane * cap, * __restrict__ cr = a.out + (size_t)lane * cap;
    const uint8_t* __restrict__ st = a.status + (size_t)lane * cap;
    int n_surv = 0;                                                    // the running base: block-uniform
    for (int base = 0; base < cnt; base += KLT_BLOCK) {
        const int slot = base + tid;
        float2 pl = make_float2(0.0f, 0.0f), pr = pl;
        bool ok = false;
        if (slot < cnt) {
            pl = cl[slot]; pr = cr[slot];
            const float disp = pl.x - pr.x;
            ok = st[slot] == 1 && klt_finite(pl.x) && klt_finite(pl.y) && klt_finite(pr.x) && klt_finite(pr.y)
                 && fabsf(pl.y - pr.y) <= a.max_dy && disp >= a.min_disp && disp <= a.max_disp;
        }
        const unsigned long long bs = __ballot(ok);
        if (wl == 63) wsurv[wave] = __popcll(bs);
        __syncthreads();
        int i = n_surv + __popcll(bs & ((1ull << wl) - 1ull)), tot = 0;
#pragma unroll
        for (int w = 0; w < KLT_WAVES; w++) { if (w < wave) i += wsurv[w]; tot += wsurv[w]; }
        if (ok && n0 + i < cap) {
            pts[n0 + i] = pl; pts[cap + n0 + i] = pr;
            meta[KLT_ID * cap + n0 + i] = kl.next_id + i; meta[KLT_AGE * cap + n0 + i] = 0;
            meta[KLT_IDX * cap + n0 + i] = -1; meta[KLT_PIDX * cap + n0 + i] = -1;
        }
        n_surv += tot;
        __syncthreads();                       // the per-wave words are free for the next chunk; every thread has read the lane words
    }
    __syncthreads();                           // (a lane without corners ran no chunk: every thread has read the lane words here too)
    if (tid == 0) {
        const int m = n_surv < cap - n0 ? n_surv : cap - n0;
        a.t.lane[lane].n = n0 + m; a.t.lane[lane].next_id = kl.next_id + m;
        tinfo[0] = cnt; tinfo[1] = ginfo[1]; tinfo[2] = m; tinfo[3] = KLT_TOPUP_OK;
    }
}

void launch_klt_topup_append(const KltTopupArgs& a, int only_lane, hipStream_t st)
{
    if (a.t.n_lanes <= 0) return;
    hipLaunchKernelGGL(k_klt_topup_append, dim3(only_lane >= 0 ? 1u : (unsigned)a.t.n_lanes), dim3(KLT_BLOCK), 0, st, a, only_lane);
}
