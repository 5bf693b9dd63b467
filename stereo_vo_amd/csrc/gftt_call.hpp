// gftt_call.hpp -- what one svo_gftt_detect call IS, decided on the host without a device: whether its parameters, jobs and flags are
// acceptable (check_gftt_call), the cell grid of the distance rule (gftt_cells) and where everything lies in the call's buffers
// (plan_gftt_call).  Host only, no HIP: svo_api.hip acts on these decisions, k_gftt.hip reads the records they fill, and
// tools/gftt_check.cpp drives them under the sanitizers on the CPU (`make hostcheck`).
#pragma once
#include "../../include/svo_hip.h"
#include <stdint.h>
#include <string>
#include <vector>

namespace svo_gftt {

enum { GFTT_MAX_CELLS_SIDE = 64, GFTT_MIN_CAND_CAP = 1024, GFTT_TILE = 32, GFTT_MAX_CAND_CAP = 1 << 24 };

// the parameter ranges of svo_gftt_params (max_corners against max_kps is a capacity, checked by check_gftt_call); SVO_OK, or
// SVO_ERR_ARG with the text
int check_gftt_params(const svo_gftt_params& p, std::string& why);

// what the context can take: svo_config.max_kps, 4 * n_lanes * max_octaves, max_w, max_h, svo_config.max_cand
struct Caps { int max_kps, max_jobs, max_w, max_h, max_cand; };
// every refusal of svo_gftt_detect, in order: flags, parameters, max_corners against max_kps, a context whose max_cand exceeds 2^24 (the
// sort pads to a power of two and the scratch offsets are 32-bit: SVO_ERR_CAPACITY), the job count, then job by job the counts,
// pointers, sizes and strides.  SVO_OK, or the status (SVO_ERR_ARG / SVO_ERR_CAPACITY) with the text in `why`.  jobs may be NULL only
// when n_jobs == 0.
int check_gftt_call(const svo_gftt_job* jobs, int n_jobs, const svo_gftt_params& p, uint32_t flags, const Caps& caps, std::string& why);

// the candidates a job may collect: max(1024, max_cand), the context's level-0 candidate capacity; and the keys a job's row holds,
// that number rounded up to a power of two (the sort pads to one)
int gftt_cand_cap(int max_cand);
int gftt_key_stride(int cand_cap);

// the cell grid of the distance rule: the smallest cell side >= max(min_distance, 1) with at most 64 cells along each axis, so that the
// 3 x 3 cells around a point hold everything closer than min_distance
struct Cells { int cell, gw, gh; };
Cells gftt_cells(int w, int h, int min_distance);

// the layout of an accepted call: per job the offset of its response map (floats, 64-float aligned), of its image copy (bytes, 256-byte
// aligned; host images only), its first seed and its first result in the flat arrays; the totals the buffers are sized by; the largest
// image (the grids of the two per-pixel kernels)
struct Plan {
    std::vector<long long> map_off, img_off; std::vector<int> seed0, pts0; std::vector<Cells> cells;
    long long map_floats, img_bytes; int n_seeds, n_pts, max_w, max_h;
};
Plan plan_gftt_call(const svo_gftt_job* jobs, int n_jobs, const svo_gftt_params& p, bool device_images);

}
