// lk_call.hpp -- what one svo_lk_track call IS, decided on the host without a device: whether its parameters, jobs and flags are acceptable
// (check_lk_call), the pyramid geometry of every image (lk_geometry) and where everything lies in the call's buffers (plan_lk_call).
// Host only, no HIP: svo_api.hip acts on these decisions, k_lk.hip reads the records they fill, and tools/lk_check.cpp drives them under
// the sanitizers on the CPU (`make hostcheck`).
#pragma once
#include "../../include/svo_hip.h"
#include <stdint.h>
#include <string>
#include <vector>

namespace svo_lk {

enum { LK_MAX_LEVELS = 6 };                      // max_level 0 .. 5

// the levels of one w x h image: level 0 is the image, level k + 1 is ((w + 1) / 2, (h + 1) / 2) of level k and exists while
// k + 1 <= max_level and both of its sides are at least win + 4.  off[k]: byte offset of level k in the image's block of tightly packed
// levels (pitch = w[k]); without level 0 (a device image read in place) off[0] = -1 and level 1 starts the block.
struct Geometry { int nl; int w[LK_MAX_LEVELS], h[LK_MAX_LEVELS]; long long off[LK_MAX_LEVELS]; long long bytes; };
Geometry lk_geometry(int w, int h, int win, int max_level, bool with_level0);

// the parameter ranges of svo_lk_params; SVO_OK, or SVO_ERR_ARG with the text
int check_lk_params(const svo_lk_params& p, std::string& why);

// what the context can take: svo_config.max_kps, 4 * n_lanes * max_octaves, max_w, max_h
struct Caps { int max_kps, max_jobs, max_w, max_h; };
// every refusal of svo_lk_track, in order: flags, parameters, the job count, then job by job the point count, pointers, sizes and
// strides.  SVO_OK, or the status (SVO_ERR_ARG / SVO_ERR_CAPACITY) with the text in `why`.  jobs may be NULL only when n_jobs == 0.
int check_lk_call(const svo_lk_job* jobs, int n_jobs, const svo_lk_params& p, uint32_t flags, const Caps& caps, std::string& why);

// the layout of an accepted call: per job its geometry, the offsets of its two image blocks in the pyramid buffer and its first index in
// the flat point arrays; the totals the buffers are sized by; the deepest level count of any job (the number of pyrdown launches + 1)
struct Plan {
    std::vector<Geometry> geom; std::vector<long long> img_off; std::vector<int> pt0;
    long long pyr_bytes; int n_pts; int max_nl; bool any_init;
};
Plan plan_lk_call(const svo_lk_job* jobs, int n_jobs, const svo_lk_params& p, bool device_images);

// svo_lk_set_photometric, in order: a capturing stream (SVO_ERR_STATE), then the mode, 0 .. 1 (SVO_ERR_ARG).  Nothing else is asked: the
// setter needs no svo_set_params and no front end
enum { LK_PHOTO_RAW = 0, LK_PHOTO_GAIN_BIAS = 1 };
int check_lk_set_photometric(int mode, bool capturing, std::string& why);

// the kernel instantiation a window size runs: the number of window pixels a lane owns at most, ceil(win^2 / 64) rounded up to 2, 7 or 16
int lk_pixels_per_lane(int win);

}
