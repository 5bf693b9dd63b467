// state_format.hpp -- the estimator state file as bytes: writer and validating parser, host only (no HIP, no context).
//
// svo_save_state / svo_load_state (svo_api.hip) move the lists between the device and a svo_state::State; this unit turns a State
// into the file's bytes and back.  The parser works on a memory image of the whole file and validates ALL of it before it returns
// success, so that a loader never touches a lane on behalf of a file it will refuse.  tools/state_format_fuzz.cpp drives both under
// the address and undefined-behaviour sanitizers on the CPU.
//
// Layout, little-endian, no padding anywhere (the byte-for-byte description is beside svo_save_state in include/svo_hip.h and in
// stereo_vo_amd/state_file.py, which reads the same bytes independently):
//   base       what CStereoOdometryEstimator::saveStateToFile writes (common.cpp:475-543): npyr, the PRE and CUR groups of octave 0, the tail
//   extension  optional, directly behind the tail: magic, version, n_oct, w, h, has-windows bytes, the groups of octaves 1 .. n_oct - 1,
//              the windows of every frame that has them
#ifndef SVO_STATE_FORMAT_HPP
#define SVO_STATE_FORMAT_HPP
#include "../../include/svo_types.h"
#include <stdint.h>
#include <stddef.h>
#include <string>
#include <vector>

namespace svo_state {

enum : uint32_t { EXT_MAGIC = 0x58455653u /* "SVEX" */, EXT_VERSION = 1u, MAX_OCTAVES = 4u };

struct List { std::vector<svo_keypoint> kps; std::vector<uint8_t> desc; };                  // desc: 32 bytes per keypoint
struct Group { List left, right; std::vector<svo_dmatch> matches; std::vector<int32_t> ids; };   // one frame of one octave
struct Windows { std::vector<uint8_t> flag, win; };                                         // flag: one byte per keypoint; win: 64 bytes per keypoint

struct State {
    uint64_t npyr = 1;
    std::vector<Group> frame[2];          // [0] PRE, [1] CUR (the file's order); one Group per octave, octave 0 first
    uint8_t m_reset = 0;
    uint64_t tail[5] = { 0, 0, 0, 0, 0 }; // m_lastID, m_num_tracked_pairs_from_last_kf, ..._from_last_frame, m_last_match_ID, m_kf_max_match_ID
    bool has_ext = false;
    uint32_t n_oct = 1, w = 0, h = 0;     // of the extension block (n_oct = 1 without one)
    uint8_t has_win[2] = { 0, 0 };        // [0] PRE, [1] CUR
    std::vector<Windows> win[2];          // [frame][octave * 2 + side], only for frames with has_win
};

// the file's bytes for `s`.  The extension block is written when s.has_ext is set; s.frame[f] must then hold s.n_oct groups and, for
// every frame with has_win, s.win[f] must hold 2 * n_oct entries whose counts equal those of their lists.  false: `s` is inconsistent.
bool write(const State& s, std::vector<uint8_t>& out);

// Parse and validate a whole file image.  max_kps bounds every count.  true: `out` holds the file; false: `err` says what is wrong and
// where, and `out` is unspecified.  Never reads outside [p, p + n).
bool parse(const uint8_t* p, size_t n, size_t max_kps, State& out, std::string& err);

}  // namespace svo_state
#endif
