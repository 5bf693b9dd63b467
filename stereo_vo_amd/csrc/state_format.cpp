// state_format.cpp -- writer and validating parser of the estimator state file (state_format.hpp).  Host only.
#include "state_format.hpp"
#include <stdio.h>
#include <string.h>

namespace svo_state {
namespace {

void put(std::vector<uint8_t>& o, const void* p, size_t n) { const uint8_t* b = (const uint8_t*)p; o.insert(o.end(), b, b + n); }

void dump_keypoints(std::vector<uint8_t>& o, const List& L)              // m_dump_keypoints_to_stream (C:88-133)
{
    const uint64_t n = L.kps.size();
    put(o, &n, 8);
    for (const svo_keypoint& k : L.kps) {
        const float v[5] = { k.x, k.y, k.response, k.size, k.angle };
        const int32_t w[2] = { k.octave, k.class_id };
        put(o, v, sizeof(v)); put(o, w, sizeof(w));
    }
    const int32_t hdr[3] = { (int32_t)n, n ? 32 : 0, 0 /* CV_8UC1 */ };
    put(o, hdr, sizeof(hdr));
    if (!L.desc.empty()) put(o, L.desc.data(), L.desc.size());
}
void dump_matches(std::vector<uint8_t>& o, const std::vector<svo_dmatch>& m, const std::vector<int32_t>& ids)   // m_dump_matches_to_stream (C:138-163)
{
    const uint64_t n = m.size(), ni = ids.size();
    put(o, &n, 8); put(o, &ni, 8);
    for (size_t i = 0; i < m.size(); i++) {
        if (n == ni) { const uint64_t id = (uint64_t)(int64_t)ids[i]; put(o, &id, 8); }
        put(o, &m[i].queryIdx, 4); put(o, &m[i].trainIdx, 4); put(o, &m[i].distance, 4); put(o, &m[i].imgIdx, 4);
    }
}
void dump_group(std::vector<uint8_t>& o, const Group& g) { dump_keypoints(o, g.left); dump_keypoints(o, g.right); dump_matches(o, g.matches, g.ids); }

// a cursor over the file image: every read is checked against the end first
struct Reader {
    const uint8_t* p; size_t n, off; const char* what;
    bool rd(void* dst, size_t k) { if (k > n - off) return false; memcpy(dst, p + off, k); off += k; return true; }
};

bool load_keypoints(Reader& r, List& L, size_t cap)         // m_load_keypoints_from_stream (C:168-211)
{
    uint64_t n = 0;
    if (!r.rd(&n, 8) || n > cap) return false;
    if (n * 28 > r.n - r.off) return false;                  // (before the allocation: a count the file cannot hold)
    L.kps.resize((size_t)n);
    for (svo_keypoint& k : L.kps) {
        float v[5]; int32_t w[2];
        if (!r.rd(v, sizeof(v)) || !r.rd(w, sizeof(w))) return false;
        k.x = v[0]; k.y = v[1]; k.response = v[2]; k.size = v[3]; k.angle = v[4]; k.octave = w[0]; k.class_id = w[1];
    }
    int32_t hdr[3];
    if (!r.rd(hdr, sizeof(hdr)) || hdr[0] < 0 || hdr[1] < 0) return false;
    if ((uint64_t)hdr[0] != n || (n && hdr[1] != 32)) return false;             // this path only knows 256-bit descriptors
    if (n * 32 > r.n - r.off) return false;
    L.desc.resize((size_t)n * 32);
    return L.desc.empty() || r.rd(L.desc.data(), L.desc.size());
}
bool load_matches(Reader& r, std::vector<svo_dmatch>& m, std::vector<int32_t>& ids, size_t cap)    // m_load_matches_from_stream (C:216-255)
{
    uint64_t n = 0, ni = 0;
    if (!r.rd(&n, 8) || !r.rd(&ni, 8) || n > cap || ni > cap) return false;
    if (n * 16 > r.n - r.off) return false;
    m.resize((size_t)n); ids.assign((size_t)ni, 0);
    for (size_t i = 0; i < m.size(); i++) {
        if (n == ni) { uint64_t id; if (!r.rd(&id, 8)) return false; ids[i] = (int32_t)id; }
        if (!r.rd(&m[i].queryIdx, 4) || !r.rd(&m[i].trainIdx, 4) || !r.rd(&m[i].distance, 4) || !r.rd(&m[i].imgIdx, 4)) return false;
    }
    return true;
}
bool load_group(Reader& r, Group& g, size_t cap) { return load_keypoints(r, g.left, cap) && load_keypoints(r, g.right, cap) && load_matches(r, g.matches, g.ids, cap); }

bool fail(std::string& err, const char* what, size_t off)
{
    char msg[160]; snprintf(msg, sizeof(msg), "%s (at byte %zu)", what, off);
    err = msg; return false;
}

}  // namespace

bool write(const State& s, std::vector<uint8_t>& out)
{
    out.clear();
    const uint32_t n_oct = s.has_ext ? s.n_oct : 1;
    if (n_oct < 1 || n_oct > MAX_OCTAVES || s.frame[0].size() < n_oct || s.frame[1].size() < n_oct) return false;
    put(out, &s.npyr, 8);
    for (int f = 0; f < 2; f++) dump_group(out, s.frame[f][0]);                      // PRE first, then CUR (C:491-527)
    put(out, &s.m_reset, 1); put(out, s.tail, sizeof(s.tail));
    if (!s.has_ext) return true;
    const uint32_t head[5] = { EXT_MAGIC, EXT_VERSION, n_oct, s.w, s.h };
    put(out, head, sizeof(head));
    const uint8_t hw[2] = { (uint8_t)(s.has_win[0] ? 1 : 0), (uint8_t)(s.has_win[1] ? 1 : 0) };
    put(out, hw, 2);
    for (uint32_t o = 1; o < n_oct; o++) for (int f = 0; f < 2; f++) dump_group(out, s.frame[f][o]);
    for (int f = 0; f < 2; f++) {
        if (!hw[f]) continue;
        if (s.win[f].size() < 2 * (size_t)n_oct) return false;
        for (uint32_t o = 0; o < n_oct; o++)
            for (int side = 0; side < 2; side++) {
                const Windows& w = s.win[f][o * 2 + side];
                const uint64_t n = w.flag.size();
                if (n != (side ? s.frame[f][o].right : s.frame[f][o].left).kps.size() || w.win.size() != n * 64) return false;
                put(out, &n, 8);
                if (n) { put(out, w.flag.data(), (size_t)n); put(out, w.win.data(), (size_t)n * 64); }
            }
    }
    return true;
}

bool parse(const uint8_t* p, size_t n, size_t max_kps, State& s, std::string& err)
{
    s = State();
    Reader r{ p, n, 0, "" };
    if (!r.rd(&s.npyr, 8)) return fail(err, "truncated before npyr", r.off);
    for (int f = 0; f < 2; f++) {
        s.frame[f].resize(1);
        if (!load_group(r, s.frame[f][0], max_kps)) return fail(err, f ? "malformed or truncated CUR lists of octave 0 (or a count above max_kps)" : "malformed or truncated PRE lists of octave 0 (or a count above max_kps)", r.off);
    }
    if (!r.rd(&s.m_reset, 1) || !r.rd(s.tail, sizeof(s.tail))) return fail(err, "truncated tail", r.off);
    if (r.off == n) return true;                             // the reference's layout alone: octave 0, no windows
    uint32_t head[5];
    if (!r.rd(head, sizeof(head))) return fail(err, "truncated extension header", r.off);
    if (head[0] != EXT_MAGIC) return fail(err, "bytes behind the tail that do not begin with the extension's magic word", r.off);
    if (head[1] != EXT_VERSION) return fail(err, "unknown extension version", r.off);
    if (head[2] < 1 || head[2] > MAX_OCTAVES) return fail(err, "extension: n_oct outside 1 .. 4", r.off);
    if (head[3] < 1 || head[4] < 1 || head[3] > (1u << 16) || head[4] > (1u << 16)) return fail(err, "extension: image size outside 1 .. 65536", r.off);
    s.has_ext = true; s.n_oct = head[2]; s.w = head[3]; s.h = head[4];
    if (!r.rd(s.has_win, 2) || s.has_win[0] > 1 || s.has_win[1] > 1) return fail(err, "extension: has-windows bytes truncated or not 0 / 1", r.off);
    for (int f = 0; f < 2; f++) s.frame[f].resize(s.n_oct);
    for (uint32_t o = 1; o < s.n_oct; o++)
        for (int f = 0; f < 2; f++)
            if (!load_group(r, s.frame[f][o], max_kps)) return fail(err, "extension: malformed or truncated lists of a higher octave (or a count above max_kps)", r.off);
    for (int f = 0; f < 2; f++) {
        if (!s.has_win[f]) continue;
        s.win[f].resize(2 * (size_t)s.n_oct);
        for (uint32_t o = 0; o < s.n_oct; o++)
            for (int side = 0; side < 2; side++) {
                Windows& w = s.win[f][o * 2 + side];
                uint64_t cnt = 0;
                if (!r.rd(&cnt, 8)) return fail(err, "extension: truncated windows count", r.off);
                if (cnt != (side ? s.frame[f][o].right : s.frame[f][o].left).kps.size()) return fail(err, "extension: a windows count differs from its list's count", r.off);
                if (cnt * 65 > r.n - r.off) return fail(err, "extension: truncated windows", r.off);
                w.flag.resize((size_t)cnt); w.win.resize((size_t)cnt * 64);
                if (cnt && (!r.rd(w.flag.data(), (size_t)cnt) || !r.rd(w.win.data(), (size_t)cnt * 64))) return fail(err, "extension: truncated windows", r.off);
            }
    }
    if (r.off != n) return fail(err, "bytes behind the end of the extension block", r.off);
    return true;
}

}  // namespace svo_state
