// state_format_fuzz.cpp -- the state file's writer and parser (stereo_vo_amd/csrc/state_format.cpp) under the address and
// undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc fuzz && tools/state_format_fuzz
//
// Writes a valid three-octave file with windows on both frames, parses it back and compares; then parses EVERY truncation of it and
// a few thousand seeded single-byte corruptions.  Each parse must end in a clean refusal or a clean parse (a corrupted coordinate is
// still a file); a sanitizer report or a crash fails the run.  Every input is copied into a heap block of exactly its length first, so
// that one byte read behind it is a report.  Exit status 0 and a last line "ok" when everything held.
#include "state_format.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

using namespace svo_state;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

static List make_list(int n)
{
    List L; L.kps.resize((size_t)n); L.desc.resize((size_t)n * 32);
    for (int i = 0; i < n; i++) {
        svo_keypoint& k = L.kps[(size_t)i];
        k.x = (float)(rnd() % 25100) / 100.f; k.y = (float)(rnd() % 18700) / 100.f; k.size = 7.f; k.angle = -1.f; k.response = (float)(rnd() % 1000);
        k.octave = 0; k.class_id = -1;
    }
    for (uint8_t& b : L.desc) b = (uint8_t)rnd();
    return L;
}
static Group make_group(int nl, int nr, int nm, bool with_ids)
{
    Group g; g.left = make_list(nl); g.right = make_list(nr);
    g.matches.resize((size_t)nm);
    for (int i = 0; i < nm; i++) { g.matches[(size_t)i].queryIdx = (int32_t)(rnd() % (uint32_t)nl); g.matches[(size_t)i].trainIdx = (int32_t)(rnd() % (uint32_t)nr); g.matches[(size_t)i].imgIdx = 0; g.matches[(size_t)i].distance = (float)(rnd() % 400); }
    if (with_ids) { g.ids.resize((size_t)nm); for (int i = 0; i < nm; i++) g.ids[(size_t)i] = (int32_t)(rnd() % 100000); }
    return g;
}
static Windows make_windows(size_t n)
{
    Windows w; w.flag.resize(n); w.win.resize(n * 64);
    for (uint8_t& b : w.flag) b = (uint8_t)(rnd() % 5 == 0);
    for (uint8_t& b : w.win) b = (uint8_t)rnd();
    return w;
}

static bool same_list(const List& a, const List& b) { return a.kps.size() == b.kps.size() && (a.kps.empty() || !memcmp(a.kps.data(), b.kps.data(), a.kps.size() * sizeof(svo_keypoint))) && a.desc == b.desc; }
static bool same_group(const Group& a, const Group& b)
{
    return same_list(a.left, b.left) && same_list(a.right, b.right) && a.matches.size() == b.matches.size() &&
           (a.matches.empty() || !memcmp(a.matches.data(), b.matches.data(), a.matches.size() * sizeof(svo_dmatch))) && a.ids == b.ids;
}

// parse a private heap copy of exactly n bytes
static bool parse_copy(const uint8_t* p, size_t n, size_t cap, State& out, std::string& err)
{
    uint8_t* q = (uint8_t*)malloc(n ? n : 1);
    if (!q) { fprintf(stderr, "out of memory\n"); exit(2); }
    if (n) memcpy(q, p, n);
    const bool ok = parse(q, n, cap, out, err);
    free(q);
    return ok;
}

int main(int argc, char** argv)
{
    const int n_corrupt = argc > 1 ? atoi(argv[1]) : 4000;
    const size_t cap = 64;
    State s;
    s.has_ext = true; s.n_oct = 3; s.w = 251; s.h = 187; s.npyr = 3; s.m_reset = 1;
    s.tail[1] = 17; s.tail[2] = 23; s.tail[3] = 4711; s.tail[4] = 42;
    s.has_win[0] = 1; s.has_win[1] = 1;
    const int nl[3] = { 23, 11, 5 }, nr[3] = { 19, 13, 0 };
    for (int f = 0; f < 2; f++) {
        for (int o = 0; o < 3; o++) s.frame[f].push_back(make_group(nl[o] + f, nr[o], nr[o] ? 7 - 2 * o : 0, o != 1));
        for (int o = 0; o < 3; o++) { s.win[f].push_back(make_windows(s.frame[f][(size_t)o].left.kps.size())); s.win[f].push_back(make_windows(s.frame[f][(size_t)o].right.kps.size())); }
    }
    std::vector<uint8_t> file;
    if (!write(s, file)) { fprintf(stderr, "write refused a consistent record\n"); return 1; }
    State t; std::string err;
    if (!parse_copy(file.data(), file.size(), cap, t, err)) { fprintf(stderr, "the valid file was refused: %s\n", err.c_str()); return 1; }
    bool same = t.has_ext && t.n_oct == 3 && t.w == 251 && t.h == 187 && t.npyr == 3 && t.m_reset == 1 && !memcmp(t.tail, s.tail, sizeof(s.tail)) && t.has_win[0] == 1 && t.has_win[1] == 1;
    for (int f = 0; f < 2 && same; f++) {
        for (size_t o = 0; o < 3 && same; o++) same = same_group(s.frame[f][o], t.frame[f][o]);
        for (size_t i = 0; i < 6 && same; i++) same = s.win[f][i].flag == t.win[f][i].flag && s.win[f][i].win == t.win[f][i].win;
    }
    if (!same) { fprintf(stderr, "the round trip changed the record\n"); return 1; }
    std::vector<uint8_t> again;
    if (!write(t, again) || again != file) { fprintf(stderr, "writing the parsed record gave other bytes\n"); return 1; }
    // a record whose windows do not belong to its lists is not written
    { State bad = s; bad.win[1][2].flag.pop_back(); std::vector<uint8_t> o; if (write(bad, o)) { fprintf(stderr, "an inconsistent record was written\n"); return 1; } }

    // the legacy prefix (up to and including the tail) is itself a file: octave 0, no block
    size_t legacy = 0;
    {
        State one = s; one.has_ext = false;
        std::vector<uint8_t> o; if (!write(one, o)) return 1;
        legacy = o.size();
        if (legacy >= file.size() || memcmp(o.data(), file.data(), legacy)) { fprintf(stderr, "the block does not follow the unchanged legacy bytes\n"); return 1; }
    }
    // every truncation: refused, except the legacy prefix
    size_t refused = 0, parsed = 0;
    for (size_t n = 0; n < file.size(); n++) {
        const bool ok = parse_copy(file.data(), n, cap, t, err);
        if (ok != (n == legacy)) { fprintf(stderr, "truncation to %zu bytes: %s\n", n, ok ? "parsed" : err.c_str()); return 1; }
        if (ok && t.has_ext) { fprintf(stderr, "the legacy prefix reported a block\n"); return 1; }
        ok ? parsed++ : refused++;
    }
    printf("truncations: %zu refused, %zu parsed (the legacy prefix at %zu of %zu bytes)\n", refused, parsed, legacy, file.size());
    // a count above the capacity is refused
    if (parse_copy(file.data(), file.size(), 16, t, err)) { fprintf(stderr, "a count above max_kps was accepted\n"); return 1; }
    // seeded single-byte corruptions: whatever the verdict, nothing may be read outside the file and a parse must be self-consistent
    refused = parsed = 0;
    std::vector<uint8_t> c = file;
    for (int i = 0; i < n_corrupt; i++) {
        const size_t at = rnd() % file.size();
        const uint8_t old = c[at];
        c[at] = (uint8_t)(old ^ (1u + rnd() % 255u));
        if (parse_copy(c.data(), c.size(), cap, t, err)) {
            parsed++;
            bool sane = t.frame[0].size() == t.n_oct && t.frame[1].size() == t.n_oct;
            for (int f = 0; f < 2 && sane; f++)
                for (size_t o = 0; o < t.n_oct && sane; o++) {
                    const Group& g = t.frame[f][o];
                    sane = g.left.kps.size() <= cap && g.right.kps.size() <= cap && g.matches.size() <= cap && g.ids.size() <= cap && g.left.desc.size() == g.left.kps.size() * 32;
                    if (sane && t.has_win[f]) sane = t.win[f][o * 2].flag.size() == g.left.kps.size() && t.win[f][o * 2 + 1].win.size() == g.right.kps.size() * 64;
                }
            if (!sane) { fprintf(stderr, "corruption at byte %zu parsed into an inconsistent record\n", at); return 1; }
            std::vector<uint8_t> o;
            if (!write(t, o)) { fprintf(stderr, "corruption at byte %zu parsed into a record the writer refuses\n", at); return 1; }
        } else refused++;
        c[at] = old;
    }
    printf("corruptions: %zu refused, %zu parsed\n", refused, parsed);
    printf("ok\n");
    return 0;
}
