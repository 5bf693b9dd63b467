// knobs_check.cpp -- the parsing of the SVO_* environment knobs (stereo_vo_amd/csrc/svo_knobs.cpp) and the grouping of the debug modes
// (svo_knobs.hpp), under the address and undefined-behaviour sanitizers, on the CPU: no HIP, no GPU, no Python.
//
//   make -C stereo_vo_amd/csrc hostcheck && tools/knobs_check
//
// Every expected value below is written from the rules the launchers and svo_create applied before the knobs had a unit of their
// own (the table in INTEGRATION.md states them), not taken from a run of knobs_read.  Exit status 0 and a last line "ok" when
// everything held.
#include "svo_knobs.hpp"
#include <stdio.h>
#include <string.h>
#include <functional>

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: %s   [%s = %s]\n", __FILE__, __LINE__, #cond, env_name ? env_name : "-", env_value ? env_value : "(unset)"); failures++; } } while (0)

// the environment of one check: at most one variable set
static const char* env_name = nullptr;
static const char* env_value = nullptr;
static const char* table_get(const char* name) { return (env_name && !strcmp(name, env_name)) ? env_value : nullptr; }

static const char* const ALL[] = { "SVO_DEBUG_MODE", "SVO_REST_PRIO", "SVO_TIMELINE", "SVO_HAM_FP4", "SVO_HAM_SPLITS", "SVO_COPY_PRIO", "SVO_RS_C0",
                                   "SVO_RC_SPLIT", "SVO_GN_NT", "SVO_DESC_KPW", "SVO_DESC_TL", "SVO_NMS_NT" };

// what an empty environment gives
static Knobs defaults()
{
    Knobs k; memset(&k, 0, sizeof(k));
    k.debug_mode = 0; k.rest_prio = 0; k.timeline = false; k.ham_fp4 = true; k.ham_splits = 0; k.copy_prio_normal = false; k.rs_c0 = 0;
    k.rc_split[0] = 1; k.rc_split[1] = 1; k.rc_split[2] = 1; k.gn_nt = 384; k.desc_kpw = 8; k.desc_tl = true; k.nms_nt = 0;
    return k;
}
static bool same(const Knobs& a, const Knobs& b)
{
    return a.debug_mode == b.debug_mode && a.rest_prio == b.rest_prio && a.timeline == b.timeline && a.ham_fp4 == b.ham_fp4 && a.ham_splits == b.ham_splits &&
           a.copy_prio_normal == b.copy_prio_normal && a.rs_c0 == b.rs_c0 && a.rc_split[0] == b.rc_split[0] && a.rc_split[1] == b.rc_split[1] &&
           a.rc_split[2] == b.rc_split[2] && a.gn_nt == b.gn_nt && a.desc_kpw == b.desc_kpw && a.desc_tl == b.desc_tl && a.nms_nt == b.nms_nt;
}
// name = value alone in the environment gives the defaults with `change` applied: the knob takes its value and no other knob moves
static void expect(const char* name, const char* value, const std::function<void(Knobs&)>& change)
{
    env_name = name; env_value = value;
    Knobs got; memset(&got, 0x5A, sizeof(got));               // knobs_read must write every field
    knobs_read(&got, table_get);
    Knobs want = defaults(); change(want);
    CHECK(same(got, want));
    env_name = nullptr; env_value = nullptr;
}
static void expect_int(const char* name, int Knobs::*field, const char* value, int want) { expect(name, value, [&](Knobs& k) { k.*field = want; }); }
static void expect_bool(const char* name, bool Knobs::*field, const char* value, bool want) { expect(name, value, [&](Knobs& k) { k.*field = want; }); }
static void expect_split(const char* value, int s0, int s1, int s2) { expect("SVO_RC_SPLIT", value, [&](Knobs& k) { k.rc_split[0] = s0; k.rc_split[1] = s1; k.rc_split[2] = s2; }); }

static void check_parsing()
{
    // nothing set, and every knob set to nothing a rule accepts as a number: "abc" and "" are 0 to atoi
    expect(nullptr, nullptr, [](Knobs&) {});
    static_assert(SVO_RANSAC_CHUNK0 == 32 && SVO_RANSAC_CHUNK1 == 160 && SVO_RANSAC_FEW == 320 && RC16_NSPLIT0 == 1, "the expectations below are written for these");

    // SVO_DEBUG_MODE: atoi, default 0, any integer
    const char* n = "SVO_DEBUG_MODE";
    expect_int(n, &Knobs::debug_mode, "", 0); expect_int(n, &Knobs::debug_mode, "0", 0); expect_int(n, &Knobs::debug_mode, "1", 1); expect_int(n, &Knobs::debug_mode, "abc", 0);
    expect_int(n, &Knobs::debug_mode, "53", 53); expect_int(n, &Knobs::debug_mode, "-3", -3); expect_int(n, &Knobs::debug_mode, "99", 99); expect_int(n, &Knobs::debug_mode, "12x", 12);
    // SVO_REST_PRIO: atoi & 3
    n = "SVO_REST_PRIO";
    expect_int(n, &Knobs::rest_prio, "", 0); expect_int(n, &Knobs::rest_prio, "0", 0); expect_int(n, &Knobs::rest_prio, "1", 1); expect_int(n, &Knobs::rest_prio, "abc", 0);
    expect_int(n, &Knobs::rest_prio, "3", 3); expect_int(n, &Knobs::rest_prio, "4", 0); expect_int(n, &Knobs::rest_prio, "5", 1); expect_int(n, &Knobs::rest_prio, "-1", 3);
    // SVO_TIMELINE: on iff the first character is '1'
    n = "SVO_TIMELINE";
    expect_bool(n, &Knobs::timeline, "", false); expect_bool(n, &Knobs::timeline, "0", false); expect_bool(n, &Knobs::timeline, "1", true); expect_bool(n, &Knobs::timeline, "abc", false);
    expect_bool(n, &Knobs::timeline, "10", true); expect_bool(n, &Knobs::timeline, "01", false); expect_bool(n, &Knobs::timeline, " 1", false);
    // SVO_HAM_FP4: the int8 form iff set and atoi == 0 -- so also for "" and "abc"
    n = "SVO_HAM_FP4";
    expect_bool(n, &Knobs::ham_fp4, "", false); expect_bool(n, &Knobs::ham_fp4, "0", false); expect_bool(n, &Knobs::ham_fp4, "1", true); expect_bool(n, &Knobs::ham_fp4, "abc", false);
    expect_bool(n, &Knobs::ham_fp4, "2", true); expect_bool(n, &Knobs::ham_fp4, "-1", true);
    // SVO_HAM_SPLITS: a value > 0 forces, anything else derives (0)
    n = "SVO_HAM_SPLITS";
    expect_int(n, &Knobs::ham_splits, "", 0); expect_int(n, &Knobs::ham_splits, "0", 0); expect_int(n, &Knobs::ham_splits, "1", 1); expect_int(n, &Knobs::ham_splits, "abc", 0);
    expect_int(n, &Knobs::ham_splits, "6", 6); expect_int(n, &Knobs::ham_splits, "-2", 0);
    // SVO_COPY_PRIO: normal priority iff set and atoi == 0
    n = "SVO_COPY_PRIO";
    expect_bool(n, &Knobs::copy_prio_normal, "", true); expect_bool(n, &Knobs::copy_prio_normal, "0", true); expect_bool(n, &Knobs::copy_prio_normal, "1", false);
    expect_bool(n, &Knobs::copy_prio_normal, "abc", true); expect_bool(n, &Knobs::copy_prio_normal, "-1", false);
    // SVO_RS_C0: one of the three chunk ends, else derive (0)
    n = "SVO_RS_C0";
    expect_int(n, &Knobs::rs_c0, "", 0); expect_int(n, &Knobs::rs_c0, "0", 0); expect_int(n, &Knobs::rs_c0, "1", 0); expect_int(n, &Knobs::rs_c0, "abc", 0);
    expect_int(n, &Knobs::rs_c0, "32", 32); expect_int(n, &Knobs::rs_c0, "160", 160); expect_int(n, &Knobs::rs_c0, "320", 320);
    expect_int(n, &Knobs::rs_c0, "33", 0); expect_int(n, &Knobs::rs_c0, "31", 0); expect_int(n, &Knobs::rs_c0, "321", 0); expect_int(n, &Knobs::rs_c0, "1000", 0);
    // SVO_RC_SPLIT: "%d,%d,%d"; entries not given repeat the last one given; each accepted iff 1..8, otherwise its default (1, 1, 1)
    expect_split("", 1, 1, 1); expect_split("0", 1, 1, 1); expect_split("1", 1, 1, 1); expect_split("abc", 1, 1, 1);
    expect_split("4", 4, 4, 4); expect_split("4,2", 4, 2, 2); expect_split("4,2,3", 4, 2, 3); expect_split("9,2", 1, 2, 2);
    expect_split(",", 1, 1, 1); expect_split("4,,3", 4, 4, 4);
    expect_split("8", 8, 8, 8); expect_split("9", 1, 1, 1); expect_split("-1", 1, 1, 1);
    expect_split("0,8,9", 1, 8, 1); expect_split("8,0,1", 8, 1, 1); expect_split("2,9", 2, 1, 1); expect_split("2,3,0", 2, 3, 1); expect_split("5,4,3,2", 5, 4, 3);
    // SVO_GN_NT: 256 / 384 / 512, else 384
    n = "SVO_GN_NT";
    expect_int(n, &Knobs::gn_nt, "", 384); expect_int(n, &Knobs::gn_nt, "0", 384); expect_int(n, &Knobs::gn_nt, "1", 384); expect_int(n, &Knobs::gn_nt, "abc", 384);
    expect_int(n, &Knobs::gn_nt, "255", 384); expect_int(n, &Knobs::gn_nt, "256", 256); expect_int(n, &Knobs::gn_nt, "257", 384); expect_int(n, &Knobs::gn_nt, "384", 384);
    expect_int(n, &Knobs::gn_nt, "512", 512); expect_int(n, &Knobs::gn_nt, "513", 384); expect_int(n, &Knobs::gn_nt, "1024", 384);
    // SVO_DESC_KPW: 1..64, else 8
    n = "SVO_DESC_KPW";
    expect_int(n, &Knobs::desc_kpw, "", 8); expect_int(n, &Knobs::desc_kpw, "0", 8); expect_int(n, &Knobs::desc_kpw, "1", 1); expect_int(n, &Knobs::desc_kpw, "abc", 8);
    expect_int(n, &Knobs::desc_kpw, "64", 64); expect_int(n, &Knobs::desc_kpw, "65", 8); expect_int(n, &Knobs::desc_kpw, "-1", 8); expect_int(n, &Knobs::desc_kpw, "16", 16);
    // SVO_DESC_TL: registers iff set and atoi == 0
    n = "SVO_DESC_TL";
    expect_bool(n, &Knobs::desc_tl, "", false); expect_bool(n, &Knobs::desc_tl, "0", false); expect_bool(n, &Knobs::desc_tl, "1", true); expect_bool(n, &Knobs::desc_tl, "abc", false);
    // SVO_NMS_NT: atoi, as it is (the launcher looks for 512)
    n = "SVO_NMS_NT";
    expect_int(n, &Knobs::nms_nt, "", 0); expect_int(n, &Knobs::nms_nt, "0", 0); expect_int(n, &Knobs::nms_nt, "1", 1); expect_int(n, &Knobs::nms_nt, "abc", 0);
    expect_int(n, &Knobs::nms_nt, "512", 512); expect_int(n, &Knobs::nms_nt, "1024", 1024); expect_int(n, &Knobs::nms_nt, "511", 511);

    // every name knobs_read asks for is one of the twelve, and each of the twelve is asked for
    static int unknown = 0; static bool asked[sizeof(ALL) / sizeof(ALL[0])];
    Knobs k;
    knobs_read(&k, [](const char* name) -> const char* {
        bool known = false;
        for (size_t i = 0; i < sizeof(ALL) / sizeof(ALL[0]); i++) if (!strcmp(ALL[i], name)) { known = true; asked[i] = true; }
        if (!known) unknown++;
        return nullptr; });
    CHECK(unknown == 0 && same(k, defaults()));
    for (bool a : asked) CHECK(a);
}

// the request for a kernel form that only the A/B library holds
static void check_ab_request()
{
    Knobs k = defaults();
    CHECK(!svo_ab_form_requested(k));
    k.ham_fp4 = false; CHECK(svo_ab_form_requested(k));
    k = defaults(); k.debug_mode = 14; CHECK(svo_ab_form_requested(k));
    k.debug_mode = 52; CHECK(svo_ab_form_requested(k));
    for (int m : { 0, 13, 16, 50, 51, 53, 54, 22, 99, -14 }) { k.debug_mode = m; CHECK(!svo_ab_form_requested(k)); }
}

// the three groups partition exactly these numbers; every other integer of 0 .. 99 (and a few outside) is in none
static void check_mode_groups()
{
    bool form[100] = {}, ab[100] = {}, abl[100] = {};
    for (int m : { 8, 9, 12, 13, 16, 50, 51, 53, 54 }) form[m] = true;
    for (int m : { 14, 52 }) ab[m] = true;
    for (int m = 1; m <= 7; m++) abl[m] = true;
    for (int m : { 10, 11, 31 }) abl[m] = true;
    for (int m = 21; m <= 26; m++) abl[m] = true;
    for (int m = 41; m <= 46; m++) abl[m] = true;
    for (int m = 60; m <= 67; m++) abl[m] = true;
    for (int m = 0; m < 100; m++) {
        if (debug_mode_is_form(m) != form[m] || debug_mode_is_ab_form(m) != ab[m] || debug_mode_is_ablation(m) != abl[m]) {
            fprintf(stderr, "mode %d: form %d (want %d), A/B form %d (want %d), ablation %d (want %d)\n", m, debug_mode_is_form(m), form[m], debug_mode_is_ab_form(m), ab[m], debug_mode_is_ablation(m), abl[m]);
            failures++;
        }
        CHECK((int)form[m] + (int)ab[m] + (int)abl[m] <= 1);
        CHECK(debug_mode_gn_loop_ablation(m) == (m >= 60 && m <= 63));
    }
    for (int m : { -1, -8, 100, 108, 1 << 30 }) CHECK(!debug_mode_is_form(m) && !debug_mode_is_ab_form(m) && !debug_mode_is_ablation(m) && !debug_mode_gn_loop_ablation(m));
    // the numbers are the knob's public face
    static_assert(DBG_NONE == 0 && DBG_FAST_STOP_STAGED == 1 && DBG_FAST_STOP_COMPACTED == 2 && DBG_FAST_STOP_SCORED == 3 && DBG_FAST_NO_PUBLISH == 4 &&
                  DBG_RESIZE_NO_STAGING == 5 && DBG_RESIZE_NO_BLEND == 6 && DBG_RESIZE_NO_STORE == 7 && DBG_LINEAR_TILES == 8 && DBG_DESCRIBE_BEFORE_NMS == 9 &&
                  DBG_GN_STOP_SETUP == 10 && DBG_GN_ONE_ITER == 11 && DBG_NO_SPEC_FAST_TH == 12 && DBG_RC_REPLAY_ALL == 13 && DBG_RC_VALU16 == 14 &&
                  DBG_RC_NO_EARLY_STOP == 16 && DBG_NMS_STOP_KEYS == 21 && DBG_NMS_STOP_SORT == 22 && DBG_NMS_STOP_GRID == 23 && DBG_NMS_STOP_ACCEPT == 24 &&
                  DBG_NMS_STOP_ROWSORT == 25 && DBG_NMS_STOP_CELLS == 26 && DBG_SELECT_STOP_HIST == 31 && DBG_SSORT_STOP_RANGE == 41 &&
                  DBG_SSORT_STOP_BUCKETS == 42 && DBG_SSORT_STOP_OFFSETS == 43 && DBG_SSORT_STOP_SCATTER == 44 && DBG_SSORT_STOP_RANK == 45 &&
                  DBG_DESCRIBE_NO_TRIG == 46 && DBG_RH_LANES16 == 50 && DBG_RH_THREAD == 51 && DBG_RC_MFMA4 == 52 && DBG_RC_MFMA16 == 53 &&
                  DBG_RC_MFMA16_REPLAY == 54 && DBG_GN_NO_TRACK_LOOP == 60 && DBG_GN_NO_SOLVE == 61 && DBG_GN_NO_ROT_UPDATE == 62 &&
                  DBG_GN_NO_SOLVE_NO_ROT == 63 && DBG_GN_STOP_GATHER == 64 && DBG_GN_STOP_SORT == 65 && DBG_GN_STOP_MASK == 66 && DBG_GN_STOP_TRIANGULATE == 67,
                  "the numeric values of SVO_DEBUG_MODE never change");
}

int main()
{
    check_parsing();
    check_ab_request();
    check_mode_groups();
    if (failures) { fprintf(stderr, "%d check(s) failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
