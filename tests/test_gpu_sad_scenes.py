"""smSAD (k_match_lr_rbr<true>) and ifmSAD (k_track_win<true>) on the hand-built windows of tests/sad_scenes.py: SADs on the thresholds,
ties, 1-to-1 claims that differ above bit 8, keypoints on the border rule, row ranges on their roundings, the search windows on
their clamps, flagged pairings, octave 1 of a two-octave frame, indices from 8192 on.  tests/test_sad_scenes_cpu.py asserts on the
reference walks alone that the scenes reach those rules and that each rule, broken, changes its scene.

The lists are put, the windows gathered from the painted images (svo_gather_windows), one stage is run on them.  Everything is
compared bit for bit with tests/sad_ref.py -- every value is an integer or an integer-valued float -- and the status word is 0.
Every test needs a real MI355X: `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
import sad_ref as S                                             # noqa: E402
import sad_scenes as SS                                         # noqa: E402
from oracle import oracle as O                                  # noqa: E402
from test_gpu_put_windows import np_windows                     # noqa: E402

pytestmark = pytest.mark.gpu


def base():
    return S.photo_params(hip.default_params(), orb_nfeats=300)


def context(n_lanes, max_kps=512, max_octaves=1):
    return hip.Context(n_lanes=n_lanes, max_w=SS.W, max_h=SS.H, max_kps=max_kps, max_cand=1 << 14, max_octaves=max_octaves)


def check_windows(ctx, lane, which, side, img, k, tag, octave=0):
    """the gathered windows and flags of one list against the painted image"""
    win, flag = ctx.windows(lane, which, side, octave)
    w0, f0 = np_windows(img, k)
    assert len(flag) == len(k) and (flag == f0).all(), (tag, "flags", np.flatnonzero(flag != f0)[:8])
    assert (f0 == [SS.is_flagged(x, y, img.shape[1], img.shape[0]) for x, y in zip(k["x"], k["y"])]).all(), (tag, "the flag rule")
    assert (win[f0 == 0] == w0[f0 == 0]).all(), (tag, "windows")


def lane_state(ctx, lane, whiches=(0, 1), n_oct=1):
    """everything a call must leave alone in an idle lane (whiches: the slots that hold a frame)"""
    out = []
    for o in range(n_oct):
        for which in whiches:
            for side in (0, 1):
                k = ctx.keypoints(lane, which, side, o)[0]
                out += [k.tobytes(), ctx.row_index(lane, which, side, o).tobytes()]
                if len(k):
                    out += [a.tobytes() for a in ctx.windows(lane, which, side, o)]
            out += [ctx.matches(lane, which, o).tobytes(), ctx.matches_row_index(lane, which, o).tobytes()]
        out.append(ctx.tracked(lane, o).tobytes())
    return out + [bytes(ctx.result(lane)), ctx.status_word(lane)]


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------------------------------
def put_stereo(ctx, lane, s, which=0):
    for side, k in enumerate((s["kl"], s["kr"])):
        ctx.put_features(lane, which, side, k, None, s["W"], s["H"])
        assert list(ctx.row_index(lane, which, side)[:s["H"]]) == list(SS.features_row_index(k, s["H"])), ("row table of a put list", lane, side)


def reference_stereo(s, p):
    m = S.match_lr_sad(s["imgs"][0], s["imgs"][1], s["kl"], s["kr"], SS.features_row_index(s["kl"], s["H"]), SS.features_row_index(s["kr"], s["H"]),
                       p.sad_max_distance, p.max_y_diff, p.enable_robust_1to1_match, p.minimum_ORB_response if p.detect_method == 0 else 0.0)
    return m, S.matches_row_index(m, s["kl"], s["H"])


def check_stereo(tag, ctx, lane, s, p):
    m, ri = reference_stereo(s, p)
    got = ctx.matches(lane, 0)
    assert got.tobytes() == m.tobytes(), (tag, "pairings", got.tolist()[:12], m.tolist()[:12])
    assert list(ctx.matches_row_index(lane, 0)[:s["H"] + 1]) == list(ri), (tag, "pairings' row table")
    assert int(ctx.result(lane).stereo_matches[0]) == len(m), (tag, "stereo_matches")
    assert ctx.status_word(lane) == 0, (tag, "status word", ctx.status_word(lane))
    return len(m)


def merged(defaults, variants):
    out = []
    for v in variants:
        v = dict(defaults, **v)
        if v not in out:
            out.append(v)
    return out


def test_stage3_scenes_side_by_side():
    """the seven one-octave stage-3 scenes as the lanes of one context, under the union of their variants and both assignment rules;
    an eighth lane is matched once and then left out by the mask: its lists, windows and pairings stay what they were"""
    names = SS.stereo_names()
    scenes = [SS.scene(nm) for nm in names]
    n, active = len(names), list(range(len(names)))
    variants = merged(SS.STEREO_DEFAULTS, SS.all_variants(names))
    assert n == 7 and len(variants) == 11
    ctx = context(n + 1)
    ctx.set_params(SS.stereo_params(base(), {}, 1))
    put_stereo(ctx, n, scenes[3])
    for lane, s in enumerate(scenes):
        put_stereo(ctx, lane, s)
    ctx.gather_windows([s["imgs"] for s in scenes] + [scenes[3]["imgs"]], which=0)
    ctx.run_stages(hip.RUN_MATCH)
    failed, total, pairings = [], 0, 0
    try:
        assert check_stereo("the lane to be idle", ctx, n, scenes[3], SS.stereo_params(base(), {}, 1)) == 7
    except AssertionError as e:
        failed.append(("the lane to be idle", str(e.args[0])[:400]))
    idle = lane_state(ctx, n, (0,))
    for v in variants:
        for robust in (0, 1):
            p = SS.stereo_params(base(), v, robust)
            ctx.set_params(p)
            for lane, s in enumerate(scenes):                                     # (set_params clears the geometry: the lists are put again,
                put_stereo(ctx, lane, s)                                          # and put lists come without windows)
            ctx.gather_windows([s["imgs"] for s in scenes] + [None], which=0, active=active)
            ctx.run_stages(hip.RUN_MATCH, active=active)
            for lane, s in enumerate(scenes):
                total += 1
                try:
                    if v is variants[0] and robust == 0:
                        for side in (0, 1):
                            check_windows(ctx, lane, 0, side, s["imgs"][side], (s["kl"], s["kr"])[side], (names[lane], side))
                    pairings += check_stereo((names[lane], v, robust), ctx, lane, s, p)
                except AssertionError as e:
                    failed.append((names[lane], str(e.args[0])[:400]))
    assert lane_state(ctx, n, (0,)) == idle, "the idle lane"
    ctx.close()
    assert total == 7 * 22 and not failed and pairings == 584, (sorted({nm for nm, _ in failed}), len(failed), failed[:12])


def test_stage3_large_indices():
    """8200 right keypoints ahead of the planted ones: index >= 8192 and distance 16320 in one left_pick word"""
    s = SS.scene("big_index")[0]
    ctx = context(1, max_kps=16384)
    for robust in (0, 1):
        p = SS.stereo_params(base(), s["variants"][0], robust)
        ctx.set_params(p)
        put_stereo(ctx, 0, s)
        ctx.gather_windows([s["imgs"]], which=0)
        ctx.run_stages(hip.RUN_MATCH)
        assert check_stereo(("big_index", robust), ctx, 0, s, p) == 2
        m = ctx.matches(0, 0)
        assert m["trainIdx"].min() >= 8192 and m["distance"].max() == 16320.0
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------------------------------------------------------------------
def put_track(ctx, lane, s, octave=0, w=None, h=None):
    """both frames of a scene, previous (which = 1) then current (which = 0)"""
    w, h = (s["W"], s["H"]) if w is None else (w, h)
    for which, (kl, kr, m, ri) in ((1, (s["pkl"], s["pkr"], s["pm"], s["pri"])), (0, (s["ckl"], s["ckr"], s["cm"], s["cri"]))):
        ctx.put_features(lane, which, 0, kl, None, w, h, octave=octave)
        ctx.put_features(lane, which, 1, kr, None, w, h, octave=octave)
        ctx.put_matches(lane, which, m, octave=octave)
        assert list(ctx.matches_row_index(lane, which, octave)[:s["H"] + 1]) == list(ri), ("row table of put pairings", lane, which, octave)


def reference_track(s, p):
    pf, cf = SS.frames(s)
    pot = S.track_sad(pf, cf, p.ifm_win_w, p.ifm_win_h, p.ifm_sad_max_distance, skip_flagged=True)
    return S.filter_candidates(O, pf, cf, pot)


def check_track(tag, ctx, lane, want):
    tracked, stats = want
    got, got_stats = ctx.tracked(lane), [int(v) for v in ctx.result(lane).track_stats[:8]]
    assert got.tobytes() == tracked.tobytes(), (tag, "tracked pairs", got.tolist()[:12], tracked.tolist()[:12])
    assert got_stats == [int(v) for v in stats], (tag, "stage-4 counters", got_stats, [int(v) for v in stats])
    assert ctx.status_word(lane) == 0, (tag, "status word", ctx.status_word(lane))
    return len(tracked)


def gather_track(ctx, scenes, idle_lanes=0, active=None):
    ctx.gather_windows([s["pimgs"] for s in scenes] + [None] * idle_lanes, which=1, active=active)
    ctx.gather_windows([s["cimgs"] for s in scenes] + [None] * idle_lanes, which=0, active=active)


def test_stage4_scenes_side_by_side():
    """the five one-octave stage-4 scenes as the lanes of one context, under the union of their variants; a sixth lane is tracked once and
    then left out by the mask"""
    names = SS.track_names()
    scenes = [SS.scene(nm) for nm in names]
    n, active = len(names), list(range(len(names)))
    variants = merged(SS.TRACK_DEFAULTS, SS.all_variants(names))
    assert n == 5 and len(variants) == 6
    ctx = context(n + 1)
    p = SS.track_params(base(), {})
    ctx.set_params(p)
    for lane, s in enumerate(scenes + [scenes[0]]):
        put_track(ctx, lane, s)
    gather_track(ctx, scenes + [scenes[0]])
    ctx.run_stages(hip.RUN_TRACK)
    failed, total, pairs = [], 0, 0
    try:
        assert check_track("the lane to be idle", ctx, n, reference_track(scenes[0], p)) == 3
    except AssertionError as e:
        failed.append(("the lane to be idle", str(e.args[0])[:400]))
    idle = lane_state(ctx, n)
    for v in variants:
        p = SS.track_params(base(), v)
        ctx.set_params(p)
        for lane, s in enumerate(scenes):
            put_track(ctx, lane, s)
        gather_track(ctx, scenes, 1, active)
        ctx.run_stages(hip.RUN_TRACK, active=active)
        for lane, s in enumerate(scenes):
            total += 1
            try:
                if v is variants[0]:
                    for which, imgs, ks in ((1, s["pimgs"], (s["pkl"], s["pkr"])), (0, s["cimgs"], (s["ckl"], s["ckr"]))):
                        for side in (0, 1):
                            check_windows(ctx, lane, which, side, imgs[side], ks[side], (names[lane], which, side))
                pairs += check_track((names[lane], v), ctx, lane, reference_track(s, p))
            except AssertionError as e:
                failed.append((names[lane], str(e.args[0])[:400]))
    assert lane_state(ctx, n) == idle, "the idle lane"
    ctx.close()
    assert total == 5 * 6 and not failed and pairs == 109, (sorted({nm for nm, _ in failed}), len(failed), failed[:12])


def test_one_scene_alone_previous_then_current():
    """trk_gates alone in a one-lane context: the previous frame is put and gathered at which = 1, then the current one at which = 0; stage
    4 on the two, then stage 3 on the current frame's lists and windows"""
    s = SS.scene("trk_gates")
    ctx = context(1)
    for v in s["variants"]:
        p = SS.track_params(base(), v)
        ctx.set_params(p)
        put_track(ctx, 0, s)
        ctx.gather_windows([s["pimgs"]], which=1)
        ctx.gather_windows([s["cimgs"]], which=0)
        ctx.run_stages(hip.RUN_TRACK)
        assert check_track(("trk_gates alone", v), ctx, 0, reference_track(s, p)) == len(s["want"](v))
    q = SS.stereo_params(base(), dict(sad_max_distance=-1), 1)
    ctx.set_params(q)
    cur = dict(kl=s["ckl"], kr=s["ckr"], imgs=s["cimgs"], W=s["W"], H=s["H"])
    put_stereo(ctx, 0, cur)
    ctx.gather_windows([s["cimgs"]], which=0)
    ctx.run_stages(hip.RUN_MATCH)
    assert check_stereo("trk_gates' current frame", ctx, 0, cur, q) >= 3
    ctx.close()


def test_two_octaves():
    """dmFASTER geometry, two octaves: the windows of octave 1 come from the half-size image, and its borders are its own"""
    s0, s1, imgs0 = SS.scene("trk_octaves")
    ctx = context(1, max_octaves=2)
    for i, v in enumerate(s1["variants"]):
        p = F.faster_params(hip.default_params(), orb_nfeats=300, n_oct=2)
        p.ifm_sad_max_distance, p.ifm_win_w, p.ifm_win_h = v["ifm_sad_max_distance"], SS.TRACK_DEFAULTS["ifm_win_w"], SS.TRACK_DEFAULTS["ifm_win_h"]
        ctx.set_params(p)
        put_track(ctx, 0, s0, 0, SS.W, SS.H); put_track(ctx, 0, s1, 1, SS.W, SS.H)
        ctx.gather_windows([tuple(imgs0[:2])], which=1)
        ctx.gather_windows([tuple(imgs0[2:])], which=0)
        if i == 0:
            for which, imgs, ks in ((1, s1["pimgs"], (s1["pkl"], s1["pkr"])), (0, s1["cimgs"], (s1["ckl"], s1["ckr"]))):
                for side in (0, 1):
                    check_windows(ctx, 0, which, side, imgs[side], ks[side], ("octave 1", which, side), octave=1)
            assert (ctx.level(0, 0, 1) == s1["cimgs"][0]).all() and (ctx.level(0, 1, 1) == s1["cimgs"][1]).all()
        ctx.run_stages(hip.RUN_TRACK)
        want = [reference_track(s, p) for s in (s0, s1)]
        for o in (0, 1):
            assert ctx.tracked(0, o).tobytes() == want[o][0].tobytes(), (v, "tracked pairs of octave", o, ctx.tracked(0, o).tolist(), want[o][0].tolist())
        assert [(int(a), int(b)) for a, b in want[1][0].tolist()] == s1["want"](v)
        stats = [int(a) + int(b) for a, b in zip(want[0][1], want[1][1])]
        assert [int(x) for x in ctx.result(0).track_stats[:8]] == stats, (v, list(ctx.result(0).track_stats[:8]), stats)
        assert ctx.status_word(0) == 0
    ctx.close()


def test_stage4_large_indices():
    """8200 previous pairings ahead of the planted ones: (sum << 16 | index) with the sum 32640 and an index >= 8192"""
    s = SS.scene("big_index")[1]
    p = SS.track_params(base(), s["variants"][0])
    ctx = context(1, max_kps=16384)
    ctx.set_params(p)
    put_track(ctx, 0, s)
    gather_track(ctx, [s])
    ctx.run_stages(hip.RUN_TRACK)
    assert check_track("big_index", ctx, 0, reference_track(s, p)) == 2
    assert ctx.tracked(0)["first"].min() >= 8192
    ctx.close()
