"""dmFASTER's dynamic threshold on the HIP path (svo_set_dyn_fast_threshold) against the literal walk of tests/faster_dyn_ref.py.

Everything is compared bit for bit: the thresholds each image was detected at, the corner counts, the threshold left for the next
frame, and -- downstream -- the keypoint lists, row tables and pairings of every octave.  (Poses, where a test runs stage 5, under the
tolerances of test_gpu_sad.assert_same_as_reference, as every dmFASTER test does.)  160 x 120 frames, three octaves, 3 - 8 frames.
tests/test_faster_dyn_cpu.py holds the scenes and pins, from the reference alone, that each one reaches its case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_dyn_ref as D                                      # noqa: E402
import faster_ref as F                                          # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_faster_dyn_cpu import H, KLT_WIN, N_OCT, W, overflow_max_cand, params, scene, scene_walk      # noqa: E402
from test_gpu_faster import assert_same_lists, assert_same_pairings, snapshot       # noqa: E402
from test_gpu_frame_layouts import lay_out                      # noqa: E402
from test_gpu_parity import O                                   # noqa: E402
from test_gpu_sad import assert_same_as_reference, assert_same_snapshot             # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_UNSUPPORTED, SVO_ERR_STATE = -2, -3, -6
ST_CAND_OVERFLOW = 1
DETECT_MATCH = hip.RUN_DETECT | hip.RUN_MATCH
CAM = StereoCamera.simple(400.0 * W / 640.0, W / 2.0, H / 2.0, 0.12, W, H)
KW = dict(max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, max_octaves=N_OCT)


def context(p, target, n_lanes=1, **kw):
    ctx = hip.Context(n_lanes=n_lanes, **dict(KW, **kw))
    ctx.set_params(p); ctx.set_camera(CAM)
    ctx.set_dyn_fast_threshold(True, target)
    return ctx


def assert_same_stats(ctx, lane, stats, frame, tag, n_oct=N_OCT):
    got = ctx.faster_stats(lane).as_dict(n_oct)
    want = dict(stats, frame=frame)
    assert got == want, (tag, got, want)


def lists_bytes(ctx, lane, n_oct=N_OCT):
    return tuple(ctx.keypoints(lane, 0, side, o)[0].tobytes() + ctx.row_index(lane, 0, side, o).tobytes() for o in range(n_oct) for side in (0, 1))


def run_scene(name, flags=DETECT_MATCH):
    """a scene through a one-lane context, every frame held to the reference: thresholds, counts, lists, row tables, pairings"""
    frames, p, target = scene(name)
    ctx = context(p, target)
    for t, ((l, r), (feats, stats)) in enumerate(zip(frames, scene_walk(name))):
        ctx.process_host([(l, r)], flags)
        res = ctx.result(0)
        tag = "%s t=%d" % (name, t)
        assert ctx.status_word(0) == 0 and res.n_octaves == N_OCT, tag
        assert_same_stats(ctx, 0, stats, t + 1, tag)
        assert_same_lists(ctx, 0, feats, tag, res)
        assert_same_pairings(ctx, 0, feats, p, tag, res)
    return ctx


def test_rising():
    """a tiny target: every call finds too many corners, so the thresholds go T, T+1, T+2, ... -- the right image of a frame already
    one above its left image.  Then the same on one octave through all five stages against the composed SAD reference"""
    run_scene("rising").close()
    frames, p3, target = scene("rising")
    p = params(p3.initial_FAST_threshold, n_oct=1)
    p.ifm_win_w = p.ifm_win_h = 24; p.sad_max_distance = p.ifm_sad_max_distance = 800       # (so that these small dense frames track: valid poses from the second frame on)
    ctx = context(p, target)
    st = S.SadStream(O(), p, CAM)
    for t, ((l, r), (feats, stats)) in enumerate(zip(frames[:4], D.walk(frames[:4], p, target, KLT_WIN))):
        assert stats["used_left"] == [5 + 2 * t] and stats["used_right"] == [6 + 2 * t]
        ctx.process_host([(l, r)])
        res = ctx.result(0)
        assert_same_stats(ctx, 0, stats, t + 1, "rising, one octave t=%d" % t, 1)
        assert_same_lists(ctx, 0, feats, "rising, one octave t=%d" % t, res)
        o = st.step((l, r), feats[0][0], feats[0][1], feats[0][2], feats[0][3])
        assert len(o["matches"]) >= 150 and (not t or (o["valid"] and len(o["tracked"]) >= 8)), (t, len(o["matches"]), len(o["tracked"]))
        assert_same_as_reference(ctx, 0, res, o, "rising, one octave t=%d" % t)
    ctx.close()


def test_falling_to_the_floor():
    """target 1.0: 3, 2, 1, 1, ...; and initial_FAST_threshold 0 is used once, then 1"""
    run_scene("falling").close()
    run_scene("falling_from_0").close()


def test_settling():
    """target 0.085: the thresholds move, enter the band at (24, 26, 20) and stop.  From then on every octave's lists are those of a
    feature-off context whose constant threshold is that octave's"""
    ctx = run_scene("settling")
    settled = list(ctx.faster_stats(0).next)[:N_OCT]
    ctx.close()
    frames, p, target = scene("settling")
    walk = scene_walk("settling")
    for T in sorted(set(settled)):
        off = hip.Context(n_lanes=1, **KW)
        off.set_params(params(T)); off.set_camera(CAM)
        for t in range(len(frames) - 4, len(frames)):
            off.process_host([frames[t]], hip.RUN_DETECT)
            for o in (o for o in range(N_OCT) if settled[o] == T):
                f = walk[t][0][o]
                for side in (0, 1):
                    k = off.keypoints(0, 0, side, o)[0]
                    assert len(k) >= 30 and k.tobytes() == f[side].tobytes(), ("feature off at", T, t, o, side)
                    assert (off.row_index(0, 0, side, o) == f[2 + side]).all()
        off.close()


def test_saturation():
    """0 / 255 blocks at initial 254: octave 0 oscillates 254 <-> 255; at 255 the right lists are empty, nothing pairs, and the frames
    complete with voecFirstIteration, then the bad-tracking code, as the composed reference says (one octave, all five stages)"""
    run_scene("saturated").close()
    frames, p3, target = scene("saturated")
    p = params(254, n_oct=1)
    ctx = context(p, target)
    st = S.SadStream(O(), p, CAM)
    for t, ((l, r), (feats, stats)) in enumerate(zip(frames[:3], D.walk(frames[:3], p, target, KLT_WIN))):
        assert (stats["used_left"], stats["used_right"], stats["next"]) == ([254], [255], [254]) and len(feats[0][1]) == 0
        ctx.process_host([(l, r)])
        res = ctx.result(0)
        assert_same_stats(ctx, 0, stats, t + 1, "saturated, one octave t=%d" % t, 1)
        assert_same_lists(ctx, 0, feats, "saturated, one octave t=%d" % t, res)
        o = st.step((l, r), feats[0][0], feats[0][1], feats[0][2], feats[0][3])
        assert not o["valid"] and len(o["matches"]) == 0
        assert_same_as_reference(ctx, 0, res, o, "saturated, one octave t=%d" % t)
        assert res.error_code == (4 if t == 0 else 5), (t, res.error_code)
    ctx.close()


def test_lanes_move_independently_and_idle_lanes_keep_theirs():
    """flat / world / noise in three lanes; lane 1 sits frames 2 and 3 out.  Every lane equals the reference walked over the frames
    that lane took part in, and lane 1 equals a one-lane context fed those frames"""
    names = ("lane_flat", "lane_world", "lane_noise")
    frames = [scene(n)[0] for n in names]
    p, target = scene(names[0])[1], scene(names[0])[2]
    took = [list(range(6)), [0, 1, 4, 5], list(range(6))]
    walks = [D.walk([frames[g][t] for t in took[g]], p, target, KLT_WIN) for g in range(3)]
    ctx = context(p, target, n_lanes=3)
    seen = [0, 0, 0]
    kept = None
    mine = []
    for t in range(6):
        act = [g for g in range(3) if t in took[g]]
        ctx.process_host([frames[g][t] if g in act else None for g in range(3)], hip.RUN_DETECT, active=act)
        for g in range(3):
            if g in act:
                feats, stats = walks[g][seen[g]]
                seen[g] += 1
                assert_same_stats(ctx, g, stats, seen[g], (names[g], t))
                assert_same_lists(ctx, g, feats, (names[g], t))
                if g == 1:
                    mine.append((ctx.faster_stats(1).as_dict(), lists_bytes(ctx, 1)))
                    kept = mine[-1]
            else:
                assert (ctx.faster_stats(g).as_dict(), lists_bytes(ctx, g)) == kept, ("idle lane", g, t)
    after = [list(ctx.faster_stats(g).next)[:N_OCT] for g in range(3)]
    assert len({tuple(a) for a in after}) == 3, after
    ctx.close()
    alone = context(p, target)
    for i, t in enumerate(took[1]):
        alone.process_host([frames[1][t]], hip.RUN_DETECT)
        assert (alone.faster_stats(0).as_dict(), lists_bytes(alone, 0)) == mine[i], ("lane 1 alone", t)
    alone.close()


def test_state_rules():
    frames, p, target = scene("rising")
    walk = scene_walk("rising")
    ctx = hip.Context(n_lanes=2, **KW)
    ctx.set_params(p); ctx.set_camera(CAM)
    L = ctx.L
    st = hip.FasterStats()
    # off by default; the getter refuses; bad targets are refused and nothing moves
    assert ctx.dyn_fast_threshold() == (False, 10. / 1000.)
    assert L.svo_get_faster_stats(ctx.h, 0, C.byref(st)) == SVO_ERR_STATE and b"svo_set_dyn_fast_threshold" in L.svo_last_error(ctx.h)
    for bad in (-1e-9, float("nan"), float("inf"), -float("inf")):
        assert L.svo_set_dyn_fast_threshold(ctx.h, 1, bad) == SVO_ERR_ARG and b"target_feats_per_pixel" in L.svo_last_error(ctx.h), bad
        assert ctx.dyn_fast_threshold() == (False, 10. / 1000.)
    # while off: the constant threshold, as ever
    ctx.process_host([frames[0]] * 2, hip.RUN_DETECT)
    assert_same_lists(ctx, 1, F.faster_features(frames[0][0], frames[0][1], p, KLT_WIN), "off")
    # on: every lane starts at initial_FAST_threshold
    ctx.set_dyn_fast_threshold(True, target)
    assert ctx.dyn_fast_threshold() == (True, target)
    fresh = dict(next=[5] * 3, used_left=[0] * 3, used_right=[0] * 3, corners_left=[0] * 3, corners_right=[0] * 3, frame=0)
    assert ctx.faster_stats(0).as_dict(3) == ctx.faster_stats(1).as_dict(3) == fresh and list(ctx.faster_stats(0).next) == [5] * 4
    assert L.svo_get_faster_stats(ctx.h, 2, C.byref(st)) == SVO_ERR_ARG and L.svo_get_faster_stats(ctx.h, 0, None) == SVO_ERR_ARG
    for t in range(2):
        ctx.process_host([frames[t]] * 2, hip.RUN_DETECT)
    for g in (0, 1):
        assert_same_stats(ctx, g, walk[1][1], 2, "two frames")
    moved = ctx.faster_stats(0).as_dict(3)
    assert moved["next"] == [9] * 3
    # a bad target while on: refused, the values in force stay
    assert L.svo_set_dyn_fast_threshold(ctx.h, 1, -1.0) == SVO_ERR_ARG and ctx.dyn_fast_threshold() == (True, target)
    # a call refused before anything is enqueued moves nothing
    fr = (hip.Frame * 2)()
    assert L.svo_process(ctx.h, fr, hip.RUN_DETECT) == SVO_ERR_ARG                       # NULL images
    assert ctx.faster_stats(0).as_dict(3) == moved
    # svo_reset(lane): that lane alone starts over
    ctx.reset(1)
    assert ctx.faster_stats(1).as_dict(3) == fresh and ctx.faster_stats(0).as_dict(3) == moved
    # svo_set_params that changes initial_FAST_threshold alone: nothing moves; a new target alone: nothing moves
    q = p.copy(); q.initial_FAST_threshold = 40
    ctx.set_params(q)
    assert ctx.faster_stats(0).as_dict(3) == moved and ctx.faster_stats(1).as_dict(3) == fresh
    ctx.set_dyn_fast_threshold(True, 0.5)
    assert ctx.faster_stats(0).as_dict(3) == moved and ctx.dyn_fast_threshold() == (True, 0.5)
    # ... one that changes the octave count: every lane starts over, at the initial threshold now in force
    q.nOctaves = 2
    ctx.set_params(q)
    for g in (0, 1):
        assert ctx.faster_stats(g).as_dict(3) == dict(fresh, next=[40] * 3), g
    ctx.set_dyn_fast_threshold(True, target)
    ctx.process_host([frames[0]] * 2, hip.RUN_DETECT)
    feats, stats = D.walk(frames[:1], q, target, KLT_WIN)[0]
    assert stats["used_left"] == [40, 40] and stats["next"] == [42, 42]
    assert_same_stats(ctx, 0, stats, 1, "two octaves", 2)
    assert_same_lists(ctx, 0, feats, "two octaves")
    assert list(ctx.faster_stats(0).next)[2:] == [40, 40]                                 # octaves the parameters do not use stay as initialised
    # on -> off -> on: starts over; while off the getter refuses and the detector is the constant one
    ctx.set_dyn_fast_threshold(False, target)
    assert L.svo_get_faster_stats(ctx.h, 0, C.byref(st)) == SVO_ERR_STATE
    ctx.process_host([frames[1]] * 2, hip.RUN_DETECT)
    assert_same_lists(ctx, 0, F.faster_features(frames[1][0], frames[1][1], q, KLT_WIN), "off again")
    ctx.set_dyn_fast_threshold(True, target)
    assert ctx.faster_stats(0).as_dict(2) == dict(next=[40] * 2, used_left=[0] * 2, used_right=[0] * 2, corners_left=[0] * 2, corners_right=[0] * 2, frame=0)
    # entry points that do not detect never move it
    ctx.process_host([frames[0]] * 2, DETECT_MATCH)
    one = ctx.faster_stats(0).as_dict(2)
    ctx.gather_windows([frames[0]] * 2)
    ctx.run_stages(hip.RUN_MATCH)
    assert ctx.faster_stats(0).as_dict(2) == one and one["frame"] == 1
    ctx.close()
    # inert under another detector: accepted, nothing moves
    orb = hip.Context(n_lanes=1, **KW)
    po = hip.default_params(); po.orb_nfeats = 300; po.orb_nlevels = 4
    orb.set_params(po); orb.set_camera(CAM)
    orb.set_dyn_fast_threshold(True, 0.01)
    orb.process_host([frames[0]], hip.RUN_DETECT)
    assert len(orb.keypoints(0, 0, 0)[0]) >= 50
    assert orb.faster_stats(0).as_dict(3) == dict(fresh, next=[po.initial_FAST_threshold] * 3)
    orb.close()


def test_frame_parallel_streams_refuse():
    from stereo_vo_amd.pipeline import FrameParallelStream
    _, p, target = scene("rising")
    fp = FrameParallelStream(p, CAM, W, H, lanes=1, contexts=2, max_kps=1024, max_cand=1 << 15, max_octaves=N_OCT)
    assert fp.L.svo_fpstream_set_dyn_fast_threshold(fp.h, 1, target) == SVO_ERR_UNSUPPORTED and b"frame t - 1" in fp.L.svo_fpstream_last_error(fp.h)
    assert fp.L.svo_fpstream_set_dyn_fast_threshold(fp.h, 1, -1.0) == SVO_ERR_ARG
    with pytest.raises(hip.SvoError):
        fp.set_dyn_fast_threshold(True, target)
    fp.set_dyn_fast_threshold(False, target)
    assert [c.dyn_fast_threshold()[0] for c in fp.ctxs] == [False, False]
    fp.close()


def full_snapshot(ctx, lane, res):
    return ctx.faster_stats(lane).as_dict(), snapshot(ctx, lane, res, N_OCT)


def assert_same_full(a, b, tag):
    assert a[0] == b[0], (tag, a[0], b[0])
    assert_same_snapshot(a[1], b[1], tag)


def test_schedules():
    """the same sequences as plain calls, under svo_use_graphs (captured, then replayed), under the NO_POST / POST split and in a
    pipelined batch of 2 x 2 lanes with the detector running ahead: identical thresholds, statistics, lists and results"""
    import torch
    from stereo_vo_amd.pipeline import StreamBatch
    names = ("lane_world", "settling", "saturated", "lane_noise")
    T = 6
    streams = [scene(n)[0][:T] for n in names]
    _, p, _ = scene("settling")
    target = 0.085
    base = []
    for g in range(4):
        ctx = context(p, target)
        snaps = []
        for t in range(T):
            ctx.process_host([streams[g][t]])
            snaps.append(full_snapshot(ctx, 0, ctx.result(0)))
        ctx.close()
        base.append(snaps)
    assert base[1][-1][0]["next"][:N_OCT] == [24, 26, 20]               # (the settling scene under its own parameters: known to the reference)
    assert len({tuple(b[-1][0]["next"]) for b in base}) == 4
    # graphs: the thresholds are device data, so the second pass replays what the first captured
    ctx = context(p, target)
    ctx.use_graphs(True)
    for rep in range(2):
        ctx.reset()
        for t in range(T):
            ctx.process_host([streams[0][t]])
            assert_same_full(full_snapshot(ctx, 0, ctx.result(0)), base[0][t], ("graphs", rep, t))
    captured, replayed = ctx.graph_count()
    assert captured >= 1 and replayed >= T, (captured, replayed)
    ctx.close()
    # the split detect call: the thresholds are committed by the detect call itself
    ctx = context(p, target)
    for t in range(T):
        ctx.process_host([streams[1][t]], hip.RUN_DETECT | hip.FLAG_DETECT_NO_POST)
        ctx.run_stages(hip.RUN_DETECT_POST | hip.RUN_MATCH | hip.RUN_TRACK | hip.RUN_OPTIMIZE)
        assert_same_full(full_snapshot(ctx, 0, ctx.result(0)), base[1][t], ("split", t))
    ctx.close()
    # the pipelined batch: two contexts of two lanes, detect ahead
    batch = StreamBatch(p, CAM, W, H, 4, 2, max_kps=1024, max_cand=1 << 15, max_octaves=N_OCT)
    batch.set_dyn_fast_threshold(True, target)
    assert [c.dyn_fast_threshold() for c in batch.ctxs] == [(True, target)] * 2
    steps = [lay_out([s[t] for s in streams], "rows", W, [(0, 0)] * 4, seed=t) for t in range(T)]
    for t, (ptrs, buf, host) in enumerate(steps):
        batch.step(ptrs)
        batch.synchronize()
        res, stats = batch.results(), batch.faster_stats()
        for g in range(4):
            c, lane = batch.lane(g)
            assert stats[g].as_dict() == base[g][t][0], ("batch stats", g, t)
            assert_same_full(full_snapshot(c, lane, res[g]), base[g][t], ("batch", g, t))
    batch.close()
    torch.cuda.synchronize()


def test_candidate_overflow_does_not_change_the_rule():
    """the rising scene with a candidate list that cuts octave 0 in the first two frames: status bit 1 is raised there, and the corner
    counts and thresholds are the reference's all the same (which corners survive a cut is unordered: statistics only); from the
    third frame on everything fits and the lists are the reference's again"""
    frames, p, target = scene("rising")
    cap = overflow_max_cand()
    ctx = context(p, target, max_cand=cap)
    for t, ((l, r), (feats, stats)) in enumerate(zip(frames, scene_walk("rising"))):
        ctx.process_host([(l, r)], hip.RUN_DETECT)
        cut = max(stats["corners_left"][0], stats["corners_right"][0]) > cap
        assert cut == (t < 2)
        assert_same_stats(ctx, 0, stats, t + 1, "overflow t=%d" % t)
        if cut:
            assert ctx.status_word(0) & ST_CAND_OVERFLOW and ctx.result(0).status & ST_CAND_OVERFLOW, t
        else:
            assert ctx.status_word(0) == 0, (t, ctx.status_word(0))
            assert_same_lists(ctx, 0, feats, "overflow t=%d" % t, ctx.result(0))
    ctx.close()
