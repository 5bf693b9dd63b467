"""dmFASTER's dynamic threshold without a GPU: the exported rule (svo_faster_threshold_step) against the reference's expression, the
REACH of every scene of tests/test_gpu_faster_dyn.py pinned on tests/faster_dyn_ref.py alone -- so that a scene cannot quietly stop
exercising its case --, the INI reader and the refusals that need no device.

The scenes live here and the GPU tests import them: each is (frames, parameters, target) and a cached walk of the reference."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import FasterStats, Params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_dyn_ref as D                                      # noqa: E402
import faster_ref as F                                          # noqa: E402
import image_content as IC                                      # noqa: E402
from test_gpu_frame_layouts import make_frames                  # noqa: E402

SVO_ERR_ARG = -2
W, H, N_OCT, NFE, KLT_WIN = 160, 120, 3, 300, 4
OCT_PIXELS = [(W >> o) * (H >> o) for o in range(N_OCT)]


def params(t, n_oct=N_OCT):
    return F.faster_params(hip.default_params(), t=t, orb_nfeats=NFE, n_oct=n_oct)


@functools.lru_cache(maxsize=None)
def world(n=8, seed=41):
    return make_frames("world", W, H, n, seed=seed)


@functools.lru_cache(maxsize=None)
def saturated(n=6):
    """random 0 / 255 blocks of 2 x 2 pixels, moving: the only corners at threshold 254 are isolated blocks, and at 255 there are none"""
    base = IC.binary_blocks(W, H, seed=1, block=2)
    return [(IC.moved(base, 3 * t, 2 * t), IC.right_of(IC.moved(base, 3 * t, 2 * t), 6)) for t in range(n)]


@functools.lru_cache(maxsize=None)
def flat(n=6):
    img = np.full((H, W), 90, np.uint8)
    return [(img, img)] * n


@functools.lru_cache(maxsize=None)
def noise(n=6):
    rng = np.random.RandomState(5)
    return [(rng.randint(0, 256, (H, W)).astype(np.uint8), rng.randint(0, 256, (H, W)).astype(np.uint8)) for _ in range(n)]


# name -> (frames, initial_FAST_threshold, target_feats_per_pixel)
SCENES = {
    "rising": (lambda: world()[:7], 5, 1e-9),
    "falling": (lambda: world()[:6], 3, 1.0),
    "falling_from_0": (lambda: world()[:3], 0, 1.0),
    "settling": (lambda: world()[:8], 20, 0.085),
    "saturated": (lambda: saturated(), 254, 1e-4),
    "lane_flat": (lambda: flat(), 20, D.DEFAULT_TARGET),
    "lane_world": (lambda: world(6, 43), 20, D.DEFAULT_TARGET),
    "lane_noise": (lambda: noise(), 20, D.DEFAULT_TARGET),
}


def scene(name):
    """(frames, params, target)"""
    frames, t0, target = SCENES[name]
    return frames(), params(t0), target


@functools.lru_cache(maxsize=None)
def scene_walk(name):
    """[(feats, stats)] per frame of a fresh estimator: computed once, shared by every test, never modified"""
    frames, p, target = scene(name)
    return D.walk(frames, p, target, KLT_WIN)


def used(name):
    """the thresholds in call order: [left frame 0, right frame 0, left frame 1, ...] per octave"""
    w = scene_walk(name)
    return [[x for _, s in w for x in (s["used_left"][o], s["used_right"][o])] for o in range(N_OCT)]


# ---- 1. the exported rule ----------------------------------------------------------------------------------------------------------
def test_exported_step_equals_the_rule_on_a_sweep():
    L = hip.lib()
    assert L.svo_faster_threshold_step(20, 0, 160, 120, C.c_double(0.01)) == 19
    rng = np.random.RandomState(7)
    n_checked = 0
    for target in (0.0, 1e-9, 1e-4, 0.01, 0.05, 0.085, 0.1, 0.3, 1.0, 2.0):
        for w, h in ((160, 120), (80, 60), (40, 30), (251, 187), (1280, 960), (7, 7)):
            wh = w * h
            # around both bounds, the ends, and random counts (beyond w * h too: the rule does not know what a pixel is)
            ns = {0, 1, wh - 1, wh, 2 * wh} | {int(np.floor(f * target * wh)) + k for f in (0.8, 1.2) for k in (-1, 0, 1, 2)} | set(rng.randint(0, wh + 1, 8).tolist())
            for n in sorted(x for x in ns if 0 <= x < 2 ** 31):
                for T in (0, 1, 2, 19, 20, 254, 255):
                    assert hip.faster_threshold_step(T, n, w, h, target) == D.step(T, n, wh, target), (T, n, w, h, target)
                    n_checked += 1
    assert n_checked > 5000
    # exact boundaries (tools/faster_dyn_check.cpp searches for them; two by hand): 8 / 1000 == 0.8 * 0.01 and 12 / 1000 == 1.2 * 0.01 as doubles?
    for n, wh, target in ((1, 10, 0.125), (3, 20, 0.125)):      # 0.1 == 0.8 * 0.125 and 0.15 == 1.2 * 0.125 -- held to the rule as Python computes it
        assert hip.faster_threshold_step(20, n, wh, 1, target) == D.step(20, n, wh, target)
    assert D.step(20, 1, 8, 0.15625) == 20 and 1 / 8.0 == 0.8 * 0.15625       # on the lower bound: stays (0.125 is exact)
    assert hip.faster_threshold_step(20, 1, 8, 1, 0.15625) == 20 and hip.faster_threshold_step(20, 0, 8, 1, 0.15625) == 19


def test_threshold_stays_in_0_255():
    for T in range(0, 256):
        for n in (0, 1, 10 ** 6):
            for target in (0.0, 0.01, 1.0):
                t2 = D.step(T, n, 19200, target)
                assert (1 if T else 0) <= t2 <= 256 and abs(t2 - T) <= 1 and (T < 255 or n > 0 or t2 <= 255)      # (0 stays 0 only inside the band)
    # 256 is only reachable from 255 with corners, and at 255 there are none: no pixel passes I + 255
    img = np.zeros((20, 20), np.uint8); img[10, 10] = 255
    assert len(F.fast12(img, 254)[0]) == 1 and len(F.fast12(img, 255)[0]) == 0


# ---- 2. the reach of the GPU scenes -------------------------------------------------------------------------------------------------
def test_rising_rises_on_every_call():
    u = used("rising")
    for o in range(N_OCT):
        assert u[o] == list(range(5, 5 + 14)), (o, u[o])         # T, T+1, T+2, ...: left and right interleave within a frame
    w = scene_walk("rising")
    assert all(min(s["corners_left"] + s["corners_right"]) >= 100 for _, s in w)        # every list has something to compare
    assert all(len(f[0]) >= 60 and len(f[1]) >= 60 for fs, _ in w for f in fs)


def test_falling_reaches_1_and_stays():
    u = used("falling")
    for o in range(N_OCT):
        assert u[o] == [3, 2] + [1] * 10, (o, u[o])
    assert scene_walk("falling")[-1][1]["next"] == [1, 1, 1]
    u0 = used("falling_from_0")
    for o in range(N_OCT):
        assert u0[o] == [0] + [1] * 5, (o, u0[o])                # 0 is used once (a valid threshold), then the floor
    # threshold 0 and 1 are not the same detector on these frames
    assert scene_walk("falling_from_0")[0][1]["corners_left"][0] > scene_walk("falling")[1][1]["corners_left"][0]


def test_settling_enters_the_band_and_stops():
    w = scene_walk("settling")
    _, _, target = scene("settling")
    settled = w[-1][1]["next"]
    assert settled == [24, 26, 20], settled
    u = used("settling")
    for o in range(N_OCT):
        assert u[o][-8:] == [settled[o]] * 8, (o, u[o])          # the last four frames: both calls at the settled threshold
        for _, s in w[-4:]:
            for n in (s["corners_left"][o], s["corners_right"][o]):
                assert 0.8 * target <= n / float(OCT_PIXELS[o]) <= 1.2 * target, (o, n)
    assert u[0][:4] == [20, 21, 22, 23] and u[1][:4] == [20, 21, 22, 23]                  # ... after moving first
    assert [s["next"] for _, s in w[:4]] == [[22, 22, 20], [24, 24, 20], [24, 26, 20], [24, 26, 20]]


def test_saturated_oscillates_254_255():
    w = scene_walk("saturated")
    u = used("saturated")
    assert u[0] == [254, 255] * 6, u[0]
    for fs, s in w:
        assert s["corners_left"][0] >= 400 and s["corners_right"][0] == 0 and s["next"][0] == 254
        assert len(fs[0][0]) >= 200 and len(fs[0][1]) == 0       # T = 255: an empty right list
    assert max(u[1]) == 255 and min(u[2]) < 250                 # octave 1 touches 255 too, octave 2 (no saturated corner left) falls


def test_lane_scenes_move_apart():
    nxt = {k: [s["next"] for _, s in scene_walk(k)] for k in ("lane_flat", "lane_world", "lane_noise")}
    assert nxt["lane_flat"][-1] == [8, 8, 8]                    # nothing to find: falls on every call
    assert nxt["lane_world"][-1][0] == 32 and nxt["lane_noise"][-1][0] == 32             # dense: octave 0 rises on every call
    assert nxt["lane_world"][-1] != nxt["lane_noise"][-1]       # ... and the higher octaves tell the two apart
    assert len({tuple(v[-1]) for v in nxt.values()}) == 3


def test_overflow_scene_cuts_the_first_two_frames_only():
    """the rising scene with max_cand = the largest octave-0 count from the third frame on (overflow_max_cand)"""
    w = scene_walk("rising")
    cap = overflow_max_cand()
    cut = [max(s["corners_left"][0], s["corners_right"][0]) > cap for _, s in w]
    assert cut == [True, True] + [False] * 5, cut
    assert all(max(s["corners_left"][o], s["corners_right"][o]) <= 1024 for _, s in w for o in (1, 2))     # the higher octaves' lists (1024 entries at least) always fit


def overflow_max_cand():
    w = scene_walk("rising")
    return max(max(s["corners_left"][0], s["corners_right"][0]) for _, s in w[2:])


# ---- 3. ABI, INI reader, refusals without a device ----------------------------------------------------------------------------------
def test_abi_and_ini(tmp_path):
    L = hip.lib()
    for name in ("svo_set_dyn_fast_threshold", "svo_get_dyn_fast_threshold", "svo_dyn_fast_load_ini", "svo_get_faster_stats", "svo_faster_stats_size",
                 "svo_faster_threshold_step", "svo_batch_set_dyn_fast_threshold", "svo_batch_faster_stats", "svo_fpstream_set_dyn_fast_threshold"):
        assert getattr(L, name) is not None
    assert L.svo_faster_stats_size() == C.sizeof(FasterStats) == 96
    sizes = (C.c_int32 * 6)()
    L.svo_abi_sizes(sizes)
    assert sizes[3] == C.sizeof(Params) == 160                  # the switch and the target live on the context: svo_params did not grow
    ini = tmp_path / "ref.ini"
    ini.write_text("[DETECT]\ndetect_method = 2\ntarget_feats_per_pixel = 0.0125   // per square pixel\ninitial_FAST_threshold = 25\n[OTHER]\nx = 1\n")
    assert hip.load_dyn_fast_ini(ini, "DETECT") == 0.0125
    assert hip.load_dyn_fast_ini(ini, "detect", 0.5) == 0.0125  # section names are case-insensitive, as in the parameter loader
    assert hip.load_dyn_fast_ini(ini, "OTHER", 0.5) == 0.5      # key absent: the value stays
    assert hip.load_dyn_fast_ini(ini, "NONE", 0.25) == 0.25     # section absent
    assert hip.load_dyn_fast_ini(ini, "", 0.25) == 0.25
    assert hip.load_dyn_fast_ini(ini, "NONE") == 10. / 1000.    # S2:46
    with pytest.raises(hip.SvoError):
        hip.load_dyn_fast_ini(tmp_path / "missing.ini", "DETECT")
    p = hip.load_params_ini(ini, ["", "DETECT", "", "", "", "", ""])       # the parameter loader goes on ignoring the key
    assert (p.detect_method, p.initial_FAST_threshold) == (2, 25)


def test_refusals_without_a_device():
    L = hip.lib()
    st = FasterStats()
    assert L.svo_set_dyn_fast_threshold(None, 1, 0.01) == SVO_ERR_ARG
    assert L.svo_get_dyn_fast_threshold(None, None, None) == SVO_ERR_ARG
    assert L.svo_get_faster_stats(None, 0, C.byref(st)) == SVO_ERR_ARG
    assert L.svo_batch_set_dyn_fast_threshold(None, 1, 0.01) == SVO_ERR_ARG and L.svo_batch_faster_stats(None, None) == SVO_ERR_ARG
    assert L.svo_fpstream_set_dyn_fast_threshold(None, 1, 0.01) == SVO_ERR_ARG
    assert L.svo_dyn_fast_load_ini(None, b"DETECT", None) == SVO_ERR_ARG
