"""Stage 4's F-matrix RANSAC in its MANY-LANE form -- k_ransac_hyp_thread, k_ransac_count_mfma16 with its screen, guards, tile tails,
pair splits and tickets, the 32 / 160 / 1000 sample chunks with their moving bound and floors -- on inputs built to reach what
well-behaved frames never do (tests/ransac_scenes.py; tests/test_ransac_scenes_cpu.py asserts on the oracle alone that they do):
pairs at error exactly 1 and a hair beyond it, pairs on the epipole (|l|^2 tiny, zero, the error infinite or NaN), list lengths around
every tile and super-tile edge, coordinates far outside the image, contaminated lists that need hundreds of samples.

Stage 4 alone on caller-supplied lists; the tracked pairs byte for byte, all eight stage counters and SVO_ST_INTERNAL (status bit 8)
down, against the oracle's stage 4.  Every test needs a real MI355X: run with `pytest -m gpu`."""
import os
import subprocess
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_scenes as RS                                                          # noqa: E402

pytestmark = pytest.mark.gpu


def load_small(golden_dir):
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    return g, cam, p


def context(golden_dir, n_lanes=1):
    """640 x 480, 1024 keypoints per list (the golden lists are put as what they are, 256 x 192: every list brings its own image size)"""
    _, cam, p = load_small(golden_dir)
    ctx = hip.Context(n_lanes=n_lanes, max_w=640, max_h=480, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    return ctx, p


@pytest.mark.parametrize("mode", ["51", "53", "54"])
def test_forced_forms_on_one_lane(golden_dir, monkeypatch, mode):
    """One thread per sample (51), the 16 x 16 matrix-core count with its screen (53) and the same with every verdict replayed (54), forced
    on a one-lane context: every hand-built scene -- sideways, forward, far --, the thinned golden lists and the line scenes."""
    monkeypatch.setenv("SVO_DEBUG_MODE", mode)
    ctx, p = context(golden_dir)
    failed = []
    for name, s in RS.all_cases(golden_dir):
        try:
            RS.check_case(name, RS.run_case(ctx, s), RS.oracle_track(p, s, key=name))
        except AssertionError as e:
            failed.append(e.args[0])
    ctx.close()
    assert not failed, (mode, len(failed), failed[:6])


def _lane_scenes(golden_dir):
    """twelve lanes: scenes of every generator, the list lengths spread (7 .. 530 candidates), one lane empty"""
    names = ["sideways-530", "forward-64", "far-257", "sideways-7", "forward-272", None, "sideways-17", "forward-150", "forward-48", "sideways-257", "forward-11", "far-33"]
    return [(nm, None if nm is None else RS.scene(nm)) for nm in names]


def _empty_like(s):
    """zero-length lists: what a lane that had lists in an earlier round is given when its turn is to have none"""
    e = dict(s)
    for k in ("pkl", "pkr", "pdl", "pdr", "pm", "ckl", "ckr", "cdl", "cdr", "cm"):
        e[k] = s[k][:0]
    return e


def _rounds(ctx, p, lanes, tag):
    """three rounds, the scenes rotated by five lanes each time: every lane follows a longer list by a shorter one and vice versa"""
    n = len(lanes)
    template = next(s for _, s in lanes if s is not None)
    for rnd in range(3):
        now = [lanes[(i + 5 * rnd) % n] for i in range(n)]
        for lane, (name, s) in enumerate(now):
            if s is not None:
                RS.put_scene(ctx, lane, s)
            elif rnd > 0:
                RS.put_scene(ctx, lane, _empty_like(template))
        ctx.run_stages(hip.RUN_TRACK)
        for lane, (name, s) in enumerate(now):
            got = (ctx.tracked(lane), [int(v) for v in ctx.result(lane).track_stats[:8]], ctx.status_word(lane))
            if s is None:                                                            # no lists at all: nothing tracked, every counter zero
                assert len(got[0]) == 0 and got[1] == [0] * 8 and not (got[2] & 8), (tag, rnd, lane, got)
            else:
                RS.check_case((tag, "round %d" % rnd, "lane %d" % lane, name), got, RS.oracle_track(p, s, key=name))


def test_many_lanes_select_the_batched_forms(golden_dir, monkeypatch):
    """Nothing forced: a twelve-lane context selects k_ransac_hyp_thread, k_ransac_count_mfma16 and the chunk ends 32 / 160 by itself.
    Each lane gets another scene (one lane none), every lane is compared with its own oracle run; then the scenes move on by five lanes,
    twice: model slots, counts, floors and tickets an earlier frame left in a lane must not leak into the next."""
    for k in ("SVO_DEBUG_MODE", "SVO_RC_SPLIT", "SVO_RS_C0"):
        monkeypatch.delenv(k, raising=False)
    ctx, p = context(golden_dir, n_lanes=12)
    _rounds(ctx, p, _lane_scenes(golden_dir), "brute force")
    ctx.close()


def test_many_lanes_windowed_tracker_on_thinned_lists(golden_dir, monkeypatch):
    """The same three rounds with the windowed tracker (ifm_method 1), which hands the RANSAC the survivors in the CURRENT list's order:
    thinned golden lists only (the hand-built scenes carry no row index), their lengths spread over the lanes, one lane empty."""
    for k in ("SVO_DEBUG_MODE", "SVO_RC_SPLIT", "SVO_RS_C0"):
        monkeypatch.delenv(k, raising=False)
    _, cam, p = load_small(golden_dir)
    p.ifm_method = 1; p.ifm_win_w = 20; p.ifm_win_h = 30
    ctx = hip.Context(n_lanes=12, max_w=640, max_h=480, max_kps=1024, max_cand=1 << 15)
    ctx.set_params(p); ctx.set_camera(cam)
    thinned = dict(RS.thinned_cases(golden_dir))
    names = ["thinned-64-0", "thinned-7-0", "thinned-32-1", "thinned-15-0", "thinned-48-0", None, "thinned-8-1", "thinned-64-1", "thinned-16-0", "thinned-24-0", "thinned-14-0", "thinned-17-1"]
    _rounds(ctx, p, [(nm, None if nm is None else thinned[nm]) for nm in names], "windowed")
    ctx.close()


KNOBS = [{"SVO_DEBUG_MODE": "53", "SVO_RC_SPLIT": "4,2,3"}, {"SVO_DEBUG_MODE": "53", "SVO_RC_SPLIT": "3", "SVO_RS_C0": "32"}, {"SVO_DEBUG_MODE": "51", "SVO_RS_C0": "160"}]


def test_pair_splits_and_forced_chunk_ends(golden_dir, tmp_path):
    """The pairs of a lane split over 4 / 2 / 3 blocks per chunk (partial counts, tickets; 17, 33, 255, 257, 272 pairs end `tiles_per * split`
    inside, at and past the list), three blocks everywhere under the many-lane chunk ends 32 / 160, and the one-thread hypothesis kernel
    under the chunk ends 160 / 160: knobs a context reads when it is created; each setting gets a fresh child (one after the other)
    that runs every case of the forced-form test and writes what it got; the parent compares with the oracle."""
    _, _, p = load_small(golden_dir)
    helper = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ransac_scene_run.py")
    cases = RS.all_cases(golden_dir)
    for i, env in enumerate(KNOBS):
        out_path = str(tmp_path / ("knobs%d.npz" % i))
        full = {k: v for k, v in os.environ.items() if k not in ("SVO_DEBUG_MODE", "SVO_RC_SPLIT", "SVO_RS_C0")}
        full.update(env)
        out = subprocess.run([sys.executable, helper, golden_dir, out_path], env=full, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0 and "done %d" % len(cases) in out.stdout, (env, out.stdout[-400:], out.stderr[-1200:])
        got = np.load(out_path)
        failed = []
        for name, s in cases:
            try:
                RS.check_case(name, (got["trk/" + name], list(got["ts/" + name]), int(got["st/" + name])), RS.oracle_track(p, s, key=name))
            except AssertionError as e:
                failed.append(e.args[0])
        assert not failed, (env, len(failed), failed[:6])


def test_a_knob_belongs_to_the_context_created_under_it(golden_dir, monkeypatch):
    """The SVO_* knobs are read once per context, by svo_create.  In ONE process: context A is created under SVO_RS_C0=32 and SVO_GN_NT=256,
    both are taken out of the environment, context B is created; the three frames of the small sequence then go through A and B in turn.
    A runs chunk 1 of the sample schedule (with 32 forced it exists), B never does (one lane defaults to SVO_RANSAC_FEW, whose chunk 1 is
    empty) -- whichever context launched first --, and both give the golden lists bit for bit and the oracle's result records."""
    from oracle import oracle as O
    for k in ("SVO_DEBUG_MODE", "SVO_RC_SPLIT", "SVO_HAM_FP4"):
        monkeypatch.delenv(k, raising=False)
    g, cam, p = load_small(golden_dir)

    def make():
        ctx = hip.Context(n_lanes=1, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=1024, max_cand=1 << 15, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam)
        return ctx
    monkeypatch.setenv("SVO_RS_C0", "32"); monkeypatch.setenv("SVO_GN_NT", "256")
    a = make()
    monkeypatch.delenv("SVO_RS_C0"); monkeypatch.delenv("SVO_GN_NT")
    b = make()
    orc = O.Oracle(p)
    for t in range(3):
        ro = orc.process(g["L%d" % t], g["R%d" % t], cam)
        for tag, ctx in (("A", a), ("B", b)):
            ctx.process_host([(g["L%d" % t], g["R%d" % t])])
            r = ctx.result(0)
            for side in (0, 1):
                k, d = ctx.keypoints(0, 0, side)
                assert k.tobytes() == g["kps%d_%d" % (side, t)].tobytes() and (d == g["desc%d_%d" % (side, t)]).all(), (tag, t, "features", side)
            assert ctx.matches(0).tobytes() == g["matches%d" % t].tobytes(), (tag, t, "pairings")
            assert ctx.tracked(0).tobytes() == g["tracked%d" % t].tobytes(), (tag, t, "tracked pairs")
            assert (r.valid, r.error_code) == (ro.valid, ro.error_code), (tag, t, r.valid, r.error_code, ro.valid, ro.error_code)
            assert (r.detected_left[0], r.detected_right[0], r.stereo_matches[0]) == (ro.detected_left[0], ro.detected_right[0], ro.stereo_matches[0]), (tag, t)
            assert (r.n_residual, r.n_outliers) == (ro.n_residual, ro.n_outliers), (tag, t)
            assert list(r.track_stats) == list(ro.track_stats), (tag, t, list(r.track_stats), list(ro.track_stats))
            if ro.valid:
                dp = np.abs(np.array(r.outPose) - np.array(ro.outPose))
                assert dp[:3].max() < 1e-3 and dp[3:].max() < 1e-4, (tag, t, dp)
                assert r.tracked_feats_from_last_frame == ro.tracked_feats_from_last_frame, (tag, t)
            assert ctx.status_word(0) == 0, (tag, t)
    calls_a, calls_b = a.kernel_times()["ransac_hyp_1"][1], b.kernel_times()["ransac_hyp_1"][1]
    a.close(); b.close()
    assert calls_a > 0, calls_a
    assert calls_b == 0, calls_b
