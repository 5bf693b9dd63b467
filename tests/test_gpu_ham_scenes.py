"""The product brute-force matcher k_hamming_f4 (FP4 matrix-core products, csrc/k_match.hip) and its int8 A/B form on the hand-built lists
of tests/ham_scenes.py: ties at every accumulator register, lane half, tile and split boundary, list lengths around the 32-row tiles and
the 256-query blocks, distances 0 .. 256, train indices on both sides of 8192, and pairing lists that are no identity -- under every
count of train-side splits.  tests/test_ham_scenes_cpu.py asserts on the oracle alone that the scenes do reach those edges and that no
stage-3 / stage-4 filter hides a word of the matcher there.

Stage 3 / stage 4 alone on caller-supplied lists, byte for byte against popcount + argmin in numpy AND against the oracle.  Every test
needs a real MI355X: `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ham_scenes as HS                                                              # noqa: E402

pytestmark = pytest.mark.gpu

N_STEREO = sum(v for k, v in HS.FAMILY_COUNTS.items() if k != "wide")


def params():
    return north_star_params(hip.default_params(), orb_nfeats=600)      # (the detector is not run: its quota only has to fit the smallest context)


def context(n_lanes=1, max_kps=1024, p=None, **kw):
    ctx = hip.Context(n_lanes=n_lanes, max_w=HS.W, max_h=HS.H, max_kps=max_kps, max_cand=1 << 15, kernel_times=True, **kw)
    ctx.set_params(HS.stereo_params(params()) if p is None else p)
    assert ctx.orb_threshold() == HS.ORB_TH
    return ctx


def report(failed):
    """the names of the scenes that failed, on one line, and the first three failures in full"""
    return " ".join(nm for nm, _ in failed), [text for _, text in failed[:3]]


def calls(ctx, *names):
    kt = ctx.kernel_times()
    return [int(kt[n][1]) for n in names]


_ORACLE = {}


def oracle_match(nm, img=None):
    """the oracle's stage 3 on a scene, once per process"""
    if (nm, img) not in _ORACLE:
        from oracle import oracle
        _ORACLE[nm, img] = HS.oracle_match(HS.stereo_params(north_star_params(oracle.default_params(), orb_nfeats=600)), HS.scene(nm), img)
    return _ORACLE[nm, img]


def oracle_track(nm):
    from oracle import oracle
    return HS.oracle_track(HS.track_params(north_star_params(oracle.default_params(), orb_nfeats=600)), HS.scene(nm), key=("ham-scenes", nm))


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------------------------------
def put_stereo(ctx, lane, s, octave=0):
    for side, (k, d) in enumerate(((s["kl"], s["dl"]), (s["kr"], s["dr"]))):
        ctx.put_features(lane, 0, side, k, d, s["W"], s["H"], octave=octave)


def check_stereo(tag, ctx, lane, nm, octave=0, use_oracle=True):
    """the lane's pairings byte for byte against popcount + argmin and against the oracle; their row table, stereo_matches, SVO_ST_INTERNAL down"""
    s = HS.scene(nm)
    h = s["H"] >> octave
    got, got_ri = ctx.matches(lane, 0, octave), ctx.matches_row_index(lane, 0, octave)
    if got.tobytes() != s["want"].tobytes():
        bad = [int(q) for q in np.flatnonzero((got["trainIdx"] != s["want"]["trainIdx"]) | (got["distance"] != s["want"]["distance"]))] if len(got) == len(s["want"]) else None
        first = None if not bad else (bad[0], int(got["trainIdx"][bad[0]]), float(got["distance"][bad[0]]), int(s["want"]["trainIdx"][bad[0]]), float(s["want"]["distance"][bad[0]]))
        raise AssertionError((tag, nm, "pairings against numpy", len(got), len(s["want"]), "wrong queries", bad and bad[:8], "first (q, got, want)", first))
    assert list(got_ri[:h + 1]) == list(s["want_ri"][:h + 1]), (tag, nm, "pairings' row table")
    if use_oracle:
        m, ri = oracle_match(nm, None if octave == 0 else (s["W"] >> octave, h))
        assert got.tobytes() == m.tobytes() and list(got_ri[:h + 1]) == list(ri), (tag, nm, "against the oracle")
    assert int(ctx.result(lane).stereo_matches[octave]) == len(s["want"]), (tag, nm, "stereo_matches")
    assert not (ctx.status_word(lane) & 8), (tag, nm, "SVO_ST_INTERNAL")


def run_stereo_scenes(ctx, names, use_oracle=True):
    """every named scene through stage 3 in lane 0: (scenes run, first line of every failure)"""
    failed = []
    for nm in names:
        put_stereo(ctx, 0, HS.scene(nm))
        ctx.run_stages(hip.RUN_MATCH)
        try:
            check_stereo("lane 0", ctx, 0, nm, use_oracle=use_oracle)
        except AssertionError as e:
            failed.append((nm, str(e.args[0]).split("\n")[0]))
    return len(names), failed


@pytest.mark.parametrize("splits", [None, 1, 2, 3, 7, 8])
def test_stage3_scenes_under_every_split_count(splits, monkeypatch):
    """every stage-3 scene of 1024 rows or fewer, with the train list cut into the splits a one-lane context derives (8) and into 1, 2,
    3, 7 and 8 forced ones (SVO_HAM_SPLITS, read when the context is created): the narrow kernel runs once per scene, the wide one never"""
    if splits is None:
        monkeypatch.delenv("SVO_HAM_SPLITS", raising=False)
    else:
        monkeypatch.setenv("SVO_HAM_SPLITS", str(splits))
    ctx = context()
    monkeypatch.delenv("SVO_HAM_SPLITS", raising=False)
    total, failed = run_stereo_scenes(ctx, HS.stereo_names())
    n_lr, n_wide = calls(ctx, "hamming_lr", "hamming_lr_wide")
    ctx.close()
    assert total == N_STEREO == 48 and not failed, (splits, len(failed)) + report(failed)
    assert (n_lr, n_wide) == (total, 0)


def test_stage3_wide_lists():
    """train lists of 8191 .. 16384 rows in a max_kps = 16384 context: k_hamming_f4<true>, whose index bits reach 8192 .. 16383"""
    ctx = context(max_kps=16384)
    total, failed = run_stereo_scenes(ctx, HS.wide_names() + ["ties-positions", "len-513-289"])
    n_lr, n_wide = calls(ctx, "hamming_lr", "hamming_lr_wide")
    ctx.close()
    assert total == HS.FAMILY_COUNTS["wide"] + 2 and not failed, (len(failed),) + report(failed)
    assert (n_lr, n_wide) == (0, total)


def test_stage3_lanes_side_by_side():
    """five lanes, five lists of different lengths (one without a train list, one without a query list) in one call; then lane 1 gets
    another list and stays idle through active=, while two active lanes swap theirs"""
    ctx = context(n_lanes=5)
    for lane, nm in enumerate(HS.LANES):
        put_stereo(ctx, lane, HS.scene(nm))
    ctx.run_stages(hip.RUN_MATCH)
    for lane, nm in enumerate(HS.LANES):
        check_stereo("all lanes", ctx, lane, nm)
    put_stereo(ctx, 1, HS.scene(HS.LANE_SWAP))
    for lane in (0, 3):
        put_stereo(ctx, lane, HS.scene(HS.LANES[3 - lane]))
    ctx.run_stages(hip.RUN_MATCH, active=[0, 2, 3, 4])
    assert ctx.matches(1, 0).tobytes() == HS.scene(HS.LANES[1])["want"].tobytes(), "the idle lane's pairings moved"
    for lane, k in ((0, 3), (3, 0), (2, 2), (4, 4)):
        check_stereo("one idle", ctx, lane, HS.LANES[k])
    ctx.close()


def test_stage3_two_octaves():
    """one lane of a two-octave context (FAST + ORB geometry), a list of its own per octave"""
    p = HS.stereo_params(params())
    p.detect_method, p.nOctaves = 1, 2
    ctx = context(p=p, max_octaves=2)
    for o, nm in enumerate(HS.OCTAVES):
        put_stereo(ctx, 0, HS.scene(nm), octave=o)
    ctx.run_stages(hip.RUN_MATCH)
    for o, nm in enumerate(HS.OCTAVES):
        check_stereo("octave %d" % o, ctx, 0, nm, octave=o)
    ctx.close()


def test_stage3_twenty_lanes_derive_six_splits():
    """a context of twenty lanes cuts the train lists into 1024 / (8 * 20) = 6 splits: the scenes with a planted tie or distance, dealt over
    the lanes, three calls (the last one with idle lanes)"""
    names = [nm for nm in HS.stereo_names() if HS.scene(nm)["plan"]]
    ctx = context(n_lanes=20)
    failed = []
    for at in range(0, len(names), 20):
        batch = names[at:at + 20]
        for lane, nm in enumerate(batch):
            put_stereo(ctx, lane, HS.scene(nm))
        ctx.run_stages(hip.RUN_MATCH, active=list(range(len(batch))))
        for lane, nm in enumerate(batch):
            try:
                check_stereo("lane %d" % lane, ctx, lane, nm)
            except AssertionError as e:
                failed.append((nm, str(e.args[0]).split("\n")[0]))
    ctx.close()
    assert len(names) == 46 and not failed, (len(failed),) + report(failed)


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------------------------------------------------------------------
def put_track(ctx, lane, s):
    HS.put_scene(ctx, lane, s)
    for which, key in ((1, "pri"), (0, "cri")):
        assert list(ctx.matches_row_index(lane, which)[:s["H"] + 1]) == list(s[key]), ("row table of put pairings", lane, which)


def check_track(nm, ctx, lane, use_oracle=True):
    s = HS.scene(nm)
    got = ctx.tracked(lane), [int(v) for v in ctx.result(lane).track_stats[:8]], ctx.status_word(lane)
    if got[0].tobytes() != s["want"].tobytes():
        a, b = set(map(tuple, got[0].tolist())), set(map(tuple, s["want"].tolist()))
        raise AssertionError((nm, "tracked pairs against numpy", len(got[0]), len(s["want"]), "not wanted", sorted(a - b)[:6], "missing", sorted(b - a)[:6]))
    if use_oracle:
        HS.check_case(nm, got, oracle_track(nm))
    assert not (got[2] & 8), (nm, "SVO_ST_INTERNAL")


def run_track_scenes(ctx, names, use_oracle=True):
    failed = []
    for nm in names:
        put_track(ctx, 0, HS.scene(nm))
        ctx.run_stages(hip.RUN_TRACK)
        try:
            check_track(nm, ctx, 0, use_oracle)
        except AssertionError as e:
            failed.append((nm, str(e.args[0]).split("\n")[0]))
    return len(names), failed


@pytest.mark.parametrize("splits", [None, 3])
def test_stage4_scenes(splits, monkeypatch):
    """every stage-4 scene that fits 1024 keypoints: the descriptors gathered through pairing lists that are no identity, copies of the
    wanted pairing further on, decoys in unpaired keypoints -- tracked pairs, all eight counters, the status word"""
    if splits is not None:
        monkeypatch.setenv("SVO_HAM_SPLITS", str(splits))
    ctx = context(p=HS.track_params(params()))
    monkeypatch.delenv("SVO_HAM_SPLITS", raising=False)
    total, failed = run_track_scenes(ctx, HS.track_names())
    n_trk, n_wide = calls(ctx, "hamming_track", "hamming_track_wide")
    ctx.close()
    assert total == 9 and not failed, (splits, len(failed)) + report(failed)
    assert (n_trk, n_wide) == (total, 0)


def test_stage4_wide_pairing_list():
    """8200 current pairings in a max_kps = 16384 context: wanted pairings and their copies on both sides of 8191 / 8192"""
    ctx = context(max_kps=16384, p=HS.track_params(params()))
    total, failed = run_track_scenes(ctx, [nm for nm, _, _ in HS.TRACK_WIDE] + ["track-257-97"])
    n_trk, n_wide = calls(ctx, "hamming_track", "hamming_track_wide")
    ctx.close()
    assert total == 2 and not failed, report(failed)
    assert (n_trk, n_wide) == (0, total)


def test_stage4_lanes_side_by_side():
    """five lanes, five scenes in one call; then lane 1 gets other lists and stays idle"""
    names = ["track-257-257", "track-32-33", "track-256-65", "track-33-97", "track-255-257"]
    ctx = context(n_lanes=5, p=HS.track_params(params()))
    for lane, nm in enumerate(names):
        put_track(ctx, lane, HS.scene(nm))
    ctx.run_stages(hip.RUN_TRACK)
    for lane, nm in enumerate(names):
        check_track(nm, ctx, lane)
    HS.put_scene(ctx, 1, HS.scene("track-33-64"))
    ctx.run_stages(hip.RUN_TRACK, active=[0, 2, 3, 4])
    assert ctx.tracked(1).tobytes() == HS.scene(names[1])["want"].tobytes(), "the idle lane's tracked pairs moved"
    for lane in (0, 2, 3, 4):
        check_track(names[lane], ctx, lane)
    ctx.close()


# ---------------------------------------------------------------------------------------------------------------------------------------
# the int8 A/B form
# ---------------------------------------------------------------------------------------------------------------------------------------
def replay_everything():
    """every stage-3 and stage-4 scene in a narrow and in a wide context, against numpy (run by the child process below)"""
    for max_kps, stereo, track in ((1024, HS.stereo_names(), HS.track_names()), (16384, HS.wide_names(), [nm for nm, _, _ in HS.TRACK_WIDE])):
        ctx = context(max_kps=max_kps)
        n3, failed3 = run_stereo_scenes(ctx, stereo, use_oracle=False)
        ctx.set_params(HS.track_params(params()))
        n4, failed4 = run_track_scenes(ctx, track, use_oracle=False)
        narrow, wide = calls(ctx, "hamming_lr", "hamming_track"), calls(ctx, "hamming_lr_wide", "hamming_track_wide")
        ctx.close()
        assert not failed3 and not failed4, (max_kps,) + report(failed3) + report(failed4)
        assert (narrow, wide) == (([n3, n4], [0, 0]) if max_kps == 1024 else ([0, 0], [n3, n4])), (max_kps, narrow, wide)
    print("same")


def test_int8_form_of_the_matcher():
    """the A/B-only int8 form (SVO_HAM_FP4=0, libsvo_hip_ab.so), k_hamming and k_hamming_wide: all scenes once more in a fresh process"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import os, sys\n"
            "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
            "import test_gpu_ham_scenes as G\n"
            "G.replay_everything()\n") % (root, root)
    env = dict(os.environ, SVO_HAM_FP4="0", SVO_HIP_LIB=os.path.join(root, "stereo_vo_amd", "libsvo_hip_ab.so"))
    env.pop("SVO_HAM_SPLITS", None)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "same" in out.stdout, (out.stdout[-400:], out.stderr[-1500:])
