"""The dynamic-LDS carve-ups of the matcher and tracker kernels at every context size, on the smallest input.

A kernel of k_match.hip places its LDS arrays at offsets that depend on max_kps, not on the length of the lists: the four frames of
tests/golden/oracle_small_seq.npz (256 x 192, about 220 keypoints and 100 pairings per frame) go through contexts with max_kps 4096,
8192 and 16384 -- k_track_filter<16 | 32 | 64> and every total that exceeds the default 64 KB -- under three selector pairs:

  bf       brute force + 1-to-1 filter (k_match_lr_filter), brute-force tracker (k_track_filter)
  rbr_win  smDescRbR (k_match_lr_rbr<false>), ifmDescWin (k_track_win<false>)
  sad      smSAD (k_match_lr_rbr<true>), ifmSAD (k_track_win<true>), thresholds 1500 (at the reference's ~200 this small sequence
           leaves fewer than eight candidates per frame)

k_track_finalize runs under all three, and vo_use_matches_ids is on, so k_match_ids does too.  The reference of bf and rbr_win is the
CPU oracle; the oracle refuses the SAD selectors, whose reference is tests/sad_ref.py on the oracle's keypoints, as everywhere else.
Every frame is compared as test_gpu_parity.assert_same_frame / test_gpu_sad.assert_same_as_reference do (lists exact, poses within their
tolerances), plus the pairings' row table and the match IDs.  The references are computed once per process and never modified."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_lists as B                                           # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_gpu_parity import O                                   # noqa: E402
from test_gpu_big_lists import same_as_record                   # noqa: E402
from test_gpu_sad import assert_same_features, assert_same_as_reference      # noqa: E402

N_FRAMES = 4
# pair -> (match_method, ifm_method, svo_kernel_times names of its stage-3 filter and its tracker)
PAIRS = {"bf": (0, 0, "match_lr_filter", "track_filter"), "rbr_win": (1, 1, "match_lr_filter", "track_filter"), "sad": (2, 2, "match_lr_sad", "track_sad")}
_cache = {}


def small(golden_dir):
    if "g" not in _cache:
        g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
        _cache["g"] = g, StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    return _cache["g"]


def params(g, pair):
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    p.match_method, p.ifm_method, p.vo_use_matches_ids = PAIRS[pair][0], PAIRS[pair][1], 1
    if pair != "bf":
        p.max_y_diff, p.ifm_win_w, p.ifm_win_h = 2.0, 16, 16
    if pair == "sad":
        p.sad_max_distance = p.ifm_sad_max_distance = 1500
    return p


def reference(golden_dir, pair):
    """per frame: bf / rbr_win -- the oracle's record (big_lists.record) with its match IDs; sad -- (features, SadStream.step's record)"""
    if pair not in _cache:
        g, cam = small(golden_dir)
        p, out = params(g, pair), []
        if pair == "sad":
            st = S.SadStream(O(), p, cam)
            for t in range(N_FRAMES):
                L, R = g["L%d" % t], g["R%d" % t]
                f = S.oracle_features(O(), p, L, R, cam)
                out.append((f, st.step((L, R), f[0], f[2], f[4], f[5], f[1], f[3])))
        else:
            orc = O().Oracle(p)
            for t in range(N_FRAMES):
                rec = B.record(orc, orc.process(g["L%d" % t], g["R%d" % t], cam))
                rec["ids"] = orc.match_ids(0).copy()
                out.append(rec)
        _cache[pair] = out
    return _cache[pair]


@pytest.mark.parametrize("pair", list(PAIRS))
def test_small_sequence_has_something_to_compare(golden_dir, pair):
    """from the references alone: pairings on every frame, and every later frame valid with tracked pairs -- no case below passes on
    an empty list"""
    for t, rec in enumerate(reference(golden_dir, pair)):
        m, tracked, valid = (rec[1]["matches"], rec[1]["tracked"], rec[1]["valid"]) if pair == "sad" else (rec["m"], rec["tracked"], rec["valid"])
        assert len(m) >= 60, (pair, t, len(m))
        if t:
            assert valid and len(tracked) >= 20, (pair, t, valid, len(tracked))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("max_kps", [4096, 8192, 16384])
def test_small_sequence_at_every_context_size(golden_dir, max_kps, pair):
    g, cam = small(golden_dir)
    ref = reference(golden_dir, pair)
    ctx = hip.Context(n_lanes=1, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=max_kps, max_cand=1 << 15, kernel_times=True)
    ctx.set_params(params(g, pair)); ctx.set_camera(cam)
    for t in range(N_FRAMES):
        ctx.process_host([(g["L%d" % t], g["R%d" % t])])
        tag = "%s max_kps %d t=%d" % (pair, max_kps, t)
        if pair == "sad":
            r = ctx.result(0)
            assert_same_features(ctx, 0, ref[t][0], tag)
            assert_same_as_reference(ctx, 0, r, ref[t][1], tag, ids=True)
        else:
            r = same_as_record(ctx, 0, ref[t], tag)
            assert (ctx.match_ids(0, 0) == ref[t]["ids"]).all(), (tag, "match IDs")
        assert r.status == 0 and ctx.status_word(0) == 0, (tag, r.status, ctx.status_word(0))
    assert r.valid and r.tracked_feats_from_last_frame >= 20 and len(ctx.tracked(0)) == r.tracked_feats_from_last_frame, (tag, r.valid, r.tracked_feats_from_last_frame)
    # the kernels the case is about were launched every frame, under the names they have always had (k_match_ids is timed with k_track_finalize)
    kt = ctx.kernel_times()
    lr, trk = PAIRS[pair][2], PAIRS[pair][3]
    if pair == "bf" and max_kps == 16384:
        trk = "track_filter_64"
    assert kt[lr][1] == N_FRAMES and kt[trk][1] == N_FRAMES and kt["track_finalize"][1] == 2 * N_FRAMES, (tag, {k: v[1] for k, v in kt.items() if v[1]})
    ctx.close()
