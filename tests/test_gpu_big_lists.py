"""Contexts with max_kps = 16384: every selector that works at 8192 entries per octave works at 16384, bit-exact against the oracle.

Inputs and parameter sets are those of tests/big_lists.py (cases A-D; their properties are asserted from the oracle alone in
test_big_lists_cpu.py and again here before anything is compared).  Lists are compared exactly, poses and residuals within the
tolerances of test_gpu_parity.assert_same_frame.  The oracle's records of a case are computed once per process and shared."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import big_lists as B                                           # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_gpu_parity import O, assert_same_frame, POSE_TOL_M, POSE_TOL_RAD      # noqa: E402
from test_gpu_sad import assert_same_features, assert_same_as_reference         # noqa: E402

pytestmark = pytest.mark.gpu

# the kernel instantiations only a 16384-entry context launches, by their svo_kernel_times names
NEW_KERNELS = ("select_8192", "nms_rowsort_16", "hamming_lr_wide", "hamming_track_wide", "track_filter_64")


def big_context(n_lanes=1, **kw):
    ctx = hip.Context(n_lanes=n_lanes, max_w=B.W, max_h=B.H, max_kps=B.MAX_KPS, max_cand=B.MAX_CAND, **kw)
    ctx.set_camera(B.camera())
    return ctx


def in_range(n):
    return B.LO < n <= B.HI


def same_as_record(ctx, lane, rec, tag):
    r = ctx.result(lane)
    assert_same_frame(ctx, lane, B.Replay(rec), r, rec["result"], tag)
    assert (ctx.matches_row_index(lane, 0) == rec["mri"]).all(), (tag, "row table of the pairings")
    return r


def test_create_accepts_16384_and_nothing_else_new():
    """svo_create: 16384 is a legal max_kps (it was SVO_ERR_ARG); 32768 and a value that is no power of two still are not"""
    ctx = hip.Context(n_lanes=1, max_w=640, max_h=480, max_kps=16384, max_cand=1 << 16)
    assert ctx.h
    ctx.close()
    for bad in (32768, 12000):
        with pytest.raises(hip.SvoError, match="invalid argument"):
            hip.Context(n_lanes=1, max_w=640, max_h=480, max_kps=bad, max_cand=1 << 16)


def test_case_a_orb_eight_levels():
    """ORB x 8 levels, orb_nfeats 10900: 16350 corners through k_select<8192> / k_select_sort<8192>, the NMS and row sort on 16384 keys
    (k_nms_rowsort<16>), 9.7 k x 9.7 k descriptors through the wide matcher, Gauss-Newton on more than 1024 tracks"""
    recs = B.oracle_run(O(), "A", B.params_a())
    for t, r in enumerate(recs):
        assert in_range(len(r["kl"][0])) and in_range(len(r["kr"][0])), (t, len(r["kl"][0]), len(r["kr"][0]))
        assert not t or (r["valid"] and len(r["tracked"]) > 1000), (t, r["valid"], len(r["tracked"]))
    ctx = big_context()
    # one step further does not fit: 16500 keypoints asked of the detector -- refused with the numbers before any frame
    with pytest.raises(hip.SvoError, match=r"capacity.*16500 keypoints.*max_kps is 16384"):
        ctx.set_params(B.params_a(11000))
    ctx.set_params(B.params_a())
    for t, (L, R) in enumerate(B.frames()):
        ctx.process_host([(L, R)])
        r = same_as_record(ctx, 0, recs[t], "A t=%d" % t)
        assert r.detected_left[0] > B.LO and r.status == 0 and ctx.status_word(0) == 0, (t, r.detected_left[0], r.status)
    ctx.close()


@pytest.mark.parametrize("ifm", [0, 1])
def test_case_b_every_fast_corner_pairings_above_8192(ifm):
    """FAST+ORB, one octave, no NMS, threshold 5: 14.4 k keypoints per image in raster order, 9.3 k row-by-row pairings, then the
    brute-force tracker (k_hamming_f4<true> in its pairing-list mode, k_track_filter<64>: more than 8192 candidates in the joint
    collision filter) or the 40 x 40 window tracker; the RANSAC sees more than 4000 point pairs, Gauss-Newton more than 1024 tracks"""
    recs = B.oracle_run(O(), "B%d" % ifm, B.params_b(ifm))
    for t, r in enumerate(recs):
        assert in_range(len(r["kl"][0])) and in_range(len(r["kr"][0])) and in_range(len(r["m"])), (t, len(r["kl"][0]), len(r["kr"][0]), len(r["m"]))
        assert not t or (r["valid"] and len(r["tracked"]) > 1000), (t, r["valid"], len(r["tracked"]))
        if t and ifm == 0:
            assert r["stats"][0] > B.LO and r["stats"][1] > 4000, r["stats"]
    ctx = big_context()
    ctx.set_params(B.params_b(ifm))
    for t, (L, R) in enumerate(B.frames()):
        ctx.process_host([(L, R)])
        r = same_as_record(ctx, 0, recs[t], "B ifm=%d t=%d" % (ifm, t))
        assert r.stereo_matches[0] > B.LO and r.status == 0 and ctx.status_word(0) == 0, (t, r.stereo_matches[0], r.status)
        if t and ifm == 0:
            assert r.track_stats[0] > B.LO, list(r.track_stats)
    ctx.close()


@pytest.mark.parametrize("one", [0, 1])
def test_case_b_prime_brute_force_matcher(one):
    """the same frames with match_method 0: 14.5 k x 14.5 k descriptors through k_hamming_f4<true>, with and without the 1-to-1 rule"""
    recs = B.oracle_run(O(), "B'%d" % one, B.params_b(0, match_method=0, one_to_one=one))
    for t, r in enumerate(recs):
        assert in_range(len(r["kl"][0])) and in_range(len(r["kr"][0])) and len(r["m"]) > 4096, (t, len(r["kl"][0]), len(r["kr"][0]), len(r["m"]))
        assert not t or r["valid"], (t, r["error_code"])
        assert r["m"]["trainIdx"].max() > B.LO                   # train indices beyond 13 bits are really in play
    ctx = big_context()
    ctx.set_params(B.params_b(0, match_method=0, one_to_one=one))
    for t, (L, R) in enumerate(B.frames()):
        ctx.process_host([(L, R)])
        r = same_as_record(ctx, 0, recs[t], "B' 1to1=%d t=%d" % (one, t))
        assert r.status == 0 and ctx.status_word(0) == 0
    ctx.close()


def test_case_b_prime_int8_form_of_the_matcher(tmp_path):
    """the A/B-only int8 form of the brute force (SVO_HAM_FP4=0, libsvo_hip_ab.so) packs 13 bits of train index in its accumulator; its
    16384-row kernel rebuilds the key per tile.  Two frames of case B' (1-to-1) in a fresh process under the knob (the library reads
    it once per process), matcher and tracker, every list against the oracle's"""
    import subprocess
    recs = B.oracle_run(O(), "B'1", B.params_b(0, match_method=0, one_to_one=1))
    assert all(in_range(len(r["kl"][0])) and r["m"]["trainIdx"].max() > B.LO for r in recs[:2]) and recs[1]["valid"]
    want = str(tmp_path / "want.npz")
    np.savez(want, **{"%s%d" % (k, t): (recs[t][k][0] if k in ("kl", "kr") else recs[t][k]) for t in (0, 1) for k in ("kl", "kr", "m", "tracked")})
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import os, sys, numpy as np\n"
        "sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, 'tests'))\n"
        "from stereo_vo_amd import hip\n"
        "import big_lists as B\n"
        "g = np.load(%r)\n"
        "ctx = hip.Context(n_lanes=1, max_w=B.W, max_h=B.H, max_kps=B.MAX_KPS, max_cand=B.MAX_CAND, kernel_times=True)\n"
        "ctx.set_params(B.params_b(0, match_method=0, one_to_one=1)); ctx.set_camera(B.camera())\n"
        "for t in (0, 1):\n"
        "    ctx.process_host([B.frames()[t]])\n"
        "    r = ctx.result(0)\n"
        "    for side, k in ((0, 'kl'), (1, 'kr')):\n"
        "        assert ctx.keypoints(0, 0, side)[0].tobytes() == g['%%s%%d' %% (k, t)].tobytes(), ('keypoints', t, side)\n"
        "    assert ctx.matches(0).tobytes() == g['m%%d' %% t].tobytes(), ('pairings', t, len(ctx.matches(0)), len(g['m%%d' %% t]))\n"
        "    assert ctx.tracked(0).tobytes() == g['tracked%%d' %% t].tobytes(), ('tracked', t)\n"
        "    assert r.status == 0 and ctx.status_word(0) == 0\n"
        "kt = ctx.kernel_times()\n"
        "assert kt['hamming_lr_wide'][1] == 2 and kt['hamming_track_wide'][1] == 2 and kt['hamming_lr'][1] == 0, kt\n"
        "ctx.close(); print('same')\n"
    ) % (root, root, want)
    env = dict(os.environ, SVO_HAM_FP4="0", SVO_HIP_LIB=os.path.join(root, "stereo_vo_amd", "libsvo_hip_ab.so"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "same" in out.stdout, (out.stdout[-400:], out.stderr[-1500:])


def test_case_c_sad_matchers():
    """case A's keypoints under smSAD / ifmSAD (thresholds 400, window 40 x 40) against the walks of tests/sad_ref.py"""
    p, cam = B.params_c(), B.camera()
    st = S.SadStream(O(), p, cam)
    ctx = big_context()
    ctx.set_params(p)
    for t, (L, R) in enumerate(B.frames()[:2]):
        f = S.oracle_features(O(), p, L, R, cam)
        assert in_range(len(f[0])) and in_range(len(f[2])), (t, len(f[0]), len(f[2]))
        o = st.step((L, R), f[0], f[2], f[4], f[5], f[1], f[3], ctx.orb_threshold())
        assert len(o["matches"]) > 1000, (t, len(o["matches"]))
        if t:
            assert o["valid"] and len(o["candidates"]) >= 50, (o["valid"], len(o["candidates"]))
        ctx.process_host([(L, R)])
        assert_same_features(ctx, 0, f, "C t=%d" % t)
        assert_same_as_reference(ctx, 0, ctx.result(0), o, "C t=%d" % t)
    ctx.close()


@pytest.mark.parametrize("ifm", [0, 1])
def test_case_d_exactly_full_lists(ifm):
    """stage 4 alone on caller lists of exactly 16384 keypoints per side and 16384 pairings, previous and current (case B's oracle
    lists with entries repeated: tied distances, colliding claims), both trackers, against the oracle's stage 4"""
    recs = B.oracle_run(O(), "B0", B.params_b(0))
    prev, cur = B.full_lists(recs[0]), B.full_lists(recs[1])
    p = B.params_b(ifm)
    zeros = np.zeros(B.H + 1, np.int64)
    want, want_ts = O().track(p, p.orb_max_distance, prev[0], prev[1], prev[2], prev[3], prev[4], prev[5] if ifm else zeros,
                              cur[0], cur[1], cur[2], cur[3], cur[4], cur[5] if ifm else zeros, B.W, B.H, stats=True)
    assert len(want) > 100, len(want)
    if ifm == 0:
        assert want_ts[0] > B.LO and want_ts[0] > want_ts[1], list(want_ts)         # more than 8192 candidates, some lost to collisions
    ctx = big_context()
    ctx.set_params(p)
    for which, f in ((1, prev), (0, cur)):
        ctx.put_features(0, which, 0, f[0], f[1], B.W, B.H); ctx.put_features(0, which, 1, f[2], f[3], B.W, B.H)
        ctx.put_matches(0, which, f[4])
        assert (ctx.matches_row_index(0, which) == f[5]).all()
    ctx.run_stages(hip.RUN_TRACK)
    got, ts = ctx.tracked(0), ctx.result(0).track_stats
    assert got.tobytes() == want.tobytes(), (len(got), len(want))
    assert [int(v) for v in ts[:8]] == [int(v) for v in want_ts], (list(ts[:8]), list(want_ts))
    assert ctx.status_word(0) == 0
    last = B.HI - 1
    in_tracked = (got["first"] == last).any() or (got["second"] == last).any() if len(got) else False
    in_pairing = all((f[4]["queryIdx"] == last).any() and (f[4]["trainIdx"] == last).any() for f in (prev, cur))
    assert in_tracked or in_pairing
    ctx.close()


def test_case_e_overflow_stays_a_flag():
    """case B at FAST threshold 4: more corners than the lists hold.  Status bit 2 and nothing else, every list cut at 16384, and
    the context processes a threshold-5 frame correctly after svo_reset"""
    L, R = B.frames()[0]
    n4 = [len(O().fast_orb_detect(img, 4)[0]) for img in (L, R)]
    assert min(n4) > B.HI, n4
    recs = B.oracle_run(O(), "B0", B.params_b(0))
    ctx = big_context()
    ctx.set_params(B.params_b(0, fast_th=4))
    ctx.process_host([(L, R)])
    r = ctx.result(0)
    assert r.status == 2 and ctx.status_word(0) == 2, (r.status, ctx.status_word(0))
    assert r.detected_left[0] == B.HI and r.detected_right[0] == B.HI and 0 < r.stereo_matches[0] <= B.HI
    assert len(ctx.keypoints(0, 0, 0)[0]) == B.HI and len(ctx.keypoints(0, 0, 1)[0]) == B.HI and len(ctx.matches(0)) == r.stereo_matches[0]
    ctx.reset()
    ctx.set_params(B.params_b(0))
    for t in (0, 1):
        ctx.process_host([B.frames()[t]])
        r = same_as_record(ctx, 0, recs[t], "after the overflow t=%d" % t)
        assert r.status == 0 and ctx.status_word(0) == 0
    ctx.close()


def test_case_f_graphs_and_two_lanes():
    """case A under svo_use_graphs (captured, then replayed), and in a two-lane context whose second lane runs one frame ahead"""
    recs = B.oracle_run(O(), "A", B.params_a())
    ahead = B.oracle_run(O(), "A from frame 1", B.params_a(), first=1)
    assert all(in_range(len(r["kl"][0])) for r in recs + ahead) and ahead[1]["valid"]
    fr = B.frames()
    ctx = big_context()
    ctx.set_params(B.params_a()); ctx.use_graphs(True)
    for rep in range(2):
        ctx.reset()
        for t in range(3):
            ctx.process_host([fr[t]])
            same_as_record(ctx, 0, recs[t], "graphs pass %d t=%d" % (rep, t))
    ctx.close()
    two = big_context(n_lanes=2)
    two.set_params(B.params_a())
    for t in range(2):
        two.process_host([fr[t], fr[t + 1]])
        same_as_record(two, 0, recs[t], "two lanes, lane 0 t=%d" % t)
        same_as_record(two, 1, ahead[t], "two lanes, lane 1 t=%d" % t)
        assert two.status_word(0) == 0 and two.status_word(1) == 0
    two.close()


def test_case_f_hand_over_and_state_file(tmp_path):
    """case A: one svo_export_frame -> svo_import_frame hop between two 16384-entry contexts equals the sequential run, and a frame
    with more than 8192 keypoints survives svo_save_state / svo_load_state"""
    import torch
    from stereo_vo_amd.state_file import read_state
    recs = B.oracle_run(O(), "A", B.params_a())
    fr = B.frames()
    a, b, c = big_context(), big_context(), big_context()
    for x in (a, b, c):
        x.set_params(B.params_a())
    for t in range(2):
        a.process_host([fr[t]]); a.wait()
    # the importer runs stages 2-3 of its own frame first, takes the record as its previous frame, then runs stages 4-5
    b.process_host([fr[0]]); b.wait()                          # (an unrelated frame of its own behind it, for the record to replace)
    b.process_host([fr[2]], hip.RUN_DETECT | hip.RUN_MATCH)
    nb = a.handover_bytes()
    assert nb == b.handover_bytes() and nb > 2 * B.HI * (28 + 32)
    blob = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a.export_frame(blob.data_ptr(), nb); a.wait()
    b.import_frame(blob.data_ptr(), nb); b.wait()
    assert b.status_word(0) & 4 == 0
    b.run_stages(hip.RUN_TRACK | hip.RUN_OPTIMIZE)
    same_as_record(b, 0, recs[2], "after the hop")
    path = str(tmp_path / "big_state.bin")
    a.save_state(0, path)
    s = read_state(path)
    for which, name, rec in ((1, "pre", recs[0]), (0, "cur", recs[1])):
        for side, sn in ((0, "left"), (1, "right")):
            ko, do = rec["kr" if side else "kl"]
            assert len(ko) > B.LO and s[name][sn][0].tobytes() == ko.tobytes() and (s[name][sn][1] == do).all(), (name, sn)
        assert s[name]["matches"].tobytes() == rec["m"].tobytes(), name
    c.load_state(0, path)
    c.process_host([fr[2]])
    rc, ro = c.result(0), recs[2]["result"]
    for side in (0, 1):
        assert c.keypoints(0, 0, side)[0].tobytes() == recs[2]["kr" if side else "kl"][0].tobytes()
    assert c.matches(0).tobytes() == recs[2]["m"].tobytes() and c.tracked(0).tobytes() == recs[2]["tracked"].tobytes()
    # (the file does not carry m_last_computed_pose: the resumed lane starts its Gauss-Newton from the identity)
    assert (rc.valid, rc.error_code, rc.tracked_feats_from_last_frame) == (ro.valid, ro.error_code, ro.tracked_feats_from_last_frame)
    dp = np.abs(np.array(rc.outPose) - np.array(ro.outPose))
    assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, dp
    for x in (a, b, c):
        x.close()


def test_case_g_nothing_moved_below():
    """the inputs of test_five_thousand_keypoints_in_one_octave give the same lists on a 16384-entry context as on the 8192-entry one;
    with kernel_times on, contexts of 4096 and 8192 entries launch none of the new instantiations, a 16384-entry one all of them"""
    from stereo_vo_amd.abi import north_star_params
    fr, cam = B.frames(), B.camera()
    p = north_star_params(hip.default_params(), orb_nfeats=5000)
    snaps = {}
    for mk in (8192, 16384):
        ctx = hip.Context(n_lanes=1, max_w=B.W, max_h=B.H, max_kps=mk, max_cand=B.MAX_CAND, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam)
        out = []
        for t in range(3):
            ctx.process_host([fr[t]])
            r = ctx.result(0)
            out.append((ctx.keypoints(0, 0, 0)[0].tobytes(), ctx.keypoints(0, 0, 0)[1].tobytes(), ctx.keypoints(0, 0, 1)[0].tobytes(), ctx.keypoints(0, 0, 1)[1].tobytes(),
                        ctx.matches(0).tobytes(), ctx.tracked(0).tobytes(), tuple(r.track_stats), r.valid, r.error_code, r.n_residual, r.n_outliers,
                        ctx.outliers(0).tobytes(), r.status, tuple(r.outPose)))
            assert r.detected_left[0] > 4096 and r.status == 0
        snaps[mk] = out
        kt = ctx.kernel_times()
        if mk == 8192:
            assert [kt[k][1] for k in NEW_KERNELS] == [0] * 5, {k: kt[k] for k in NEW_KERNELS}
            assert kt["select"][1] == 3 and kt["nms_rowsort"][1] == 3 and kt["hamming_lr"][1] == 3 and kt["hamming_track"][1] == 3 and kt["track_filter"][1] == 3
        else:
            # (7500 keypoints asked of the detector: the NMS runs on 8192 keys, k_nms_rowsort<8>, in this context too)
            assert [kt[k][1] for k in NEW_KERNELS] == [3, 0, 3, 3, 3], {k: kt[k] for k in NEW_KERNELS}
            assert kt["nms_rowsort"][1] == 3 and kt["select"][1] == 0 and kt["hamming_lr"][1] == 0 and kt["track_filter"][1] == 0
        ctx.close()
    for t in range(3):
        assert snaps[8192][t][:-1] == snaps[16384][t][:-1], (t, [i for i, (x, y) in enumerate(zip(snaps[8192][t], snaps[16384][t])) if x != y])
        dp = np.abs(np.array(snaps[8192][t][-1]) - np.array(snaps[16384][t][-1]))
        assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (t, dp)
    # a 4096-entry context on a request that fits it
    q = north_star_params(hip.default_params(), orb_nfeats=2000)
    small = hip.Context(n_lanes=1, max_w=B.W, max_h=B.H, max_kps=4096, max_cand=B.MAX_CAND, kernel_times=True)
    small.set_params(q); small.set_camera(cam)
    for t in range(2):
        small.process_host([fr[t]])
    kt = small.kernel_times()
    assert [kt[k][1] for k in NEW_KERNELS] == [0] * 5 and kt["select"][1] == 2 and kt["track_filter"][1] == 2, kt
    small.close()
    # and the 16384-entry context of case A launches the sixteen-key NMS
    big = big_context(kernel_times=True)
    big.set_params(B.params_a())
    big.process_host([fr[0]])
    kt = big.kernel_times()
    assert kt["nms_rowsort_16"][1] == 1 and kt["nms_rowsort"][1] == 0 and kt["select_8192"][1] == 1, kt
    big.close()
