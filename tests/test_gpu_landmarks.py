"""The landmark records of stage 5 (svo_set_landmarks, k_landmarks in csrc/k_gn.hip) held to the 50-digit reference of
tests/landmarks_ref.py.

Lanes are filled through svo_put_* and run with SVO_RUN_OPTIMIZE alone.  With initial_max_iters = max_iters = 0 stage 5 iterates
nowhere: under use_custom_initial_pose the returned delta is ZERO bit for bit (the start SVO_RUN_OPTIMIZE takes, S5:504-505 with
P:338's default argument), the mask is the NMS survivors, and every record is one evaluation at a known point -- the point
tests/test_landmarks_ref_cpu.py qualifies without a GPU.  A non-zero delta known bit for bit is reached through the warm start.  The
tolerances are FACTOR = 16 times what a plain float64 walk of the same formulas reaches (constants and their measurement: that file).
Then the tracked counts on the edges of the grid, three octaves and the cut at max_kps, degenerate pairings, the lane states, the
interplay with the pose covariance, real frames with the feature on and off, several lanes, idle lanes, graphs, the other block sizes
of k_gauss_newton, the device copy, the launch count and the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stage5_ref as S
import pose_cov_ref as Pc
import landmarks_ref as Lr
from stereo_vo_amd import hip
from stereo_vo_amd.abi import (Landmark, LandmarksInfo, PoseCov, StereoCamera, north_star_params, DM_FAST_ORB,
                               LMK_FINITE, LMK_INLIER, LMK_USED, LMK_POSE, LMK_POSE_TERM, LMK_NONE, LMK_OK, LMK_POINTS_ONLY)
from test_landmarks_ref_cpu import K_XYZ, K_COV, K_RES, FACTOR, DMID_MIN

pytestmark = pytest.mark.gpu

EPS = Lr.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = Lr.gpu_cases()
BY_NAME = {c[0]: c for c in CASES}
_ids = lambda cases: [c[0] for c in cases]


def base_params():
    return north_star_params(hip.default_params(), orb_nfeats=40)


def new_context(max_kps, n_lanes=1, **kw):
    return hip.Context(n_lanes=n_lanes, max_w=S.W, max_h=S.H, max_kps=max_kps, max_cand=1 << 15, **kw)


@pytest.fixture(scope="module")
def contexts():
    """one one-lane context per max_kps with the feature on (std_noise_pixels 1), shared by the tests of this file"""
    made = {}
    def get(max_kps):
        if max_kps not in made:
            made[max_kps] = new_context(max_kps)
            made[max_kps].set_camera(S.camera())
        made[max_kps].set_landmarks(True, 1.0)
        return made[max_kps]
    yield get
    for c in made.values(): c.close()


def put_lists(ctx, lane, lists, octave=None):
    """the seven lists of one octave (None: octave 0 through svo_put_tracked, which empties the lane's other octaves)"""
    t, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r = lists
    o = 0 if octave is None else octave
    ctx.put_features(lane, 1, 0, pre_l, None, S.W, S.H, o); ctx.put_features(lane, 1, 1, pre_r, None, S.W, S.H, o)
    ctx.put_features(lane, 0, 0, cur_l, None, S.W, S.H, o); ctx.put_features(lane, 0, 1, cur_r, None, S.W, S.H, o)
    ctx.put_matches(lane, 1, pre_m, o); ctx.put_matches(lane, 0, cur_m, o)
    ctx.put_tracked(lane, t, octave)


def as_dict(rec):
    return {n: rec[n] for n in rec.dtype.names}


def check_records(tag, info, rec, f, ref, kappa=0.0, state=LMK_OK, std=1.0, ids=None):
    """the lane's records against the reference: integers, indices, octaves, flags and IDs exact; doubles within FACTOR x the CPU test's
    constants; every covariance positive semi-definite from its six stored entries; records that are not finite all zero"""
    T = len(ref["flags"])
    assert (info.n, info.state, info.std_noise_pixels) == (T, state, std), (tag, info.n, info.state, info.std_noise_pixels)
    assert len(rec) == T
    assert np.array_equal(rec["prev_match"], f["prev_match"]) and np.array_equal(rec["cur_match"], f["cur_match"]) and np.array_equal(rec["octave"], f["octave"]), tag
    assert np.array_equal(rec["flags"], ref["flags"]), (tag, "flags", np.nonzero(rec["flags"] != ref["flags"])[0][:8], rec["flags"][:8], ref["flags"][:8])
    assert not rec["reserved"].any()
    assert np.array_equal(rec["match_id"], np.full(T, -1) if ids is None else ids), (tag, "match IDs")
    fin = (ref["flags"] & LMK_FINITE) != 0
    assert (info.n_finite, info.n_inliers) == (int(fin.sum()), int(((ref["flags"] & LMK_INLIER) != 0).sum())), (tag, info.n_finite, info.n_inliers)
    for name in ("xyz_prev", "cov_prev", "xyz_cur", "cov_cur", "residual"):
        assert not rec[name][~fin].any(), (tag, name, "every double of a record that is not finite is 0")
        assert np.isfinite(rec[name]).all(), (tag, name)
    pose = (ref["flags"] & LMK_POSE) != 0
    assert not rec["xyz_cur"][~pose].any() and not rec["cov_cur"][~pose].any() and not rec["residual"][(ref["flags"] & LMK_USED) == 0].any(), tag
    e = Lr.errors(as_dict(rec), ref, kappa)
    bound = dict(xyz_prev=FACTOR * K_XYZ, xyz_cur=FACTOR * K_XYZ, cov_prev=FACTOR * K_COV, cov_cur=FACTOR * K_COV, residual=FACTOR * K_RES)
    print("\n%s: T %d, finite %d, inliers %d, state %d; of the unit: %s" % (tag, T, info.n_finite, info.n_inliers, info.state,
          ", ".join("%s %.4g (bound %.4g)" % (k, e[k], bound[k]) for k in e)))
    for k in e: assert e[k] <= bound[k], (tag, k, e[k], bound[k])
    for name in ("cov_prev", "cov_cur"):
        sel = fin if name == "cov_prev" else (fin & pose)
        if sel.any():
            ratio = Lr.min_eigenvalue_ratio(rec[name][sel])
            assert (ratio >= -8 * EPS).all(), (tag, name, "not positive semi-definite", ratio.min())
            assert (np.linalg.eigvalsh(Lr.tri_to_mat(rec[name][sel]))[:, 2] > 0).all(), (tag, name)


def run_zero(ctx, case, with_cov, robust=1):
    """SVO_RUN_OPTIMIZE with both iteration limits at zero from the custom (zero) start: (result, info, records)"""
    ctx.set_pose_covariance(with_cov)
    ctx.set_params(Pc.zero_iteration_params(base_params(), robust, case[3]))
    put_lists(ctx, 0, Lr.case_scene(case))
    ctx.run_stages(hip.RUN_OPTIMIZE)
    r = ctx.result(0)
    assert r.valid and (r.num_it, r.num_it_final, r.error_code, r.status) == (0, 0, 0, 0), (case[0], r.valid, r.num_it, r.num_it_final, r.error_code, r.status)
    assert bytes(r.delta) == Lr.ZERO.tobytes(), (case[0], "the returned delta is the zero start, bit for bit")
    info, rec = ctx.landmarks(0)
    return r, info, rec


@pytest.mark.parametrize("with_cov", [True, False], ids=["pose-cov", "no-pose-cov"])
@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_single_evaluation_at_a_known_pose(contexts, case, with_cov):
    """T = 8, 63 / 64 / 65 (a wave of the grid and one more), 255 / 256 / 257 (a block and one more), 1100 on 2048 entries (above
    LdsGaussNewton::lc(): k_gauss_newton's scratch path), T = max_kps at 64, a mask that removes a real share, the degenerate pairings
    beside good ones and the collinear scene (SVO_COV_RANK_DEFICIENT: no pose term).  With the pose covariance on, cov_cur includes
    D cov_delta D^T exactly where the lane's record is SVO_COV_OK / SVO_COV_DELTA_ONLY; with it off SVO_LMK_POSE_TERM is clear and
    cov_cur = R cov_prev R^T."""
    name, mk, build, md = case
    ctx = contexts(mk)
    f, surv, pc, ref = Lr.case_reference(case, Lr.ZERO, 1.0, with_cov)
    r, info, rec = run_zero(ctx, case, with_cov)
    t = ctx.tracked(0)
    assert np.array_equal(rec["prev_match"], t["first"]) and np.array_equal(rec["cur_match"], t["second"]), "svo_get_tracked_oct"
    if with_cov:
        cov = ctx.pose_covariance(0)
        term = cov.state in (Pc.COV_OK, Pc.COV_DELTA_ONLY)
        assert term == (name != "collinear-eps0"), (name, cov.state)
        if name == "collinear-eps0": assert cov.state == Pc.COV_RANK_DEFICIENT
        assert bool((rec["flags"] & LMK_POSE_TERM).any()) == term
    else:
        assert not (rec["flags"] & LMK_POSE_TERM).any()
        assert np.array_equal(rec["cov_cur"][rec["flags"] & LMK_POSE != 0], rec["cov_prev"][rec["flags"] & LMK_POSE != 0]), "delta = 0: R = I exactly"
    check_records("%s %s" % (name, "with the pose covariance" if with_cov else "without"), info, rec, f, ref, pc["kappa"])
    if name == "degenerate-T40":
        d = Lr.DEGENERATE
        z = rec[d["zero_den"]]
        assert z["flags"] == LMK_INLIER and not np.r_[z["xyz_prev"], z["cov_prev"], z["xyz_cur"], z["cov_cur"], z["residual"]].any()
        for k in ("negative_disparity", "far_outside"):
            assert rec[d[k]]["flags"] & LMK_FINITE and rec[d[k]]["xyz_prev"][2] < 0 and rec[d[k]]["xyz_cur"][2] < 0, k
        assert info.n_finite == info.n - 1


def test_warm_start_gives_a_nonzero_delta_known_bit_for_bit(contexts):
    """a full run stores its delta as the lane's warm start; a second call with both limits at zero starts there and returns it bit
    for bit: one evaluation at a rotation and translation that are not zero, with the pose term (the exact Rodrigues rotation and its
    derivatives away from zero).  The reference is evaluated at the delta read back, over the NMS survivors."""
    case = BY_NAME["T257-mk1024"]
    ctx = contexts(1024)
    ctx.set_pose_covariance(True); ctx.set_landmarks(True, 0.5)
    lists = Lr.case_scene(case)
    p = base_params(); p.use_previous_pose_as_initial = 1; p.use_custom_initial_pose = 0; p.min_distance = 2
    ctx.reset(0); ctx.set_params(p)
    put_lists(ctx, 0, lists)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    r1 = ctx.result(0)
    assert r1.valid and np.abs(np.array(r1.delta) - S.BASE_TRUE).max() < 5e-3, list(r1.delta)
    p.initial_max_iters = 0; p.max_iters = 0
    ctx.set_params(p)
    put_lists(ctx, 0, lists)                      # (new parameters: the lists are put again; the lane's warm start stays)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    r2 = ctx.result(0)
    assert r2.valid and (r2.num_it, r2.num_it_final) == (0, 0) and bytes(r2.delta) == bytes(r1.delta)
    delta = np.array(r2.delta)
    surv = S.nms_survivors(lists, 2)
    pc = Pc.reference(lists, S.camera(), delta, p.use_robust_kernel, p.kernel_param, surv)
    assert pc["rel_pd"] >= 1e3 and ctx.pose_covariance(0).state == Pc.COV_OK
    f = Lr.flat([lists])
    ref = Lr.reference(f["obs"], S.camera(), 0.5, delta, surv, pc["cov_delta"])
    assert ref["dmid"] >= DMID_MIN, ref["dmid"]
    info, rec = ctx.landmarks(0)
    check_records("warm start T257", info, rec, f, ref, pc["kappa"], std=0.5)
    ctx.reset(0)
    assert ctx.landmarks_info(0).state == LMK_NONE and ctx.landmarks_info(0).n == 0, "svo_reset: SVO_LMK_NONE"


def test_tracked_counts_zero_seven_and_eight(contexts):
    """T = 0: no record; T = 7: stage 5 returns early (fewer than 8 in the mask): SVO_LMK_POINTS_ONLY with the previous-frame fields;
    T = 8: every field"""
    ctx = contexts(1024)
    ctx.set_pose_covariance(True)
    ctx.set_params(Pc.zero_iteration_params(base_params(), 1, 2))
    cam = S.camera()
    for T in (0, 7, 8):
        lists = S.synthetic(cam, S.BASE_TRUE, max(T, 1), seed=900 + T, noise=0.2)
        if T == 0: lists = (lists[0][:0],) + lists[1:]
        assert int(S.nms_survivors(lists, 2).sum()) == T if T else True
        put_lists(ctx, 0, lists)
        ctx.run_stages(hip.RUN_OPTIMIZE)
        r = ctx.result(0)
        info, rec = ctx.landmarks(0)
        f = Lr.flat([lists])
        assert bool(r.valid) == (T == 8), (T, r.valid)
        if T == 8:
            surv = S.nms_survivors(lists, 2)
            pc = Pc.reference(lists, cam, Lr.ZERO, 1, 3.0, surv)
            check_records("T8", info, rec, f, Lr.reference(f["obs"], cam, 1.0, Lr.ZERO, surv, pc["cov_delta"]), pc["kappa"])
        else:
            check_records("T%d" % T, info, rec, f, Lr.reference(f["obs"], cam, 1.0), state=LMK_POINTS_ONLY)
            assert ctx.pose_covariance(0).state == Pc.COV_NONE
            if T: assert (rec["flags"] == LMK_FINITE).all() and rec["xyz_prev"][:, 2].min() > 1.0


def octave_params():
    p = base_params()
    p.detect_method = DM_FAST_ORB; p.nOctaves = 3
    return Pc.zero_iteration_params(p, 1, 2)


@pytest.mark.parametrize("counts", [(30, 20, 12), (50, 45, 40)], ids=["T62", "T135-cut-at-128"])
def test_three_octaves_and_the_cut_at_max_kps(counts):
    """pairings in each of three octaves through svo_put_*_oct: scale_norm 1 / 2 / 4 brings every octave's pixels back to the camera's,
    the records are octave by octave with their `octave`, and 135 pairings on a 128-entry context are cut as stage 5 cuts them:
    status bit 2 and n = max_kps"""
    cam = S.camera()
    ctx = new_context(128, max_octaves=3)
    ctx.set_camera(cam); ctx.set_params(octave_params()); ctx.set_landmarks(True)
    octs = Lr.octave_scene(cam, counts)
    for o, lists in enumerate(octs): put_lists(ctx, 0, lists, o)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    r = ctx.result(0)
    total = sum(counts)
    T = min(total, 128)
    assert r.valid and bytes(r.delta) == Lr.ZERO.tobytes() and r.tracked_feats_from_last_frame == T
    assert (r.status & 2 != 0) == (total > 128) and (ctx.status_word(0) & 2 != 0) == (total > 128)
    f = Lr.flat(octs, cap=T)
    for o in range(3):
        t = ctx.tracked(0, o)
        sel = f["octave"] == o
        assert np.array_equal(f["prev_match"][sel], t["first"][:sel.sum()]) and np.array_equal(f["cur_match"][sel], t["second"][:sel.sum()])
    # the mask of the cut list: the NMS walk over the flat previous-left pixels
    flat_lists = Lr.lists_of_obs(f["obs"])
    resp = np.concatenate([S.gather(l)[0]["response"] for l in octs])[:T]
    flat_lists[3]["response"] = resp
    surv = S.nms_survivors(flat_lists, 2)
    ref = Lr.reference(f["obs"], cam, 1.0, Lr.ZERO, surv, None)
    info, rec = ctx.landmarks(0)
    check_records("three octaves %s" % (counts,), info, rec, f, ref)
    assert sorted(set(rec["octave"])) == ([0, 1, 2] if total <= 128 else sorted(set(f["octave"]))) and (np.diff(rec["octave"]) >= 0).all()
    assert rec["xyz_prev"][:, 2].min() > 1.0, "every octave triangulates in the camera's units"
    ctx.close()


def full_case_params(name):
    case = {c[0]: c for c in S.full_run_cases()}[name]
    return case, S.with_overrides(base_params(), case[3])


def test_states_first_frame_and_cost_abort(contexts):
    """no previous frame: SVO_LMK_NONE, n = 0.  A cost abort (stage 5 runs to its end and returns valid = 0): SVO_LMK_POINTS_ONLY with the
    previous-frame fields of every pairing and nothing of the pose"""
    cam = S.camera()
    ctx = new_context(1024)
    ctx.set_camera(cam); ctx.set_params(base_params()); ctx.set_landmarks(True); ctx.set_pose_covariance(True)
    assert ctx.landmarks_info(0).state == LMK_NONE and ctx.landmarks_info(0).n == 0, "no call yet"
    lists = Lr.case_scene(BY_NAME["T65-mk1024"])
    t, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r = lists
    ctx.put_features(0, 0, 0, cur_l, None, S.W, S.H); ctx.put_features(0, 0, 1, cur_r, None, S.W, S.H); ctx.put_matches(0, 0, cur_m)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    info, rec = ctx.landmarks(0)
    assert (info.state, info.n, info.n_finite, info.n_inliers) == (LMK_NONE, 0, 0, 0) and len(rec) == 0 and not ctx.result(0).valid
    case, p = full_case_params("stage1-cost-abort")
    ctx.set_params(p)
    lists = case[2](cam)
    put_lists(ctx, 0, lists)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    r = ctx.result(0)
    assert not r.valid and r.error_code == 2, (r.valid, r.error_code)
    info, rec = ctx.landmarks(0)
    f = Lr.flat([lists])
    check_records("cost abort", info, rec, f, Lr.reference(f["obs"], cam, 1.0), state=LMK_POINTS_ONLY)
    assert (rec["flags"] == LMK_FINITE).all() and ctx.pose_covariance(0).state == Pc.COV_NONE
    ctx.close()


def small_sequence():
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_small_seq.npz"))
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    return g, cam, p, [(g["L%d" % t], g["R%d" % t]) for t in range(4)]


def seq_context(g, **kw):
    return hip.Context(n_lanes=1, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=1024, max_cand=1 << 15, **kw)


def lane_lists(ctx, lane=0):
    """the seven lists of the frame just processed, through the getters"""
    return (ctx.tracked(lane), ctx.matches(lane, 1), ctx.matches(lane, 0), ctx.keypoints(lane, 1, 0)[0], ctx.keypoints(lane, 1, 1)[0],
            ctx.keypoints(lane, 0, 0)[0], ctx.keypoints(lane, 0, 1)[0])


def everything(ctx):
    """every observable list and record of lane 0 as bytes"""
    out = [bytes(ctx.result(0)), ctx.tracked(0).tobytes(), ctx.residuals(0).tobytes(), ctx.outliers(0).tobytes(), ctx.status_word(0)]
    for which in (0, 1):
        out += [ctx.matches(0, which).tobytes(), ctx.match_ids(0, which).tobytes()]
        for side in (0, 1):
            k, d = ctx.keypoints(0, which, side)
            out += [k.tobytes(), d.tobytes()]
    return out


def test_bad_tracking_gives_points_only_on_real_frames():
    """bad_tracking_th above every tracked count: stage 4 reports voecBadTracking, k_gauss_newton returns before its gather, and the
    records still hold the previous-frame fields of every tracked pairing (the kernel gathers for itself), SVO_LMK_POINTS_ONLY"""
    g, cam, p, frames = small_sequence()
    p.bad_tracking_th = 100000
    ctx = seq_context(g); ctx.set_params(p); ctx.set_camera(cam); ctx.set_landmarks(True, 2.0)
    ctx.process_host([frames[0]])
    assert (ctx.landmarks_info(0).state, ctx.landmarks_info(0).n) == (LMK_NONE, 0), "first frame"
    ctx.process_host([frames[1]])
    r = ctx.result(0)
    assert not r.valid and r.error_code == 5
    lists = lane_lists(ctx)
    assert len(lists[0]) >= 20
    info, rec = ctx.landmarks(0)
    f = Lr.flat([lists])
    check_records("bad tracking", info, rec, f, Lr.reference(f["obs"], cam, 2.0), state=LMK_POINTS_ONLY, std=2.0)
    ctx.close()


def test_real_frames_on_and_off_ids_launch_counts_and_graphs():
    """over the committed sequence: svo_result, every list getter and the residuals are bit for bit the same with the feature on, off
    after on, and never on; the pose-covariance record is too; "landmarks" is listed and counts one call per stage-5 enqueue only
    while on; the records of a valid frame agree with the reference at the returned delta over the returned inliers, with the current
    frame's match IDs; a captured graph replays the same records and toggling drops the graphs"""
    g, cam, p, frames = small_sequence()
    p.vo_use_matches_ids = 1
    never = seq_context(g, kernel_times=True); never.set_params(p); never.set_camera(cam); never.set_pose_covariance(True)
    want, want_cov = [], []
    for pair in frames:
        never.process_host([pair]); want.append(everything(never)); want_cov.append(bytes(never.pose_covariance(0)))
    kt_never = never.kernel_times(appended=True)
    assert "landmarks" not in kt_never and list(kt_never)[-1] == "pose_covariance"
    rc = never.L.svo_get_landmarks_info(never.h, 0, C.byref(LandmarksInfo()))
    assert rc == -6 and b"svo_set_landmarks" in never.L.svo_last_error(never.h)
    assert never.L.svo_get_landmarks(never.h, 0, None, 0) == -6 and never.L.svo_copy_landmarks_async(never.h, C.c_void_p(8), None, 0) == -6
    assert never.landmarks_enabled() == (False, 1.0)
    never.close()
    on = seq_context(g, kernel_times=True); on.set_params(p); on.set_camera(cam); on.set_pose_covariance(True)
    on.set_landmarks(True); on.set_landmarks(False)                                   # off -> on -> off
    for i, pair in enumerate(frames):
        on.process_host([pair])
        assert everything(on) == want[i] and bytes(on.pose_covariance(0)) == want_cov[i], i
    kt_off = on.kernel_times(appended=True)
    assert list(kt_off) == list(kt_never) and [c for _, c in kt_off.values()] == [c for _, c in kt_never.values()], "off: no launch more"
    on.kernel_times_reset(); on.reset(); on.set_landmarks(True, 0.0)
    assert on.landmarks_enabled() == (True, 1.0), "0 means the reference's default of 1"
    plain, n_valid = [], 0
    for i, pair in enumerate(frames):
        on.process_host([pair])
        assert everything(on) == want[i] and bytes(on.pose_covariance(0)) == want_cov[i], (i, "nothing else moves")
        info, rec = on.landmarks(0)
        plain.append((bytes(info), rec.tobytes()))
        r = on.result(0)
        if i == 0:
            assert info.state == LMK_NONE and info.n == 0
            continue
        lists = lane_lists(on)
        assert info.n == len(lists[0]) == r.tracked_feats_from_last_frame and info.state == (LMK_OK if r.valid else LMK_POINTS_ONLY), (i, info.n, info.state)
        ids = on.match_ids(0, 0)
        assert np.array_equal(rec["match_id"], ids[rec["cur_match"]]), (i, "the current frame's match IDs")
        if not r.valid: continue
        n_valid += 1
        delta = np.array(r.delta)
        mask = Pc.inlier_mask(lists, on.outliers(0))
        pc = Pc.reference(lists, cam, delta, p.use_robust_kernel, p.kernel_param, mask)
        f = Lr.flat([lists])
        ref = Lr.reference(f["obs"], cam, 1.0, delta, mask, pc["cov_delta"])
        assert ref["dmid"] >= DMID_MIN and pc["rel_pd"] >= 1e3, (i, ref["dmid"], pc["rel_pd"])
        check_records("sequence frame %d" % i, info, rec, f, ref, pc["kappa"], ids=ids[f["cur_match"]])
    assert n_valid >= 2
    kt = on.kernel_times(appended=True)
    assert list(kt)[:-1] == list(kt_never) and list(kt)[-1] == "landmarks"
    assert kt["landmarks"][1] == kt["gauss_newton"][1] == kt["pose_covariance"][1] == len(frames), "one k_landmarks call per stage-5 enqueue"
    on.close()
    gr = seq_context(g); gr.set_params(p); gr.set_camera(cam); gr.set_pose_covariance(True); gr.set_landmarks(True); gr.use_graphs(True)
    for i, pair in enumerate(frames):
        gr.process_host([pair])
        info, rec = gr.landmarks(0)
        assert everything(gr) == want[i] and (bytes(info), rec.tobytes()) == plain[i], (i, "under svo_use_graphs")
    captured, replayed = gr.graph_count()
    assert captured >= 1 and replayed >= 1, (captured, replayed)
    gr.set_landmarks(True)
    assert gr.graph_count()[0] == captured, "the same value again changes nothing"
    gr.set_landmarks(True, 0.5)
    assert gr.graph_count()[0] == 0, "another std_noise_pixels is another kernel argument: the captured graphs go"
    gr.process_host([frames[0]]); gr.process_host([frames[1]]); gr.process_host([frames[1]])
    assert gr.graph_count()[0] >= 1
    gr.set_landmarks(False)
    assert gr.graph_count()[0] == 0, "a change of value drops the captured graphs"
    gr.close()


def lane_content(cam):
    return {0: S.permuted(cam, S.BASE_TRUE, 1100, seed=51, noise=0.3, n_out=100),           # scratch path of k_gauss_newton, five blocks of k_landmarks
            1: S.permuted(cam, S.BASE_TRUE, 40, seed=52, noise=0.3, n_out=4),
            2: S.permuted(cam, S.BASE_TRUE, 300, seed=53, noise=0.3, n_out=30)}


def test_lanes_idle_lanes_and_the_device_copy():
    """three lanes through svo_put_*, full runs: every lane's info and records are, bit for bit, those of a one-lane context on the
    same lists.  Then lanes 0 and 2 swap their lists and a step leaves lane 1 out: its info and records keep every byte.
    svo_copy_landmarks_async into torch tensors delivers the getters' bytes."""
    import torch
    cam = S.camera()
    p = base_params(); p.use_previous_pose_as_initial = 0
    content = lane_content(cam)
    one = {}
    for lane, lists in content.items():
        c1 = new_context(2048); c1.set_params(p); c1.set_camera(cam); c1.set_pose_covariance(True); c1.set_landmarks(True, 0.8)
        put_lists(c1, 0, lists); c1.run_stages(hip.RUN_OPTIMIZE)
        info, rec = c1.landmarks(0)
        assert c1.result(0).valid and info.state == LMK_OK and info.n == len(lists[0]) and 8 <= info.n_inliers < info.n
        one[lane] = (bytes(info), rec.tobytes())
        c1.close()
    ctx = new_context(2048, n_lanes=3)
    ctx.set_params(p); ctx.set_camera(cam); ctx.set_pose_covariance(True); ctx.set_landmarks(True, 0.8)
    for lane, lists in content.items(): put_lists(ctx, lane, lists)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    got = lambda lane: (lambda ir: (bytes(ir[0]), ir[1].tobytes()))(ctx.landmarks(lane))
    for lane in content: assert got(lane) == one[lane], lane
    d_info = torch.zeros(3 * C.sizeof(LandmarksInfo), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(3 * 2048 * Landmark.itemsize, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.copy_landmarks_async(d_info.data_ptr(), d_rec.data_ptr(), d_rec.numel())
    ctx.wait()
    h_info, h_rec = d_info.cpu().numpy(), d_rec.cpu().numpy().view(Landmark).reshape(3, 2048)
    for lane, lists in content.items():
        assert h_info[32 * lane:32 * lane + 32].tobytes() == one[lane][0] and h_rec[lane, :len(lists[0])].tobytes() == one[lane][1], lane
    assert ctx.L.svo_copy_landmarks_async(ctx.h, C.c_void_p(d_info.data_ptr()), C.c_void_p(d_rec.data_ptr()), C.c_size_t(d_rec.numel() - 1)) == -2, "too small a destination: SVO_ERR_ARG"
    put_lists(ctx, 0, content[2]); put_lists(ctx, 2, content[0])
    ctx.run_stages(hip.RUN_OPTIMIZE, active=[0, 2])
    assert got(1) == one[1], "an idle lane keeps its info and its records"
    assert got(0) == one[2] and got(2) == one[0], "the active lanes are rewritten"
    ctx.close()


def gn_nt_child():
    """the body of the child process of test_other_block_sizes: SVO_GN_NT is read when a context is created, from the environment of its process"""
    case = BY_NAME["T257-mk1024"]
    ctx = new_context(case[1]); ctx.set_camera(S.camera()); ctx.set_landmarks(True, 1.0)
    for with_cov in (True, False):
        f, surv, pc, ref = Lr.case_reference(case, Lr.ZERO, 1.0, with_cov)
        r, info, rec = run_zero(ctx, case, with_cov)
        check_records(case[0], info, rec, f, ref, pc["kappa"])
    ctx.close()
    print("bounds hold")


@pytest.mark.parametrize("nt", [256, 512])
def test_other_block_sizes(nt):
    """SVO_GN_NT = 256 and 512: the other instances of k_gauss_newton and k_pose_covariance in front of k_landmarks, on the T = 257 case"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_landmarks as G; G.gn_nt_child()" % (ROOT, here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SVO_GN_NT=str(nt)), capture_output=True, text=True, timeout=300)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "bounds hold" in out.stdout, (nt, out.stdout[-600:], out.stderr[-1500:])


def test_refusals():
    """a negative or NaN std_noise_pixels: SVO_ERR_ARG with a text, the values in force stay; frame-parallel streams refuse the feature"""
    from stereo_vo_amd.pipeline import FrameParallelStream
    ctx = new_context(64)
    ctx.set_landmarks(True, 0.25)
    for bad in (-1.0, float("nan"), float("inf")):
        assert ctx.L.svo_set_landmarks(ctx.h, 1, C.c_double(bad)) == -2, "SVO_ERR_ARG"
        assert b"std_noise_pixels" in ctx.L.svo_last_error(ctx.h)
        assert ctx.L.svo_set_landmarks(ctx.h, 0, C.c_double(bad)) == -2
    assert ctx.landmarks_enabled() == (True, 0.25)
    assert ctx.L.svo_get_landmarks(ctx.h, 1, None, 0) == -2 and ctx.L.svo_get_landmarks_info(ctx.h, 0, None) == -2
    ctx.close()
    fp = FrameParallelStream(base_params(), S.camera(), S.W, S.H, lanes=1, contexts=2, max_kps=64, max_cand=1 << 15)
    with pytest.raises(hip.SvoError, match="frame-parallel"): fp.set_landmarks(True)
    with pytest.raises(hip.SvoError): fp.set_landmarks(False, -1.0)
    fp.set_landmarks(False)
    assert all(c.landmarks_enabled()[0] is False for c in fp.ctxs)
    fp.close()
