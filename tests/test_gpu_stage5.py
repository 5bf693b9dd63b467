"""Stage 5 on the device (k_gauss_newton, csrc/k_gn.hip) held to the extended-precision reference of tests/stage5_ref.py.

Its sums are reduced in another order than the oracle's loop, so stage 5 is the one kernel that cannot be compared byte for byte,
and the pose tolerance of the pipeline tests (1e-3 m / 1e-4 rad) is a few percent of a frame's motion: a wrong Jacobian entry or a
dropped partial sum hides behind it after a few more iterations.  Here the kernel performs ONE evaluation from a given start
(initial_max_iters 0, max_iters 1, a custom initial pose), whose only discontinuity is the (float) rounding of the projected
pixels; tests/test_stage5_ref_cpu.py establishes, without a GPU, that no pixel of any case lies within 1e-10 px of a rounding
midpoint.  Then the float residuals are those of the reference exactly and the step agrees with it to float64 rounding scaled by the
condition number of H -- some eight orders of magnitude below the pose tolerance.

Then: full runs against the oracle, one per branch of stage 5's control flow; the same lists through svo_put_* on several lanes
of one context, bit for bit against the one-lane entry; and both of the other block sizes (SVO_GN_NT), each in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

import stage5_ref as S
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params

pytestmark = pytest.mark.gpu

# The largest K_oracle = (||step - x|| - rounding of start + x) / (||x|| * kappa_2(H) * 2^-52) the ORACLE reaches over the single-step
# cases below, measured by tests/test_stage5_ref_cpu.py (0.2391, at the collinear scene with 0.1 px of perturbation, robust kernel;
# 0.049 over the well-conditioned cases), rounded up.  That test fails when the figure moves above it or below half of it.
K_ORACLE_MAX = 0.24
# The kernel's bound: 16 times that.  The factor covers a reciprocal and a reciprocal square root within ~2 ulp where the oracle's
# are correctly rounded, sums taken as a tree over up to 512 threads, and a maximum over some hundred runs understating the
# oracle's own worst case.  A kernel that needs more has something to explain; the number does not move.
K_STEP = 16 * K_ORACLE_MAX
# residuals: the four float components are identical under the midpoint condition; what is left is r0^2 + r1^2 + r2^2 + r3^2 in
# float64 with or without contraction
RESID_RTOL = 4 * 2.0 ** -52

SINGLE = S.single_step_cases()
CONDITIONING = S.conditioning_cases()
FULL = S.full_run_cases()
_ids = lambda cases: [c[0] for c in cases]
_worst = {}


def O():
    from oracle import oracle
    return oracle


def base_params():
    return north_star_params(hip.default_params(), orb_nfeats=40)        # (the detector is not run: a count the 64-entry context accepts)


def new_context(max_kps, n_lanes=1):
    return hip.Context(n_lanes=n_lanes, max_w=S.W, max_h=S.H, max_kps=max_kps, max_cand=1 << 15)


@pytest.fixture(scope="module")
def contexts():
    """one one-lane context per max_kps, shared by the tests of this file"""
    made = {}
    def get(max_kps):
        if max_kps not in made: made[max_kps] = new_context(max_kps)
        return made[max_kps]
    yield get
    for c in made.values(): c.close()


def check_single_step(ctx, case, robust, oracle_survivors=False):
    """one evaluation of `case` on `ctx` against the reference; returns the step's ratio against kappa * 2^-52 * ||x||"""
    name, mk, build, start, md = case
    lists = S.scene(case)
    T = len(lists[0])
    p = S.single_step_params(base_params(), robust, md)
    ctx.set_params(p)
    v, r, resid, outl = ctx.change_in_pose(*lists, S.camera(), init6=start)
    assert v and (r.num_it, r.num_it_final, r.n_residual, r.error_code, r.status) == (0, 1, T, 0, 0), (name, v, r.num_it, r.num_it_final, r.n_residual, r.error_code)
    got = resid < 1e300
    if oracle_survivors:
        # the survivors as the kernel returned them go into the reference; that they are the right ones is the oracle's word
        o = O().Oracle(p)
        _, _, resid_o, _ = o.change_in_pose(*lists, S.camera(), init6=start)
        o.close()
        assert np.array_equal(got, resid_o < 1e300), (name, "survivors of the stage-5 NMS mask")
        lists, ref = S.reference(case, robust, survivors=got)
    else:
        lists, ref = S.reference(case, robust)
    assert np.array_equal(got, ref["used"]), (name, "DBL_MAX pattern", int((got != ref["used"]).sum()))
    assert (resid[~got] == S.DBL_MAX).all()
    rel = np.abs(resid[got] - ref["resid"][got]) / ref["resid"][got]
    assert rel.max() <= RESID_RTOL, (name, "residuals", float(rel.max()) / 2.0 ** -52)
    ratio = S.step_ratio(r.delta, start, ref)
    print("\n%s %s: T %d, kappa %.3g, step error %.4f of kappa * 2^-52 * ||x|| (bound %.2f), residuals within %.2f * 2^-52"
          % (name, "robust" if robust else "plain", T, ref["kappa"], ratio, K_STEP, float(rel.max()) / 2.0 ** -52))
    assert ratio <= K_STEP, (name, robust, ratio)
    if not ref["keep"].all():
        # the reference cuts an eigenvalue: the step is the minimum-norm one, with nothing along the cut direction
        x = np.array(r.delta) - start
        for i in np.nonzero(~ref["keep"])[0]:
            assert abs(ref["vec"][:, i] @ x) < 1e-6 * np.linalg.norm(ref["x"]), (name, "component along a cut eigenvector", float(ref["vec"][:, i] @ x))
    if _worst.get("ratio", ("", -1.0))[1] < ratio: _worst["ratio"] = ("%s %s" % (name, "robust" if robust else "plain"), ratio)
    return ratio


@pytest.mark.parametrize("robust", [1, 0])
@pytest.mark.parametrize("case", SINGLE + CONDITIONING, ids=_ids(SINGLE + CONDITIONING))
def test_single_evaluation_against_the_reference(contexts, case, robust):
    """Shapes around every wave count, the LDS limit (1024 / 1025) and the smallest context; starts on either side of the small-angle
    switch (1e-5 rad) and of gn_sincos's (0.5 rad), 0.59 rad with three components (S5:162), +-0.3 m; permuted index lists under a
    mask that removes a real share (min_distance 3 and 12); zero-disparity points and points behind the camera among good ones; the
    collinear scene down to a rank-deficient H.

    collinear-eps0 is the case that found a defect in chol6 / solve_sym6: the fifth LDL^T pivot of its H is genuine but small
    (8.7e-9 * H_55), the elimination through it amplifies rounding noise into a sixth "pivot" of +-(1e-11 .. 1e-10) * max H_ii whose
    sign depends on the summation order, and the pivot test `s > 1e-13 * dmax` let a positive one pass: Cholesky then solved a
    rank-deficient system and the step carried ~2000 * ||x|| along the direction the reference and the oracle cut (ratio 1.4e16).
    The pivot test now also bounds the noise the earlier columns can have put into a pivot (k_gn.hip, at chol6)."""
    check_single_step(contexts(case[1]), case, robust, oracle_survivors=case[0].startswith("perm"))


def test_worst_single_step_ratio():
    """prints the worst ratio the single evaluations above reached against K_STEP (nothing to report when run on its own)"""
    name, ratio = _worst.get("ratio", ("none ran", 0.0))
    print("\nstage 5 single evaluations: worst step error %.4f of kappa * 2^-52 * ||x|| at %s; bound K_STEP = 16 * %.2f = %.2f" % (ratio, name, K_ORACLE_MAX, K_STEP))
    assert ratio <= K_STEP


def assert_same_run(tag, got, want, T):
    """test_change_in_pose_against_oracle's tolerances: delta within 1e-7, residuals rtol 1e-6, iteration counts within 1, every other
    integer and the inlier list exact"""
    (v, r, resid, outl), (vo, ro, resid_o, outl_o) = got, want
    assert v == vo and (r.n_residual, r.n_outliers, r.error_code, r.valid) == (ro.n_residual, ro.n_outliers, ro.error_code, ro.valid), \
        (tag, v, vo, (r.n_residual, r.n_outliers, r.error_code), (ro.n_residual, ro.n_outliers, ro.error_code))
    assert abs(r.num_it - ro.num_it) <= 1 and abs(r.num_it_final - ro.num_it_final) <= 1, (tag, r.num_it, ro.num_it, r.num_it_final, ro.num_it_final)
    assert np.array_equal(outl, outl_o), (tag, "inlier list")
    if ro.n_residual:
        fin = resid_o < 1e300
        assert np.array_equal(resid < 1e300, fin), (tag, "DBL_MAX pattern")
        if vo: assert np.allclose(resid[fin], resid_o[fin], rtol=1e-6, atol=1e-9), (tag, "residuals")
    if vo:
        assert np.abs(np.array(r.delta) - np.array(ro.delta)).max() < 1e-7, (tag, "delta", list(r.delta), list(ro.delta))
        assert np.abs(np.array(r.outPose) - np.array(ro.outPose)).max() < 1e-6, (tag, "pose")
        assert r.tracked_feats_from_last_frame == T                      # S5:724 (the oracle's getChangeInPose entry leaves it alone)


@pytest.mark.parametrize("case", FULL, ids=_ids(FULL))
def test_full_runs_against_oracle(case):
    """One case per branch of stage 5's control flow, each called twice (the second call starts from the stored pose): the defaults
    on either side of the LDS limit, voecBadCondNumber, fewer than 8 points after the gate, a rotation of 0.6 rad with the gate
    closed and open (phase 2 through the library sin / cos), both cost aborts, three pairs of iteration limits, T < 8, and T = 8
    with one point masked.  tests/test_stage5_ref_cpu.py holds ref_stage5 to the oracle on the same cases."""
    name, mk, build, ov, expect = case
    lists = build(S.camera())
    p = S.with_overrides(base_params(), ov)
    ctx = new_context(mk)
    ctx.set_params(p)
    orc = O().Oracle(p)
    for call in range(2):
        got = ctx.change_in_pose(*lists, S.camera())
        want = orc.change_in_pose(*lists, S.camera())
        assert_same_run((name, call), got, want, len(lists[0]))
        if call == 0:
            for k, v in (expect or {}).items():
                assert (int(got[0]) if k == "valid" else getattr(got[1], k)) == v, (name, k, v)
    orc.close(); ctx.close()


def test_capacity_is_refused_before_any_launch(contexts):
    """n_tracked = max_kps + 1: SVO_ERR_CAPACITY, and the context goes on working"""
    ctx = contexts(64)
    case = [c for c in SINGLE if c[0] == "shape-T64-mk64"][0]
    before = check_single_step(ctx, case, 1)
    t, m, m2, pl, pr, cl, cr = S.scene(case)
    with pytest.raises(hip.SvoError, match="capacity"):
        ctx.change_in_pose(np.concatenate([t, t[:1]]), m, m2, pl, pr, cl, cr, S.camera(), init6=case[3])
    assert check_single_step(ctx, case, 1) == before


STAGE5_FIELDS = ("num_it", "num_it_final", "valid", "error_code", "tracked_feats_from_last_KF", "tracked_feats_from_last_frame", "n_outliers", "n_residual", "status")


def test_lanes_through_put_and_run_optimize_alone():
    """svo_put_features / svo_put_matches / svo_put_tracked on four lanes of a five-lane context, then SVO_RUN_OPTIMIZE on its own
    with lane 3 left out.  Each lane runs the same kernel on the same lists with the same thread count as svo_change_in_pose on a
    one-lane context of the same max_kps -- only the lane's offsets into the lists, gn_obs / gn_lmk / residual / outliers and
    gn_scratch (lane_id * pmax * 30 bytes) differ -- so the record, the residuals and the inlier list are equal BIT FOR BIT.
    Compared: every field stage 5 writes.  Not compared: detected_left / detected_right / stereo_matches, which svo_put_* fill
    with the list lengths (P:171-176, 274-276) and the one-lane entry leaves at zero, n_octaves (the begin-of-frame kernel's) and
    track_stats (stage 4's)."""
    cam = S.camera()
    p = base_params()
    content = {0: S.permuted(cam, S.BASE_TRUE, 1500, seed=41, noise=0.3, n_out=150),        # scratch path
               1: S.permuted(cam, S.BASE_TRUE, 40, seed=42, noise=0.3, n_out=4),
               2: S.synthetic(cam, S.BASE_TRUE, 6, seed=43),                                 # fewer than 8: invalid
               4: S.permuted(cam, S.BASE_TRUE, 1025, seed=44, noise=0.3, n_out=100)}         # first scratch size
    ctx = new_context(2048, n_lanes=5)
    ctx.set_params(p); ctx.set_camera(cam)
    for lane, (t, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r) in content.items():
        ctx.put_features(lane, 1, 0, pre_l, None, S.W, S.H); ctx.put_features(lane, 1, 1, pre_r, None, S.W, S.H)
        ctx.put_features(lane, 0, 0, cur_l, None, S.W, S.H); ctx.put_features(lane, 0, 1, cur_r, None, S.W, S.H)
        ctx.put_matches(lane, 1, pre_m); ctx.put_matches(lane, 0, cur_m)
        ctx.put_tracked(lane, t)
        assert ctx.tracked(lane).tobytes() == t.tobytes()
    idle_before = (bytes(ctx.result(3)), ctx.status_word(3), len(ctx.tracked(3)), len(ctx.matches(3, 0)), len(ctx.matches(3, 1)), len(ctx.keypoints(3, 0, 0)[0]))
    ctx.run_stages(hip.RUN_OPTIMIZE, active=[0, 1, 2, 4])
    ctx.wait()
    for lane, lists in content.items():
        T = len(lists[0])
        r = ctx.result(lane)
        one = new_context(2048)
        one.set_params(p)
        v1, r1, resid1, outl1 = one.change_in_pose(*lists, cam)
        one.close()
        assert bytes(r.outPose) == bytes(r1.outPose) and bytes(r.delta) == bytes(r1.delta), (lane, list(r.delta), list(r1.delta))
        assert [getattr(r, f) for f in STAGE5_FIELDS] == [getattr(r1, f) for f in STAGE5_FIELDS], (lane, [(f, getattr(r, f), getattr(r1, f)) for f in STAGE5_FIELDS])
        assert ctx.residuals(lane).tobytes() == resid1.tobytes(), (lane, "residuals")
        assert ctx.outliers(lane).tobytes() == outl1.tobytes(), (lane, "inlier list")
        assert (r.detected_left[0], r.detected_right[0], r.stereo_matches[0]) == (len(lists[5]), len(lists[6]), len(lists[2]))
        orc = O().Oracle(p)
        want = orc.change_in_pose(*lists, cam)
        orc.close()
        assert_same_run(("lane", lane), (bool(r.valid), r, ctx.residuals(lane), ctx.outliers(lane)), want, T)
        assert bool(r.valid) == (T >= 8)
    assert idle_before == (bytes(ctx.result(3)), ctx.status_word(3), len(ctx.tracked(3)), len(ctx.matches(3, 0)), len(ctx.matches(3, 1)), len(ctx.keypoints(3, 0, 0)[0]))
    ctx.close()


GN_NT_SHAPES = [(t, 2048) for t in (255, 256, 257, 511, 512, 513, 1025)]


def gn_nt_child():
    """the body of the child process of test_other_block_sizes: SVO_GN_NT is read when a context is created, from the environment of its process"""
    made = {}
    worst = 0.0
    for T, mk in GN_NT_SHAPES:
        case = ("shape-T%d-mk%d" % (T, mk), mk, (lambda cam, T=T: S.synthetic(cam, S.BASE_TRUE, T, seed=100 + T)), S.BASE_TRUE * 0.98, 2)
        if mk not in made: made[mk] = new_context(mk)
        for robust in (1, 0):
            worst = max(worst, check_single_step(made[mk], case, robust))
    for c in made.values(): c.close()
    case = FULL[1]                                                      # the defaults at T = 1025
    lists = case[2](S.camera())
    ctx = new_context(case[1]); ctx.set_params(base_params())
    orc = O().Oracle(base_params())
    for call in range(2):
        assert_same_run((case[0], call), ctx.change_in_pose(*lists, S.camera()), orc.change_in_pose(*lists, S.camera()), len(lists[0]))
    orc.close(); ctx.close()
    print("same; worst single-step ratio %.4f of %.2f" % (worst, K_STEP))


@pytest.mark.parametrize("nt", [256, 512])
def test_other_block_sizes(nt):
    """SVO_GN_NT = 256 and 512 (four and eight waves: other instances of the kernel template, other trip counts of every
    strided loop, another number of partial sums): the single-step checks at T around both block sizes and at the first scratch
    size, and one default full run, in a fresh process each."""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_stage5 as G; G.gn_nt_child()" % (os.path.dirname(here), here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SVO_GN_NT=str(nt)), capture_output=True, text=True, timeout=300)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "same; worst" in out.stdout, (nt, out.stdout[-600:], out.stderr[-1500:])
