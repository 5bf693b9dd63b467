"""The oracle's stage 5 held to the extended-precision reference of tests/stage5_ref.py, and the inputs of the GPU tests in
tests/test_gpu_stage5.py qualified (CPU only).

What the GPU tests may assert rests on what is established here without a GPU: that the oracle's single evaluation agrees with
the reference to rounding (its residuals bit for bit, its step within K_oracle * kappa * 2^-52), that no projected pixel of any
case sits close enough to a binary32 rounding midpoint for two correct implementations to round it differently, that no residual
sits on the gate, that no eigenvalue sits on a rank decision, and that the expected outcomes of the control-flow cases are those of
a second, literal reading of stage 5 (ref_stage5) and not of the oracle alone."""
import numpy as np
import pytest

import stage5_ref as S
from oracle import oracle as O
from stereo_vo_amd.abi import north_star_params
from test_independent_own_logic import ref_stage5

SINGLE = S.single_step_cases() + S.conditioning_cases()
FULL = S.full_run_cases()
_ids = lambda cases: [c[0] for c in cases]


def base_params():
    return north_star_params(O.default_params(), orb_nfeats=40)


_oracle_steps = {}


def oracle_step(case, robust):
    """(result record, residuals, reference) of the oracle's single evaluation of a case, run once per process"""
    key = (case[0], robust)
    if key not in _oracle_steps:
        lists, ref = S.reference(case, robust)
        o = O.Oracle(S.single_step_params(base_params(), robust, case[4]))
        v, r, resid, outl = o.change_in_pose(*lists, S.camera(), init6=case[3])
        o.close()
        _oracle_steps[key] = (v, r, resid, ref)
    return _oracle_steps[key]


@pytest.mark.parametrize("robust", [1, 0])
@pytest.mark.parametrize("case", SINGLE, ids=_ids(SINGLE))
def test_oracle_single_step_against_the_reference(case, robust):
    """initial_max_iters 0, max_iters 1, a custom start: stage 5 is exactly one m_evalRGN.  The float residual components are the
    reference's, so their squares added in the written order are too: bit for bit on the survivors, DBL_MAX elsewhere."""
    v, r, resid, ref = oracle_step(case, robust)
    T = len(S.scene(case)[0])
    assert v and (r.num_it, r.num_it_final, r.n_residual, r.error_code) == (0, 1, T, 0)
    assert np.array_equal(resid, ref["resid"]), (case[0], int((resid != ref["resid"]).sum()))
    assert ref["used"].sum() >= 8
    from test_gpu_stage5 import K_ORACLE_MAX
    assert S.step_ratio(r.delta, case[3], ref) <= K_ORACLE_MAX, (case[0], robust, S.step_ratio(r.delta, case[3], ref))


def test_oracle_constant_and_midpoint_condition():
    """Prints the largest K_oracle = ||step - x|| / (||x|| kappa 2^-52) over all single-step cases (the constant K_ORACLE_MAX of
    test_gpu_stage5.py is this figure, rounded up) and the smallest dmid.  dmid >= 1e-10 px is a condition on the INPUTS, from the
    reference alone: a double evaluation of a pixel is accurate to ~1e-13 px, so every implementation then rounds every pixel to
    the same float.  A case that violates it gets another seed, not a smaller number."""
    from test_gpu_stage5 import K_ORACLE_MAX
    worst, dmid = ("", 0.0), ("", np.inf)
    for case in SINGLE:
        for robust in (1, 0):
            v, r, resid, ref = oracle_step(case, robust)
            k = S.step_ratio(r.delta, case[3], ref)
            if k > worst[1]: worst = (case[0] + (" robust" if robust else " plain"), k)
            if ref["dmid"] < dmid[1]: dmid = (case[0], ref["dmid"])
            assert ref["dmid"] >= 1e-10, (case[0], ref["dmid"])
    print("\nstage 5 single steps, %d cases x 2: largest K_oracle %.4f (%s); smallest dmid %.3g px (%s)" % (len(SINGLE), worst[1], worst[0], dmid[1], dmid[0]))
    assert worst[1] <= K_ORACLE_MAX and worst[1] > K_ORACLE_MAX / 2, "K_ORACLE_MAX in test_gpu_stage5.py no longer states what the oracle reaches"


def test_non_finite_points_are_the_ones_built_in():
    """the mixed scene: the zero-disparity points are skipped (S5:322), the points behind the camera are NOT (their Jacobian is finite)"""
    for case in SINGLE:
        if not case[0].startswith("nonfinite"): continue
        lists, ref = S.reference(case, 1)
        l1l, l1r, _, _ = S.gather(lists)
        zero = l1l["x"] == l1r["x"]
        surv = S.nms_survivors(lists, case[4])
        assert zero.sum() >= 25 and (ref["used"] == (surv & ~zero)).all()
        lmk = S.triangulate64(l1l, l1r, S.camera())
        behind = (lmk[:, 2] + case[3][5] < 0) & ~zero
        assert behind.sum() >= 25 and ref["used"][behind & surv].all()


@pytest.mark.parametrize("case", S.conditioning_cases(), ids=_ids(S.conditioning_cases()))
def test_eigenvalue_margin(case):
    """A rank decision must not sit where two correct implementations may take it differently.  Two thresholds exist: the
    pseudo-inverse keeps an eigenvalue above 6 * DBL_EPSILON * lambda_max (this one decides the ANSWER: a cut eigenvalue's
    direction is left out of the step), and chol6 / solve_sym6 leave the Cholesky path when a pivot is not above 1e-13 * max H_ii
    (this one decides the ALGORITHM only: both solve the full system while the eigenvalue is kept).

    Required of every case: lambda_min at least 100 times away from the pseudo-inverse's cut, on either side.  Where the
    reference cuts, lambda_min must also lie 100 times below the pivot threshold, so that no implementation can take the Cholesky
    path and solve for a direction the reference leaves out.  Where the reference keeps every eigenvalue the position against the
    pivot threshold is printed, not asserted: the two thresholds are only 75 times apart (1e-13 / 1.33e-15), so an eigenvalue
    between them cannot be 100 times away from both, which is where the collinear scene at 1e-3 px sits whatever its geometry
    (lambda_min / max H_ii ~ eps^2 / f^2) -- and either path is a correct full solve there."""
    for robust in (1, 0):
        lists, ref = S.reference(case, robust)
        print("\n%s: lambda_min / pseudo-inverse cut = %.3g, lambda_min / pivot threshold = %.3g, kappa (kept) = %.3g, kept %d of 6"
              % (case[0], ref["rel_pinv"], ref["rel_chol"], ref["kappa"], ref["keep"].sum()))
        assert ref["rel_pinv"] >= 100 or ref["rel_pinv"] <= 0.01, (case[0], ref["rel_pinv"])
        if ref["rel_pinv"] <= 0.01:
            assert ref["rel_chol"] <= 0.01 and ref["keep"].sum() == 5, (case[0], ref["rel_chol"])
        else:
            assert ref["keep"].all()


def _runs(case):
    """the oracle's two calls of a full-run case: [(valid, record, residuals, inlier list)] * 2"""
    name, mk, build, ov, expect = case
    lists = build(S.camera())
    p = S.with_overrides(base_params(), ov)
    o = O.Oracle(p)
    out = [o.change_in_pose(*lists, S.camera()) for _ in range(2)]
    o.close()
    return lists, p, out


@pytest.mark.parametrize("case", FULL, ids=_ids(FULL))
def test_ref_stage5_on_the_control_flow_cases(case):
    """the literal walk of stage 5 against the oracle on every full-run case, with the assertions of test_stage5_control_flow,
    and the outcome the GPU test expects of the first call"""
    lists, p, out = _runs(case)
    last = None
    for call, (valid, r, resid, outl) in enumerate(out):
        want = ref_stage5(*lists, S.camera(), p, S.W, S.H, last)
        assert (bool(valid), r.num_it, r.num_it_final) == (want["valid"], want["num_it"], want["num_it_final"]), (case[0], call, r.error_code, want["error_code"])
        assert r.error_code == want["error_code"], (case[0], call)
        assert list(outl) == want["outliers"], (case[0], call)
        if want["valid"]:
            assert np.abs(np.array(r.delta) - want["delta"]).max() < 1e-9, (case[0], call)
            a, b = np.array(resid), np.array(want["residual"])
            fin = b < 1e300
            assert ((a < 1e300) == fin).all() and np.allclose(a[fin], b[fin], rtol=1e-7, atol=1e-12), (case[0], call)
        # (the estimator keeps the pose of every call that reaches the end of stage 5, valid or not: S5:720-721 comes before S5:727)
        last = want.get("delta")
    valid, r, resid, outl = out[0]
    for k, v in (case[4] or {}).items():
        assert (int(valid) if k == "valid" else getattr(r, k)) == v, (case[0], k, v)


@pytest.mark.parametrize("case", FULL, ids=_ids(FULL))
def test_gate_margin(case):
    """No residual at the gate (S5:601-611: the values of phase 1's last evaluation) within a relative 1e-4 of residual_threshold,
    in either call: otherwise the inlier list could differ between two correct implementations.  The gate's residuals are read
    from a run whose phase 2 is given no iterations."""
    name, mk, build, ov, expect = case
    lists = build(S.camera())
    p = S.with_overrides(base_params(), ov)
    q = p.copy(); q.max_iters = 0
    worst = np.inf
    for call in range(2):
        o = O.Oracle(p)
        for _ in range(call): o.change_in_pose(*lists, S.camera())        # the estimator's state before this call
        o.set_params(q)
        _, r, resid, _ = o.change_in_pose(*lists, S.camera())
        o.close()
        fin = resid[resid < 1e300] if r.num_it > 0 else np.zeros(0)
        if len(fin): worst = min(worst, float(np.abs(fin / p.residual_threshold - 1).min()))
    print("\n%s: smallest |residual / threshold - 1| at the gate: %.3g" % (name, worst))
    assert worst >= 1e-4, (name, worst)
