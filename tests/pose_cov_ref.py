"""The covariance of a pose increment (svo_pose_cov, include/svo_types.h) in extended precision, a plain float64 walk of the same
formulas, and the cases the CPU and GPU tests share (TEST INFRASTRUCTURE, CPU only, no native library).

reference() evaluates once more at a given delta over a given mask, as stage5_ref.eval_step does -- the gather, the float64
triangulation and the extended-precision rotation are that file's, imported -- and goes on in the x87 80-bit format to the weighted
information A = sum w J^T J and sigma2 = sum w s / (4 n - 6).  A^-1 is formed in mpmath at 50 digits.  G = d outPose / d delta is
mpmath.diff of a 50-digit delta -> outPose written from the definition (exact Rodrigues, inverse, yaw pitch roll): nothing of the
kernel's analytic G is in it.

double_walk() is the same quantity in numpy float64 with the kernel's formulas (its rotation, its series for G): what plain double
arithmetic reaches against the reference is the unit the kernel's tolerance is stated in (tests/test_pose_cov_ref_cpu.py)."""
import numpy as np
import mpmath

import stage5_ref as S

LD = S.LD
EPS = 2.0 ** -52
COV_NONE, COV_OK, COV_RANK_DEFICIENT, COV_NO_DOF, COV_DELTA_ONLY = range(5)
PITCH_COS2_MIN = 1e-12


def _evaluate(lists, cam, delta6, survivors, dt):
    """J (n, 4, 6), the float residuals (n, 4), the mask of the points used and the pixels, in dtype dt (LD or float64)"""
    T = len(lists[0])
    mask = np.zeros(T, bool); mask[np.asarray(survivors)] = True
    l1l, l1r, l2l, l2r = S.gather(lists)
    lmk = S.triangulate64(l1l, l1r, cam).astype(dt)
    delta6 = np.asarray(delta6, np.float64)
    if dt is LD: R, dR = S.rotation_ld(delta6[:3])
    else: R, dR = rotation64(delta6[:3])
    t = delta6[3:].astype(dt)
    c = lambda v: dt(v)
    with np.errstate(all="ignore"):
        X = lmk @ R.T + t
        X2 = X[:, 0] - c(cam.baseline); Z = X[:, 2]
        pix = np.stack([c(cam.l_fx) * X[:, 0] / Z + c(cam.l_cx), c(cam.l_fy) * X[:, 1] / Z + c(cam.l_cy),
                        c(cam.r_fx) * X2 / Z + c(cam.r_cx), c(cam.r_fy) * X[:, 1] / Z + c(cam.r_cy)], 1)
        J = np.zeros((T, 4, 6), dt)
        for j in range(6):
            Xd = lmk @ dR[j].T if j < 3 else np.tile(np.eye(3, dtype=dt)[j - 3], (T, 1))
            J[:, 0, j] = c(cam.l_fx) * ((Xd[:, 0] * Z - X[:, 0] * Xd[:, 2]) / (Z * Z))
            J[:, 1, j] = c(cam.l_fy) * ((Xd[:, 1] * Z - X[:, 1] * Xd[:, 2]) / (Z * Z))
            J[:, 2, j] = c(cam.r_fx) * ((Xd[:, 0] * Z - X2 * Xd[:, 2]) / (Z * Z))
            J[:, 3, j] = c(cam.r_fy) * ((Xd[:, 1] * Z - X[:, 1] * Xd[:, 2]) / (Z * Z))
        used = mask & np.isfinite(J.astype(np.float64)).all(axis=(1, 2))                                # S5:322
        obs = np.stack([l2l["x"], l2l["y"], l2r["x"], l2r["y"]], 1).astype(np.float32)
        r32 = obs - pix.astype(np.float32)                                                              # float - float, S5:335-338
    u = np.nonzero(used)[0]
    return J[u], r32[u].astype(dt), used, pix[u]


def _weights(s, robust, kernel_param, dt):
    return 1 / np.sqrt(1 + s / (dt(kernel_param) * dt(kernel_param))) if robust else np.ones(len(s), dt)


def _pose_mp(d):
    """delta -> outPose from the definition, in mpmath: R = exp([w]x), the inverse transform, x y z yaw pitch roll"""
    w1, w2, w3, t1, t2, t3 = d
    th = mpmath.sqrt(w1 * w1 + w2 * w2 + w3 * w3)
    a = mpmath.sin(th) / th if th != 0 else mpmath.mpf(1)
    b = (1 - mpmath.cos(th)) / (th * th) if th != 0 else mpmath.mpf(1) / 2
    K = mpmath.matrix([[0, -w3, w2], [w3, 0, -w1], [-w2, w1, 0]])
    R = mpmath.eye(3) + a * K + b * (K * K)
    M = R.T
    p = -(M * mpmath.matrix([t1, t2, t3]))
    yaw = mpmath.atan2(M[1, 0], M[0, 0])
    pitch = mpmath.atan2(-M[2, 0], mpmath.sqrt(M[0, 0] ** 2 + M[1, 0] ** 2))
    roll = mpmath.atan2(M[2, 1], M[2, 2])
    return [p[0], p[1], p[2], yaw, pitch, roll], M[0, 0] ** 2 + M[1, 0] ** 2


def g_matrix_mp(delta6):
    """G = d outPose / d delta by mpmath.diff (6 x 6 mpmath matrix) and cos^2(pitch)"""
    x = tuple(mpmath.mpf(float(v)) for v in delta6)
    G = mpmath.matrix(6, 6)
    for i in range(6):
        for k in range(6):
            G[i, k] = mpmath.diff(lambda *a, i=i: _pose_mp(a)[0][i], x, tuple(1 if j == k else 0 for j in range(6)))
    return G, _pose_mp(x)[1]


def reference(lists, cam, delta6, robust, kernel_param, survivors, digits=50):
    """The record of svo_pose_cov at `delta6` over `survivors`, extended precision / 50 digits, rounded to float64 at the end.
    Also: kappa = kappa_2(A), dmid as stage5_ref.eval_step gives it, rel_pd = lambda_min(A) / (1e-13 * max A_ii), cos2 = cos^2(pitch).
    state is COV_NO_DOF / COV_DELTA_ONLY / COV_OK from the definition; whether A passes the kernel's pivot test is judged by the
    caller from rel_pd (the covariances are returned whenever A is invertible at 50 digits)."""
    J, r, used, pix = _evaluate(lists, cam, delta6, survivors, LD)
    n = len(J); dof = 4 * n - 6
    s = (r * r).sum(axis=1)
    w = _weights(s, robust, kernel_param, LD)
    A = np.einsum("n,nia,nib->ab", w, J, J)
    out = dict(n_used=n, dof=dof, used=used, info=A.astype(np.float64), sigma2=0.0, cov_delta=np.zeros((6, 6)), cov_pose=np.zeros((6, 6)),
               dmid=float(S._midpoint_distance(pix).min()) if n else np.inf, kappa=np.inf, rel_pd=0.0, cos2=1.0, state=COV_NO_DOF)
    if dof <= 0: return out
    sig = (w * s).sum() / LD(dof)
    out["sigma2"] = float(sig)
    with mpmath.workdps(digits):
        Am = mpmath.matrix(6, 6)
        for i in range(6):
            for j in range(6): Am[i, j] = (S._mpf(A[i, j]) + S._mpf(A[j, i])) / 2
        lam = sorted(mpmath.eigsy(Am, eigvals_only=True))
        out["kappa"] = float(abs(lam[-1]) / abs(lam[0])) if lam[0] != 0 else np.inf
        out["rel_pd"] = float(lam[0] / (mpmath.mpf(S.CHOL_PIVOT_REL) * max(Am[i, i] for i in range(6))))
        G, cos2 = g_matrix_mp(delta6)
        out["cos2"] = float(cos2)
        out["state"] = COV_DELTA_ONLY if cos2 < PITCH_COS2_MIN else COV_OK
        if lam[0] > 0:
            Cm = S._mpf(sig) * mpmath.inverse(Am)
            out["cov_delta"] = np.array([[float(Cm[i, j]) for j in range(6)] for i in range(6)])
            if out["state"] == COV_OK:
                Pm = G * Cm * G.T
                out["cov_pose"] = np.array([[float(Pm[i, j]) for j in range(6)] for i in range(6)])
    return out


# ---- the double walk: the kernel's formulas in numpy float64 -----------------------------------------------------------------------

def rotation64(w):
    """rodrigues_with_derivs (k_gn.hip) in float64: the small-angle form below 1e-5 rad, else S5:102-163 with the S5:162 entry"""
    w = np.asarray(w, np.float64)
    G = [g.astype(np.float64) for g in S._G]
    Wm = w[0] * G[0] + w[1] * G[1] + w[2] * G[2]
    th = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    I = np.eye(3)
    if th < 1e-5: return I + Wm, [g.copy() for g in G]
    s, c = np.sin(th), np.cos(th)
    u = (c - 1) / th ** 2; v = s / th
    du = [((-s * wk / th) * th ** 2 - (c - 1) * 2 * wk) / th ** 4 for wk in w]
    dv = [wk * (th * c - s) / th ** 3 for wk in w]
    W2 = Wm @ Wm
    R = I + v * Wm - u * W2
    dR = [dv[k] * Wm + v * G[k] - du[k] * W2 - u * (G[k] @ Wm + Wm @ G[k]) for k in range(3)]
    dR[2][2, 2] = (w[1] ** 2 + w[2] ** 2) * du[2]
    return R, dR


def rotation_derivs64(w):
    """cov_rotation_derivs (k_gn.hip): R = I + a K + b K^2 and its exact derivatives, the four coefficients by series below 0.5 rad"""
    w = np.asarray(w, np.float64)
    z = float(w @ w)
    if z < 0.25:
        t, p = 1.0, 1.0 / 6.0
        a = b = al = be = 0.0
        for n in range(12):
            a += t; b += t / (2 * n + 2)
            al -= (2 * n + 2) * p; be -= (2 * n + 2) * p / (2 * n + 4)
            t = -t * z / ((2 * n + 2) * (2 * n + 3)); p = -p * z / ((2 * n + 4) * (2 * n + 5))
    else:
        th = np.sqrt(z); sn, cs = np.sin(th), np.cos(th)
        a = sn / th; b = (1 - cs) / z; al = (cs - a) / z; be = (a - 2 * b) / z
    G = [g.astype(np.float64) for g in S._G]
    K = w[0] * G[0] + w[1] * G[1] + w[2] * G[2]
    I = np.eye(3); ww = np.outer(w, w)
    R = I * (1 - b * z) + a * K + b * ww
    dR = []
    for k in range(3):
        e = np.zeros(3); e[k] = 1
        dR.append(al * w[k] * K + a * G[k] + be * w[k] * (ww - z * I) + b * (np.outer(e, w) + np.outer(w, e) - 2 * w[k] * I))
    return R, dR


def g_matrix64(delta6):
    """the kernel's analytic G (None where cos^2(pitch) < 1e-12) and cos^2(pitch)"""
    d = np.asarray(delta6, np.float64)
    R, dR = rotation_derivs64(d[:3])
    m00, m10, m20, m21, m22 = R[0, 0], R[0, 1], R[0, 2], R[1, 2], R[2, 2]          # M = R^T
    c2 = m00 * m00 + m10 * m10
    if c2 < PITCH_COS2_MIN: return None, c2
    hy = np.sqrt(c2); r2 = m21 * m21 + m22 * m22; n2 = m20 * m20 + c2
    G = np.zeros((6, 6))
    for k in range(3):
        D = dR[k]
        G[:3, k] = -(D.T @ d[3:]); G[:3, 3 + k] = -R[k, :]
        d00, d10, d20, d21, d22 = D[0, 0], D[0, 1], D[0, 2], D[1, 2], D[2, 2]
        G[3, k] = (m00 * d10 - m10 * d00) / c2
        G[4, k] = (-hy * d20 + m20 * (m00 * d00 + m10 * d10) / hy) / n2
        G[5, k] = (m22 * d21 - m21 * d22) / r2
    return G, c2


def double_walk(lists, cam, delta6, robust, kernel_param, survivors):
    """info, sigma2, cov_delta, cov_pose (None where undefined) in float64"""
    J, r, used, _ = _evaluate(lists, cam, delta6, survivors, np.float64)
    n = len(J); dof = 4 * n - 6
    s = (r * r).sum(axis=1)
    w = _weights(s, robust, kernel_param, np.float64)
    A = np.einsum("n,nia,nib->ab", w, J, J)
    A = np.triu(A) + np.triu(A, 1).T
    out = dict(n_used=n, dof=dof, info=A, sigma2=None, cov_delta=None, cov_pose=None)
    if dof <= 0: return out
    out["sigma2"] = float((w * s).sum() / dof)
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return out
    Li = np.linalg.solve(L, np.eye(6))
    Ci = Li.T @ Li
    C = out["sigma2"] * (np.triu(Ci) + np.triu(Ci, 1).T)
    out["cov_delta"] = C
    G, _ = g_matrix64(delta6)
    if G is not None:
        P = G @ C @ G.T
        out["cov_pose"] = np.triu(P) + np.triu(P, 1).T
    return out


def errors(got, ref):
    """(K_info, K_sig, K_cov_delta, K_cov_pose) of a record (dict or PoseCov-like with 6 x 6 arrays) against the reference, in the units
    of the tolerance: info and sigma2 in 2^-52 relative, the covariances in kappa(A) * 2^-52 relative (Frobenius); None where either
    side has no such field"""
    fro = np.linalg.norm
    k_info = fro(got["info"] - ref["info"]) / (fro(ref["info"]) * EPS)
    k_sig = None if got["sigma2"] is None or ref["sigma2"] == 0 else abs(got["sigma2"] - ref["sigma2"]) / (ref["sigma2"] * EPS)
    kc = []
    for f in ("cov_delta", "cov_pose"):
        if got[f] is None or not ref[f].any(): kc.append(None)
        else: kc.append(fro(got[f] - ref[f]) / (fro(ref[f]) * ref["kappa"] * EPS))
    return k_info, k_sig, kc[0], kc[1]


# ---- the cases of tests/test_gpu_pose_cov.py --------------------------------------------------------------------------------------

SINGLE_NAMES = ["shape-T8-mk1024", "shape-T64-mk1024", "shape-T65-mk1024", "shape-T1024-mk2048", "shape-T1025-mk2048", "shape-T64-mk64",
                "start-rot3e-6-T400", "start-rot1.1e-5-T400", "perm-md12-T400", "nonfinite-T400"]
PITCH_START = np.array([0.0, np.pi / 2, 0.0, 0.0, 0.0, 0.0])


def single_cases():
    """the single-evaluation cases of the GPU test, by name from stage5_ref's lists, then the four collinear ones"""
    by = {c[0]: c for c in S.single_step_cases()}
    return [by[n] for n in SINGLE_NAMES] + S.conditioning_cases()


def pitch_case():
    """the scene of shape-T64-mk1024 evaluated from a rotation of pi / 2 about the camera's y axis: cos(pitch) = 0 (SVO_COV_DELTA_ONLY)"""
    c = {c[0]: c for c in S.single_step_cases()}["shape-T64-mk1024"]
    return ("pitch-T64-mk1024", c[1], c[2], PITCH_START, c[4])


def _one_good_point(cam):
    """nine points of which eight have zero disparity (a non-finite Jacobian, S5:322): the mask holds nine, n_used = 1, dof = -2"""
    p0, p1, response, _ = S.scene_pixels(cam, S.BASE_TRUE, 9, seed=109)
    p0[1:, 2] = p0[1:, 0]
    return S.identity_lists(p0, p1, response)


def no_dof_case():
    """stage 5 ends valid at zero iterations (nine points in the mask) but one point is left to evaluate: SVO_COV_NO_DOF"""
    return ("nodof-T9-mk1024", 1024, _one_good_point, S.BASE_TRUE * 0.98, 2)


def zero_iteration_params(base, robust, min_distance):
    """S.single_step_params with max_iters = 0 as well: both loops run zero times, delta is the custom start, the mask the NMS survivors"""
    p = S.single_step_params(base, robust, min_distance)
    p.max_iters = 0
    return p


_REF = {}


def case_reference(case, robust, kernel_param=3.0, survivors=None):
    """(lists, reference record) of a single case at its start over the NMS survivors (or the mask given), computed once per process"""
    name, mk, build, start, md = case
    key = (name, bool(robust), None if survivors is None else np.asarray(survivors, bool).tobytes())
    if key not in _REF:
        lists = case_scene(case)
        surv = S.nms_survivors(lists, md) if survivors is None else np.asarray(survivors, bool)
        _REF[key] = (lists, reference(lists, S.camera(), start, robust, kernel_param, surv), surv)
    return _REF[key]


def case_scene(case):
    """the seven lists of a case, built once per process (the pitch case shares the scene of shape-T64-mk1024)"""
    if case[0] == "pitch-T64-mk1024": return S.scene({c[0]: c for c in S.single_step_cases()}["shape-T64-mk1024"])
    return S.scene(case)


def inlier_mask(lists, inlier_list):
    """the tracked pairs named by a returned inlier list (result.outliers holds the cur-match index of every inlier, S5:603-610)"""
    return np.isin(lists[0]["second"], np.asarray(inlier_list))


FULL_VALID = ["defaults-T385", "defaults-T1025"]
FULL_INVALID = ["bad-cond-number", "few-after-gate", "stage1-cost-abort"]


def full_cases():
    by = {c[0]: c for c in S.full_run_cases()}
    return [by[n] for n in FULL_VALID + FULL_INVALID]
