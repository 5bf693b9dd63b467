"""The landmarks of a frame (svo_landmark, include/svo_types.h) in mpmath at 50 digits from the float32 pixels, a plain float64 walk of
the kernel's formulas, and the scenes the CPU and GPU tests share (TEST INFRASTRUCTURE, CPU only, no native library).

reference() takes the definitions as the header states them: the triangulation X Y Z = B / den * (fr (ul - cul), fr (vl - cvl), fl fr),
cov_prev = std^2 J J^T with J = d(X, Y, Z) / d(ul, vl, ur), xyz_cur = R(w) X + t with R = exp([w]x), cov_cur = R cov_prev R^T
(+ D cov_delta D^T, D = [d(R X)/dw | I3]).  J is written out in mpmath here and held to mpmath.diff of the triangulation by j_by_diff();
dR/dw IS mpmath.diff of the rotation written from its definition.  Nothing of either is transcribed from the kernel.  The residual is
the one more evaluation of svo_pose_cov, taken from pose_cov_ref._evaluate (extended precision, pixels cast to float, float minus float).

double_walk() is the same record in numpy float64 with the kernel's formulas (k_gn.hip, k_landmarks): what plain double arithmetic
reaches against the reference is the unit the kernel's tolerance is stated in (tests/test_landmarks_ref_cpu.py)."""
import numpy as np
import mpmath

import stage5_ref as S
import pose_cov_ref as Pc
from stereo_vo_amd.abi import (LMK_FINITE, LMK_INLIER, LMK_USED, LMK_POSE, LMK_POSE_TERM, LMK_NONE, LMK_OK, LMK_POINTS_ONLY,
                               keypoint_dtype, dmatch_dtype, index_pair_dtype)

EPS = 2.0 ** -52
DIGITS = 50
TRI = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]          # xx xy xz yy yz zz


# ---- lists -> the flat order of stage 5 -------------------------------------------------------------------------------------------

def flat(octave_lists, n_oct=None, cap=None):
    """octave_lists: one (tracked, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r) per octave.  Returns the pairings in the order stage 5
    concatenates them (S5:419-461), cut at `cap`: obs (T, 8) float32 = l1.xy r1.xy l2.xy r2.xy times scale_norm = 2^octave (applied
    only with more than one octave, S5:422; the product is exact in float32), and octave / prev_match / cur_match (T,) int32"""
    n_oct = len(octave_lists) if n_oct is None else n_oct
    obs, octs, pm, cm = [], [], [], []
    for o, lists in enumerate(octave_lists):
        l1l, l1r, l2l, l2r = S.gather(lists)
        sn = np.float32(1 << o) if n_oct > 1 else np.float32(1)
        a = np.stack([l1l["x"], l1l["y"], l1r["x"], l1r["y"], l2l["x"], l2l["y"], l2r["x"], l2r["y"]], 1).astype(np.float32)
        obs.append(a * sn if n_oct > 1 else a)
        octs.append(np.full(len(a), o, np.int32)); pm.append(lists[0]["first"].astype(np.int32)); cm.append(lists[0]["second"].astype(np.int32))
    obs = np.concatenate(obs) if obs else np.zeros((0, 8), np.float32)
    out = dict(obs=obs.astype(np.float32), octave=np.concatenate(octs), prev_match=np.concatenate(pm), cur_match=np.concatenate(cm))
    if cap is not None: out = {k: v[:cap] for k, v in out.items()}
    return out


def lists_of_obs(obs):
    """identity index lists over the flat pairings (what pose_cov_ref._evaluate gathers from); coordinates as they are"""
    n = len(obs)
    m = np.zeros(n, dmatch_dtype); m["queryIdx"] = np.arange(n); m["trainIdx"] = np.arange(n)
    t = np.zeros(n, index_pair_dtype); t["first"] = np.arange(n); t["second"] = np.arange(n)
    def kp(xy):
        k = np.zeros(n, keypoint_dtype); k["x"], k["y"] = xy[:, 0], xy[:, 1]; return k
    return (t, m, m.copy(), kp(obs[:, 0:2]), kp(obs[:, 2:4]), kp(obs[:, 4:6]), kp(obs[:, 6:8]))


# ---- the definitions in mpmath --------------------------------------------------------------------------------------------------------

def _cam_mp(cam):
    return {k: mpmath.mpf(float(getattr(cam, k))) for k in ("l_fx", "l_cx", "l_cy", "r_fx", "r_cx", "baseline")}


def triangulate_mp(c, ul, vl, ur):
    """(den, [X, Y, Z]) of S5:529-544; den = 0 raises ZeroDivisionError"""
    den = c["l_fx"] * (c["r_cx"] - ur) + c["r_fx"] * (ul - c["l_cx"])
    b_d = c["baseline"] / den
    return den, [b_d * c["r_fx"] * (ul - c["l_cx"]), b_d * c["r_fx"] * (vl - c["l_cy"]), b_d * c["l_fx"] * c["r_fx"]]


def j_mp(c, ul, vl, ur):
    """J = d(X, Y, Z) / d(ul, vl, ur), from X = B fr (ul - cul) / den etc. with d den / d ul = fr, d den / d ur = -fl"""
    den, X = triangulate_mp(c, ul, vl, ur)
    fl, fr, B = c["l_fx"], c["r_fx"], c["baseline"]
    return [[B * fr / den - X[0] * fr / den, mpmath.mpf(0), X[0] * fl / den],
            [-X[1] * fr / den, B * fr / den, X[1] * fl / den],
            [-X[2] * fr / den, mpmath.mpf(0), X[2] * fl / den]]


def j_by_diff(cam, ul, vl, ur):
    """the same J by mpmath.diff of triangulate_mp: 3 x 3 list of mpf (the cross-check of j_mp)"""
    with mpmath.workdps(DIGITS):
        c = _cam_mp(cam)
        x = (mpmath.mpf(float(ul)), mpmath.mpf(float(vl)), mpmath.mpf(float(ur)))
        return [[mpmath.diff(lambda a, b, d, r=r: triangulate_mp(c, a, b, d)[1][r], x, tuple(1 if j == k else 0 for j in range(3))) for k in range(3)] for r in range(3)]


def rotation_mp(w):
    """R = exp([w]x) = I + a K + b K^2, a = sin t / t, b = (1 - cos t) / t^2: the exact Rodrigues rotation (3 x 3 mpmath matrix)"""
    w1, w2, w3 = w
    th = mpmath.sqrt(w1 * w1 + w2 * w2 + w3 * w3)
    a = mpmath.sin(th) / th if th != 0 else mpmath.mpf(1)
    b = (1 - mpmath.cos(th)) / (th * th) if th != 0 else mpmath.mpf(1) / 2
    K = mpmath.matrix([[0, -w3, w2], [w3, 0, -w1], [-w2, w1, 0]])
    return mpmath.eye(3) + a * K + b * (K * K)


def rotation_derivs_mp(w):
    """(R, [dR/dw_0, dR/dw_1, dR/dw_2]) at the float64 rotation vector w: the derivatives by mpmath.diff of rotation_mp"""
    x = tuple(mpmath.mpf(float(v)) for v in w)
    R = rotation_mp(x)
    dR = []
    for k in range(3):
        D = mpmath.matrix(3, 3)
        for i in range(3):
            for j in range(3):
                D[i, j] = mpmath.diff(lambda a, b, c, i=i, j=j: rotation_mp((a, b, c))[i, j], x, tuple(1 if q == k else 0 for q in range(3)))
        dR.append(D)
    return R, dR


def conditioning(obs, cam):
    """(|fl (cur - ur)| + |fr (ul - cul)|) / |den| per pairing in float64 (inf where den = 0): how far the subtraction in den amplifies the
    rounding of its two products"""
    ul, ur = obs[:, 0].astype(np.float64), obs[:, 2].astype(np.float64)
    a, b = cam.l_fx * (cam.r_cx - ur), cam.r_fx * (ul - cam.l_cx)
    with np.errstate(all="ignore"):
        return (np.abs(a) + np.abs(b)) / np.abs(a + b)


def _residuals(obs, cam, delta6, mask, dt):
    """(s (T,) float64, used (T,) bool, dmid) of the one more evaluation over `mask` (pose_cov_ref._evaluate in dtype dt)"""
    T = len(obs)
    s = np.zeros(T); used = np.zeros(T, bool)
    if T == 0 or not mask.any(): return s, used, np.inf
    J, r, used, pix = Pc._evaluate(lists_of_obs(obs), cam, delta6, np.nonzero(mask)[0], dt)
    s[used] = (r * r).sum(axis=1).astype(np.float64)
    dmid = float(S._midpoint_distance(pix.astype(S.LD)).min()) if len(pix) else np.inf
    return s, used, dmid


def _empty(T):
    return dict(xyz_prev=np.zeros((T, 3)), cov_prev=np.zeros((T, 6)), xyz_cur=np.zeros((T, 3)), cov_cur=np.zeros((T, 6)), residual=np.zeros(T),
                flags=np.zeros(T, np.uint32))


def reference(obs, cam, std, delta6=None, mask=None, cov_delta=None):
    """The records of `obs` (flat(): (T, 8) float32) as float64 arrays rounded from 50 digits.  delta6 None: the lane's stage 5 did not
    end valid (SVO_LMK_POINTS_ONLY: nothing of the pose).  mask: the mask stage 5 ended with (T,) bool.  cov_delta: 6 x 6 (any real
    type) when the pose term is included, else None.  Also cond (conditioning()), dmid (of the residual evaluation) and scale_cur =
    |R X| + |t| per pairing, the magnitude xyz_cur's error is measured against."""
    T = len(obs)
    out = _empty(T)
    out["cond"] = conditioning(obs, cam); out["dmid"] = np.inf; out["scale_cur"] = np.zeros(T)
    ok = delta6 is not None
    mask = np.zeros(T, bool) if mask is None else np.asarray(mask, bool)
    fl64 = lambda v: float(v)
    with mpmath.workdps(DIGITS):
        c = _cam_mp(cam)
        var = mpmath.mpf(float(std)) ** 2
        if ok:
            R, dR = rotation_derivs_mp(delta6[:3])
            t = [mpmath.mpf(float(v)) for v in delta6[3:]]
            C = None if cov_delta is None else [[S._mpf(cov_delta[i][j]) for j in range(6)] for i in range(6)]
        for i in range(T):
            ul, vl, ur = (mpmath.mpf(float(obs[i, k])) for k in (0, 1, 2))
            den = c["l_fx"] * (c["r_cx"] - ur) + c["r_fx"] * (ul - c["l_cx"])
            flags = 0
            if den != 0:
                _, X = triangulate_mp(c, ul, vl, ur)
                J = j_mp(c, ul, vl, ur)
                Cp = [[var * sum(J[r][k] * J[s][k] for k in range(3)) for s in range(3)] for r in range(3)]
                x64 = np.array([fl64(v) for v in X]); cp64 = np.array([fl64(Cp[r][s]) for r, s in TRI])
                if np.isfinite(x64).all() and np.isfinite(cp64).all():
                    flags |= LMK_FINITE
                    out["xyz_prev"][i] = x64; out["cov_prev"][i] = cp64
                    if ok:
                        flags |= LMK_POSE | (LMK_POSE_TERM if C is not None else 0)
                        RX = [sum(R[r, k] * X[k] for k in range(3)) for r in range(3)]
                        out["xyz_cur"][i] = [fl64(RX[r] + t[r]) for r in range(3)]
                        out["scale_cur"][i] = fl64(mpmath.sqrt(sum(v * v for v in RX)) + mpmath.sqrt(sum(v * v for v in t)))
                        M = [[sum(R[r, k] * Cp[k][s] for k in range(3)) for s in range(3)] for r in range(3)]
                        Cc = [[sum(M[r][k] * R[s, k] for k in range(3)) for s in range(3)] for r in range(3)]
                        if C is not None:
                            D = [[sum(dR[k][r, q] * X[q] for q in range(3)) for k in range(3)] + [mpmath.mpf(1 if r == k else 0) for k in range(3)] for r in range(3)]
                            E = [[sum(D[r][k] * C[k][s] for k in range(6)) for s in range(6)] for r in range(3)]
                            for r in range(3):
                                for s in range(3): Cc[r][s] += sum(E[r][k] * D[s][k] for k in range(6))
                        out["cov_cur"][i] = [fl64(Cc[r][s]) for r, s in TRI]
            if ok and mask[i]: flags |= LMK_INLIER
            out["flags"][i] = flags
    if ok:
        s, used, dmid = _residuals(obs, cam, delta6, mask, S.LD)
        out["dmid"] = dmid
        out["flags"][used] |= LMK_USED
        fin = (out["flags"] & LMK_FINITE) != 0
        out["residual"] = np.where(fin, s, 0.0)
    return out


# ---- the double walk: the kernel's formulas in numpy float64 -----------------------------------------------------------------------

def double_walk(obs, cam, std, delta6=None, mask=None, cov_delta=None):
    """the same record with k_landmarks' formulas in float64 (the triangulation operation by operation as stage5_ref.triangulate64, the
    rotation and its derivatives by pose_cov_ref.rotation_derivs64, which is cov_rotation_derivs)"""
    T = len(obs)
    out = _empty(T)
    ok = delta6 is not None
    mask = np.zeros(T, bool) if mask is None else np.asarray(mask, bool)
    if T == 0: return out
    fl, fr, cul, cvl, cur_, B = cam.l_fx, cam.r_fx, cam.l_cx, cam.l_cy, cam.r_cx, cam.baseline
    ul, vl, ur = (obs[:, k].astype(np.float64) for k in (0, 1, 2))
    var = float(std) * float(std)
    with np.errstate(all="ignore"):
        den = fl * (cur_ - ur) + fr * (ul - cul)
        b_d = B / den
        X = np.stack([b_d * fr * (ul - cul), b_d * fr * (vl - cvl), b_d * fl * fr + 0 * ul], 1)
        idn = 1.0 / den; bf = (B / den) * fr; kl = fr * idn; kr = fl * idn
        J = np.zeros((T, 3, 3))
        J[:, 0, 0] = bf - X[:, 0] * kl; J[:, 0, 2] = X[:, 0] * kr
        J[:, 1, 0] = -X[:, 1] * kl; J[:, 1, 1] = bf; J[:, 1, 2] = X[:, 1] * kr
        J[:, 2, 0] = -X[:, 2] * kl; J[:, 2, 2] = X[:, 2] * kr
        Cp = var * np.einsum("nrk,nsk->nrs", J, J)
        tri = np.stack([Cp[:, r, s] for r, s in TRI], 1)
        fin = (den != 0) & np.isfinite(X).all(1) & np.isfinite(tri).all(1)
        out["xyz_prev"][fin] = X[fin]; out["cov_prev"][fin] = tri[fin]
        out["flags"][fin] |= LMK_FINITE
        if ok:
            d = np.asarray(delta6, np.float64)
            R, dR = Pc.rotation_derivs64(d[:3])
            xc = X @ R.T + d[3:]
            Cc = np.einsum("rk,nks,qs->nrq", R, Cp, R)
            if cov_delta is not None:
                C = np.asarray(cov_delta, np.float64)
                D = np.zeros((T, 3, 6))
                for k in range(3): D[:, :, k] = X @ dR[k].T
                D[:, :, 3:] = np.eye(3)
                Cc = Cc + np.einsum("nrk,ks,nqs->nrq", D, C, D)
            out["xyz_cur"][fin] = xc[fin]; out["cov_cur"][fin] = np.stack([Cc[:, r, s] for r, s in TRI], 1)[fin]
            out["flags"][fin] |= LMK_POSE | (LMK_POSE_TERM if cov_delta is not None else 0)
            out["flags"][mask] |= LMK_INLIER
            s, used, _ = _residuals(obs, cam, d, mask, np.float64)
            out["flags"][used] |= LMK_USED
            out["residual"] = np.where(fin, s, 0.0)
    return out


def tri_to_mat(tri):
    tri = np.asarray(tri)
    return tri[..., [0, 1, 2, 1, 3, 4, 2, 4, 5]].reshape(tri.shape[:-1] + (3, 3))


def errors(got, ref, kappa=0.0):
    """The error of every field of `got` (dict of arrays as reference() returns, or a numpy array of abi.Landmark) against the reference,
    maximum over the finite pairings, in the units of the tolerance:
      xyz_prev   |dX| / (|X_ref| cond 2^-52)                 cov_prev  |dC|_F / (|C_ref|_F cond 2^-52)
      xyz_cur    |dX| / ((|R X| + |t|) cond 2^-52)           cov_cur   |dC|_F / (|C_ref|_F (cond + kappa) 2^-52), kappa = kappa_2 of the pose
                                                                       record's information where the pose term is included, else 0
      residual   |ds| / (s_ref 2^-52) where s_ref > 0 (where it is 0 the two must be equal: reported as inf otherwise)
    Returns a dict of floats (0.0 where there is nothing to compare)."""
    fin = (ref["flags"] & LMK_FINITE) != 0
    out = dict(xyz_prev=0.0, cov_prev=0.0, xyz_cur=0.0, cov_cur=0.0, residual=0.0)
    if not fin.any(): return out
    cond = ref["cond"][fin]
    n2 = lambda a: np.linalg.norm(a, axis=-1)
    g = lambda f: np.asarray(got[f], np.float64)[fin]
    out["xyz_prev"] = float((n2(g("xyz_prev") - ref["xyz_prev"][fin]) / (n2(ref["xyz_prev"][fin]) * cond * EPS)).max())
    cm = lambda a: n2(tri_to_mat(a).reshape(len(a), 9))
    out["cov_prev"] = float((cm(g("cov_prev") - ref["cov_prev"][fin]) / (cm(ref["cov_prev"][fin]) * cond * EPS)).max())
    pose = ((ref["flags"] & LMK_POSE) != 0)[fin]
    if pose.any():
        out["xyz_cur"] = float((n2(g("xyz_cur") - ref["xyz_cur"][fin])[pose] / (ref["scale_cur"][fin][pose] * cond[pose] * EPS)).max())
        term = ((ref["flags"] & LMK_POSE_TERM) != 0)[fin][pose]
        unit = cm(ref["cov_cur"][fin])[pose] * (cond[pose] + np.where(term, kappa, 0.0)) * EPS
        out["cov_cur"] = float((cm(g("cov_cur") - ref["cov_cur"][fin])[pose] / unit).max())
    s_ref, s_got = ref["residual"][fin], g("residual")
    pos = s_ref > 0
    if pos.any(): out["residual"] = float((np.abs(s_got - s_ref)[pos] / (s_ref[pos] * EPS)).max())
    if (s_got[~pos] != 0).any(): out["residual"] = np.inf
    return out


def min_eigenvalue_ratio(tri):
    """lambda_min / lambda_max of the 3 x 3 matrices of upper triangles (n, 6); 0 / 0 counts as 0"""
    if len(tri) == 0: return np.zeros(0)
    lam = np.linalg.eigvalsh(tri_to_mat(np.asarray(tri, np.float64)))
    with np.errstate(all="ignore"):
        return np.where(lam[:, 2] > 0, lam[:, 0] / lam[:, 2], 0.0)


# ---- scenes of the landmarks' own ---------------------------------------------------------------------------------------------------

def degenerate_scene(cam, T=40, seed=71):
    """S.synthetic with three pairings replaced beside good neighbours: [5] ur = ul (den = 0 exactly: fl = fr and cul = cur, so the two
    products are exact opposites), [11] a negative disparity (ur = ul + 7 px: a finite point BEHIND the camera), [17] ur far outside the
    image (ul + 40000 px: finite, negative Z, 2 mm from the camera).  Their responses are the three smallest, so they displace no good
    point from the NMS mask.  [17] sits a quarter of a pixel from [18], in its grid cell, and the mask drops it: inside the mask its
    Jacobian (f / Z^2 at Z = 2 mm) swamps the unweighted Hessian and stage 5 gates nearly every point away (5 inliers left of 40; the
    oracle, probed while this scene was built).  [5] and [11] stay in the mask.  Stage 5 then ends valid on it, with the default limits
    and with none (tests/test_landmarks_ref_cpu.py checks that through the oracle)."""
    p0, p1, response, _ = S.scene_pixels(cam, S.BASE_TRUE, T, seed, noise=0.2)
    p0 = p0.copy(); p1 = p1.copy()
    p0[5, 2] = p0[5, 0]
    p0[11, 2] = p0[11, 0] + 7.0
    p0[17, :2] = p0[18, :2] + 0.25; p0[17, 3] = p0[17, 1]; p1[17] = p1[18] + 0.25
    p0[17, 2] = p0[17, 0] + 40000.0
    response = response.copy(); response[[5, 11, 17]] = [1e-7, 2e-7, 3e-7]
    n = len(p0)
    m = np.zeros(n, dmatch_dtype); m["queryIdx"] = np.arange(n); m["trainIdx"] = np.arange(n)
    t = np.zeros(n, index_pair_dtype); t["first"] = np.arange(n); t["second"] = np.arange(n)
    return (t, m, m.copy(), S.kp_array(p0[:, :2], response), S.kp_array(p0[:, 2:], response), S.kp_array(p1[:, :2], response), S.kp_array(p1[:, 2:], response))


DEGENERATE = dict(zero_den=5, negative_disparity=11, far_outside=17)

# ---- the single evaluations of tests/test_gpu_landmarks.py ------------------------------------------------------------------------
# (name, max_kps, builder, min_distance).  SVO_RUN_OPTIMIZE takes no start from its caller: with use_custom_initial_pose the start is
# zero (S5:504-505 with P:338's default argument), so with both iteration limits at 0 the returned delta is ZERO, bit for bit; a
# non-zero delta known bit for bit is reached through the warm start (the GPU test evaluates the reference at the delta it reads back).
ZERO = np.zeros(6)
GPU_T = [8, 63, 64, 65, 255, 256, 257]


def gpu_cases():
    cases = [("T%d-mk1024" % T, 1024, (lambda cam, T=T: S.synthetic(cam, S.BASE_TRUE, T, seed=100 + T, noise=0.2)), 2) for T in GPU_T]
    cases.append(("T1100-mk2048", 2048, (lambda cam: S.permuted(cam, S.BASE_TRUE, 1100, seed=51, noise=0.3, n_out=100)), 2))       # above LdsGaussNewton::lc() = 1024: k_gauss_newton's scratch path
    cases.append(("T64-mk64", 64, (lambda cam: S.synthetic(cam, S.BASE_TRUE, 64, seed=164, noise=0.2)), 2))
    cases.append(("perm-md12-T400", 1024, (lambda cam: S.permuted(cam, S.BASE_TRUE, 400, seed=700)), 12))                          # the mask removes a real share
    cases.append(("degenerate-T40", 1024, degenerate_scene, 2))
    cases.append(("collinear-eps0", 1024, (lambda cam: S.collinear(cam, S.COLLINEAR_TRUE, 0.0)), 2))                               # SVO_COV_RANK_DEFICIENT: no pose term
    return cases


_SCENES, _REFS = {}, {}


def case_scene(case):
    if case[0] not in _SCENES: _SCENES[case[0]] = case[2](S.camera())
    return _SCENES[case[0]]


def pose_term_of(pc_ref):
    """whether a pose record described by pose_cov_ref.reference() carries a cov_delta: SVO_COV_OK or SVO_COV_DELTA_ONLY with A invertible"""
    return pc_ref["dof"] > 0 and pc_ref["state"] in (Pc.COV_OK, Pc.COV_DELTA_ONLY) and bool(pc_ref["cov_delta"].any())


def case_reference(case, delta6=ZERO, std=1.0, with_pose_cov=True, robust=1, kernel_param=3.0):
    """(flat pairings, mask, pose-covariance reference, landmark reference) of a case at delta6 over its NMS survivors, once per process"""
    key = (case[0], np.asarray(delta6, np.float64).tobytes(), float(std), bool(with_pose_cov), bool(robust))
    if key not in _REFS:
        lists = case_scene(case)
        f = flat([lists])
        surv = S.nms_survivors(lists, case[3])
        pc = Pc.reference(lists, S.camera(), delta6, robust, kernel_param, surv)
        # (the kernel's record is SVO_COV_RANK_DEFICIENT where A fails chol6's pivot test: rel_pd < 1; the CPU test holds every case to
        # rel_pd >= 1e3 or < 1, so that the state is the definition's to predict)
        term = with_pose_cov and pose_term_of(pc) and pc["rel_pd"] >= 1e3
        _REFS[key] = (f, surv, pc, reference(f["obs"], S.camera(), std, delta6, surv, pc["cov_delta"] if term else None))
    return _REFS[key]


def octave_scene(cam, counts=(30, 20, 12), seed=81):
    """one permuted scene per octave with the pixel coordinates divided by 2^octave (what the x1/2 octave images would show), so that
    scale_norm brings every octave back to the same camera: lists for svo_put_*_oct"""
    out = []
    for o, T in enumerate(counts):
        lists = S.permuted(cam, S.BASE_TRUE, T, seed=seed + o, noise=0.2, extra=9)
        scaled = []
        for a in lists:
            a = a.copy()
            if a.dtype == keypoint_dtype:
                a["x"] = a["x"] / np.float32(1 << o); a["y"] = a["y"] / np.float32(1 << o)
                a["response"] = a["response"] + np.float32(3e-7 * o)          # no two tracked points of the lane share a response: the NMS order has no ties
            scaled.append(a)
        out.append(tuple(scaled))
    return out
