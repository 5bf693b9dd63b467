"""The yardstick of the landmark records (svo_landmark), qualified without a GPU: tests/landmarks_ref.py against its own
finite-difference and mpmath.diff forms, the constants the GPU test's tolerances are stated in, the conditions its cases must meet,
and the parts of the feature that need no device: the record's size and the INI loader (CPU only)."""
import ctypes as C
import os
import re

import numpy as np
import mpmath
import pytest

import stage5_ref as S
import pose_cov_ref as Pc
import landmarks_ref as Lr
from stereo_vo_amd import hip
from stereo_vo_amd.abi import Landmark, LandmarksInfo, LMK_FINITE, LMK_INLIER, LMK_USED, LMK_POSE, LMK_POSE_TERM, north_star_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The largest errors of the DOUBLE WALK (landmarks_ref.double_walk: k_landmarks' formulas in plain numpy float64) against the 50-digit
# reference, in the units landmarks_ref.errors states -- 2^-52 relative, scaled by the triangulation's conditioning
# cond = (|fl (cur - ur)| + |fr (ul - cul)|) / |den|, and for cov_cur by cond + kappa_2 of the pose record's information where the pose
# term is included -- over every evaluation of every_evaluation() below, as test_tolerance_constants measures them, rounded up
# (the run of `pytest -s tests/test_landmarks_ref_cpu.py::test_tolerance_constants` on the tree that added the feature, x86-64, which
# printed "xyz_prev 0.9181 (T255-mk1024), xyz_cur 0.9181 (T255-mk1024), cov_prev 2.402 (T255-mk1024), cov_cur 2.402 (T255-mk1024
# no-cov), cov_cur_term 0.2323 (nonfinite-T400), residual 0.8535 (pitch-T64-mk1024)"):
#   xyz_prev, xyz_cur   K_XYZ   0.92: three roundings in den (two products and their difference, which cond scales), then a division and
#                               two products
#   cov_prev, cov_cur   K_COV   2.40 without the pose term; with it 0.23 of its wider unit (the walk's cov_delta is within
#                               22 kappa 2^-52 of the reference's, K_COV of test_pose_cov_ref_cpu.py, and D cov_delta D^T is a part of cov_cur)
#   residual            K_RES   |s - s_ref| / (s_ref 2^-52): 0.85 (four exact float differences, squared and summed in double)
# test_tolerance_constants fails when a maximum moves above its constant or below a quarter of it.  The kernel's bounds are FACTOR = 16
# times these, the project's margin for k_pose_covariance and for its reasons: fma contraction and gn_rcp / gn_rsqrt inside gn_point,
# and a maximum over a few thousand pairings understating the walk's own worst case.
K_XYZ = 1.0
K_COV = 2.5
K_RES = 0.9
FACTOR = 16
COND_MAX = 1.0e4          # no pairing of any case closer to den = 0 than this, other than the one built to sit on it
DMID_MIN = 1e-10          # no predicted pixel within this of a binary32 rounding midpoint (the residual's float casts are then exact)


def base_params():
    from oracle import oracle as O
    return north_star_params(O.default_params(), orb_nfeats=40)


def every_evaluation():
    """(tag, flat pairings, std_noise_pixels, delta, mask, kappa of the pose record, reference, the walk's cov_delta or None) of: the GPU
    test's single evaluations at delta = 0 with and without the pose term, and the pose covariance's single cases from THEIR starts
    (rotations on both sides of the small-angle switch, up to 0.6 rad) with the term"""
    cam = S.camera()
    for case in Lr.gpu_cases():
        for with_cov in (True, False):
            f, surv, pc, ref = Lr.case_reference(case, Lr.ZERO, 1.0, with_cov)
            term = bool((ref["flags"] & LMK_POSE_TERM).any())
            wc = Pc.double_walk(Lr.case_scene(case), cam, Lr.ZERO, 1, 3.0, surv)["cov_delta"] if term else None
            yield ("%s%s" % (case[0], "" if with_cov else " no-cov"), f["obs"], 1.0, Lr.ZERO, surv, pc["kappa"], ref, wc)
    names = ["shape-T65-mk1024", "start-rot3e-6-T400", "start-rot1.1e-5-T400", "nonfinite-T400"]
    by = {c[0]: c for c in S.single_step_cases()}
    for case in [by[n] for n in names] + [by["start-rot0.499-T400"], by["start-rot0.59-T400"], Pc.pitch_case()]:
        lists, pc, surv = Pc.case_reference(case, 1)
        f = Lr.flat([lists])
        term = Lr.pose_term_of(pc) and pc["rel_pd"] >= 1e3
        ref = Lr.reference(f["obs"], cam, 0.7, case[3], surv, pc["cov_delta"] if term else None)
        wc = Pc.double_walk(lists, cam, case[3], 1, 3.0, surv)["cov_delta"] if term else None
        yield (case[0], f["obs"], 0.7, case[3], surv, pc["kappa"], ref, wc)


def test_jacobian_and_rotation_derivatives_against_their_definitions():
    """J of the triangulation, written out in mpmath, equals mpmath.diff of the triangulation and a central difference of it; dR/dw
    (mpmath.diff of exp([w]x)) equals a central difference of the rotation, at zero, on both sides of the small-angle switch and at 0.6 rad"""
    cam = S.camera()
    f = Lr.flat([Lr.case_scene({c[0]: c for c in Lr.gpu_cases()}["degenerate-T40"])])
    with mpmath.workdps(Lr.DIGITS):
        c = Lr._cam_mp(cam)
        for i in (0, 3, Lr.DEGENERATE["negative_disparity"], Lr.DEGENERATE["far_outside"], 30):
            x = [mpmath.mpf(float(v)) for v in f["obs"][i, :3]]
            J, Jd = Lr.j_mp(c, *x), Lr.j_by_diff(cam, *f["obs"][i, :3])
            h = mpmath.mpf(10) ** -20
            for k in range(3):
                xp, xm = list(x), list(x); xp[k] += h; xm[k] -= h
                fd = [(a - b) / (2 * h) for a, b in zip(Lr.triangulate_mp(c, *xp)[1], Lr.triangulate_mp(c, *xm)[1])]
                for r in range(3):
                    scale = max(abs(J[r][k]), mpmath.mpf(10) ** -30)
                    assert abs(J[r][k] - Jd[r][k]) <= scale * mpmath.mpf(10) ** -35, (i, r, k)
                    assert abs(J[r][k] - fd[r]) <= scale * mpmath.mpf(10) ** -25 + mpmath.mpf(10) ** -30, (i, r, k)
        for w in (np.zeros(3), S.STARTS["rot3e-6"][:3], S.STARTS["rot1.1e-5"][:3], S.STARTS["rot0.59"][:3], Pc.PITCH_START[:3]):
            R, dR = Lr.rotation_derivs_mp(w)
            assert mpmath.norm(R * R.T - mpmath.eye(3)) < mpmath.mpf(10) ** -45
            h = mpmath.mpf(10) ** -18
            for k in range(3):
                wp = [mpmath.mpf(float(v)) for v in w]; wm = list(wp); wp[k] += h; wm[k] -= h
                fd = (Lr.rotation_mp(wp) - Lr.rotation_mp(wm)) / (2 * h)
                assert mpmath.norm(fd - dR[k]) < mpmath.mpf(10) ** -30, (w, k)


def test_reference_properties():
    """the reference's own records: cov_prev = std^2 J J^T is positive definite, scales with std^2, cov_cur - R cov_prev R^T is positive
    semi-definite (the pose term only adds), and xyz_cur projects where stage 5 predicts the current pixels"""
    case = {c[0]: c for c in Lr.gpu_cases()}["T65-mk1024"]
    cam = S.camera()
    f, surv, pc, ref = Lr.case_reference(case, Lr.ZERO, 1.0, True)
    _, _, _, ref0 = Lr.case_reference(case, Lr.ZERO, 1.0, False)
    ref2 = Lr.reference(f["obs"], cam, 2.0, Lr.ZERO, surv, None)
    assert (ref["flags"] & LMK_FINITE).all() and (ref["flags"] & LMK_POSE_TERM).all() and not (ref0["flags"] & LMK_POSE_TERM).any()
    assert (Lr.min_eigenvalue_ratio(ref["cov_prev"]) > 0).all()
    assert np.allclose(ref2["cov_prev"], 4.0 * ref0["cov_prev"], rtol=1e-15, atol=0) and np.array_equal(ref2["xyz_prev"], ref0["xyz_prev"])
    assert np.array_equal(ref0["cov_cur"], ref0["cov_prev"]) and np.array_equal(ref0["xyz_cur"], ref0["xyz_prev"]), "delta = 0: R = I, t = 0"
    extra = np.linalg.eigvalsh(Lr.tri_to_mat(ref["cov_cur"] - ref0["cov_cur"]))
    assert (extra[:, 0] >= -1e-12 * extra[:, 2]).all() and (extra[:, 2] > 0).all()
    d = S.BASE_TRUE
    refd = Lr.reference(f["obs"], cam, 1.0, d, surv, None)
    pix = S.pixels(cam, refd["xyz_cur"])
    assert np.abs(pix - f["obs"][:, 4:].astype(np.float64)).max() < 2.0, "the scene moves by BASE_TRUE: the landmarks project onto the current pixels (0.2 px noise)"
    assert np.allclose(refd["residual"][surv], ((pix - f["obs"][:, 4:]) ** 2).sum(1)[surv], rtol=1e-3)
    assert not refd["residual"][~surv].any() and np.array_equal((refd["flags"] & LMK_INLIER) != 0, surv)


def test_tolerance_constants():
    """the double walk against the reference over every evaluation: integers and flags equal, the maxima are the constants above"""
    cam = S.camera()
    worst = {k: ("", 0.0) for k in ("xyz_prev", "xyz_cur", "cov_prev", "cov_cur", "cov_cur_term", "residual")}
    for tag, obs, std, delta, mask, kappa, ref, walk_cov in every_evaluation():
        w = Lr.double_walk(obs, cam, std, delta, mask, walk_cov)
        assert np.array_equal(w["flags"], ref["flags"]), (tag, np.nonzero(w["flags"] != ref["flags"])[0][:5])
        e = Lr.errors(w, ref, kappa)
        term = bool((ref["flags"] & LMK_POSE_TERM).any())
        for k, v in e.items():
            key = "cov_cur_term" if (k == "cov_cur" and term) else k
            if v > worst[key][1]: worst[key] = (tag, v)
    print("\nlandmarks, double walk against the reference: " + ", ".join("%s %.4g (%s)" % (k, v[1], v[0]) for k, v in worst.items()))
    for keys, const in ((("xyz_prev", "xyz_cur"), K_XYZ), (("cov_prev", "cov_cur", "cov_cur_term"), K_COV), (("residual",), K_RES)):
        top = max(worst[k][1] for k in keys)
        assert const / 4 < top <= const, (keys, [worst[k] for k in keys], const)


def test_conditions_on_the_cases():
    """no pairing within COND_MAX of den = 0 but the one built to sit on it; no predicted pixel within DMID_MIN of a rounding midpoint;
    every pose record clear of chol6's pivot test on one side or the other; the degenerate pairings are what the GPU test says they are"""
    zero_den = Lr.DEGENERATE["zero_den"]
    for tag, obs, std, delta, mask, kappa, ref, walk_cov in every_evaluation():
        cond = ref["cond"].copy()
        fin = (ref["flags"] & LMK_FINITE) != 0
        if tag.startswith("degenerate"):
            assert not fin[zero_den] and np.isinf(cond[zero_den]) and fin.sum() == len(fin) - 1, tag
            cond[zero_den] = 1.0
        elif tag.startswith("nonfinite"): cond[~fin] = 1.0          # the scene's own zero-disparity points (ur = ul exactly)
        else: assert fin.all(), tag
        assert np.isinf(ref["cond"][~fin]).all(), (tag, "a pairing that is not finite sits on den = 0 exactly")
        assert cond.max() <= COND_MAX, (tag, cond.max())
        assert ref["dmid"] >= DMID_MIN, (tag, ref["dmid"])
    for case in Lr.gpu_cases():
        f, surv, pc, ref = Lr.case_reference(case, Lr.ZERO, 1.0, True)
        assert pc["rel_pd"] >= 1e3 or pc["rel_pd"] < 1.0, (case[0], pc["rel_pd"])
        assert bool((ref["flags"] & LMK_POSE_TERM).any()) == (case[0] != "collinear-eps0"), case[0]
        assert int(surv.sum()) >= 8, case[0]
    f, surv, pc, ref = Lr.case_reference({c[0]: c for c in Lr.gpu_cases()}["degenerate-T40"], Lr.ZERO, 1.0, True)
    d = Lr.DEGENERATE
    assert not ref["flags"][d["zero_den"]] & LMK_FINITE and not np.r_[ref["xyz_prev"][d["zero_den"]], ref["cov_prev"][d["zero_den"]], ref["cov_cur"][d["zero_den"]], ref["residual"][d["zero_den"]]].any()
    for k in ("negative_disparity", "far_outside"):
        assert ref["flags"][d[k]] & LMK_FINITE and ref["xyz_prev"][d[k], 2] < 0, k
    assert surv[d["zero_den"]] and surv[d["negative_disparity"]] and not surv[d["far_outside"]], "two of the degenerate pairings are in the mask, the NMS drops the third"
    assert ref["flags"][d["zero_den"]] & LMK_INLIER and not ref["flags"][d["zero_den"]] & LMK_USED, "in the mask, dropped by the evaluation (S5:322)"
    assert ref["flags"][d["negative_disparity"]] & LMK_USED and ref["residual"][d["negative_disparity"]] > 0
    assert not ref["flags"][d["far_outside"]] & (LMK_INLIER | LMK_USED) and ref["residual"][d["far_outside"]] == 0


def test_stage_5_ends_valid_on_the_degenerate_scene():
    """through the oracle: with the default iteration limits and with none (the GPU test's single evaluation)"""
    from oracle import oracle as O
    lists = Lr.case_scene({c[0]: c for c in Lr.gpu_cases()}["degenerate-T40"])
    for p in (base_params(), Pc.zero_iteration_params(base_params(), 1, 2)):
        o = O.Oracle(p)
        v, r, resid, outl = o.change_in_pose(*lists, S.camera())
        o.close()
        assert v and r.error_code == 0, (v, r.error_code)


def test_three_octaves_flatten_in_stage_5_order():
    """flat(): octave by octave, scale_norm 1 / 2 / 4 brings every octave back to full-resolution pixels exactly, the cut is a prefix"""
    cam = S.camera()
    octs = Lr.octave_scene(cam)
    f = Lr.flat(octs)
    counts = [len(o[0]) for o in octs]
    assert list(f["octave"]) == sum(([o] * n for o, n in enumerate(counts)), []) and len(f["obs"]) == sum(counts)
    off = 0
    for o, lists in enumerate(octs):
        l1l = S.gather(lists)[0]
        assert np.array_equal(f["obs"][off:off + counts[o], 0], l1l["x"] * np.float32(1 << o))
        assert np.array_equal(f["prev_match"][off:off + counts[o]], lists[0]["first"])
        off += counts[o]
    assert (f["obs"][:, 0] > 1).all() and (f["obs"][:, 0] < S.W).all()
    cut = Lr.flat(octs, cap=40)
    assert len(cut["obs"]) == 40 and np.array_equal(cut["obs"], f["obs"][:40])
    assert np.array_equal(Lr.flat(octs[:1])["obs"][:, 0], S.gather(octs[0])[0]["x"]), "one octave: no scale_norm"


def test_record_size_against_the_library_and_the_header():
    """svo_landmark_abi_size() (callable without a device) = the numpy record = the header's static_assert"""
    L = hip.lib()
    assert L.svo_landmark_abi_size() == Landmark.itemsize == 176 and Landmark.itemsize % 16 == 0
    assert C.sizeof(LandmarksInfo) == 32
    text = open(os.path.join(ROOT, "include", "svo_types.h")).read()
    m = re.search(r"static_assert\(sizeof\(svo_landmark\) == (\d+) && sizeof\(svo_landmark\) % 16 == 0", text)
    assert m and int(m.group(1)) == Landmark.itemsize
    assert re.search(r"static_assert\(sizeof\(svo_landmarks_info\) == 32", text)
    offsets = {n: Landmark.fields[n][1] for n in Landmark.names}
    assert offsets == dict(xyz_prev=0, cov_prev=24, xyz_cur=72, cov_cur=96, residual=144, match_id=152, prev_match=156, cur_match=160, octave=164, flags=168, reserved=172)
    for name in ("svo_set_landmarks", "svo_get_landmarks_enabled", "svo_landmarks_load_ini", "svo_get_landmarks_info", "svo_get_landmarks",
                 "svo_copy_landmarks_async", "svo_landmark_abi_size", "svo_fpstream_set_landmarks", "svo_put_tracked_oct"):
        assert hasattr(L, name), name


def test_std_noise_pixels_from_an_ini_file(tmp_path):
    """svo_landmarks_load_ini: the key present, absent (the value passed in stays), negative (SVO_ERR_ARG, the value stays), and a
    section that is not there; it needs no device"""
    ini = tmp_path / "vo.ini"
    ini.write_text("[LEAST_SQUARES]\nstd_noise_pixels = 0.35\nmax_iters = 7\n\n[EMPTY_LS]\nmax_iters = 7\n\n[BAD_LS]\nstd_noise_pixels = -2\n")
    assert hip.load_landmarks_ini(ini, "LEAST_SQUARES") == 0.35
    assert hip.load_landmarks_ini(ini, "EMPTY_LS", 1.25) == 1.25
    assert hip.load_landmarks_ini(ini, "NO_SUCH_SECTION", 1.5) == 1.5
    assert hip.load_landmarks_ini(ini, "", 1.75) == 1.75
    v = C.c_double(2.5)
    assert hip.lib().svo_landmarks_load_ini(str(ini).encode(), b"BAD_LS", C.byref(v)) == -2 and v.value == 2.5, "SVO_ERR_ARG"
    with pytest.raises(hip.SvoError): hip.load_landmarks_ini(ini, "BAD_LS")
    with pytest.raises(hip.SvoError): hip.load_landmarks_ini(tmp_path / "missing.ini", "LEAST_SQUARES")
    # the key travels beside svo_params: the record's loader goes on ignoring it
    p = hip.load_params_ini(ini, ["", "", "", "", "LEAST_SQUARES", "", ""])
    assert p.max_iters == 7
