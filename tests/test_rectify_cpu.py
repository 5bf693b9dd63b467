"""Rectification maps from a calibration, the parts that need no GPU: svo_stereo_rectify (a pure host function of libsvo_hip.so, which
loads without a device) against the independent walk of tests/rectify_ref.py and against properties that do not rest on the walk,
and the reach of the calibrations the GPU tests use."""
import ctypes as C
import os
import sys
import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCalibration, StereoRectification

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rectify_ref as RR                                           # noqa: E402

CASES = [("A", RR.calibration_a, 0), ("A", RR.calibration_a, 1), ("B", RR.calibration_b, 0), ("B", RR.calibration_b, 1)]
IDS = ["%s-zd%d" % (n, z) for n, _, z in CASES]
ERR_ARG, ERR_UNSUPPORTED = -2, -3

_walks = {}


def walked(name, fn, zd):
    """one walk per calibration, shared by the tests (read only)"""
    if (name, zd) not in _walks:
        cal = fn(zd)
        _walks[(name, zd)] = (cal,) + RR.walk(cal)
    return _walks[(name, zd)]


def test_status_codes_are_the_headers():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svo_hip.h")).read()
    import re
    assert int(re.search(r"SVO_ERR_ARG\s*=\s*(-?\d+)", hdr).group(1)) == ERR_ARG
    assert int(re.search(r"SVO_ERR_UNSUPPORTED\s*=\s*(-?\d+)", hdr).group(1)) == ERR_UNSUPPORTED


@pytest.mark.parametrize("name,fn,zd", CASES, ids=IDS)
def test_reach_of_the_calibrations(name, fn, zd):
    """The tables of A and B reach past the image (sentinel entries) and onto its -1 / last row and column: the floors are the counts
    the calibrations were chosen for, so that a later change of them cannot quietly lose what the exact GPU comparison exercises."""
    cal, _, sides = walked(name, fn, zd)
    w, h = cal["w"], cal["h"]
    got = [RR.reach(s["fixed"][0], w, h) for s in sides]
    floors = {"A": ((334, 200), (1655, 200)), "B": ((2929, 529), (10600, 529))}[name]
    for side in range(2):
        assert got[side][0] >= floors[side][0] and got[side][1] >= floors[side][1], (name, zd, side, got[side], floors[side])
        assert got[side][1] >= 100
    assert max(g[0] for g in got) >= 0.05 * w * h
    # and every entry that is no sentinel names a first tap in -1 .. size - 1 with 5-bit fractions
    for s in sides:
        xy, frac = s["fixed"]
        ok = xy != 0xFFFFFFFF
        assert ((xy[ok] & 0xFFFF) <= w).all() and ((xy[ok] >> 16) <= h).all() and ((frac & 0xFF) < 32).all() and ((frac >> 8) < 32).all() and (frac[~ok] == 0).all()


def test_identity_rig():
    w, h, f, cx, cy, b = 97, 61, 83.25, 47.3, 29.9, 0.25
    for zd in (0, 1):
        cal = dict(left=(f, f, cx, cy, (0.0,) * 8), right=(f, f, cx, cy, (0.0,) * 8), R=np.eye(3), T=(-b, 0.0, 0.0), w=w, h=h, zero_disparity=zd, alpha=-1.0)
        out = hip.stereo_rectify(RR.to_ctypes(cal))
        assert (out.rotation(0) == np.eye(3)).all() and (out.rotation(1) == np.eye(3)).all()
        K = np.array([f, f, cx, cy])
        assert (np.abs(out.intrinsics(0) - K) <= 1e-12 * K).all() and (np.abs(out.intrinsics(1) - K) <= 1e-12 * K).all()
        assert out.tx == -b and out.cam.baseline == b and (out.cam.ncols, out.cam.nrows) == (w, h)
        i, j = np.mgrid[0:h, 0:w]
        for side in (0, 1):
            xy, frac = RR.fixed(*RR.float_maps(cal["left"], out.rotation(side), out.intrinsics(side), w, h))
            assert (xy == ((j + 1) | ((i + 1) << 16)).astype(np.uint32)).all() and (frac == 0).all()


@pytest.mark.parametrize("name,fn,zd", CASES + [("mild", RR.calibration_mild, 0)], ids=IDS + ["mild-zd0"])
def test_stereo_rectify_against_the_walk(name, fn, zd):
    """R1, R2 within 1e-12 absolute, P1, P2, tx within 1e-12 relative: under a hundred double operations and three libm calls of <= 1
    ulp each give < 1e-14; the margin of 100 x is there because the C library's and the interpreter's sin / cos / acos need not agree."""
    cal, r, _ = walked(name, fn, zd)
    out = hip.stereo_rectify(RR.to_ctypes(cal))
    for side, (Rk, Pk) in enumerate(((r["R1"], r["P1"]), (r["R2"], r["P2"]))):
        assert np.abs(out.rotation(side) - Rk).max() <= 1e-12, (side, np.abs(out.rotation(side) - Rk).max())
        assert (np.abs(out.intrinsics(side) - Pk) <= 1e-12 * np.abs(Pk)).all(), (side, out.intrinsics(side), Pk)
    assert abs(out.tx - r["tx"]) <= 1e-12 * abs(r["tx"])
    c = out.cam
    assert (c.l_fx, c.l_fy, c.l_cx, c.l_cy) == tuple(out.P1) and (c.r_fx, c.r_fy, c.r_cx, c.r_cy) == tuple(out.P2)
    assert c.baseline == -out.tx and (c.ncols, c.nrows) == (cal["w"], cal["h"])


@pytest.mark.parametrize("name,fn,zd", CASES, ids=IDS)
def test_epipolar_property_of_the_c_function(name, fn, zd):
    """Independent of the walk: 50 space points in front of the rig project through P1 R1 X and P2 R2 (R X + T) to rows within 1e-9
    px; R1 and R2 are rotations to 1e-12; the rectified cameras differ by (tx, 0, 0) alone."""
    cal = fn(zd)
    out = hip.stereo_rectify(RR.to_ctypes(cal))
    R1, R2, P1, P2 = out.rotation(0), out.rotation(1), out.intrinsics(0), out.intrinsics(1)
    for Rk in (R1, R2):
        assert np.abs(Rk.T @ Rk - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(Rk) - 1.0) <= 1e-12
    rng = np.random.default_rng(5)
    X = np.stack([rng.uniform(-2, 2, 50), rng.uniform(-1.5, 1.5, 50), rng.uniform(2, 10, 50)])
    Xr = np.asarray(cal["R"]) @ X + np.asarray(cal["T"])[:, None]
    a, b = R1 @ X, R2 @ Xr
    va, vb = P1[1] * a[1] / a[2] + P1[3], P2[1] * b[1] / b[2] + P2[3]
    assert np.abs(va - vb).max() <= 1e-9, np.abs(va - vb).max()
    assert np.abs(a[2] - b[2]).max() <= 1e-12 and np.abs(a[0] - b[0] + out.tx).max() <= 1e-12
    assert P1[0] == P1[1] == P2[0] == P2[1] and P1[3] == P2[3] and (P1[2] == P2[2]) == bool(zd) and out.tx < 0


def _undistort_converged(cam, u, v):
    fx, fy, cx, cy, k = cam
    x0, y0 = (u - cx) / fx, (v - cy) / fy
    x, y = x0.copy(), y0.copy()
    for _ in range(500):
        r2 = x * x + y * y
        icd = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x)
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y
        xn, yn = (x0 - dx) * icd, (y0 - dy) * icd
        done = max(np.abs(xn - x).max(), np.abs(yn - y).max()) < 1e-15
        x, y = xn, yn
        if done:
            break
    assert done, "the undistortion did not converge"
    return x, y


@pytest.mark.parametrize("name,fn,zd", CASES, ids=IDS)
def test_round_trip_of_the_map(name, fn, zd):
    """An output pixel's source, undistorted to convergence and sent through P R, is the pixel again: within 1e-6 px over the central
    half of the image, wherever the source lies inside it.  Uses the C function's R_k and P_k."""
    cal = fn(zd)
    w, h = cal["w"], cal["h"]
    out = hip.stereo_rectify(RR.to_ctypes(cal))
    for side, cam in enumerate((cal["left"], cal["right"])):
        Rk, Pk = out.rotation(side), out.intrinsics(side)
        u, v = RR.source_maps(cam, Rk, Pk, w, h)
        i, j = np.mgrid[0:h, 0:w]
        sel = (j >= w // 4) & (j < w - w // 4) & (i >= h // 4) & (i < h - h // 4) & (u >= 0) & (u <= w - 1) & (v >= 0) & (v <= h - 1)
        assert sel.sum() >= (w // 2) * (h // 2) // 2, (side, int(sel.sum()))
        x, y = _undistort_converged(cam, u[sel], v[sel])
        p = Rk @ np.stack([x, y, np.ones_like(x)])
        jj, ii = Pk[0] * p[0] / p[2] + Pk[2], Pk[1] * p[1] / p[2] + Pk[3]
        err = max(np.abs(jj - j[sel]).max(), np.abs(ii - i[sel]).max())
        assert err <= 1e-6, (side, err)


def _refusal(cal_struct):
    out = StereoRectification()
    C.memset(C.byref(out), 0x5A, C.sizeof(out))
    why = C.create_string_buffer(320)
    rc = hip.lib().svo_stereo_rectify(C.byref(cal_struct), C.byref(out), why, len(why))
    untouched = bytes(out) == b"\x5a" * C.sizeof(out)
    return rc, why.value.decode(), untouched


def _changed(**kw):
    cal = RR.calibration_a(0)
    for k, v in kw.items():
        cal[k] = v
    return RR.to_ctypes(cal)


def _with(fn):
    c = RR.to_ctypes(RR.calibration_a(0))
    fn(c)
    return c


REFUSALS = [
    ("alpha 0", lambda: _changed(alpha=0.0), ERR_UNSUPPORTED),
    ("alpha 1", lambda: _changed(alpha=1.0), ERR_UNSUPPORTED),
    ("vertical rig", lambda: _changed(T=(0.002, -0.12, -0.001)), ERR_UNSUPPORTED),
    ("right camera on the left", lambda: _changed(T=(0.12, 0.002, -0.001)), ERR_ARG),
    ("NaN intrinsic", lambda: _with(lambda c: setattr(c.left, "fx", float("nan"))), ERR_ARG),
    ("infinite distortion", lambda: _with(lambda c: c.right.dist.__setitem__(7, float("inf"))), ERR_ARG),
    ("NaN in R", lambda: _with(lambda c: c.R.__setitem__(4, float("nan"))), ERR_ARG),
    ("infinite T", lambda: _with(lambda c: c.T.__setitem__(2, float("-inf"))), ERR_ARG),
    ("NaN alpha", lambda: _changed(alpha=float("nan")), ERR_ARG),
    ("R not orthonormal", lambda: _with(lambda c: c.R.__setitem__(1, c.R[1] + 1e-5)), ERR_ARG),
    ("w 0", lambda: _changed(w=0), ERR_ARG),
    ("h negative", lambda: _changed(h=-1), ERR_ARG),
]


@pytest.mark.parametrize("what,make,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(what, make, status):
    rc, why, untouched = _refusal(make())
    assert rc == status and why and untouched, (what, rc, why, untouched)
    with pytest.raises(hip.SvoError) as e:
        hip.stereo_rectify(make())
    assert e.value.status == status


def test_an_accepted_calibration_leaves_no_text_and_r_within_1e6_passes():
    c = _with(lambda c: c.R.__setitem__(1, c.R[1] + 5e-7))
    out = StereoRectification()
    why = C.create_string_buffer(b"x" * 64, 320)
    assert hip.lib().svo_stereo_rectify(C.byref(c), C.byref(out), why, len(why)) == 0 and why.value == b""
    assert hip.lib().svo_stereo_rectify(C.byref(c), C.byref(out), None, 0) == 0
