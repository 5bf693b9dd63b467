"""The definition of the trackers under svo_lk_set_photometric(ctx, 1): tests/lk_ref.py and tests/lk_row_ref.py with an affine brightness
change between template and target estimated and removed per window, per level and per iteration.

The model is J ~ (1 + a) I + b over the win x win window.  a and b are nuisance variables: every iteration minimises
sum (J - I - a I - b - Ix u - Iy v)^2 over (u, v, a, b), and a and b are eliminated in closed form from exact integer window sums, so
nothing photometric is carried from one iteration or level to the next and nothing new is returned.  The device (k_lk_track<.., PHOTO>
and k_lk_track_row<.., PHOTO> in stereo_vo_amd/csrc/k_lk.hip) must equal this walk bit for bit: next_pts as float32 patterns, status, err.
Everything that does not change is imported from lk_ref / lk_row_ref as it is (the pyramid, Scharr, _window, _sample, _finite, Prepared,
LkParams); the walks below are their _track_point with the differences listed here and no others.  Frozen: the tests are written against it.

The sums, over the n = win^2 window pixels, exact integers (I, Ix, Iy the template samples of lk_ref, d = J - I the difference of lk_ref):
  per level      SI = sum I, SII = sum I I, Sx = sum Ix, Sy = sum Iy, SxI = sum Ix I, SyI = sum Iy I, Sxx, Sxy, Syy = sum Ix Ix, Ix Iy, Iy Iy
  per iteration  Sd = sum d, SdI = sum d I, Sdx = sum d Ix, Sdy = sum d Iy
The centred second moments times n, exact integers (the largest, n SII, is below 6.2e13 at win 31; all convert to double exactly):
  Cxx = n Sxx - Sx Sx, Cxy = n Sxy - Sx Sy, Cyy = n Syy - Sy Sy, CxI = n SxI - Sx SI, CyI = n SyI - Sy SI, CII = n SII - SI SI
  Cdx = n Sdx - Sx Sd, Cdy = n Sdy - Sy Sd, CdI = n SdI - SI Sd
The gain eliminated in double, every operator one IEEE operation in this order (X(.) = the exact conversion to double):
  A11 = (X(Cxx) - X(CxI) * X(CxI) / X(CII)) / X(n) * 2^-20       the product first, then the quotient, the difference, / n, * 2^-20
  A12 = (X(Cxy) - X(CxI) * X(CyI) / X(CII)) / X(n) * 2^-20
  A22 = (X(Cyy) - X(CyI) * X(CyI) / X(CII)) / X(n) * 2^-20
  b1  = (X(Cdx) - X(CxI) * X(CdI) / X(CII)) / X(n) * 2^-20
  b2  = (X(Cdy) - X(CyI) * X(CdI) / X(CII)) / X(n) * 2^-20
Everything behind these five values is lk_ref's walk untouched: D = A11 A22 - A12 A12, the minimum-eigenvalue test, D < 2^-23, the
2 x 2 solve, the float32 step, the eps rule, the oscillation rule, the inside rules, the lost-point rules, the NaN rule.

The row walk has one unknown: the level sums SI, SII, Sx, SxI, Sxx, the iteration sums Sd, SdI, Sdx, A11 and b1 as above, the level
test A11 / X(n) < min_eig or A11 < 2^-23 and the step float32(-b1 / A11) of lk_row_ref.

Choices the prose (include/svo_hip.h) leaves open -- the walk decides:
  * CII == 0 (a template flat to 1/32 grey level, the unit of I): the level is skipped exactly as for a small eigenvalue, at level 0 the
    point is lost.  The trace names it "skip_flat" / "flat0".  Nothing is divided by CII then.
  * A template that is an exact ramp cannot be told from an offset: its reduced matrix is singular (or negative by a rounding) and it is
    lost by lk_ref's min_eig / D test evaluated on the REDUCED A11, A12, A22 ("skip_eig" / "eig0"); the row walk tests the reduced A11.
  * The reduced values are not clamped: a reduced A11 that a rounding leaves below zero fails the tests above like any small value.
  * err = float32(double(sum |n d - Sd|) / double(32 n n)): the mean absolute CENTRED difference at the final position, in grey
    levels.  The offset is removed, the gain is not.  Sd is the sum of d at the final position, taken before the absolute pass.  0 for
    a lost point and when the final window is not inside, as in lk_ref.
  * The forward-backward pass is the compensated walk too, with the image roles swapped (the gain it removes is then about 1 / (1 + a)).
  * status, next_pts of lost points, the NaN rule, init and fb_max behave as in lk_ref / lk_row_ref.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_ref as LR                                                                    # noqa: E402
import lk_row_ref as RR                                                                # noqa: E402,F401
from lk_ref import LkParams, Prepared, _window, _sample, _finite                       # noqa: E402,F401

F = np.float32
TWO_M20 = LR.TWO_M20
TWO_M23 = LR.TWO_M23


def _isum(a):
    return int(a.sum())


def _lane_max(a):
    """the largest |partial sum| a lane of the device's 64 holds: window pixel idx (row-major) belongs to lane idx % 64 (for the traces)"""
    v = a.ravel()
    v = np.concatenate([v, np.zeros(-len(v) % 64, np.int64)]).reshape(-1, 64).sum(axis=0)
    return int(np.abs(v).max())


def _reduce(C, Ca, Cb, CII, n):
    """(X(C) - X(Ca) * X(Cb) / X(CII)) / X(n) * 2^-20 in the stated order"""
    return (float(C) - float(Ca) * float(Cb) / float(CII)) / float(n) * TWO_M20


def _centred_err(diff, n):
    Sd = _isum(diff)
    return F(float(_isum(np.abs(n * diff - Sd))) / float(32 * n * n))


def _track_point(pyr_prev, der_prev, pyr_next, pt, init, P, trace, row=False):
    """one point through the levels: (gx, gy, status, err); row: the one-unknown walk of lk_row_ref"""
    win = P.win
    n = win * win
    half = F((win - 1) // 2)
    g0 = init if init is not None else pt
    if not (_finite(pt) and _finite(g0)):
        trace["lost"] = "nan"
        return g0[0], g0[1], 0, F(0.0)
    top = len(pyr_prev) - 1
    sc = F(1.0 / (1 << top))
    gx, gy = F(g0[0] * sc), F(g0[1] * sc)
    err = F(0.0)
    for L in range(top, -1, -1):
        h, w = pyr_prev[L].shape
        sc = F(1.0 / (1 << L))
        lost = None
        # 1. template
        wd = _window(F(F(pt[0] * sc) - half), F(F(pt[1] * sc) - half), w, h, win)
        if wd is None:
            lost = "inside"
        else:
            I = _sample(pyr_prev[L].astype(np.int64), win, wd, 256, 9)
            Ix = _sample(der_prev[L][0], win, wd, 8192, 14)
            SI, SII, Sx, SxI, Sxx = _isum(I), _isum(I * I), _isum(Ix), _isum(Ix * I), _isum(Ix * Ix)
            CII, CxI, Cxx = n * SII - SI * SI, n * SxI - Sx * SI, n * Sxx - Sx * Sx
            if not row:
                Iy = _sample(der_prev[L][1], win, wd, 8192, 14)
                Sy, SyI, Sxy, Syy = _isum(Iy), _isum(Iy * I), _isum(Ix * Iy), _isum(Iy * Iy)
                CyI, Cxy, Cyy = n * SyI - Sy * SI, n * Sxy - Sx * Sy, n * Syy - Sy * Sy
            trace.setdefault("sums", []).append((L, SI, SII, CII))
            trace["lane_II"] = max(trace.get("lane_II", 0), _lane_max(I * I))
            # 2. the reduced gradient matrix
            if CII == 0:
                lost = "flat"
            elif row:
                A11 = _reduce(Cxx, CxI, CxI, CII, n)
                if A11 / float(n) < float(P.min_eig) or A11 < TWO_M23:
                    lost = "eig"
            else:
                A11 = _reduce(Cxx, CxI, CxI, CII, n)
                A12 = _reduce(Cxy, CxI, CyI, CII, n)
                A22 = _reduce(Cyy, CyI, CyI, CII, n)
                D = A11 * A22 - A12 * A12
                min_eig = (A22 + A11 - math.sqrt((A11 - A22) * (A11 - A22) + 4.0 * A12 * A12)) / (2.0 * win * win)
                if min_eig < float(P.min_eig) or D < TWO_M23:
                    lost = "eig"
        if lost:
            trace["levels"].append((L, "skip_" + lost, 0, None))
            if L == 0:
                trace["lost"] = lost + "0"
                return gx, gy, 0, F(0.0)
            gx, gy = F(gx * F(2.0)), F(gy * F(2.0))
            continue
        # 3. iterations
        nxt = pyr_next[L].astype(np.int64)
        stop, iters = "max", 0
        pdx, pdy = F(0.0), F(0.0)
        for j in range(P.max_iters):
            wj = _window(F(gx - half), F(gy - half), w, h, win)
            if wj is None:
                stop = "outside"
                break
            iters = j + 1
            Jw = _sample(nxt, win, wj, 256, 9)
            diff = Jw - I
            Sd, SdI, Sdx = _isum(diff), _isum(diff * I), _isum(diff * Ix)
            CdI, Cdx = n * SdI - SI * Sd, n * Sdx - Sx * Sd
            trace["max_J"] = max(trace.get("max_J", 0), int(Jw.max()))
            trace["lane_dI"] = max(trace.get("lane_dI", 0), _lane_max(diff * I))
            b1 = _reduce(Cdx, CxI, CdI, CII, n)
            if row:
                dx = F(-b1 / A11)
                gx = F(gx + dx)
                if float(dx) * float(dx) <= float(P.eps) * float(P.eps):
                    stop = "eps"
                    break
                if j > 0 and abs(float(F(dx + pdx))) < 0.01:
                    gx = F(gx - F(F(0.5) * dx))
                    stop = "osc"
                    break
                pdx = dx
                continue
            Sdy = _isum(diff * Iy)
            Cdy = n * Sdy - Sy * Sd
            b2 = _reduce(Cdy, CyI, CdI, CII, n)
            dx = F((A12 * b2 - A22 * b1) / D)
            dy = F((A12 * b1 - A11 * b2) / D)
            gx, gy = F(gx + dx), F(gy + dy)
            if float(dx) * float(dx) + float(dy) * float(dy) <= float(P.eps) * float(P.eps):
                stop = "eps"
                break
            if j > 0 and abs(float(F(dx + pdx))) < 0.01 and abs(float(F(dy + pdy))) < 0.01:
                gx, gy = F(gx - F(F(0.5) * dx)), F(gy - F(F(0.5) * dy))
                stop = "osc"
                break
            pdx, pdy = dx, dy
        trace["levels"].append((L, "run", iters, stop))
        if L == 0:
            if stop == "outside":
                trace["lost"] = "outside0"
                return gx, gy, 0, F(0.0)
            # 4. error: the mean absolute centred difference
            wj = _window(F(gx - half), F(gy - half), w, h, win)
            if wj is not None:
                err = _centred_err(_sample(nxt, win, wj, 256, 9) - I, n)
            else:
                trace["err_outside"] = True
            return gx, gy, 1, err
        gx, gy = F(gx * F(2.0)), F(gy * F(2.0))
    raise AssertionError("unreachable")


def _track(prev, nxt, pts, init, params, prepared, row):
    P = params or LkParams()
    P.check()
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
    init = None if init is None else np.ascontiguousarray(init, np.float32).reshape(-1, 2)
    n = len(pts)
    pre = prepared or Prepared(prev, nxt, P)
    out, status, err = np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    traces = []
    for i in range(n):
        tr = {"levels": [], "lost": None}
        gx, gy, st, e = _track_point(pre.pyr[0], pre.der[0], pre.pyr[1], pts[i], None if init is None else init[i], P, tr, row)
        out[i, 0], out[i, 1], status[i], err[i] = gx, gy, st, e
        if st and float(P.fb_max) > 0.0:
            tb = {"levels": [], "lost": None}
            bx, by, sb, _ = _track_point(pre.pyr[1], pre.der[1], pre.pyr[0], out[i].copy(), None, P, tb, row)
            tr["back"] = tb
            if not sb:
                status[i] = 0; tr["lost"] = "fb_lost"
            else:
                ddx, ddy = float(bx) - float(pts[i, 0]), 0.0 if row else float(by) - float(pts[i, 1])
                if ddx * ddx + ddy * ddy > float(P.fb_max) * float(P.fb_max):
                    status[i] = 0; tr["lost"] = "fb_dist"
        traces.append(tr)
    return out, status, err, traces


def track(prev, nxt, pts, init=None, params=None, prepared=None):
    """svo_lk_track in mode 1: (next_pts [n, 2] float32, status [n] uint8, err [n] float32, traces) of one job"""
    return _track(prev, nxt, pts, init, params, prepared, False)


def track_rows(prev, nxt, pts, init=None, params=None, prepared=None):
    """svo_lk_track_rows in mode 1"""
    return _track(prev, nxt, pts, init, params, prepared, True)
