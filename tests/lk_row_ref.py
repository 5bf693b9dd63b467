"""The definition of svo_lk_track_rows: a literal numpy walk of the row tracker, the one-dimensional form of tests/lk_ref.py.

A point's template is taken from `prev` at pt, and its partner is searched in `next` ALONG THE ROW of the guess: one unknown (x), the
gradient Ix alone, no 2 x 2 solve.  For a rectified stereo pair prev is the left image and next the right one.  The device
(stereo_vo_amd/csrc/k_lk_row.hip) must equal this walk bit for bit: next_pts as float32 patterns, status, err.  Everything the two
trackers share is imported from lk_ref as it is (LkParams, build_pyramid, scharr, _window, _sample, _finite, Prepared); the walk below is
lk_ref._track_point with the differences listed here and no others.  Frozen: the tests are written against it.

The row rule:
  * The guess g0 is init if given, else pt.  gy is NEVER updated: it is scaled to the top level (gy = float32(g0.y * 2^-top)) and doubled
    from level to level exactly as gx is, and the returned point is (gx, gy as carried to level 0).
  * The template is taken from prev at pt, I and Ix only.  A11 = double(sum Ix^2) * 2^-20.
  * A level is skipped (at level 0 the point is lost) when the template window is not inside, when A11 / double(win * win) <
    double(min_eig), or when A11 < 2^-23.
  * An iteration: b1 = double(sum diff * Ix) * 2^-20, dx = float32(-b1 / A11), gx += dx; stop when double(dx)^2 <= double(eps)^2; then
    the oscillation rule on dx alone (j > 0 and |float32(dx + pdx)| < 0.01: gx -= 0.5 * dx, stop); then pdx = dx.
  * The inside rule of the next image's window, the "outside" loss at level 0 and err at the final position are lk_ref's.

Choices the prose leaves open -- the walk decides:
  * The trace names of lk_ref are kept: a level skipped for its gradient is "skip_eig" (lost at level 0: "eig0") although the quantity
    is A11 / win^2, not an eigenvalue; a horizontal edge (Ix = 0 everywhere) is lost by that rule.
  * -b1 / A11 is one double negation (exact) and one double division, rounded once to float32.
  * 0.5 * dx is a float32 product (exact) and the subtraction one float32 operation, as in lk_ref.
  * |float32(dx + pdx)| is compared with the double constant 0.01, as in lk_ref.
  * The row of the search is the guess's, not the template's: with init.y != pt.y the template comes from row pt.y of prev and the
    search runs on row init.y of next; the returned y has init.y's bit pattern whenever the scaling by 2^-top and back is exact (it is
    unless g0.y * 2^-top is subnormal).
  * A lost point keeps the guess it had when it was lost; a NaN or infinite coordinate in pt or init copies the guess through and
    reads nothing, as in lk_ref.
  * fb_max > 0: a point the forward pass tracked is followed back from next to prev by the same rule, starting at the forward result
    with no init (so y is held at the forward result's y, and the template is taken from next there).  It is lost when the way back
    loses it or when (double(back.x) - double(pt.x))^2 > double(fb_max)^2: the distance is along x alone.  Only status changes.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_ref as LR                                                                    # noqa: E402
from lk_ref import LkParams, Prepared, build_pyramid, scharr, _window, _sample, _finite      # noqa: E402,F401

F = np.float32
TWO_M20 = LR.TWO_M20
TWO_M23 = LR.TWO_M23


def _track_point(pyr_prev, der_prev, pyr_next, pt, init, P, trace):
    """one point through the levels: (gx, gy, status, err)"""
    win = P.win
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
        A11 = 0.0
        if wd is None:
            lost = "inside"
        else:
            I = _sample(pyr_prev[L].astype(np.int64), win, wd, 256, 9)
            Ix = _sample(der_prev[L][0], win, wd, 8192, 14)
            # 2. the gradient sum
            A11 = float(int((Ix * Ix).sum())) * TWO_M20
            if A11 / float(win * win) < float(P.min_eig) or A11 < TWO_M23:
                lost = "eig"
        if lost:
            trace["levels"].append((L, "skip_" + lost, 0, None))
            if L == 0:
                trace["lost"] = lost + "0"
                return gx, gy, 0, F(0.0)
            gx, gy = F(gx * F(2.0)), F(gy * F(2.0))
            continue
        # 3. iterations along the row
        nxt = pyr_next[L].astype(np.int64)
        stop, iters = "max", 0
        pdx = F(0.0)
        for j in range(P.max_iters):
            wj = _window(F(gx - half), F(gy - half), w, h, win)
            if wj is None:
                stop = "outside"
                break
            iters = j + 1
            diff = _sample(nxt, win, wj, 256, 9) - I
            b1 = float(int((diff * Ix).sum())) * TWO_M20
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
        trace["levels"].append((L, "run", iters, stop))
        if L == 0:
            if stop == "outside":
                trace["lost"] = "outside0"
                return gx, gy, 0, F(0.0)
            # 4. error
            wj = _window(F(gx - half), F(gy - half), w, h, win)
            if wj is not None:
                s = int(np.abs(_sample(nxt, win, wj, 256, 9) - I).sum())
                err = F(float(s) / float(32 * win * win))
            else:
                trace["err_outside"] = True
            return gx, gy, 1, err
        gx, gy = F(gx * F(2.0)), F(gy * F(2.0))
    raise AssertionError("unreachable")


def track(prev, nxt, pts, init=None, params=None, prepared=None):
    """(next_pts [n, 2] float32, status [n] uint8, err [n] float32, traces) of one job; prepared: a Prepared to share"""
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
        gx, gy, st, e = _track_point(pre.pyr[0], pre.der[0], pre.pyr[1], pts[i], None if init is None else init[i], P, tr)
        out[i, 0], out[i, 1], status[i], err[i] = gx, gy, st, e
        if st and float(P.fb_max) > 0.0:
            tb = {"levels": [], "lost": None}
            bx, _, sb, _ = _track_point(pre.pyr[1], pre.der[1], pre.pyr[0], out[i].copy(), None, P, tb)
            tr["back"] = tb
            if not sb:
                status[i] = 0; tr["lost"] = "fb_lost"
            else:
                ddx = float(bx) - float(pts[i, 0])
                if ddx * ddx > float(P.fb_max) * float(P.fb_max):
                    status[i] = 0; tr["lost"] = "fb_dist"
        traces.append(tr)
    return out, status, err, traces
