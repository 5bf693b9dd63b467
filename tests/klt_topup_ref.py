"""The specification of the resident top-up of the KLT front end (include/svo_hip.h: svo_klt_topup).

Two things live here.  `KltTopupRecipe` is the host recipe of the contract written against the public Python calls only --
Context.klt_tracks, Context.gftt_detect, Context.lk_track, Context.klt_add_points, four synchronising calls per lane -- on a context
whose steps are svo_klt_step's: the resident top-up must leave, byte for byte, what this recipe leaves.  The GPU tests run it on a
second context.  `walk` is the same recipe in numpy over tests/gftt_ref.py, tests/lk_ref.py and tests/klt_ref.py, for the scene tests
that need no device.

The reasons of svo_klt_topup_info: 0 topped up, 1 candidate overflow, 2 not below the threshold, 3 no last pair, 4 not in the mask."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402

F = np.float32
OK, OVERFLOW, ENOUGH, NO_PAIR, NOT_ASKED = range(5)


class TopupParams:
    """svo_klt_topup_params without the detector's part: the threshold, the goal and the first guess's disparity"""
    def __init__(self, cap, below=None, target=None, init_disp=0.0):
        self.below = (cap + 1) // 2 if below is None else int(below)
        self.target = cap if target is None else int(target)
        self.init_disp = F(init_disp)


def want_of(n, cap, tp):
    """None when the lane is not topped up, else the room the detector gets"""
    if n >= tp.below:
        return None
    return max(min(tp.target, cap) - n, 0)


def first_guess(corners, init_disp):
    init = np.ascontiguousarray(corners, F).reshape(-1, 2).copy()
    init[:, 0] = (init[:, 0] - F(init_disp)).astype(F)
    return init


def gate_pass(left, right, status, gate):
    """the gate of svo_klt_step item 4 on (corner, partner) pairs: a bool per pair"""
    L = np.ascontiguousarray(left, F).reshape(-1, 2); R = np.ascontiguousarray(right, F).reshape(-1, 2)
    st = np.ascontiguousarray(status, np.uint8)
    keep = np.zeros(len(L), bool)
    for s in range(len(L)):
        xl, yl, xr, yr = L[s, 0], L[s, 1], R[s, 0], R[s, 1]
        if st[s] != 1 or not (np.isfinite(xl) and np.isfinite(yl) and np.isfinite(xr) and np.isfinite(yr)):
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            dy, disp = F(abs(F(yl - yr))), F(xl - xr)
        keep[s] = bool(dy <= gate.max_dy and disp >= gate.min_disp and disp <= gate.max_disp)
    return keep


def append(table, left, right, status, gate, cap):
    """items 4 and 5 (svo_debug_klt_topup_append): (new table, appended, the bool per pair)"""
    keep = gate_pass(left, right, status, gate)
    L = np.ascontiguousarray(left, F).reshape(-1, 2); R = np.ascontiguousarray(right, F).reshape(-1, 2)
    t, m = KR.add_points(table, L[keep], R[keep], cap)
    return t, m, keep


def walk(table, left_img, right_img, cap, gate, tp, gftt_params, lk_params, cand_cap=1 << 30):
    """One lane that has a last pair and is in the mask, in numpy.  -> (new table, info (corners, candidates, appended, reason),
    details: corners, partners, status, the bool per corner)"""
    import gftt_ref as GR
    import lk_ref as LR
    n = len(table)
    want = want_of(n, cap, tp)
    if want is None:
        return table, (0, 0, 0, ENOUGH), None
    corners, _, (nc, n_cand, status), _ = GR.detect(left_img, table.left, want, gftt_params, cand_cap)
    if status:
        return table, (0, n_cand, 0, OVERFLOW), None
    out, st, _, _ = LR.track(left_img, right_img, corners, first_guess(corners, tp.init_disp), lk_params)
    t, m, keep = append(table, corners, out, st, gate, cap)
    return t, (nc, n_cand, m, OK), dict(corners=corners, partners=out, status=st, keep=keep)


class KltTopupRecipe:
    """The recipe on a context whose front end is enabled with `kp` (an abi.KltParams): four public calls per lane.  The caller tells it
    the image pairs the context's steps were given (note_step) and the resets (note_reset): the recipe's images are the host's."""

    def __init__(self, ctx, kp, tp, gftt_params):
        self.ctx, self.kp, self.tp, self.gp = ctx, kp, tp, gftt_params
        self.gate = KR.Gate(kp.max_dy, kp.min_disp, kp.max_disp, kp.lk.win)
        self.pair = [None] * ctx.n_lanes
        self.info = [(0, 0, 0, NOT_ASKED)] * ctx.n_lanes

    def note_step(self, frames, active=None):
        for l in (range(self.ctx.n_lanes) if active is None else active):
            self.pair[l] = (np.ascontiguousarray(frames[l][0]).copy(), np.ascontiguousarray(frames[l][1]).copy())

    def note_reset(self, lanes=None):
        for l in (range(self.ctx.n_lanes) if lanes is None else lanes):
            self.pair[l] = None

    def topup(self, active=None):
        c = self.ctx
        lanes = list(range(c.n_lanes)) if active is None else sorted(active)
        for l in range(c.n_lanes):
            if l not in lanes:
                self.info[l] = (0, 0, 0, NOT_ASKED)
            elif self.pair[l] is None:
                self.info[l] = (0, 0, 0, NO_PAIR)
            else:
                self.info[l] = self._lane(l)

    def _lane(self, l):
        c = self.ctx
        left, _, _, _ = c.klt_tracks(l)                                               # 1
        want = want_of(len(left), self.kp.cap, self.tp)
        if want is None:
            return (0, 0, 0, ENOUGH)
        iml, imr = self.pair[l]
        (corners, _, n_cand, status), = c.gftt_detect([(iml, left, want)], self.gp)     # 2
        if status:
            return (0, n_cand, 0, OVERFLOW)
        (out, st, _), = c.lk_track([(iml, imr, corners, first_guess(corners, self.tp.init_disp))], self.kp.lk)   # 3
        keep = gate_pass(corners, out, st, self.gate)                                 # 4
        m = c.klt_add_points(l, corners[keep], out[keep])                             # 5
        return (len(corners), n_cand, m, OK)
