"""The specification of the pose prediction of the resident KLT front end (include/svo_hip.h: svo_klt_set_prediction).

`predict` is the rule as a literal walk: items 1 to 5 in numpy float64 and float32, one operation per operator, with the move and the
projection through oracle.project (svo_oracle_project, the bit-exact restatement of k_project_points).  `KltPredictHostFrontEnd` is
the recipe a step in mode 1 is held to: tests/klt_ref.KltHostFrontEnd with the lane's result record and table read before the shift
call, the guesses computed here, and passed as `init` of both svo_lk_track jobs of the lane.  It composes with the recipe of the RANSAC
gate (tests/ransac_tracked_ref.py) by inheritance: see KltPredictRansacHostFrontEnd."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import ransac_tracked_ref as RR                                                        # noqa: E402

F = np.float32
# why a slot is not predicted: the first failing condition of item 4, in the order the rule lists them
REASONS = ("lane", "disparity", "depth", "nonfinite", "outside_left", "outside_right")


def lane_predicts(valid, delta6):
    """item 1: the record is valid and its six delta values are finite"""
    return int(valid) != 0 and bool(np.all(np.isfinite(np.asarray(delta6, np.float64))))


def triangulate(left, right, cam):
    """item 2: (disparity [n], X [n, 3]) in float64, the expressions of k_project_points with ul = xl, vl = yl, ur = xr"""
    L = np.ascontiguousarray(left, F).reshape(-1, 2); R = np.ascontiguousarray(right, F).reshape(-1, 2)
    ul, vl, ur = L[:, 0].astype(np.float64), L[:, 1].astype(np.float64), R[:, 0].astype(np.float64)
    cul, cvl, fl, cur, fr = cam.l_cx, cam.l_cy, cam.l_fx, cam.r_cx, cam.r_fx
    with np.errstate(all="ignore"):
        disparity = fl * (cur - ur) + fr * (ul - cul)
        b_d = cam.baseline / disparity
        X = np.stack([b_d * fr * (ul - cul), b_d * fr * (vl - cvl), b_d * fl * fr], axis=1)
    return disparity, X


def rotation_row3(delta6):
    """The third row of the rotation svo_oracle_project builds from delta6: oracle.project returns pixels, not the moved depth Z1c
    that item 4 compares, so the walk restates these three entries of the oracle's rodrigues_with_derivs (S5:55-123), operation for
    operation, with the C library's sqrt, sin and cos.  Below the small-angle threshold the row is (-w2, w1, 1) exactly."""
    import math
    w1, w2, w3 = (float(v) for v in np.asarray(delta6, np.float64)[:3])
    w12, w22 = w1 * w1, w2 * w2
    tt = math.sqrt(w1 * w1 + w2 * w2 + w3 * w3)
    if tt < 1e-5:
        return np.array([-w2, w1, 1.0])
    tt2 = tt * tt
    u = (math.cos(tt) - 1) / tt2
    v = math.sin(tt) / tt
    return np.array([-w2 * v - w1 * w3 * u, w1 * v - w2 * w3 * u, (w12 + w22) * u + 1])


def predict(left, right, cam, delta6, valid, w, h, tracks=True):
    """The rule for one lane's live slots.  left / right: the slots' points, [n, 2] float32; cam: an abi.StereoCamera; delta6, valid: the
    lane's record; w, h: the level-0 size of the lane's last pair; tracks: the lane is in the step's mask and has a last pair.
    Returns (left guesses [n, 2] float32, right guesses [n, 2] float32, used [n] uint8, reasons): reasons[s] is None for a predicted
    slot, else the first condition of item 4 that failed."""
    from oracle import oracle as O
    L = np.ascontiguousarray(left, F).reshape(-1, 2); R = np.ascontiguousarray(right, F).reshape(-1, 2)
    n = len(L)
    gl, gr, used = L.copy(), R.copy(), np.zeros(n, np.uint8)
    if not (tracks and lane_predicts(valid, delta6)) or n == 0:
        return gl, gr, used, ["lane"] * n
    d = np.ascontiguousarray(delta6, np.float64)
    disparity, X = triangulate(L, R, cam)
    with np.errstate(all="ignore"):
        pix, _ = O.project(X, cam, d)                                  # item 3: [n, 4] float32, uL vL uR vR
        r3 = rotation_row3(d)
        z1c = r3[0] * X[:, 0] + r3[1] * X[:, 1] + r3[2] * X[:, 2] + d[5]
    x_max, y_max = F(w - 1), F(h - 1)
    reasons = []
    for s in range(n):
        p = pix[s]
        why = None
        if not disparity[s] > 0.0:
            why = "disparity"
        elif not z1c[s] > 0.0:
            why = "depth"
        elif not np.all(np.isfinite(p)):
            why = "nonfinite"
        elif not (p[0] >= F(0) and p[0] <= x_max and p[1] >= F(0) and p[1] <= y_max):
            why = "outside_left"
        elif not (p[2] >= F(0) and p[2] <= x_max and p[3] >= F(0) and p[3] <= y_max):
            why = "outside_right"
        reasons.append(why)
        if why is None:
            gl[s], gr[s], used[s] = p[0:2], p[2:4], 1
    return gl, gr, used, reasons


def predict_slots(left, right, cap, *args, **kw):
    """the whole block of `cap` slots as the device writes it: item 5, NaN guesses and used = 0 behind the live count"""
    gl, gr, used, _ = predict(left, right, *args, **kw)
    n = len(gl)
    pad = np.full((cap - n, 2), np.nan, F)
    return np.concatenate([gl, pad]), np.concatenate([gr, pad]), np.concatenate([used, np.zeros(cap - n, np.uint8)])


class KltPredictHostFrontEnd(KR.KltHostFrontEnd):
    """the recipe of a step in mode 1.  cam: the camera stage 5 of the context runs with.  guesses: {lane: (left, right, used)} of the
    last step, for the lanes that tracked"""

    def __init__(self, ctx, params, img_h, cam, *a, **kw):
        super().__init__(ctx, params, img_h, *a, **kw)
        self.cam, self.guesses = cam, {}

    def step(self, frames, flags=KR.RUN_OPTIMIZE, active=None):
        c = self.ctx
        lanes = list(range(c.n_lanes)) if active is None else sorted(active)
        # svo_get_result and the table (svo_klt_get_tracks on a resident front end) BEFORE the shift call, which starts the record afresh
        self.guesses = {}
        for l in lanes:
            if self.prev[l] is not None:
                r, t = c.result(l), self.tables[l]
                ph, pw = self.prev[l][0].shape
                self.guesses[l] = predict(t.left, t.right, self.cam, np.array(r.delta, np.float64), r.valid, pw, ph)[:3]
        moved = self.shift(lanes)
        jobs, who = [], []
        for l in lanes:
            if self.prev[l] is not None:
                t = self.tables[l]
                gl, gr, _ = self.guesses[l]
                jobs += [(self.prev[l][0], frames[l][0], t.left, gl), (self.prev[l][1], frames[l][1], t.right, gr)]
                who.append(l)
        res = c.lk_track(jobs, self.p.lk) if jobs else []
        for l in lanes:
            t = self.tables[l]
            if l in who:
                j = 2 * who.index(l)
                (ol, sl, _), (or_, sr, _) = res[j], res[j + 1]
            else:                                  # no last pair: the points stand as they are
                ol, or_, sl, sr = t.left, t.right, np.ones(len(t), np.uint8), np.ones(len(t), np.uint8)
            h, w = frames[l][0].shape
            lists, self.tables[l], _ = KR.select(t, ol, or_, sl, sr, self.gate, moved[l], self.H)
            self.put(l, lists, w, h)
            self.prev[l] = (frames[l][0].copy(), frames[l][1].copy())
        if flags & KR.RUN_OPTIMIZE:
            c.run_stages(KR.RUN_OPTIMIZE, lanes if active is not None else None)


class KltPredictRansacHostFrontEnd(RR.KltRansacHostFrontEnd, KltPredictHostFrontEnd):
    """mode 1 under svo_klt_set_ransac: the gate's recipe around the predicted step (KltRansacHostFrontEnd.step calls the next step of
    the resolution order, which is KltPredictHostFrontEnd's)"""

    def __init__(self, ctx, params, img_h, cam, mode):
        KltPredictHostFrontEnd.__init__(self, ctx, params, img_h, cam)
        self.mode, self.rejected = int(mode), []
