"""The specification of the stereo re-association of the resident KLT front end (include/svo_hip.h: svo_klt_set_stereo).

`row_init` is the rule of the first guesses, in float32 as written.  `KltStereoHostFrontEnd` is the recipe a step in mode 1 is held to:
tests/klt_ref.KltHostFrontEnd with the second svo_lk_track job of every lane (the right list through time) replaced by a
svo_lk_track_rows job on (left[t], right[t], pts = the left job's next_pts, init = row_init).  A lane without a last pair runs that job
too: its left points stand with status 1.  With a camera it also is the recipe of svo_klt_set_prediction(1) (the left guesses of
tests/klt_predict_ref.py; the predicted right guesses are not used); it composes with the recipe of the RANSAC gate by inheritance.
`walk_sequence` is the same step through the two walks (tests/lk_ref.py, tests/lk_row_ref.py) without a device."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import lk_ref as LR                                                                    # noqa: E402
import lk_row_ref as RR_                                                               # noqa: E402
import ransac_tracked_ref as RR                                                        # noqa: E402

F = np.float32


def row_init(old_left, old_right, new_left):
    """(xl' - (xl - xr), yl') in float32 as written: one float32 subtraction for the old disparity, one for the guess"""
    ol = np.ascontiguousarray(old_left, F).reshape(-1, 2); orr = np.ascontiguousarray(old_right, F).reshape(-1, 2)
    nl = np.ascontiguousarray(new_left, F).reshape(-1, 2)
    g = nl.copy()
    with np.errstate(all="ignore"):
        d = (ol[:, 0] - orr[:, 0]).astype(F)
        g[:, 0] = (nl[:, 0] - d).astype(F)
    return g


class KltStereoHostFrontEnd(KR.KltHostFrontEnd):
    """the recipe of a step in mode 1.  cam: None, or the camera stage 5 runs with -- then the left job starts from the predicted guesses
    of svo_klt_set_prediction(1).  inits: {lane: the row job's first guesses} of the last step"""

    def __init__(self, ctx, params, img_h, cam=None):
        super().__init__(ctx, params, img_h)
        self.cam, self.guesses, self.inits = cam, {}, {}

    def step(self, frames, flags=KR.RUN_OPTIMIZE, active=None):
        c = self.ctx
        lanes = list(range(c.n_lanes)) if active is None else sorted(active)
        self.guesses, self.inits = {}, {}
        if self.cam is not None:                   # the record and the table BEFORE the shift call (tests/klt_predict_ref.py)
            import klt_predict_ref as PR
            for l in lanes:
                if self.prev[l] is not None:
                    r, t = c.result(l), self.tables[l]
                    ph, pw = self.prev[l][0].shape
                    self.guesses[l] = PR.predict(t.left, t.right, self.cam, np.array(r.delta, np.float64), r.valid, pw, ph)[:3]
        moved = self.shift(lanes)
        # 3a. the left list through time
        jobs, who = [], []
        for l in lanes:
            if self.prev[l] is not None:
                job = (self.prev[l][0], frames[l][0], self.tables[l].left)
                jobs.append(job + (self.guesses[l][0],) if l in self.guesses else job)
                who.append(l)
        res = c.lk_track(jobs, self.p.lk) if jobs else []
        left = {}
        for l in lanes:
            t = self.tables[l]
            left[l] = res[who.index(l)][:2] if l in who else (t.left, np.ones(len(t), np.uint8))      # no last pair: the points stand
        # 3b. the right partner of every left result, along its row in the new pair
        for l in lanes:
            t = self.tables[l]
            self.inits[l] = row_init(t.left, t.right, left[l][0])
        rows = c.lk_track_rows([(frames[l][0], frames[l][1], left[l][0], self.inits[l]) for l in lanes], self.p.lk)
        for k, l in enumerate(lanes):
            (ol, sl), (or_, sr, _) = left[l], rows[k]
            h, w = frames[l][0].shape
            lists, self.tables[l], _ = KR.select(self.tables[l], ol, or_, sl, sr, self.gate, moved[l], self.H)
            self.put(l, lists, w, h)
            self.prev[l] = (frames[l][0].copy(), frames[l][1].copy())
        if flags & KR.RUN_OPTIMIZE:
            c.run_stages(KR.RUN_OPTIMIZE, lanes if active is not None else None)


class KltStereoRansacHostFrontEnd(RR.KltRansacHostFrontEnd, KltStereoHostFrontEnd):
    """mode 1 under svo_klt_set_ransac: the gate's recipe around the step above (KltRansacHostFrontEnd.step calls the next step of the
    resolution order, which is KltStereoHostFrontEnd's)"""

    def __init__(self, ctx, params, img_h, mode, cam=None):
        KltStereoHostFrontEnd.__init__(self, ctx, params, img_h, cam)
        self.mode, self.rejected = int(mode), []


def walk_sequence(frames, points, lk, gate, cap, H, mode):
    """A one-lane sequence through the walks alone, the first frame without a last pair.  mode 0: both lists through time (lk_ref);
    mode 1: the left list through time, the right one by the row walk.  Per frame: (lists, table after, first guesses of the row job or
    None, (left results, right results) of the trackers)"""
    P = LR.LkParams(**lk)
    t, _ = KR.add_points(KR.Table(), points[0], points[1], cap)
    out, stepped = [], False
    for f, (left_img, right_img) in enumerate(frames):
        n = len(t)
        ones = np.ones(n, np.uint8)
        if f == 0:
            ol, sl, or_, sr = t.left, ones, t.right, ones
        else:
            ol, sl, _, _ = LR.track(frames[f - 1][0], left_img, t.left, params=P)
            if mode == 0:
                or_, sr, _, _ = LR.track(frames[f - 1][1], right_img, t.right, params=P)
        init = None
        if mode == 1:
            init = row_init(t.left, t.right, ol)
            or_, sr, _, _ = RR_.track(left_img, right_img, ol, init, P)
        lists, t2, _ = KR.select(t, ol, or_, sl, sr, gate, KR.lane_shifts(stepped, 0), H)
        out.append((lists, t2, init, (ol, or_)))
        t, stepped = t2, True
    return out
