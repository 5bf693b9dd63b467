"""The specification of svo_ransac_tracked (include/svo_hip.h): stage 4's RANSAC on the tracked pairs a lane holds.

`walk_octave` is the literal walk of one lane-octave: the lists in, the filtered pairs and the eight counters out, through
oracle.ransac_fundamental (cv::findFundamentalMat(FM_RANSAC, 1.0, 0.99) as the reference calls it).  `walk_lane` sums the counters over
a lane's octaves as svo_result.track_stats does.  `KltRansacHostFrontEnd` is the recipe the resident gate (svo_klt_set_ransac) is held
to: tests/klt_ref.KltHostFrontEnd with the public svo_ransac_tracked call between its puts and stage 5, and for mode 2 the removal of
the tracks whose pair was rejected from the host's table."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402

F = np.float32
TS_THRESHOLD, TS_COLLISION, TS_INLIERS_L, TS_INLIERS_R, TS_HYP_L, TS_HYP_R, TS_BOTH_MASKS, TS_TRACKED = range(8)
LMEDS_MAX_N = 14


class Lists:
    """one slot of one lane-octave: both keypoint lists and the pairings"""
    def __init__(self, kps_l, kps_r, matches):
        self.kps = [np.ascontiguousarray(kps_l, KR.keypoint_dtype), np.ascontiguousarray(kps_r, KR.keypoint_dtype)]
        self.matches = np.ascontiguousarray(matches, KR.dmatch_dtype)


def path_of(n):
    """which path cv::findFundamentalMat takes for n point pairs"""
    return "none" if n < 7 else "direct7" if n == 7 else "lmeds" if n <= LMEDS_MAX_N else "ransac"


def candidates(prev, cur, tracked):
    """the positions in `tracked` of the pairs with valid indices: first inside the previous pairings, second inside the current ones,
    and the four keypoint indices of the two pairings inside their lists"""
    out = []
    for i, (f, s) in enumerate(zip(tracked["first"], tracked["second"])):
        if not (0 <= f < len(prev.matches) and 0 <= s < len(cur.matches)):
            continue
        mp, mc = prev.matches[f], cur.matches[s]
        if 0 <= mp["queryIdx"] < len(prev.kps[0]) and 0 <= mp["trainIdx"] < len(prev.kps[1]) and \
           0 <= mc["queryIdx"] < len(cur.kps[0]) and 0 <= mc["trainIdx"] < len(cur.kps[1]):
            out.append(i)
    return np.array(out, np.int64)


def point_pairs(prev, cur, tracked, cand):
    """(l1, l2, r1, r2): previous and current left points, previous and current right points of the candidates, float32 [n, 2]"""
    t = tracked[cand]
    mp, mc = prev.matches[t["first"]], cur.matches[t["second"]]
    xy = lambda k, idx: np.stack([k["x"][idx], k["y"][idx]], axis=1).astype(F).reshape(-1, 2)
    return xy(prev.kps[0], mp["queryIdx"]), xy(cur.kps[0], mc["queryIdx"]), xy(prev.kps[1], mp["trainIdx"]), xy(cur.kps[1], mc["trainIdx"])


class OctaveWalk:
    pass


def walk_octave(prev, cur, tracked):
    """One lane-octave.  Returns an OctaveWalk: tracked (the survivors, in order), stats (8 ints), cand (positions of the candidates),
    keep (bool per candidate), path, use_f, inliers (per side), masks (per side)."""
    from oracle import oracle as O
    tracked = np.ascontiguousarray(tracked, KR.index_pair_dtype)
    w = OctaveWalk()
    w.cand = candidates(prev, cur, tracked)
    n = len(w.cand)
    l1, l2, r1, r2 = point_pairs(prev, cur, tracked, w.cand)
    cnt_l, mask_l, _, _, hyp_l = O.ransac_fundamental(l1, l2)
    cnt_r, mask_r, _, _, hyp_r = O.ransac_fundamental(r1, r2)
    w.path, w.inliers, w.masks = path_of(n), (int(cnt_l), int(cnt_r)), (mask_l.astype(bool), mask_r.astype(bool))
    w.use_f = cnt_l >= 8 and cnt_r >= 8
    w.keep = (w.masks[0] & w.masks[1]) if w.use_f else np.ones(n, bool)
    w.tracked = tracked[w.cand[w.keep]].copy()
    t = len(w.tracked)
    w.stats = np.array([len(tracked), n, cnt_l, cnt_r, hyp_l, hyp_r, t, t], np.int32)
    return w


def walk_lane(octaves):
    """octaves: [(prev Lists, cur Lists, tracked)] per octave.  Returns ([OctaveWalk], the lane's eight track_stats)"""
    ws = [walk_octave(*o) for o in octaves]
    return ws, np.sum([w.stats for w in ws], axis=0, dtype=np.int64).astype(np.int32) if ws else np.zeros(8, np.int32)


def prune(table, before, after):
    """mode 2 on the host's table after a selection (slot j is list index j): every slot that had a tracked pair (`before`) and is the
    second of none of `after` leaves; the others keep their order, their idx (the lists are unchanged) and everything else"""
    lost = np.setdiff1d(before["second"], after["second"])
    keep = ~np.isin(np.arange(len(table)), lost)
    t = table.copy()
    for k in ("left", "right", "ids", "age", "idx", "pidx"):
        setattr(t, k, getattr(table, k)[keep].copy())
    return t, lost


class KltRansacHostFrontEnd(KR.KltHostFrontEnd):
    """the recipe of the gate: the puts of KltHostFrontEnd, svo_ransac_tracked on the step's lanes, for mode 2 svo_get_tracked and the
    removal from the host table, then stage 5.  rejected: [(lane, the list indices that left)] of the last step / selection."""

    def __init__(self, ctx, params, img_h, mode):
        super().__init__(ctx, params, img_h)
        self.mode, self.rejected = int(mode), []

    def _gate(self, lanes, before):
        c = self.ctx
        self.rejected = []
        if self.mode == 0:
            return
        c.ransac_tracked(lanes)
        for l in lanes:
            after = c.tracked(l)
            lost = np.setdiff1d(before[l]["second"], after["second"])
            if self.mode == 2:
                self.tables[l], lost = prune(self.tables[l], before[l], after)
            self.rejected.append((l, lost))

    def step(self, frames, flags=KR.RUN_OPTIMIZE, active=None):
        c = self.ctx
        lanes = list(range(c.n_lanes)) if active is None else sorted(active)
        super().step(frames, flags=0, active=lanes)
        self._gate(lanes, {l: c.tracked(l) for l in lanes})
        if flags & KR.RUN_OPTIMIZE:
            c.run_stages(KR.RUN_OPTIMIZE, lanes if active is not None else None)

    def debug_select(self, lane, left_xy, right_xy, status_l, status_r, img_w, img_h):
        out = super().debug_select(lane, left_xy, right_xy, status_l, status_r, img_w, img_h)
        self._gate([lane], {lane: self.ctx.tracked(lane)})
        return out
