"""Inputs for svo_ransac_tracked: stereo projections of 3-D points under a known motion, with planted outliers.

A case is the lists of ONE lane-octave -- previous and current keypoints of both sides, the pairings of both slots, the tracked pairs --
with the positions of the planted outliers in the tracked list and what the case means to reach (`rule`).  The keypoint lists, the
pairings and the tracked pairs are each in an order of their own, so that every level of indirection is exercised.  The walk of
tests/ransac_tracked_ref.py turns a case into its expected output; tests/test_ransac_tracked_scenes_cpu.py pins what each case reaches
on the oracle, tests/test_gpu_ransac_tracked.py puts the cases into contexts."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import ransac_tracked_ref as RR                                                        # noqa: E402

F = np.float32
W, H = 160, 120
FOCAL, CX, CY, BASELINE = 140.0, 80.0, 60.0, 0.12
MAX_KPS = 1024
COUNTS = (0, 6, 7, 8, 14, 15, 64, 65, 256, 257, 1024)
PLANTED = ((14, 2), (40, 8), (64, 10), (257, 45), (1024, 160))           # (pairs, planted outliers): 15-20 % from 40 pairs on
HARD = (("heavy_64_30", 64, 30, 0.0), ("heavy_300_150", 300, 150, 0.0), ("noisy_65", 65, 0, 0.25), ("noisy_257_45", 257, 45, 0.25))    # (name, pairs, planted, pixel noise)


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])


MOTION_R, MOTION_T = _rot(0.02, -0.015, 0.01), np.array([0.06, -0.03, 0.15])


def project(X):
    """(left [n, 2], right [n, 2]) float32 pixels of camera-frame points"""
    u = FOCAL * X[:, 0] / X[:, 2] + CX
    v = FOCAL * X[:, 1] / X[:, 2] + CY
    return np.stack([u, v], 1).astype(F), np.stack([u - FOCAL * BASELINE / X[:, 2], v], 1).astype(F)


def keypoints(xy):
    k = np.zeros(len(xy), KR.keypoint_dtype)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"] = F(11), F(-1)
    k["class_id"] = np.arange(len(xy))
    return k


def pairings(ql, tr):
    m = np.zeros(len(ql), KR.dmatch_dtype)
    m["queryIdx"], m["trainIdx"] = ql, tr
    return m


class Case:
    def __init__(self, name, rule, prev, cur, tracked, planted=()):
        self.name, self.rule, self.prev, self.cur = name, rule, prev, cur
        self.tracked = np.ascontiguousarray(tracked, KR.index_pair_dtype)
        self.planted = np.array(sorted(planted), np.int64)               # positions in `tracked`

    def octave(self):
        return (self.prev, self.cur, self.tracked)


def stereo_case(name, rule, n, n_out=0, seed=0, noise=0.0):
    """n physical points seen in both frames; the last n_out positions drawn for `planted` get a current position moved by 6 to 16
    pixels in both images (an independently moving object); every list in its own order"""
    rng = np.random.RandomState(1000 + 7 * n + seed)
    uv = np.stack([rng.uniform(6, W - 6, n), rng.uniform(6, H - 6, n)], 1)
    z = rng.uniform(2.0, 9.0, n)
    X = np.stack([(uv[:, 0] - CX) * z / FOCAL, (uv[:, 1] - CY) * z / FOCAL, z], 1)
    pl, pr = project(X)
    cl, cr = project(X @ MOTION_R.T + MOTION_T)
    if noise > 0.0:                                                       # detector noise on the current points, each image on its own
        cl = (cl + rng.normal(0.0, noise, cl.shape)).astype(F); cr = (cr + rng.normal(0.0, noise, cr.shape)).astype(F)
    planted_pts = rng.permutation(n)[:n_out]
    if n_out:
        ang, mag = rng.uniform(0, 2 * np.pi, n_out), rng.uniform(6.0, 16.0, n_out)
        d = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1).astype(F)
        cl[planted_pts] += d; cr[planted_pts] += d
    # point j sits at keypoint position o?[j]; previous pairing a is point pp[a], current pairing b is point pc[b]; tracked pair i is point pt[i]
    opl, opr, ocl, ocr, pp, pc, pt = (rng.permutation(n) for _ in range(7))
    def placed(xy, o):
        out = np.zeros_like(xy); out[o] = xy
        return out
    prev = RR.Lists(keypoints(placed(pl, opl)), keypoints(placed(pr, opr)), pairings(opl[pp], opr[pp]))
    cur = RR.Lists(keypoints(placed(cl, ocl)), keypoints(placed(cr, ocr)), pairings(ocl[pc], ocr[pc]))
    inv_pp, inv_pc = np.argsort(pp), np.argsort(pc)
    tracked = np.zeros(n, KR.index_pair_dtype)
    tracked["first"], tracked["second"] = inv_pp[pt], inv_pc[pt]
    planted = np.flatnonzero(np.isin(pt, planted_pts))
    return Case(name, rule, prev, cur, tracked, planted)


def no_model_case():
    """20 clean pairs whose previous RIGHT keypoints all lie on one image row: every sample of the right side has collinear triples, its
    sampler gives up after 10000 attempts and the side has no model -- use_f is false and every pair stays"""
    c = stereo_case("no_model_right", "a side that finds no model: nothing is rejected", 20, seed=3)
    c.prev.kps[1]["y"] = F(41.5)
    return c


def bad_index_case():
    """24 clean pairs, and between them pairs with a negative index, an index equal to the list length, and pairs through pairings that
    point past the keypoint lists: none of those is a candidate"""
    c = stereo_case("bad_indices", "indices outside their lists are dropped before the RANSAC", 24, seed=5)
    npm, ncm = len(c.prev.matches), len(c.cur.matches)
    # two more pairings per slot that point outside the keypoints: index == list length, and a negative one
    c.prev.matches = np.concatenate([c.prev.matches, pairings([len(c.prev.kps[0]), 3], [2, -1])])
    c.cur.matches = np.concatenate([c.cur.matches, pairings([1, -7], [len(c.cur.kps[1]) + 5, 4])])
    bad = np.array([(-1, 3), (npm + 2, 0), (4, -3), (5, ncm + 2), (npm, 6), (npm + 1, 7), (8, ncm), (9, ncm + 1), (-2147483648, 2), (2, 2147483647)], KR.index_pair_dtype)
    t = list(c.tracked)
    for k, b in enumerate(bad):
        t.insert(2 * k + (k % 3), tuple(b))
    tracked = np.array(t, KR.index_pair_dtype)
    is_bad = np.array([any(tuple(x) == tuple(b) for b in bad) for x in tracked])
    c.tracked = tracked
    c.bad = np.flatnonzero(is_bad)
    c.planted = np.zeros(0, np.int64)
    return c


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out = [stereo_case("clean_%d" % n, "%d clean pairs: path '%s'" % (n, RR.path_of(n)), n) for n in COUNTS]
        out += [stereo_case("planted_%d_%d" % (n, k), "%d pairs, %d of them planted outliers" % (n, k), n, k, seed=1) for n, k in PLANTED]
        # half of the pairs planted, and pixel noise: budgets that reach the later chunks of the sample schedule
        out += [stereo_case(nm, "%d pairs, %d planted, %.2f px of noise: a long sample schedule" % (n, k, s), n, k, seed=2, noise=s) for nm, n, k, s in HARD]
        out += [no_model_case(), bad_index_case()]
        _CASES = {c.name: c for c in out}
    return _CASES


def case(name):
    return cases()[name]


_WALKS = {}


def walk(name):
    """the case through the walk, once"""
    if name not in _WALKS:
        _WALKS[name] = RR.walk_octave(*case(name).octave())
    return _WALKS[name]


def put_case(ctx, lane, c, octave=0, with_prev=True):
    """the lists of a case into a lane-octave through the public puts (with_prev False: the current slot alone)"""
    if with_prev:
        ctx.put_features(lane, 1, 0, c.prev.kps[0], None, W, H, octave); ctx.put_features(lane, 1, 1, c.prev.kps[1], None, W, H, octave)
        ctx.put_matches(lane, 1, c.prev.matches, octave)
    ctx.put_features(lane, 0, 0, c.cur.kps[0], None, W, H, octave); ctx.put_features(lane, 0, 1, c.cur.kps[1], None, W, H, octave)
    ctx.put_matches(lane, 0, c.cur.matches, octave)
    ctx.put_tracked(lane, c.tracked, octave=octave)


# ---- the image sequence of the resident gate --------------------------------------------------------------------------------------
# tests/klt_scenes.py's five frames with a textured patch pasted into both images of every frame.  The patch sits at the same rows in
# the left and the right image (disparity PATCH_DISP, so its tracks pass the stereo gate) and moves (PATCH_DX, PATCH_DY) pixels per frame
# whatever the camera does: an independently moving object.  The camera moves forward, its epipole lies near the image centre; the patch
# sits in a corner and moves across the epipolar lines there.  Four tracks start on it, next to the 48 grid tracks of the scene.
PATCH, PATCH_X0, PATCH_Y0, PATCH_DISP, PATCH_DX, PATCH_DY = 28, 114, 6, 4, 4, 4
_gate_seq = {}


def gate_sequence_frames():
    if "frames" not in _gate_seq:
        import klt_scenes as KS
        rng = np.random.RandomState(11)
        tex = rng.randint(0, 256, (PATCH + 2, PATCH + 2)).astype(np.float64)
        tex = sum(tex[dy:dy + PATCH, dx:dx + PATCH] for dy in range(3) for dx in range(3)) / 9.0      # a 3 x 3 box blur: gradients a tracker can follow
        tex = np.clip(np.round((tex - tex.mean()) * 2.5 + 128.0), 0, 255).astype(np.uint8)
        out = []
        for t, (l, r) in enumerate(KS.sequence_frames()):
            l, r = l.copy(), r.copy()
            x, y = PATCH_X0 + PATCH_DX * t, PATCH_Y0 + PATCH_DY * t
            l[y:y + PATCH, x:x + PATCH] = tex
            r[y:y + PATCH, x - PATCH_DISP:x - PATCH_DISP + PATCH] = tex
            out.append((l, r))
        _gate_seq["frames"] = out
    return _gate_seq["frames"]


def gate_sequence_points():
    """the 48 grid points of tests/klt_scenes.py, then four on the patch; the patch points are the last four IDs"""
    import klt_scenes as KS
    l0, r0 = KS.sequence_points()
    pl = np.array([(PATCH_X0 + dx, PATCH_Y0 + dy) for dy in (11, 17) for dx in (11, 17)], F)
    pr = pl - np.array([PATCH_DISP, 0], F)
    return np.concatenate([l0, pl]), np.concatenate([r0, pr])


def lists_of(L):
    """a selection's lists (tests/klt_ref.py) as the walk's Lists"""
    return RR.Lists(L.kps[0], L.kps[1], L.matches)


# ---- hand-built steps for the resident gate (svo_debug_klt_select) ------------------------------------------------------------------
# n physical points seen from a camera that makes the same motion from step to step; step k's arrays are their projections, and the
# tracks at the slots of SEAMS (the wave and 256-chunk seams of the compactions) have slid by 6 to 16 pixels in that step alone.
SEAMS = (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257, 298, 299)


class StepWorld:
    def __init__(self, n, seed=0, steps=4):
        rng = np.random.RandomState(500 + seed)
        uv = np.stack([rng.uniform(10, W - 10, n), rng.uniform(10, H - 10, n)], 1)
        z = rng.uniform(2.0, 9.0, n)
        X = np.stack([(uv[:, 0] - CX) * z / FOCAL, (uv[:, 1] - CY) * z / FOCAL, z], 1)
        self.n, self.pts = n, []
        for _ in range(steps):
            self.pts.append(project(X))
            X = X @ MOTION_R.T + MOTION_T
        ang, mag = rng.uniform(0, 2 * np.pi, (steps, n)), rng.uniform(6.0, 16.0, (steps, n))
        self.slide = np.stack([mag * np.cos(ang), mag * np.sin(ang)], 2).astype(F)      # [step][point] what a slid track is off by

    def arrays(self, k, ids, slid_slots=()):
        """(left, right) of step k for the tracks `ids` (a track's ID is its point), the slots of slid_slots displaced"""
        l, r = self.pts[k][0][ids].copy(), self.pts[k][1][ids].copy()
        s = np.array([s for s in slid_slots if s < len(ids)], np.int64)
        if len(s):
            l[s] += self.slide[k][ids[s]]; r[s] += self.slide[k][ids[s]]
        return l, r, s
