"""Hand-built tables and pose increments for the prediction rule of the resident KLT front end (svo_debug_klt_predict), and the
fast-motion sequence its step is held to.

A scene is one lane's live table (left, right: [n, 2] float32), an increment `delta` (six float64) and `valid`, at the image size, cap
and camera of tests/klt_scenes.py.  Every scene states the rule it means to hit (`rule`) and what must come out of the walk of
tests/klt_predict_ref.py for it to have hit it (`expect`: slot -> reason of the walk or None for a predicted slot; `predicted`: a
count; `check`: a predicate on the walk's output).  tests/test_klt_predict_scenes_cpu.py asserts that reach on the walk alone;
tests/test_gpu_klt_predict.py runs the device through the scenes.

The sequence: a SyntheticStereoWorld at 160 x 120 whose trajectory is overwritten with a hand-made one -- a yaw per frame that ramps
up -- tracked with a shallow pyramid: every pair after the first lies beyond the reach of the unpredicted tracker and within it once
the last increment is applied."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_predict_ref as PR                                                           # noqa: E402
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402

F = np.float32
W, H, CAP, MAX_KPS, WIN = KS.W, KS.H, KS.CAP, KS.MAX_KPS, KS.WIN
BASELINE = 0.12
COUNTS = (0, 1, 255, 256, 257, CAP)               # the block edges of a grid of 256-thread blocks over cap = 300 slots
SMALL_ANGLE = 1e-5                                # rodrigues_with_derivs' threshold on the rotation angle
MOTION = np.array([0.002, 0.03, -0.004, 0.02, -0.01, -0.15])      # an ordinary increment: 1.7 degrees of yaw, 15 cm forward


def camera():
    """the camera of tests/klt_scenes.sequence_world(), without building the world"""
    from stereo_vo_amd.abi import StereoCamera
    return StereoCamera.simple(KS.SEQ_FOCAL, (W - 1) / 2.0, (H - 1) / 2.0, BASELINE, W, H)


def up(v):
    return np.nextafter(F(v), F(np.inf))


def down(v):
    return np.nextafter(F(v), F(-np.inf))


class Scene:
    def __init__(self, name, rule, left, right, delta, valid=1, expect=None, predicted=None, check=None):
        self.name, self.rule = name, rule
        self.left, self.right = np.ascontiguousarray(left, F).reshape(-1, 2), np.ascontiguousarray(right, F).reshape(-1, 2)
        self.delta, self.valid = np.ascontiguousarray(delta, np.float64), int(valid)
        self.expect, self.predicted, self.check = expect or {}, predicted, check


def depth_of(left, right, slot=0):
    """Z of a slot as item 2 triangulates it (float64)"""
    return float(PR.triangulate(left, right, camera())[1][slot, 2])


def scenes():
    out = []
    zero = np.zeros(6)
    for n in COUNTS:
        l, r = KS.good(n)
        out.append(Scene("count_%d" % n, "a live count of %d under an ordinary increment: the block edges of the grid" % n, l, r, MOTION,
                         check=lambda o, n=n: len(o.used) == n and (n == 0 or o.used.any())))

    # the disparity compare: exactly zero (cul == cur: the two products cancel exactly), negative, and the smallest positive ones
    l, r = KS.good(6, 1)
    r[0] = l[0]                                                          # den == 0: b_d is infinite
    r[1] = (l[1][0] + F(5.0), l[1][1])                                   # negative: a finite guess from behind the camera
    r[2] = (down(l[2][0]), l[2][1])                                      # one float32 step of disparity: a point 200 km away
    r[3] = (up(l[3][0]), l[3][1])                                        # one step on the other side
    out.append(Scene("disparity", "disparity exactly 0, negative (a finite guess from behind the camera), and one float32 step either side of 0",
                     l, r, zero, expect={0: "disparity", 1: "disparity", 2: None, 3: "disparity", 4: None, 5: None}))

    # Z1c through a backward translation of exactly the slot's depth: the rotation is the identity, so Z1c = Z + t3 in one addition
    l, r = KS.good(4, 2)
    z = depth_of(l, r, 0)
    for name, t3, why in (("depth_zero", -z, "depth"), ("depth_below", np.nextafter(-z, -np.inf), "depth"), ("depth_above", np.nextafter(-z, np.inf), "outside_left")):
        out.append(Scene(name, "Z1c of slot 0 %s: t3 = %r against a depth of %r" % (name[6:], t3, z), l, r, [0, 0, 0, 0, 0, t3], expect={0: why}))

    # the image edges, compared in float32 on the projected pixel.  With a zero increment the projection returns the slot's own
    # coordinates wherever the double rounding (1e-14) is below half a float32 step: everywhere but around 0
    l = np.array([(W - 1, 50), (up(W - 1), 50), (100, H - 1), (100, up(H - 1)), (60, 40)], F)
    r = l - np.array([5.0, 0.0], F)
    out.append(Scene("edges_left", "left guesses exactly on x = w - 1 and y = h - 1 and one float32 step outside each", l, r, zero,
                     expect={0: None, 1: "outside_left", 2: None, 3: "outside_left", 4: None}))
    l1 = np.array([(30 + 11 * k, 0.0) for k in range(10)], F)             # left y = 0 at ten columns and disparities: as for x = 0 below
    r1 = l1 - np.stack([np.arange(10) * 1.5 + 2.0, np.zeros(10)], axis=1).astype(F)
    both = lambda o, why: any(w is None for w in o.reasons) and any(w == why for w in o.reasons)
    out.append(Scene("edge_left_zero", "left guesses at y = 0 (ten disparities: the projection lands on 0 or within 1e-13 either side of it)",
                     l1, r1, zero, check=lambda o: both(o, "outside_left") and all(abs(float(v)) < 1e-12 for v in o.gl[:, 1])))
    r2 = np.array([(0.0, 20 + 9 * k) for k in range(10)], F)              # right x = 0 at ten rows and disparities: around 0 the double rounding decides
    l2 = r2 + np.stack([np.arange(10) * 1.5 + 2.0, np.zeros(10)], axis=1).astype(F)
    out.append(Scene("edge_right_zero", "right guesses at x = 0 (ten disparities: the projection lands on 0 or within 1e-13 either side of it)",
                     l2, r2, zero, check=lambda o: both(o, "outside_right") and all(abs(float(v)) < 1e-12 for v in o.gr[:, 0])))
    l3 = np.array([(12.0, 30.0), (12.0, 31.0)], F)
    r3 = np.array([(0.0, 30.0), (0.0, 31.0)], F)
    # a right guess pushed outside by the increment alone: 1 cm to the right moves the right pixel of a 1.4 m deep point by a pixel
    out.append(Scene("outside_right", "a right guess that leaves the image on the left while the left guess stays inside", l3, r3, [0, 0, 0, -0.02, 0, 0],
                     expect={0: "outside_right", 1: "outside_right"}))

    # a non-finite pixel with a positive disparity and a positive Z1c: the float32 conversion overflows
    l, r = KS.good(3, 3)
    z = depth_of(l, r, 0)
    out.append(Scene("nonfinite_pixel", "Z1c one step above 0 and a sideways translation of 1e25: uL overflows float32", l, r,
                     [0, 0, 0, 1e25, 0, np.nextafter(-z, np.inf)], expect={0: "nonfinite"}))

    # the increment itself
    l, r = KS.good(40, 4)
    out.append(Scene("delta_zero", "delta identically zero: every guess is the slot's own point, the right one on the left point's row", l, r, zero, predicted=40,
                     check=lambda o: o.gl.tobytes() == o.left.tobytes() and o.gr[:, 0].tobytes() == o.right[:, 0].tobytes() and o.gr[:, 1].tobytes() == o.left[:, 1].tobytes()))
    out.append(Scene("small_angle_below", "a rotation just below the small-angle threshold", l, r, [0, 0.9 * SMALL_ANGLE, 0, 0.01, 0, -0.1], predicted=40))
    out.append(Scene("small_angle_above", "a rotation just above the small-angle threshold", l, r, [0, 1.1 * SMALL_ANGLE, 0, 0.01, 0, -0.1], predicted=40))
    out.append(Scene("roll_near_pi", "a rotation of almost pi about the optical axis: the image turns upside down", l, r, [0, 0, 3.14159, 0, 0, 0],
                     check=lambda o: o.used.sum() >= 30 and (np.abs(o.gl[o.used == 1] - o.left[o.used == 1]) > 1).any()))
    out.append(Scene("yaw_near_pi", "a rotation of almost pi about the vertical axis: every point ends behind the camera", l, r, [0, 3.14159, 0, 0, 0, 0],
                     expect={s: "depth" for s in range(40)}))
    for k in (0, 4):
        for bad, tag in ((np.nan, "nan"), (np.inf, "inf"), (-np.inf, "minus_inf")):
            d = MOTION.copy(); d[k] = bad
            out.append(Scene("delta_%s_%d" % (tag, k), "%s in delta[%d] with valid = 1: the lane does not predict" % (tag, k), l, r, d,
                             expect={s: "lane" for s in range(40)}))
    out.append(Scene("not_valid", "valid = 0 with a finite delta: the lane does not predict", l, r, MOTION, valid=0, expect={s: "lane" for s in range(40)}))
    out.append(Scene("valid_other_than_1", "valid = -3: anything but 0 is valid", l, r, MOTION, valid=-3, predicted=40))

    # live slots that hold no point: NaN and infinities in each coordinate (the slots behind the live count hold NaN in every table).
    # The rule reads xl, yl and xr: such a value in one of them leaves the slot unpredicted; yr is not consulted
    l, r = KS.good(14, 5)
    exp = {0: None, 13: None}
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for c in range(4):
            s = 1 + 4 * k + c
            (l if c < 2 else r)[s, c & 1] = bad
            exp[s] = None if c == 3 else True
    out.append(Scene("nonfinite_slots", "NaN, +inf and -inf in each of a live slot's four coordinates: xl, yl and xr stop the prediction, yr is not read", l, r, MOTION,
                     expect={s: w for s, w in exp.items() if w is None}, check=lambda o, exp=exp: all(o.reasons[s] is not None for s, w in exp.items() if w)))
    return out


_SCENES = None


def scene(name):
    global _SCENES
    if _SCENES is None:
        _SCENES = {s.name: s for s in scenes()}
    return _SCENES[name]


class Walked:
    pass


def walk(sc):
    """a scene through the walk alone"""
    o = Walked()
    o.left, o.right = sc.left, sc.right
    o.gl, o.gr, o.used, o.reasons = PR.predict(sc.left, sc.right, camera(), sc.delta, sc.valid, W, H)
    return o


# ---- the fast-motion sequence -------------------------------------------------------------------------------------------------------
FAST_FRAMES = 5
FAST_YAW_DEG = (0.0, 1.6, 3.2, 4.8, 6.4)          # the yaw of frame t against frame t - 1: it ramps up by 1.6 degrees per frame
FAST_FWD = 0.05
FAST_LK = dict(win=WIN, max_level=1, max_iters=30, eps=0.01, min_eig=2e-3, fb_max=1.0)     # the round trip gives a wrong convergence up: status 0 inside the image
FAST_GATE = dict(max_dy=0.5, min_disp=0.2, max_disp=np.inf)
FAST_CAP = 64
_fast = {}


def fast_world():
    """the world of tests/klt_scenes.py (same scene, same textures) on a hand-made trajectory"""
    if "world" not in _fast:
        import torch
        from stereo_vo_amd.synth import SyntheticStereoWorld
        w = SyntheticStereoWorld(W, H, KS.SEQ_FOCAL, BASELINE, seed=7, n_frames=FAST_FRAMES, device=torch.device("cpu"), noise_sigma=1.0)
        w.poses, w.deltas = [np.eye(4)], [np.eye(4)]
        for t in range(1, FAST_FRAMES):
            a = math.radians(FAST_YAW_DEG[t])
            D = np.eye(4)
            D[:3, :3] = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
            D[:3, 3] = [0.0, 0.0, FAST_FWD]
            w.deltas.append(D); w.poses.append(w.poses[-1] @ D)
        _fast["world"] = w
    return _fast["world"]


def fast_frames():
    if "frames" not in _fast:
        w = fast_world()
        _fast["frames"] = [tuple(np.ascontiguousarray(e.cpu().numpy()) for e in w.render(t)) for t in range(FAST_FRAMES)]
    return _fast["frames"]


def fast_points():
    """left points on a grid of frame 0, kept to the part of the image that stays in view while the camera turns right, and their right
    partners by the ground-truth disparity"""
    if "points" not in _fast:
        w = fast_world()
        xs = np.linspace(60.0, W - 12.0, 8); ys = np.linspace(12.0, H - 13.0, 6)
        left = np.array([(x, y) for y in ys for x in xs], F)
        z = KS.gt_depth(w, 0, left)
        right = left.copy()
        right[:, 0] = (left[:, 0] - w.f * w.B / z).astype(F)
        _fast["points"] = (left, right)
    return _fast["points"]


def fast_gt_delta(t):
    """the increment stage 5 estimates for frame t, from the ground truth: points of frame t - 1 expressed in frame t, as the six values of
    svo_result.delta (rotation vector, translation)"""
    D = np.linalg.inv(fast_world().deltas[t])
    a = math.atan2(D[0, 2], D[0, 0])                # a rotation about y
    return np.array([0.0, a, 0.0, D[0, 3], D[1, 3], D[2, 3]])


def fast_walk(predicted):
    """The sequence through tests/lk_ref.py and the selection walk, with the guesses of the rule (predicted) or without.  The lane's
    record is modelled by the ground truth: valid from the second tracked pair on, delta = the increment of the pair before (what a
    stage 5 that works returns; the GPU test uses the device's own record on both of its sides).  Per frame: (table after, the two
    jobs' per-slot status, their traces (None at frame 0), used, the IDs of the slots before the frame)."""
    key = "walk%d" % int(predicted)
    if key not in _fast:
        import lk_ref as LR
        frames, (l0, r0) = fast_frames(), fast_points()
        P = LR.LkParams(**FAST_LK)
        g = KR.Gate(win=WIN, **FAST_GATE)
        t, _ = KR.add_points(KR.Table(), l0, r0, FAST_CAP)
        out, stepped = [], False
        for f in range(FAST_FRAMES):
            n = len(t)
            used = np.zeros(n, np.uint8)
            if f == 0:
                res = [(t.left, np.ones(n, np.uint8), None), (t.right, np.ones(n, np.uint8), None)]
            else:
                gl = gr = None
                if predicted:
                    valid = 1 if f >= 2 else 0
                    gl, gr, used, _ = PR.predict(t.left, t.right, camera(), fast_gt_delta(f - 1) if f >= 2 else np.zeros(6), valid, W, H)
                res = []
                for sd, init in ((0, gl), (1, gr)):
                    o, s, _, tr = LR.track(frames[f - 1][sd], frames[f][sd], t.left if sd == 0 else t.right, init=init, params=P)
                    res.append((o, s, tr))
            _, t2, _ = KR.select(t, res[0][0], res[1][0], res[0][1], res[1][1], g, KR.lane_shifts(stepped, 0), H)
            out.append((t2, (res[0][1].copy(), res[1][1].copy()), (res[0][2], res[1][2]), used, t.ids.copy()))
            t, stepped = t2, True
        _fast[key] = out
    return _fast[key]
