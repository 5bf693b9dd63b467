"""Hand-built stereo pairs for the resident top-up of the KLT front end (svo_klt_topup).

A scene is one lane: a left and a right image, the tracks the lane holds before the top-up (added with svo_klt_add_points), the
front end's and the top-up's parameters, and what the walk of tests/klt_topup_ref.py must make of it for the scene to do what it
claims (`expect`, checked by tests/test_klt_topup_scenes_cpu.py).  tests/test_gpu_klt_topup.py runs the device and the host recipe
through the same scenes.

The features are 3 x 3 binomial blobs on black.  The tracker's window is 9 x 9 (lk.win 9) and the scenes track on level 0 alone, so a
blob at least 7 pixels from its neighbours is alone in its window whatever the window does within a pixel: a blob the right image
shows one pixel to the left is found there (disparity 1), and a blob the right image does not show leaves the first guess where it
was -- the window sees nothing, so the step is zero and the status stays 1.  Such a corner is then dropped by the gate when the first
guess has disparity 0 (< min_disp), and by the forward-backward check when fb_max > 0 (the way back starts on a flat template).  A
grid of all-equal blobs ties every response, so the walk order is the raster order of the grid."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402

F = np.float32
W, H = 96, 64                    # the small scenes
CAP = 64
MAX_KPS = 1024                   # the contexts of the GPU tests: a power of two above the seam scene's cap of 640
MAX_CAND = 1024                  # ... and a candidate capacity a 128 x 128 dot image overflows
WIN = 9
LK = dict(win=WIN, max_level=0, max_iters=30, eps=0.01, min_eig=1e-4, fb_max=0.0)
GATE = dict(max_dy=1.5, min_disp=0.5, max_disp=40.0)
GFTT = dict(max_corners=0, block=3, min_distance=4, quality=0.01)
AMP = 60
_K = np.array([[1, 2, 1], [2, 4, 2], [1, 2, 1]], np.int64)


def blobs(w, h, pts, amps=AMP, skip=(), dx=0, dy=0):
    """3 x 3 binomial blobs of peak 4 * amp at pts (x, y), shifted by (-dx, +dy); the indices of `skip` are left out"""
    im = np.zeros((h, w), np.int64)
    amps = [amps] * len(pts) if np.isscalar(amps) else amps
    for k, ((x, y), a) in enumerate(zip(pts, amps)):
        if k not in skip:
            im[y - 1 + dy:y + 2 + dy, x - 1 - dx:x + 2 - dx] += a * _K
    assert im.max() <= 255
    return im.astype(np.uint8)


def grid(w, h, step, x0=8, y0=8):
    return [(x, y) for y in range(y0, h - 7, step) for x in range(x0, w - 7, step)]


def tracks_on(pts, disp=1.0):
    """(left, right) tracks sitting on blobs: what a lane holds before the top-up"""
    left = np.array(pts, F).reshape(-1, 2)
    right = left.copy(); right[:, 0] -= F(disp)
    return left, right


class Scene:
    def __init__(self, name, claim, left, right, tracks, expect, cap=CAP, lk=None, gate=None, gftt=None, **topup):
        self.name, self.claim, self.left, self.right, self.tracks, self.expect, self.cap = name, claim, left, right, tracks, expect, cap
        self.lk = dict(LK); self.lk.update(lk or {})
        self.gate = dict(GATE); self.gate.update(gate or {})
        self.gftt = dict(GFTT); self.gftt.update(gftt or {})
        self.topup = topup             # below, target, init_disp (None: the defaults)

    @property
    def size(self):
        return self.left.shape[1], self.left.shape[0]

    def tp(self):
        return TR.TopupParams(self.cap, **self.topup)


def _build():
    S = []
    g12 = grid(W, H, 16)                                         # 6 x 4 = 24 blobs, 16 apart
    assert len(g12) == 24
    pair = lambda pts, **kw: (blobs(W, H, pts), blobs(W, H, pts, dx=1, **kw))
    # -- how many are wanted
    l, r = pair(g12)
    S.append(Scene("want_exceeds_corners", "the image has fewer corners than the lane wants: all of them are appended",
                   l, r, tracks_on(g12[:2]), dict(corners=22, appended=22, reason=TR.OK, n_after=24)))
    S.append(Scene("want_zero", "n == target below the threshold: the detector runs with room for nothing",
                   l, r, tracks_on(g12[:4]), dict(corners=0, appended=0, reason=TR.OK, n_after=4), below=10, target=4))
    S.append(Scene("enough", "n == below: the lane is left alone",
                   l, r, tracks_on(g12[:10]), dict(corners=0, appended=0, reason=TR.ENOUGH, n_after=10), below=10))
    g8 = grid(W, H, 8)                                           # 11 x 7 = 77 blobs, 8 apart
    assert len(g8) == 77
    l8, r8 = blobs(W, H, g8), blobs(W, H, g8, dx=1)
    S.append(Scene("lands_on_cap", "n + survivors == cap exactly: 8 tracks and room for 56 of the 69 corners left",
                   l8, r8, tracks_on(g8[:8]), dict(corners=56, appended=56, reason=TR.OK, n_after=CAP)))
    S.append(Scene("target_cuts", "target below cap: 8 tracks, target 40",
                   l8, r8, tracks_on(g8[:8]), dict(corners=32, appended=32, reason=TR.OK, n_after=40), target=40))
    # -- seeds: one blob is the strongest; a live track decides whether it becomes a corner
    import gftt_scenes as GS
    amps = [AMP] * 24; amps[9] = 63
    cx, cy = g12[9]
    ls, rs = blobs(W, H, g12, amps), blobs(W, H, g12, amps, dx=1)
    md = 5
    inside = np.array([(cx + 3.0, cy + 3.5)], F)                 # 9 + 12.25 < 25
    out_x, out_y = GS.disagreeing_seeds(cx, cy, md, 1)[0]        # float32 says NOT closer than md; double would say closer
    outside = np.array([(out_x, out_y)], F)
    for name, seed, first in (("seed_inside", inside, False), ("seed_just_outside", outside, True)):
        S.append(Scene(name, "a live track %s min_distance of the strongest corner" % ("inside" if not first else "just outside (float32)"),
                       ls, rs, (seed, seed - np.array([1.0, 0.0], F)),
                       dict(corners=24 if first else 23, appended=24 if first else 23, reason=TR.OK, first_corner=(cx, cy) if first else None,
                            absent=None if first else (cx, cy)), gftt=dict(min_distance=md)))
    # -- the gate
    none = (np.zeros((0, 2), F), np.zeros((0, 2), F))
    S.append(Scene("identical", "the right image is the left one: disparity 0 is below min_disp",
                   l, l.copy(), none, dict(corners=24, appended=0, reason=TR.OK, status_ones=24)))
    S.append(Scene("shifted", "the right image one pixel to the left, first guess at disparity 0: every corner is found",
                   l, r, none, dict(corners=24, appended=24, reason=TR.OK, disparity=1.0)))
    r5 = blobs(W, H, g12, dx=5)
    S.append(Scene("shifted_5_blind", "five pixels to the left, first guess at disparity 0: the window sees nothing it knows and stays",
                   l, r5, none, dict(corners=24, appended=0, reason=TR.OK, status_ones=24)))
    S.append(Scene("shifted_5_guessed", "five pixels to the left, init_disp 5: found, but for the leftmost column, whose window leaves the image (status 0)",
                   l, r5, none, dict(corners=24, appended=20, reason=TR.OK, disparity=5.0, status_zero=[k for k in range(24) if k % 6 == 0]), init_disp=5.0))
    S.append(Scene("vertical", "the right image two rows down as well: the partners are found and |dy| exceeds max_dy",
                   l, blobs(W, H, g12, dx=1, dy=2), none, dict(corners=24, appended=0, reason=TR.OK, dy=2.0)))
    half_gone = [k for k, (x, y) in enumerate(g12) if x >= W // 2]
    S.append(Scene("textureless_fb", "the right half of the right image is flat and fb_max > 0: the way back starts on a flat template, status 0",
                   l, blobs(W, H, g12, dx=1, skip=half_gone), none,
                   dict(corners=24, appended=12, reason=TR.OK, status_zero=half_gone), lk=dict(fb_max=0.5), init_disp=1.0))
    S.append(Scene("fb_max", "fb_max > 0 on a clean pair: the round trip ends where it started", l, r, none,
                   dict(corners=24, appended=24, reason=TR.OK, disparity=1.0), lk=dict(fb_max=0.5)))
    return S


SEAM_W, SEAM_H, SEAM_CAP, SEAM_TRACKS = 200, 160, 640, 8


@functools.lru_cache(maxsize=None)
def seam():
    """27 x 21 = 567 blobs 7 apart (the closest at which a blob is alone in its 9 x 9 window, hence an image of 200 x 160); the lane
    holds tracks on the first 8; every third blob of the grid is erased in the right image.  559 corners in raster order: corner j is
    blob j + 8, dropped when (j + 8) % 3 == 0 -- so slots 63 | 64, 255 | 256 and 511 | 512 each hold one survivor and one reject, and the
    append starts at slot 8 of the table"""
    g = grid(SEAM_W, SEAM_H, 7)
    assert len(g) == 567
    erased = [k for k in range(len(g)) if k % 3 == 0]
    left, right = blobs(SEAM_W, SEAM_H, g), blobs(SEAM_W, SEAM_H, g, dx=1, skip=erased)
    keep = np.array([(j + SEAM_TRACKS) % 3 != 0 for j in range(len(g) - SEAM_TRACKS)])
    return Scene("seam", "more than 512 corners, survivors and rejects interleaved across every wave and chunk seam, append base 8",
                 left, right, tracks_on(g[:SEAM_TRACKS]), dict(corners=559, appended=int(keep.sum()), reason=TR.OK, keep=keep, n_after=SEAM_TRACKS + int(keep.sum())),
                 cap=SEAM_CAP, gftt=dict(min_distance=3))


@functools.lru_cache(maxsize=None)
def scenes():
    return tuple(_build())


def scene(name):
    if name == "seam":
        return seam()
    for s in scenes():
        if s.name == name:
            return s
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def walk(name):
    """(table before, table after, info, details) of the scene through the numpy walk"""
    import gftt_ref as GR
    import lk_ref as LR
    s = scene(name)
    t0, m = KR.add_points(KR.Table(), s.tracks[0], s.tracks[1], s.cap)
    assert m == len(s.tracks[0])
    t1, info, det = TR.walk(t0, s.left, s.right, s.cap, KR.Gate(win=WIN, **s.gate), s.tp(), GR.GfttParams(**s.gftt), LR.LkParams(**s.lk))
    return t0, t1, info, det


def overflow_image(w=128, h=128):
    """a dot every 3 pixels: 40 x 40 dots of one strength, more than 1024 candidates"""
    im = np.zeros((h, w), np.uint8)
    im[4:h - 4:3, 4:w - 4:3] = 200
    return im


# ---- arrays no image could produce, for svo_debug_klt_topup_append ----
def _ulp(v, k):
    return np.nextafter(F(v), F(np.inf) if k > 0 else F(-np.inf), dtype=F)


def append_arrays():
    """(left, right, status, the bool the gate must give per pair) under GATE: non-finite coordinates, |dy| and the disparity one ulp
    on either side of each bound and on it, status values other than 0 and 1"""
    rows = []

    def add(xl, yl, xr, yr, st, ok):
        rows.append((F(xl), F(yl), F(xr), F(yr), st, ok))
    add(30, 20, 25, 20, 1, True)
    for bad in (np.nan, np.inf, -np.inf):
        add(bad, 20, 25, 20, 1, False); add(30, bad, 25, 20, 1, False); add(30, 20, bad, 20, 1, False); add(30, 20, 25, bad, 1, False)
    md, lo, hi = F(GATE["max_dy"]), F(GATE["min_disp"]), F(GATE["max_disp"])
    for k, ok in ((-1, True), (0, True), (1, False)):
        d = md if k == 0 else _ulp(md, k)
        add(30, d, 25, 0, 1, ok); add(30, 0, 25, d, 1, ok)            # y differences exact: one operand is 0
    for k, ok in ((-1, False), (0, True), (1, True)):
        d = lo if k == 0 else _ulp(lo, k)
        add(d, 20, 0, 20, 1, ok)
    for k, ok in ((-1, True), (0, True), (1, False)):
        d = hi if k == 0 else _ulp(hi, k)
        add(d, 20, 0, 20, 1, ok)
    for st in (0, 2, 255):
        add(30, 20, 25, 20, st, False)
    add(31, 21, 26, 21, 1, True)
    a = np.array([r[:4] for r in rows], F)
    return a[:, 0:2].copy(), a[:, 2:4].copy(), np.array([r[4] for r in rows], np.uint8), np.array([r[5] for r in rows], bool)
