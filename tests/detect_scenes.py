"""Images built by hand for the tile edges of the detect chain (csrc/k_detect.hip: k_resize, k_fast / k_fast_redo, k_select, k_harris,
k_select_sort, k_describe and, behind them, k_nms_rowsort) -- numpy only; the oracle is imported by the one generator that searches with it.
The whole-frame suites (the synthetic world, noise, the photograph, tests/image_content.py) leave to chance which tile seam, which lane of a
four-pixel group, which octant of the orientation or which side of a selection cut a frame exercises; here every image is made for one.

A scene is a dict: `imgs` (a list of uint8 images of one shape, run in this order through one context: all but the `cuts` redo scene hold
one), `w`, `h`, the parameters `orb_nlevels`, `orb_nfeats`, `initial_FAST_threshold`, `nms` (non_maximal_suppression) and `min_distance`,
a `family`, a `name`, and -- where construction alone gives the answer -- `expect`:

  expect["fast"]    dots     the (x, y, FAST score) that survive the strict 3x3 NMS inside the 31-pixel border, in raster order, from three
                             rules: a single pixel that differs by d from a flat background scores |d| - 1 when |d| > th and nothing
                             otherwise -- also with ONE other dot on its circle or next to it --; of two 8-neighbours the strictly larger
                             survives, of two equal ones neither; positions x, y = 30 and dim - 31 are scored (they suppress) but never kept
  expect["kept"]    cuts     the (x, y) of the raw keypoint list of the LAST image, in list order
  expect["angle"]   orient   {(x, y): degrees} per keypoint cell: atan2(v, u) of the one weight pixel, 0 without one, 0 / 90 / 180 / 270 of an edge

Geometry the positions come from: SVO_EDGE = 31, k_fast's 62 x 62 interior tiles from (31, 31) (seams at 92 | 93), its groups of four
positions (x - 30) % 4 and blocks of eight rows (y - 30) % 8, k_resize's 128 x 32 destination tiles, k_describe's 43-row window fetched by
16-byte DMA chunks from any byte, the radius-15 disc of the orientation.  tests/test_detect_scenes_cpu.py holds the oracle to `expect` and
counts, from the oracle and these constants alone, that the scenes reach the edges; tests/test_gpu_detect_scenes.py runs the kernels."""
import functools
import math

import numpy as np

EDGE, FT, TH = 31, 62, 20                   # SVO_EDGE, SVO_FT_W = SVO_FT_H, the FAST threshold of every scene
RZ_W, RZ_H = 128, 32                        # k_resize's destination tile
W0, H0 = 160, 128                           # level-0 interior x 31 .. 128 (tile columns of 62 and 36), y 31 .. 96 (tile rows of 62 and 4)
GAUSS7 = (18, 34, 49, 55, 49, 34, 18)       # cvRound(256 g): the taps of both blur passes (include/svo_orb_tables.h)
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)      # half widths of the disc's rows
NBR8 = [(i, j) for j in (-1, 0, 1) for i in (-1, 0, 1) if i or j]


def make(name, family, imgs, nlevels=1, nfeats=500, nms=False, min_distance=3, expect=None, **more):
    imgs = [np.ascontiguousarray(i, np.uint8) for i in imgs]
    h, w = imgs[0].shape
    assert all(i.shape == (h, w) for i in imgs)
    return dict(name=name, family=family, imgs=imgs, w=w, h=h, orb_nlevels=nlevels, orb_nfeats=nfeats, initial_FAST_threshold=TH, nms=nms,
                min_distance=min_distance, expect=expect or {}, **more)


def raw_nfeatures(s):
    """what the detector asks cv::ORB for: 1.5 x orb_nfeats when the NMS follows"""
    return int(1.5 * s["orb_nfeats"]) if s["nms"] else s["orb_nfeats"]


def scene_params(base, s):
    """the scene's parameters over `base` (hip.default_params() or oracle.default_params())"""
    from stereo_vo_amd.abi import north_star_params
    p = north_star_params(base, orb_nfeats=s["orb_nfeats"])
    p.orb_nlevels, p.initial_FAST_threshold, p.non_maximal_suppression, p.min_distance = s["orb_nlevels"], s["initial_FAST_threshold"], int(s["nms"]), s["min_distance"]
    return p


def interior(x, y, w, h):
    return EDGE <= x < w - EDGE and EDGE <= y < h - EDGE


# ---------------------------------------------------------------------------------------------------------------------------------------
# dots
# ---------------------------------------------------------------------------------------------------------------------------------------
class Canvas:
    """a flat image with single-pixel dots; predicts its own FAST corners from the three rules of the module text"""

    def __init__(self, b, w=W0, h=H0):
        self.b, self.w, self.h, self.img, self.dots, self.other = b, w, h, np.full((h, w), b, np.uint8), [], []

    def fits(self, group, apart=7):
        """no dot of `group` nearer than `apart` (Chebyshev) to anything already here: the rules need at most two dots per cluster"""
        return all(max(abs(x - a), abs(y - c)) >= apart for x, y, _ in group for a, c in [(p[0], p[1]) for p in self.dots] + self.other)

    def add(self, group):
        for x, y, d in group:
            assert 0 <= self.b + d <= 255 and d != 0 and self.img[y, x] == self.b and 27 <= x < self.w - 27 and 27 <= y < self.h - 27, (x, y, d)
            self.img[y, x] = self.b + d
            self.dots.append((x, y, d))

    def paint(self, x, y, v):
        """a pixel that is no dot (at most th away from the background: the rules above stay as they are)"""
        assert abs(v - self.b) <= TH and self.img[y, x] == self.b
        self.img[y, x] = v
        self.other.append((x, y))

    def fast(self):
        score = {(x, y): abs(d) - 1 for x, y, d in self.dots if abs(d) > TH and EDGE - 1 <= x <= self.w - EDGE and EDGE - 1 <= y <= self.h - EDGE}
        return sorted(((x, y, s) for (x, y), s in score.items() if interior(x, y, self.w, self.h) and all(score.get((x + i, y + j), 0) < s for i, j in NBR8)),
                      key=lambda t: (t[1], t[0]))


BACKGROUNDS = (0, 1, 19, 20, 21, 100, 234, 235, 254, 255)
XS = (30, 31, 92, 93, 128, 129)          # outside by one, first interior column, last of tile 0, first of tile 1, last interior column, outside by one
YS = (30, 31, 92, 93, 96, 97)


def deltas(b):
    return [d for m in sorted({TH, TH + 1, 60, 255 - b, b}) for d in (m, -m) if m and 0 <= b + d <= 255]


def _pack(groups, b, apart=7):
    """the groups dealt over as few canvases as keep them `apart`"""
    out = []
    for g in groups:
        for c in out:
            if c.fits(g, apart):
                break
        else:
            c = Canvas(b)
            out.append(c)
        c.add(g)
    return out


def dot_positions():
    """every special column against some row and every special row against some column in both tile columns, the corners of the interior
    and of the four tiles that meet at (92 | 93, 92 | 93), and every group residue against both row-block residues in both tile columns"""
    pos = [(x, 44 + 7 * k) for k, x in enumerate(XS)] + [(47 + 7 * k, y) for k, y in enumerate(YS)] + [(96 + 6 * k, y) for k, y in enumerate(YS)]
    pos += [(31, 31), (128, 31), (31, 96), (128, 96), (30, 30), (129, 97), (92, 92), (93, 93), (92, 93), (93, 92)]
    for r in range(4):
        pos += [(50 + r, 38 + 16 * r), (102 + r, 46 + 16 * r), (58 + r, 37 + 16 * r), (110 + r, 45 + 16 * r)]       # (y - 30) % 8 = 0, 0, 7, 7
    return pos


def dots_scenes():
    out = []
    pos = dot_positions()
    for bi, b in enumerate(BACKGROUNDS):
        ds = deltas(b)
        groups = [[(x, y, ds[(5 * i + 3 * bi + i // len(ds)) % len(ds)])] for i, (x, y) in enumerate(pos)]
        for k, c in enumerate(_pack(groups, b, apart=6)):
            out.append(make("dots-b%d-%d" % (b, k), "dots", [c.img], expect={"fast": c.fast()}, background=b, kind="single"))
    # the packed cardinal test's neighbouring bytes at |d| = th: the bytes left and right of the compass pixels N E S W at the far end of
    # the range (0 under a dot of b + th, 255 over a dot of b - th) while staying th away from the background themselves, so that
    # nothing but the dot can be a corner; d = th + 1 beside them, which the bytes must not hide
    for b, sgn in ((20, 1), (235, -1)):
        c = Canvas(b)
        far, n = (0 if sgn > 0 else 255), 0
        for sides in ((-1,), (1,), (-1, 1)):
            for d in (TH, TH + 1):
                for r in range(4):
                    x, y = 40 + 14 * (n % 6), 40 + 12 * (n // 6)
                    x += (r - (x - 30)) % 4
                    n += 1
                    c.add([(x, y, sgn * d)])
                    for s in sides:
                        for cx, cy in ((0, -3), (3, 0), (0, 3), (-3, 0)):
                            c.paint(x + cx + s, y + cy, far)
        out.append(make("dots-thbytes-b%d" % b, "dots", [c.img], expect={"fast": c.fast()}, background=b, kind="thbytes"))
    # pairs one apart (equal: neither survives; unequal: the larger), inside a tile, across the seams 92 | 93 and across the border
    # columns / rows that are scored but never kept; then pairs three apart (each on the other's circle: both survive)
    groups = []
    slot = iter([(x, y) for y in range(36, 90, 9) for x in list(range(36, 84, 9)) + list(range(98, 124, 9))])

    def pair(x, y, i, j, da, db):
        groups.append([(x, y, da), (x + i, y + j, db)])

    for i, j in ((1, 0), (0, 1), (1, 1), (-1, 1)):
        for n, (da, db) in enumerate(((60, 60), (60, 61), (61, 60), (60, -60), (-61, 60))):
            pair(*next(slot), i, j, da, db)                                 # inside a tile
            if i: pair(92 if i > 0 else 93, 36 + 11 * n, i, j, da, db)      # across the seam in x
            if j: pair(40 + 11 * n, 92, i, j, da, db)                       # across the seam in y
            if i and j and n < 3: pair(92 if i > 0 else 93, 92, i, j, da, db)         # across both
    for da, db in ((60, 60), (60, 61), (61, 60)):
        groups += [[(30, 40, da), (31, 40, db)], [(30, 60, da), (31, 61, db)], [(128, 50, da), (129, 50, db)], [(128, 70, da), (129, 69, db)],
                   [(45, 30, da), (45, 31, db)], [(70, 30, da), (71, 31, db)], [(55, 96, da), (55, 97, db)], [(110, 96, da), (109, 97, db)]]
    for i, j in ((3, 0), (0, 3), (2, 2), (3, 1), (1, 3), (-2, 2), (-3, 1)):
        for da, db in ((60, 60), (60, 100), (-100, 60)):
            pair(*next(slot), i, j, da, db)
    pair(90, 50, 3, 0, 60, 100); pair(90, 70, 3, 1, 100, 60); pair(60, 90, 0, 3, 60, 100); pair(100, 91, 2, 2, 60, 60)      # the other dot in the next tile
    for k, c in enumerate(_pack(groups, 100, apart=8)):
        out.append(make("dots-pairs-%d" % k, "dots", [c.img], expect={"fast": c.fast()}, background=100, kind="pairs", groups=[g for g in groups if all(d in c.dots for d in g)]))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# cuts
# ---------------------------------------------------------------------------------------------------------------------------------------
CUT_GRID = [(31 + 8 * i, 31 + 8 * j) for j in range(8) for i in range(12)]       # 96 dots in raster order
RAISED = [k for k in range(96) if k % 5 == 2 or k == 95]                            # 20 of them


def _grid_image(amps):
    img = np.zeros((H0, W0), np.uint8)
    for (x, y), d in zip(CUT_GRID, amps):
        img[y, x] = d
    return img


def _kept(amps, nfeats):
    """cv::ORB's two cuts on equal-shaped dots: the best 2 n by FAST score AND whatever ties with the last of them, then the best n by
    (Harris response descending, position ascending) -- on single dots both orders are the order of |d|"""
    order = sorted(range(96), key=lambda k: (-amps[k], k))
    if len(order) > 2 * nfeats:
        last = amps[order[2 * nfeats - 1]]
        order = [k for k in order if amps[k] >= last]
    return [CUT_GRID[k] for k in order[:nfeats]]


def cuts_scenes():
    out = []
    base = [60] * 96
    for n in (10, 24, 47, 48, 49):
        out.append(make("cuts-equal-%d" % n, "cuts", [_grid_image(base)], nfeats=n, expect={"kept": _kept(base, n)}))
        assert out[-1]["expect"]["kept"] == CUT_GRID[:n]
    raised = [100 if k in RAISED else 60 for k in range(96)]
    assert len(RAISED) == 20
    for n in (10, 15, 30):
        out.append(make("cuts-raised-%d" % n, "cuts", [_grid_image(raised)], nfeats=n, expect={"kept": _kept(raised, n)}))
    # the redo: after the equal dots the level's speculated threshold is their score, 59 (3 * 10 + 32 candidates reach it); the next image
    # has five corners there, fewer than 2 * 10, so the level starts over at the caller's threshold and finds the 91 dots of score 39 too
    weak = [60 if k in (7, 33, 50, 76, 94) else 40 for k in range(96)]
    out.append(make("cuts-redo-10", "cuts", [_grid_image(base), _grid_image(weak)], nfeats=10, expect={"kept": _kept(weak, 10)}, redo=True))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# orient
# ---------------------------------------------------------------------------------------------------------------------------------------
CELL = 96
OCTANT_EDGES = [(10, 0), (10, 10), (0, 10), (-10, 10), (-10, 0), (-10, -10), (0, -10), (10, -10)]
NEAR_AXES = [(15, 1), (1, 15), (-1, 15), (-15, 1), (-15, -1), (-1, -15), (1, -15), (15, -1)]
INSIDE = [(4, 0), (0, -4), (5, 12), (-7, 3), (-3, -14), (12, -5), (-13, 7)]


def in_disc(u, v):
    return abs(v) <= 15 and abs(u) <= UMAX[abs(v)]


def orient_scenes():
    """cells of 96 x 96 with the keypoint (a dot as far from the background as a byte goes) in the middle and ONE weight pixel th away from
    the background at (u, v) inside the disc: the moments are (u, v) times that difference, whatever the background adds cancels"""
    out = []
    offs = OCTANT_EDGES + NEAR_AXES + [None] + INSIDE
    assert all(o is None or (in_disc(*o) and max(abs(o[0]), abs(o[1])) >= 4) for o in offs)
    for b, dot, delta in ((0, 255, TH), (100, 255, TH), (255, 0, -TH)):
        for part in range(2):
            img = np.full((3 * CELL, 4 * CELL), b, np.uint8)
            angle = {}
            for k, o in enumerate(offs[12 * part:12 * part + 12]):
                cx, cy = CELL * (k % 4) + 48, CELL * (k // 4) + 48
                img[cy, cx] = dot
                if o is None:
                    angle[cx, cy] = 0.0
                else:
                    u, v = (o[0], o[1]) if delta > 0 else (-o[0], -o[1])          # a darker pixel pulls the other way: mirror it, the angle stays
                    img[cy + v, cx + u] = b + delta
                    angle[cx, cy] = math.degrees(math.atan2(o[1], o[0])) % 360.0
            out.append(make("orient-b%d-%d" % (b, part), "orient", [img], nfeats=50, expect={"angle": angle}, background=b, weighted=True))
    # the largest moments: a 0 | 255 half plane through a dot of 128 -- nine contiguous circle pixels brighter than the dot, so it is a
    # corner and the straight edge around it is none; m10 or m01 is 255 times the half disc, the other moment cancels
    for nm, ang in (("right", 0.0), ("below", 90.0), ("left", 180.0), ("above", 270.0)):
        img = np.zeros((H0, W0), np.uint8)
        cx, cy = 80, 64
        if nm == "right": img[:, cx:] = 255
        if nm == "left": img[:, :cx + 1] = 255
        if nm == "below": img[cy:, :] = 255
        if nm == "above": img[:cy + 1, :] = 255
        img[cy, cx] = 128
        out.append(make("orient-edge-" + nm, "orient", [img], nfeats=50, expect={"angle": {(cx, cy): ang}}, background=None, weighted=False))
    # the quadrant choice of the steering's sine and cosine: moments (-395, -397) give the angle 225.15149, whose argument x * 2 / pi is
    # 2.5017: (int)(. + 0.5) picks k = 3, within a hundredth of the tie.  One quadrant further down the polynomials give a sine one unit in
    # the last place away, which moves the rotated sample point (7, -12) of two tests from (-13, 3) to (-13, 4).  The six pixels of 20
    # left of the disc make the blurred image 0 at the first and 1 at the second (30960 and 36360 before the rounding at 32768), so
    # test 1 reads 0 < 0 with the right quadrant and 0 < 1 with the other
    img = np.zeros((H0, W0), np.uint8)
    cx, cy = TIE_AT
    img[cy, cx] = 255
    for (u, v), val in (((-15, 0), 20), ((-5, 0), 19), ((0, -15), 20), ((0, -14), 6), ((0, -13), 1)):
        assert in_disc(u, v)
        img[cy + v, cx + u] = val
    assert not any(in_disc(-16, v) for v in range(5, 11))
    img[cy + 5:cy + 11, cx - 16] = TH
    out.append(make("orient-tie-225", "orient", [img], nfeats=50, expect={"angle": {TIE_AT: math.degrees(math.atan2(-397, -395)) % 360.0}}, background=0, weighted=True))
    return out


TIE_AT = (80, 64)


def sincos_model(x, half=0.5):
    """the oracle's sincosf in numpy's float32, one rounding per operator; `half` is the constant that picks the quadrant (the oracle's
    is 0.5): (sine, cosine, k)"""
    f = np.float32
    x = f(x)
    k = int(f(f(x * f(0.63661977)) + f(half)))
    fk = f(k)
    r = f(f(f(x - f(fk * f(1.5703125))) - f(fk * f(4.837512969970703125e-4))) - f(fk * f(7.54978995489188216e-8)))
    z = f(r * r)
    sp = f(f(f(f(f(f(f(f(-1.9515295891e-4) * z) + f(8.3321608736e-3)) * z) - f(1.6666654611e-1)) * z) * r) + r)
    cp = f(f(f(f(f(f(f(f(f(2.443315711809948e-5) * z) - f(1.388731625493765e-3)) * z) + f(4.166664568298827e-2)) * z) * z) - f(f(0.5) * z)) + f(1.0))
    return ((sp, cp), (cp, -sp), (-sp, -cp), (-cp, sp))[k & 3] + (k,)


@functools.lru_cache(maxsize=None)
def brief_pattern():
    import os
    rows = [[int(v) for v in l.split()] for l in open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orb_bit_pattern_31.txt")) if l.strip() and not l.startswith("#")]
    return np.array(rows[:256], np.float32)


def steer_model(blurred, x, y, angle, half=0.5):
    """the 256 steered tests on a blurred level in numpy's float32, with sincos_model(., half)"""
    f = np.float32
    b, a, _ = sincos_model(f(f(angle) * f(0.017453292)), half)
    p = brief_pattern()
    rot = lambda px, py: (np.rint((px * a).astype(f) - (py * b).astype(f)).astype(int), np.rint((px * b).astype(f) + (py * a).astype(f)).astype(int))
    (x0, y0), (x1, y1) = rot(p[:, 0], p[:, 1]), rot(p[:, 2], p[:, 3])
    return np.packbits((blurred[y + y0, x + x0] < blurred[y + y1, x + x1]).astype(np.uint8), bitorder="little")


# ---------------------------------------------------------------------------------------------------------------------------------------
# blur
# ---------------------------------------------------------------------------------------------------------------------------------------
def blur_positions(w=W0, h=H0):
    """every x residue modulo 16 (k_describe's window DMA starts at any byte) and the four corners of the interior"""
    pos = [(31, 31), (w - 32, 31), (31, h - 32), (w - 32, h - 32)]
    for j, y in enumerate((31, 44, 57, 70, 83, 96)):
        pos += [(x, y) for x in range(31 + 2 * j + (10 if y in (31, 96) else 0), w - 32 - (10 if y in (31, 96) else 0), 9)]
    return sorted(set(pos), key=lambda p: (p[1], p[0]))


def blur_scenes():
    out = []
    rng = np.random.RandomState(4711)

    def dotted(img, name, part):
        for x, y in blur_positions():
            img[y, x] = 255 if img[y - 3:y + 4, x - 3:x + 4].max() < 128 else 0
        out.append(make(name, "blur", [img], nfeats=200, part=part))

    for base in (0, 100, 235):              # (a) textures of range th: no corner of their own, Gaussian sums on both sides of every half
        dotted((base + rng.randint(0, TH + 1, (H0, W0))).astype(np.uint8), "blur-texture-%d" % base, "a")
        dotted((base + np.kron(rng.randint(0, TH + 1, (H0 // 2, W0 // 2)), np.ones((2, 2), np.int64))).astype(np.uint8), "blur-blocks-%d" % base, "a")
    for base in (255, 0):                   # (b) every blurred pixel away from the dots is 257 (saturated to 255), or 0
        dotted(np.full((H0, W0), base, np.uint8), "blur-flat-%d" % base, "b")
    xx, yy = np.meshgrid(np.arange(W0), np.arange(H0))
    dotted((3 * np.abs((xx + 20) % 170 - 85)).astype(np.uint8), "blur-ramp-x", "c")            # (c) slope 3, 0 .. 255 under the windows
    dotted((3 * np.abs((yy + xx // 4 + 50) % 170 - 85)).clip(0, 255).astype(np.uint8), "blur-ramp-y", "c")
    return out


def gauss_blur(img):
    """the oracle's blur of a whole level in numpy: taps GAUSS7 both ways in integers, one rounding (s + 2^15) >> 16, saturated (the
    border is replicated: no keypoint's window reaches it)"""
    a = np.pad(img.astype(np.int64), 3, mode="edge")
    h = sum(g * a[:, k:k + img.shape[1]] for k, g in enumerate(GAUSS7))
    v = sum(g * h[k:k + img.shape[0], :] for k, g in enumerate(GAUSS7))
    return np.minimum((v + 32768) >> 16, 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------------------
# levels
# ---------------------------------------------------------------------------------------------------------------------------------------
LEVEL_SIZES = ((152, 76), (154, 77), (155, 78), (157, 78), (186, 116))       # level 1: 127x63, 128x64, 129x65, 131x65, 155x97 (then 129x81)


def level_xy(k, scales):
    """level coordinates of keypoints (their x, y are level coordinates times the level's float scale)"""
    sc = np.asarray(scales, np.float32)[k["octave"]]
    return np.rint(k["x"] / sc).astype(np.int64), np.rint(k["y"] / sc).astype(np.int64)


def levels_with_interior(w, h):
    from oracle import oracle
    lw, lh, sc = oracle.pyramid_sizes(w, h, 8)
    return [l for l in range(8) if lw[l] > 2 * EDGE and lh[l] > 2 * EDGE], lw, lh, sc


def on_border(k, l, lw, lh, sc):
    """(a keypoint of level l sits on the first or last interior column, ... row)"""
    x, y = level_xy(k, sc)
    m = k["octave"] == l
    return bool((m & ((x == EDGE) | (x == lw[l] - EDGE - 1))).any()), bool((m & ((y == EDGE) | (y == lh[l] - EDGE - 1))).any())


@functools.lru_cache(maxsize=None)
def blob_image(w, h):
    """squares of 255 on 0 (convex corners: the largest Harris sums) and blobs of 2 x 2 and 3 x 3 pixels, whose level-0 positions are
    searched with the oracle until every level with an interior keeps a keypoint on a border column and on a border row of its interior"""
    from oracle import oracle
    levels, lw, lh, sc = levels_with_interior(w, h)
    img = np.zeros((h, w), np.uint8)
    img[h // 2 - 6:h // 2 + 7, w // 2 - 10:w // 2 + 10] = 255
    img[EDGE, EDGE] = 255; img[h - EDGE - 1, w - EDGE - 1] = 255                          # level 0: single dots on its interior's corners
    img[EDGE, w - EDGE - 1] = 255
    corners = lambda l: [(EDGE, EDGE), (lw[l] - EDGE - 1, EDGE), (EDGE, lh[l] - EDGE - 1), (lw[l] - EDGE - 1, lh[l] - EDGE - 1)]
    for l in levels[1:]:
        done = False
        for tx, ty in corners(l)[(l - 1) % 4:] + corners(l)[:(l - 1) % 4]:
            for size in (3, 2, 4):
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        x0, y0 = int(round((tx + 0.5) * sc[l] - size / 2.0)) + dx, int(round((ty + 0.5) * sc[l] - size / 2.0)) + dy
                        if x0 < 8 or y0 < 8 or x0 + size > w - 8 or y0 + size > h - 8 or img[y0 - 4:y0 + size + 4, x0 - 4:x0 + size + 4].any():
                            continue
                        trial = img.copy()
                        trial[y0:y0 + size, x0:x0 + size] = 255
                        k, _ = oracle.orb_detect(trial, 500, 8, TH)
                        if all(all(on_border(k, m, lw, lh, sc)) for m in levels[:levels.index(l) + 1]):
                            img, done = trial, True
                            break
                    if done: break
                if done: break
            if done: break
        assert done, ("no blob puts a keypoint on the interior's border", w, h, l)
    return img


def levels_scenes():
    out = []
    for w, h in LEVEL_SIZES:
        rng = np.random.RandomState(w * 1000 + h)
        xx, yy = np.meshgrid(np.arange(w), np.arange(h))
        last = np.full((h, w), 90, np.uint8)
        last[:, -1] = 255; last[-1, :] = 0                                            # flat but for its last column and row: the clamped taps
        contents = (("blobs", blob_image(w, h)), ("noise", rng.randint(0, 256, (h, w))), ("white", np.full((h, w), 255)), ("columns", (xx & 1) * 255),
                    ("rows", (yy & 1) * 255), ("checker", ((xx + yy) & 1) * 255), ("lastline", last))
        for nm, img in contents:
            out.append(make("levels-%dx%d-%s" % (w, h, nm), "levels", [img], nlevels=8, nfeats=500, content=nm))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# spacing
# ---------------------------------------------------------------------------------------------------------------------------------------
def spacing_scenes():
    """pairs of dots min_distance - 1, min_distance and min_distance + 1 apart in x, in y and diagonally, equal and unequal, the first dot at
    every phase of the NMS grid's cells (their side is min_distance / 2, rounded down).  The reference's grid only ever lets a keypoint
    suppress the four cells next to its own, that is up to 2 cells - 1 pixels away and never min_distance - 1: so the distances of one
    cell, one cell + 1 and two cells - 1 are here as well, where the decision does fall on both sides"""
    out = []
    for md in (3, 7):
        cell, pitch = md // 2, 12 if md == 3 else 16
        slots = [(x, y) for y in range(34, H0 - EDGE - md - 2, pitch) for x in range(34, W0 - EDGE - md - 2, pitch)]
        imgs, k = [np.zeros((H0, W0), np.uint8)], 0
        for dist in sorted({md - 1, md, md + 1, cell, cell + 1, 2 * cell - 1} - {0, 1}):
            for i, j in ((1, 0), (0, 1), (1, 1)):
                for da, db in ((200, 200), (200, 120), (120, 200)):
                    for ph in range(cell):
                        if k == len(slots):
                            imgs.append(np.zeros((H0, W0), np.uint8)); k = 0
                        x, y = slots[k]; k += 1
                        x += (ph - x) % cell; y += (ph - y) % cell
                        imgs[-1][y, x] = da; imgs[-1][y + j * dist, x + i * dist] = db
        for n, img in enumerate(imgs):
            out.append(make("spacing-%d-%d" % (md, n), "spacing", [img], nfeats=200, nms=True, min_distance=md))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
FAMILIES = {"dots": dots_scenes, "cuts": cuts_scenes, "orient": orient_scenes, "blur": blur_scenes, "levels": levels_scenes, "spacing": spacing_scenes}


@functools.lru_cache(maxsize=None)
def scenes(family):
    out = FAMILIES[family]()
    assert len({s["name"] for s in out}) == len(out) and all(s["family"] == family for s in out)
    return out


def scene(name):
    return next(s for s in scenes(name.split("-")[0]) if s["name"] == name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle's lists of a scene, once per process (shared by the tests; never modified)
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_raw(name, which=-1):
    """(keypoints, descriptors) of oracle.orb_detect on image `which` of the scene: the detector's raw list"""
    from oracle import oracle
    s = scene(name)
    return oracle.orb_detect(s["imgs"][which], raw_nfeatures(s), s["orb_nlevels"], s["initial_FAST_threshold"])


@functools.lru_cache(maxsize=None)
def oracle_final(name, which=-1):
    """(keypoints, descriptors) of the final left list after the NMS and the row sort: stage 2 of the whole oracle, the same image on both sides"""
    from oracle import oracle
    from stereo_vo_amd.abi import StereoCamera
    s = scene(name)
    orc = oracle.Oracle(scene_params(oracle.default_params(), s))
    img = s["imgs"][which]
    orc.process(img, img, StereoCamera.simple(200.0, s["w"] / 2.0, s["h"] / 2.0, 0.1, s["w"], s["h"]))
    out = orc.keypoints(0, 0), orc.keypoints(0, 1)
    orc.close()
    assert out[0][0].tobytes() == out[1][0].tobytes()
    return out[0]


@functools.lru_cache(maxsize=None)
def oracle_levels(name, which=-1):
    """the eight levels of the scene's image, oracle.resize chained from it"""
    from oracle import oracle
    s = scene(name)
    lw, lh, _ = oracle.pyramid_sizes(s["w"], s["h"], 8)
    out = [s["imgs"][which]]
    for l in range(1, 8):
        out.append(oracle.resize(out[-1], lw[l], lh[l]))
    return out
