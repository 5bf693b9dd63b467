"""Images built by hand for dmFASTER's detect chain (csrc/k_detect.hip: k_half, k_faster / k_faster_dyn, k_faster_nms =
chunked_grid_nms<FasterKeys>, k_nms_rowsort in its x1/2 mode) -- numpy only.  The photograph, its crops and the block textures of
tests/image_content.py leave to chance which arc of the segment test, which sign of the radicand, which tile seam or which cell of the
NMS grid a frame exercises; here every image is made for one.

A scene is a dict: `img` (uint8, run as the left AND the right image), `w`, `h`, the parameters `t` (initial_FAST_threshold), `win`
(KLT_win), `n_oct`, `nfeats` (orb_nfeats), `md` (min_distance; the NMS setting of the scene -- every scene is also run with the NMS
off), a `family`, a `name`, and -- where construction alone gives the answer -- `expect`:

  expect["centres"]   rings     [(x, y, is a corner)] of every ring cell's centre: a corner iff ONE arc of at least 12 contiguous circle
                                pixels differs from the centre by more than t, all to the same side
  expect["resp"]      response  {(x, y): float32 response} of single-pixel dots at win 1: klt_from_sums(2 a^2, 0, 2 a^2, 1), and +0.0 of
                                the centre of a full ring at win 1 (its 3 x 3 window reads no circle pixel)
  expect["kept"]      nms       the (x, y) the NMS keeps on octave 0, in rank order: dots at pitch 6 and win 1 do not see each other, so
                                the rank is (amplitude desc, raster asc) and grid_walk below -- m_non_max_sup once more -- gives the rest

Geometry the positions come from: k_faster's 64 x 32 tiles from (3, 3) (seams at x = 66 | 67, 130 | 131, y = 34 | 35, 66 | 67), one
column per thread and rows (y - 3) % 4 + 4 k, the halo max(3, win + 1), the border rule of the response win + 1 <= x < w - win - 1, the
cells of int(md / 2) pixels of the NMS grid and its chunks of 2048 corners.  tests/test_faster_scenes_cpu.py holds tests/faster_ref.py
to `expect` and guards that every scene has what it is named for; tests/test_gpu_faster_scenes.py runs the kernels."""
import functools

import numpy as np

import faster_ref as F

W0, H0 = 200, 104                           # three tile columns (64, 64, 64 + 2 more) and four tile rows (32, 32, 32, 2)
FK_W, FK_H, CHUNK = 64, 32, 2048


def make(name, family, img, t=20, win=4, n_oct=1, nfeats=500, md=3, expect=None, **more):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    return dict(name=name, family=family, img=img, w=w, h=h, t=t, win=win, n_oct=n_oct, nfeats=nfeats, md=md, expect=expect or {}, **more)


def scene_params(base, s, nms=True, t=None):
    """the scene's parameters over hip.default_params(): the reference's dmFASTER configuration with the scene's fields"""
    p = F.faster_params(base, t=s["t"] if t is None else t, orb_nfeats=s["nfeats"], n_oct=s["n_oct"], nms=int(nms))
    p.min_distance = s["md"]
    return p


def klt_rad(gxx, gxy, gyy, win):
    """the radicand t t - 4 de of the response, with klt_from_sums' operators"""
    f = np.float32
    side = 2 * int(win) + 1
    K = f(0.5) / f(side * side)
    Gxx, Gxy, Gyy = f(np.int32(gxx)) * K, f(np.int32(gxy)) * K, f(np.int32(gyy)) * K
    t = Gxx + Gyy
    de = Gxx * Gyy - Gxy * Gxy
    return f(t * t - f(4.0) * de)


def grid_walk(kps, md, w, h, cap):
    """m_non_max_sup (stage2_detect.cpp:296-370) on (x, y, response) triples in detector (raster) order, in plain Python: returns
    (kept indices in rank order, rank order, {index: the indices whose acceptance occupied its cell first} for the rejected ones).  The
    rank is (response desc, index asc); float32 expressions as the reference writes them"""
    f = np.float32
    order = sorted(range(len(kps)), key=lambda i: (-float(kps[i][2]), i))
    cell = int(md / 2.0)
    inv = f(1.0) / f(cell)
    glx, gly = int(f(1) + f(w) * inv), int(f(1) + f(h) * inv)
    occ, kept, blockers = {}, [], {}
    for i in order:
        if len(kept) >= cap:
            break
        sx, sy = int(f(kps[i][0]) * inv), int(f(kps[i][1]) * inv)
        if (sx, sy) in occ:
            blockers[i] = list(occ[sx, sy])
            continue
        for c in ((sx, sy), (sx - 1, sy), (sx, sy - 1), (sx + 1, sy), (sx, sy + 1)):
            if 0 <= c[0] < glx and 0 <= c[1] < gly:
                occ.setdefault(c, []).append(i)
        kept.append(i)
    return kept, order, blockers


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. rings: the segment test
# ---------------------------------------------------------------------------------------------------------------------------------------
def _arc(ring, start, length, v):
    for k in range(length):
        ring[(start + k) % 16] = v


def ring_cases(t, c):
    """[(centre value, the 16 circle values clockwise from the top, is a corner)] on a background c"""
    out = []
    for sgn in (1, -1):
        for d in (t, t + 1):
            v = c + sgn * d
            if not 0 <= v <= 255:
                continue
            for length in (11, 12, 13, 16):
                for start in range(16 if length < 16 else 1):          # every start: the wrapping arcs, and at 12 the four that leave out one cardinal pixel each
                    ring = [c] * 16
                    _arc(ring, start, length, v)
                    out.append((c, ring, length >= 12 and d > t))
    hi, lo = c + t + 1, c - t - 1
    if hi <= 255 and lo >= 0:
        for start in (0, 3, 6, 11, 14):
            ring = [c] * 16                                                # 6 brighter and 6 darker, contiguous
            _arc(ring, start, 6, hi); _arc(ring, start + 6, 6, lo)
            out.append((c, ring, False))
            ring = [c] * 16                                                # 8 and 8: every circle pixel clears the threshold, no arc of 12 on one side
            _arc(ring, start, 8, hi); _arc(ring, start + 8, 8, lo)
            out.append((c, ring, False))
    for v in (hi, lo):
        if 0 <= v <= 255:
            for start in (0, 2, 7, 13):
                ring = [c] * 16                                            # two arcs of 6 with gaps of 2 between them
                _arc(ring, start, 6, v); _arc(ring, start + 8, 6, v)
                out.append((c, ring, False))
                ring = [c] * 16                                            # 14 of 16 as arcs of 11 and 3: the count is there, the run is not
                _arc(ring, start, 11, v); _arc(ring, start + 12, 3, v)
                out.append((c, ring, False))
                ring = [v] * 16                                            # all but one pixel: an arc of 15 that wraps
                ring[start] = c
                out.append((c, ring, True))
    # the four compass pixels beyond the threshold, the rest of the arc exactly on it: the cardinal pre-test passes, the arc does not
    for sgn in (1, -1):
        on, beyond = c + sgn * t, c + sgn * (t + 1)
        if 0 <= beyond <= 255:
            for length, start in ((12, 0), (12, 3), (13, 6), (13, 15), (16, 0)):
                ring = [c] * 16
                _arc(ring, start, length, on)
                ring = [beyond if i % 4 == 0 and v == on else v for i, v in enumerate(ring)]
                out.append((c, ring, False))
    # saturated centres: nothing can be brighter than 255 - t or darker than t, whatever the arc; one grey level further it can
    for cc, v in ((255 - t, 255), (255 - t + 1, 255), (254 - t, 255), (255, 255), (t, 0), (t - 1, 0), (t + 1, 0), (0, 0), (0, t), (0, t + 1), (255, 255 - t), (255, 254 - t)):
        if 0 <= cc <= 255 and 0 <= v <= 255:
            out.append((cc, [v] * 16, abs(v - cc) > t))
    return out


RING_XS = lambda w: (3, 66, 67, 130, 131, w - 4, w - 3)                    # noqa: E731   (w - 3, h - 3: one beyond the last valid ones, never listed)
RING_YS = lambda h: (3, 34, 35, 66, 67, h - 4, h - 3, 4, 5, 6, 31, 32, 33)  # noqa: E731   ((y - 3) % 4: every residue; (y - 3) % 32 in 0 .. 3 and 28 .. 31)


class RingCanvas:
    def __init__(self, c, w=W0, h=H0):
        self.c, self.w, self.h, self.img, self.cells = c, w, h, np.full((h, w), c, np.uint8), []

    def fits(self, x, y):
        return all(max(abs(x - a), abs(y - b)) >= 8 for a, b, _ in self.cells)

    def add(self, x, y, case):
        cc, ring, corner = case
        self.img[max(0, y - 3):y + 4, max(0, x - 3):x + 4] = cc
        for (dx, dy), v in zip(F.CIRCLE, ring):
            if 0 <= x + dx < self.w and 0 <= y + dy < self.h:
                self.img[y + dy, x + dx] = v
        self.cells.append((x, y, bool(corner) and 3 <= x < self.w - 3 and 3 <= y < self.h - 3))


def ring_canvases(t, c, xs, ys, w=W0, h=H0):
    """every case on a background c: the special positions first, each on the first canvas that has room 8 pixels from every other cell,
    then a 9-pixel grid filled with the cases in turn"""
    cases, out, n = ring_cases(t, c), [], 0
    good, bad = [k for k in cases if k[2]], [k for k in cases if not k[2]]      # at the special positions: two corners, then a near miss
    for y in ys:
        for x in xs:
            for cv in out:
                if cv.fits(x, y):
                    break
            else:
                cv = RingCanvas(c, w, h)
                out.append(cv)
            cv.add(x, y, (bad if n % 3 == 2 else good)[(7 * n) % len(bad if n % 3 == 2 else good)])
            n += 1
    n, k = 0, 0
    while k < len(out) or n < len(cases):
        if k == len(out):
            out.append(RingCanvas(c, w, h))
        for y in range(12, h - 12, 9):
            for x in range(12, w - 12, 9):
                if out[k].fits(x, y):
                    out[k].add(x, y, cases[n % len(cases)])
                    n += 1
        k += 1
    assert n >= len(cases), (t, c, n, len(cases))
    return out


def rings_scenes():
    out = []
    for t, c, xs, ys in ((20, 100, RING_XS(W0), RING_YS(H0)), (1, 100, (3, 67, W0 - 4), (3, 35, H0 - 4)), (254, 0, (3, 66, W0 - 4), (3, 34, H0 - 4)), (254, 255, (67, W0 - 3), (35, H0 - 3))):
        for k, cv in enumerate(ring_canvases(t, c, xs, ys)):
            out.append(make("rings-t%d-c%d-%d" % (t, c, k), "rings", cv.img, t=t, win=4, expect={"centres": list(cv.cells)}))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. response
# ---------------------------------------------------------------------------------------------------------------------------------------
def dot_response(a):
    return np.float32(F.klt_from_sums(2 * a * a, 0, 2 * a * a, 1))


def paint_full_ring(img, x, y, v):
    for dx, dy in F.CIRCLE:
        img[y + dy, x + dx] = v


def lattice(w, h, pitch=6, x0=3, y0=3):
    """dot positions at `pitch` from (x0, y0), inside the segment test's range, in raster order"""
    return [(x, y) for y in range(y0, h - 3, pitch) for x in range(x0, w - 3, pitch)]


def clamp_patch(seed, win):
    """a (2 win + 3)^2 patch: a full ring of level + 40 over a random flat level and up to three faint pixels within one pixel of
    the centre.  Its centre is a corner at t = 20; `seed` is what a search kept because the radicand there is negative"""
    rng = np.random.RandomState(seed)
    r = win + 1
    level = int(rng.randint(30, 200))
    p = np.full((2 * r + 1, 2 * r + 1), level, np.uint8)
    paint_full_ring(p, r, r, level + 40)
    for _ in range(int(rng.randint(1, 4))):
        p[r + rng.randint(-1, 2), r + rng.randint(-1, 2)] = level + rng.randint(-3, 4)
    return p


# the first seeds of 0 .. 19999 at which clamp_patch(seed, win) has a negative radicand at its centre (the search itself is not kept: the CPU
# test recomputes the radicand)
CLAMP_SEEDS = {2: (393, 980, 1554, 1595), 4: (1554, 1643, 2137, 2746)}


def negative_patch(p, q, amps, level=100, ring=140):
    """7 x 7: a full ring around a flat level, and one gradient (p a, q a) at each of the four diagonal pixels of the centre's 3 x 3
    window (a = amps, clockwise from the lower right), painted on the eight pixels (+-2, +-1), (+-1, +-2) that no other difference of
    the window reads.  At win 1 the sums are B (p p, p q, q q) with B = sum a a: a matrix of rank one, whose determinant
    Gxx Gyy - Gxy Gxy rounds below zero for the (p, q, B) of NEGATIVE_CELLS, and with it the response"""
    out = np.full((7, 7), level, np.int32)
    paint_full_ring(out, 3, 3, ring)
    for (u, v), a in zip(((1, 1), (-1, 1), (-1, -1), (1, -1)), amps):
        out[3 + v, 3 + 2 * u] = level + u * p * a                  # dx at (u, v) = u (I(2 u, v) - I(0, v))
        out[3 + 2 * v, 3 + u] = level + v * q * a                  # dy at (u, v) = v (I(u, 2 v) - I(u, 0))
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


# (x, y, p, q, amps): responses -2^-22, -2^-21 (through two different sums), -2^-20 (two), -2^-19, -2^-18 from an enumeration of
# klt_from_sums(p p B, p q B, q q B, 1) over p, q <= 6 and B < 40; the equal ones stand on both sides of the seams
NEGATIVE_CELLS = ((66, 34, 1, 3, (3, 2, 0, 0)), (20, 12, 1, 3, (3, 2, 0, 0)), (131, 67, 1, 3, (0, 0, 3, 2)),
                  (67, 66, 2, 3, (3, 2, 0, 0)), (40, 14, 3, 2, (3, 3, 1, 0)), (130, 35, 2, 3, (2, 0, 3, 0)),
                  (100, 50, 2, 6, (3, 2, 0, 0)), (160, 20, 3, 4, (3, 3, 1, 0)), (60, 85, 4, 6, (3, 2, 0, 0)), (150, 80, 5, 6, (3, 3, 2, 0)))


def noise(w, h, seed, block=1):
    rng = np.random.RandomState(seed)
    cells = rng.randint(0, 256, ((h + block - 1) // block, (w + block - 1) // block)).astype(np.uint8)
    return np.ascontiguousarray(np.kron(cells, np.ones((block, block), np.uint8))[:h, :w])


BORDER_SEEDS = {1: 0, 4: 0, 15: 0}          # noise whose corners stand on every column and row next to the border rule (searched)
SEAM_SEED = 0                               # noise with corners on 66, 67 and on rows 34, 35, inside the border rule of win 15


def border_columns(w, win):
    return [v for v in (win, win + 1, w - win - 2, w - win - 1) if 3 <= v < w - 3]


def equal_patch_positions():
    return [(12, 10), (62, 30), (126, 50), (160, 20), (30, 62), (150, 80)]          # (62, 30): over x = 66 | 67 and y = 34 | 35; (126, 50) and (30, 62): over one seam each


def response_scenes():
    out = []
    # dots: one image holds every amplitude from t + 1 to 255 over a background of 0, 20 or 200
    for b, t in ((0, 20), (20, 20), (200, 1), (0, 254)):
        img, resp = np.full((H0, W0), b, np.uint8), {}
        for (x, y), a in zip(lattice(W0, H0), range(t + 1, 256 - b)):
            img[y, x] = b + a
            resp[x, y] = dot_response(a)
        assert len(resp) == 255 - b - t
        out.append(make("response-dots-b%d-t%d" % (b, t), "response", img, t=t, win=1, expect={"resp": resp}))
    # full rings at win 1: computed +0.0, among dots (positive) -- several of them, the last ranks of the list: position orders equal computed zeros
    img, resp = np.full((H0, W0), 60, np.uint8), {}
    for x, y in ((3, 3), (66, 34), (131, 35), (67, 66), (W0 - 4, H0 - 4), (100, 50)):
        paint_full_ring(img, x, y, 130)
        resp[x, y] = np.float32(0.0)
    for k, (x, y) in enumerate(((30, 20), (90, 20), (30, 80), (160, 60))):
        img[y, x] = 60 + 30 + k
        resp[x, y] = dot_response(30 + k)
    n = len(F.fast12(img, 20)[0])
    out.append(make("response-zero-rings", "response", img, win=1, md=3, nfeats=(n - 3) // 2, expect={"resp": resp}))      # the cap cuts inside the group of zeros
    # the clamp: patches whose centre has a negative radicand, on a flat canvas
    for win, seeds in sorted(CLAMP_SEEDS.items()):
        if seeds:
            img, at, r = np.full((H0, W0), 90, np.uint8), [], win + 1
            for k, seed in enumerate(seeds):
                x, y = (60 + 14 * k, 30 + 3 * k) if k < 6 else (20 + 14 * (k - 6), 70)
                img[y - r:y + r + 1, x - r:x + r + 1] = clamp_patch(seed, win)
                at.append((x, y))
            out.append(make("response-clamp-win%d" % win, "response", img, win=win, centres=at))
    # negative responses: ten of five values after the computed zeros of two plain rings and the positive ones of dots; the cap cuts among them
    img, at = np.full((H0, W0), 100, np.uint8), []
    for x, y, p, q, amps in NEGATIVE_CELLS:
        img[y - 3:y + 4, x - 3:x + 4] = negative_patch(p, q, amps)
        at.append((x, y))
    for x, y in ((90, 20), (30, 60)):
        paint_full_ring(img, x, y, 140)
    for k, (x, y) in enumerate(((180, 50), (110, 90), (10, 90))):
        img[y, x] = 100 + 30 + k
    n = len(F.fast12(img, 20)[0])
    out.append(make("response-negative", "response", img, win=1, md=3, nfeats=(n - 5) // 2, centres=at, zeros=[(90, 20), (30, 60)]))
    # the largest sums: 0 / 255 blocks and stripes of 2 px under win 15
    rng = np.random.RandomState(7)
    blocks = noise(W0, H0, 3, block=2) // 128 * 255
    stripes = np.tile(np.repeat(np.array([0, 255], np.uint8), 2), (H0, W0 // 4))
    flip = np.kron(rng.rand(H0 // 2, W0 // 2) < 0.08, np.ones((2, 2), bool))
    out.append(make("response-blocks2-win15", "response", blocks, win=15))
    out.append(make("response-stripes2-win15", "response", np.where(flip, 255 - stripes, stripes), win=15))
    # the border rule and the seams: noise up to the image edge
    for win, seed in sorted(BORDER_SEEDS.items()):
        out.append(make("response-border-win%d" % win, "response", noise(W0, H0, seed), win=win))
    out.append(make("response-seams-win15", "response", noise(W0, H0, SEAM_SEED), win=15))
    # equal responses: one 9 x 9 patch at several places, flat around it -- position decides
    patch = noise(9, 9, 5)
    img = np.full((H0, W0), 128, np.uint8)
    for x, y in equal_patch_positions():
        img[y:y + 9, x:x + 9] = patch
    k = F.corners(img, 20, 4)
    for md in (3, 7):                                                            # the smallest even cap from 20 on that cuts inside a group of equal responses
        kept, _, _ = grid_walk(list(zip(k["x"].tolist(), k["y"].tolist(), k["response"].tolist())), md, W0, H0, len(k))
        cap = next(c for c in range(20, len(kept), 2) if k["response"][kept[c - 1]] == k["response"][kept[c]])
        out.append(make("response-equal-md%d" % md, "response", img, win=4, md=md, nfeats=cap // 2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. sizes
# ---------------------------------------------------------------------------------------------------------------------------------------
# w, h, octaves, win.  (A 13 x 9 frame is refused -- frames are 64 x 64 at least --, so the 13 x 9 image with its interior of 7 x 3 is octave 3 of 104 x 72.)
SIZES = ((198, 102, 3, 4), (199, 103, 3, 4), (135, 135, 3, 15), (135, 71, 3, 15), (104, 72, 4, 4))
SIZE_T = 25
SIZE_SEEDS = {(198, 102): 0, (199, 103): 0, (135, 135): 7, (135, 71): 0, (104, 72): 0}                   # block noise, searched (see test_faster_scenes_cpu.py for what each has)
RING2_SIZES = ((198, 102), (199, 103))


def edge_flat(w, h):
    img = np.full((h, w), 100, np.uint8)
    img[:, w - 1] = 255
    img[h - 1, :] = 0
    return img


@functools.lru_cache(maxsize=None)
def rings2(w, h):
    """full rings of family 1 scaled by two (the circle's pixels as 2 x 2 blocks of 255 over 90) around the level-0 pixels that the x1/2
    octave's corners of its valid range, the middles of its sides and its centre come from; the phase of each (0 or 1 in x and y) is
    searched with the reference until octave 1 has a corner exactly there"""
    img = np.full((h, w), 90, np.uint8)
    w1, h1 = F.pyramid(img, 2)[1].shape[::-1]
    for x1, y1 in ((3, 3), (w1 - 4, 3), (3, h1 - 4), (w1 - 4, h1 - 4), (w1 // 2, 3), (w1 // 2, h1 - 4), (3, h1 // 2), (w1 - 4, h1 // 2), (w1 // 2, h1 // 2)):
        for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            trial = img.copy()
            for dx, dy in F.CIRCLE:
                y, x = 2 * (y1 + dy) + oy, 2 * (x1 + dx) + ox
                trial[max(0, y):max(0, y + 2), max(0, x):max(0, x + 2)] = 255
            xs, ys = F.fast12(F.pyramid(trial, 2)[1], 20)
            if ((xs == x1) & (ys == y1)).any():
                img = trial
                break
        else:
            raise AssertionError(("no phase leaves a corner on octave 1", w, h, x1, y1))
    return img


def sizes_scenes():
    out = []
    for w, h, n_oct, win in SIZES:
        out.append(make("sizes-%dx%d-noise" % (w, h), "sizes", noise(w, h, SIZE_SEEDS[w, h], 4), win=win, n_oct=n_oct, t=SIZE_T))
        out.append(make("sizes-%dx%d-edges" % (w, h), "sizes", edge_flat(w, h), win=win, n_oct=n_oct, none=True))
        if (w, h) in RING2_SIZES:
            out.append(make("sizes-%dx%d-rings2" % (w, h), "sizes", rings2(w, h), win=win, n_oct=n_oct))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. nms: dot lattices at win 1 and pitch 6
# ---------------------------------------------------------------------------------------------------------------------------------------
def dots_image(w, h, plan, b=0):
    img = np.full((h, w), b, np.uint8)
    for x, y, a in plan:
        img[y, x] = b + a
    return img


def plan_kept(plan, md, w, h, cap):
    """the (x, y) the NMS keeps of a plan [(x, y, amplitude)] (any order), in rank order"""
    plan = sorted(plan, key=lambda d: (d[1], d[0]))
    kept, _, _ = grid_walk([(x, y, float(dot_response(a))) for x, y, a in plan], md, w, h, cap)
    return [(plan[i][0], plan[i][1]) for i in kept]


def spiral(nx, ny):
    """the cells of an nx x ny lattice from the outside in"""
    out, x0, y0, x1, y1 = [], 0, 0, nx - 1, ny - 1
    while x0 <= x1 and y0 <= y1:
        out += [(x, y0) for x in range(x0, x1 + 1)] + [(x1, y) for y in range(y0 + 1, y1 + 1)]
        if y1 > y0:
            out += [(x, y1) for x in range(x1 - 1, x0 - 1, -1)]
        if x1 > x0:
            out += [(x0, y) for y in range(y1 - 1, y0, -1)]
        x0, y0, x1, y1 = x0 + 1, y0 + 1, x1 - 1, y1 - 1
    return out


def chunk_plan(rows, extra=0):
    """64 x rows dots at pitch 6 whose amplitude falls by one along every row and by two from row to row (+ `extra` dots of amplitude 21
    in the next row, from its second column on: under dots that are accepted): the 2048th rank falls inside a row"""
    plan = [(3 + 6 * c, 3 + 6 * r, 255 - c - 2 * r) for r in range(rows) for c in range(64)]
    return plan + [(9 + 6 * c, 3 + 6 * rows, 21) for c in range(extra)]


def nms_scenes():
    out = []

    def add(name, plan, w, h, md, nfeats=500, n_oct=1, b=0, **more):
        cap = F.kps_to_detect(nfeats, n_oct)[0]
        out.append(make("nms-" + name, "nms", dots_image(w, h, plan, b), win=1, md=md, nfeats=nfeats, n_oct=n_oct, plan=sorted(plan, key=lambda d: (d[1], d[0])),
                        expect={"kept": plan_kept(plan, md, w, h, cap)}, **more))

    row = [(9 + 6 * k, 9) for k in range(60)]
    falling, rising, equal = [(x, y, 255 - 2 * k) for k, (x, y) in enumerate(row)], [(x, y, 137 + 2 * k) for k, (x, y) in enumerate(row)], [(x, y, 99) for x, y in row]
    add("row-falling", falling, 384, 64, 13)              # accept, reject, accept, ...: every decision waits for the one before
    add("row-rising", rising, 384, 64, 13)
    add("row-equal", equal, 384, 64, 13)
    sp = spiral(32, 16)
    add("spiral", [(3 + 6 * x, 5 + 6 * y, 255 - (k * 234) // len(sp)) for k, (x, y) in enumerate(sp)], W0, H0, 13)
    add("md2", falling, 384, 64, 2)
    add("md3", falling, 384, 64, 3)
    # caps: inside a group of equal amplitudes (10 of 30), right behind an accepted corner of the falling row (the next rank is a reject), at 1
    add("cap-equal-10", equal, 384, 64, 13, nfeats=5)
    add("cap-falling-14", falling, 384, 64, 13, nfeats=7)
    add("cap-1", falling + [(x, y + 18, a) for x, y, a in rising], 384, 64, 13, nfeats=1, n_oct=2)
    # chunks of 2048
    add("chunks-2560", chunk_plan(40), 385, 241, 13, nfeats=2000, big=True)
    add("chunks-2048", chunk_plan(32), 385, 193, 13, nfeats=2000, big=True)
    add("chunks-2049", chunk_plan(32, 1), 385, 199, 13, nfeats=2000, big=True)
    # the row table
    add("rows-first-last", [(9 + 12 * k, 3, 60 + k) for k in range(15)] + [(15 + 12 * k, H0 - 4, 90 - k) for k in range(15)], W0, H0, 13, b=100)
    out.append(make("nms-none", "nms", np.full((H0, W0), 77, np.uint8), win=1, md=13, none=True, expect={"kept": []}))
    # cells of 3 and 2 pixels that hold 2, 3 and 4 corners: full rings (4-adjacent corners at (-3, -1), (-3, 0), (-3, 1), ...), pairs of
    # dots 1 or 2 pixels apart, triples and squares, at a pitch of 13 x 11 that walks every phase of either grid.  Expected lists: the oracle's
    img = np.full((H0, W0), 40, np.uint8)
    offs = ((1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (1, 2), (-1, 1))
    k = 0
    for j, y in enumerate(range(8, H0 - 10, 11)):
        for i, x in enumerate(range(8, W0 - 12, 13)):
            kind, a = (i + 2 * j) % 6, 60 + (k * 11) % 150
            if kind == 0:
                paint_full_ring(img, x + 2, y + 1, 40 + 30 + (k * 7) % 150)
            elif kind in (1, 2):                                              # a strong dot and two weaker ones 3 and 4 pixels away: the pair's cell has its
                dx, dy = (1, 0) if kind == 1 else (0, 1)                      # representative rejected by the strong dot's cell, the other one behind it
                img[y, x], img[y + 3 * dy, x + 3 * dx], img[y + 4 * dy, x + 4 * dx] = 40 + a, 40 + a - 25 - k % 7, 40 + a - 30 - k % 5
            elif kind == 3:                                                   # four dots in a square, on odd and on even columns and rows: one cell holds 1, 2 or 4
                img[y + j % 2:y + j % 2 + 2, x + j % 2:x + j % 2 + 2] = [[40 + a, 40 + a - 3 - k % 4], [40 + a + 2 - k % 5, 40 + a - 6]]
            elif kind == 5:                                                   # three dots in an L, likewise: 1, 2 or 3 in a cell
                sx, sy = x + j % 2, y + j % 2
                img[sy, sx], img[sy, sx + 1], img[sy + 1, sx] = 40 + a, 40 + a - 4 - k % 3, 40 + a + 3 - k % 7
            else:
                dx, dy = offs[k % 8]
                img[y, x], img[y + dy, x + dx] = 40 + a, 40 + max(21, (a + (-9, 0, 13)[k % 3]) % 215)
            k += 1
    for md in (7, 4):
        out.append(make("nms-dense-md%d" % md, "nms", img, win=1, md=md, nfeats=2000))
    return out


FAMILIES = {"rings": rings_scenes, "response": response_scenes, "sizes": sizes_scenes, "nms": nms_scenes}


@functools.lru_cache(maxsize=None)
def scenes(family):
    return tuple(FAMILIES[family]())


@functools.lru_cache(maxsize=None)
def scene(name):
    return next(s for f in FAMILIES for s in scenes(f) if s["name"] == name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the reference's lists, computed once per (scene, NMS setting, thresholds) and shared by every test
# ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pyramid(name):
    s = scene(name)
    return tuple(F.pyramid(s["img"], s["n_oct"]))


@functools.lru_cache(maxsize=None)
def reference(name, nms, thresholds=None):
    """per octave (keypoints, row table, raw corner count) of the scene's image: faster_ref.detect at the scene's threshold, or at
    `thresholds` (one per octave)"""
    s = scene(name)
    keep = F.kps_to_detect(s["nfeats"], s["n_oct"])
    return tuple(F.detect(im, s["t"] if thresholds is None else thresholds[o], s["win"], keep[o], s["md"], bool(nms)) for o, im in enumerate(pyramid(name)))


def feats(name, nms, thresholds=None):
    """the reference's lists in the layout of faster_ref.faster_features: `thresholds` = (left per octave, right per octave)"""
    l = reference(name, nms, None if thresholds is None else tuple(thresholds[0]))
    r = reference(name, nms, None if thresholds is None else tuple(thresholds[1]))
    return [(a[0], b[0], a[1], b[1], im, im, a[2], b[2]) for a, b, im in zip(l, r, pyramid(name))]
