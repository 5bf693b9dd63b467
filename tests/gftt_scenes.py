"""Hand-built inputs for svo_gftt_detect: deterministic, numpy only, images of at most 321 x 243.  Every scene is named after the property
it is built for; tests/test_gftt_scenes_cpu.py pins that the walk (tests/gftt_ref.py) really takes that branch, tests/test_gpu_gftt.py
holds the device to the walk on all of them.

The building block is a DOT: one bright pixel on black.  With block 3 its response is 12 * amp^2 at the dot and smaller around it, so a
dot is exactly one candidate of known strength; dots at least 4 pixels apart do not touch each other's candidate test.  k_gftt_response
works in tiles of 32 x 32 pixels, k_gftt_candidates in tiles of 64 x 4: the seam scenes put structure on every multiple of those."""
import functools
import numpy as np

import gftt_ref

MAX_KPS = 512          # the context the GPU tests create
MAX_CAND = 1 << 15     # ... with room for 32768 candidates per job
F = np.float32


class Scene:
    """one svo_gftt_detect call: jobs = [(image, seeds or None, cap)], params = GfttParams keyword arguments; max_cand: the context's
    (None: MAX_CAND)"""
    def __init__(self, name, jobs, max_cand=None, **params):
        self.name, self.jobs, self.params, self.max_cand = name, jobs, params, max_cand

    def ref_params(self):
        return gftt_ref.GfttParams(**self.params)

    def cand_cap(self):
        return max(1024, self.max_cand if self.max_cand is not None else MAX_CAND)


def _single(name, img, seeds=None, cap=MAX_KPS, max_cand=None, **params):
    s = None if seeds is None else np.asarray(seeds, F).reshape(-1, 2)
    return Scene(name, [(np.ascontiguousarray(img, np.uint8), s, cap)], max_cand=max_cand, **params)


def dots(w, h, pts, amps, base=0):
    im = np.full((h, w), base, np.uint8)
    for (x, y), a in zip(pts, amps):
        im[y, x] = a
    return im


def blocks(w, h, cell, seed):
    """random grey squares of `cell` pixels: a corner at most of their junctions"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, ((h + cell - 1) // cell, (w + cell - 1) // cell), dtype=np.uint8)
    return np.ascontiguousarray(np.kron(g, np.ones((cell, cell), np.uint8))[:h, :w])


def seam_image(w, h, seed):
    """2 x 2 checker junctions of random contrast centred on every corner and edge midpoint of the 32 x 32 tiles (every second one is a
    64-pixel seam; every one lies on a 4-row seam), over a faint random ground so that no two responses tie by construction"""
    rng = np.random.default_rng(seed)
    im = rng.integers(0, 8, (h, w)).astype(np.int64)
    for y in range(0, h + 1, 16):
        for x in range(0, w + 1, 16):
            if x % 32 and y % 32:
                continue
            a = int(rng.integers(60, 248))
            im[max(y - 2, 0):y, max(x - 2, 0):x] = a
            im[y:y + 2, x:x + 2] = a
    return im[:h, :w].astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _psq():
    """16 x 16 pixels of 0 .. 3: the tensors are small integers, so D = (a - c)^2 + 4 b^2 is often a perfect square with b != 0, or one
    away from one.  The best of 200 random images for that count."""
    rng = np.random.default_rng(7)
    best, best_n = None, -1
    for _ in range(200):
        im = rng.integers(0, 4, (16, 16), dtype=np.uint8)
        a, b, c = gftt_ref.tensor(im, 3)
        d = (a - c) ** 2 + 4 * b * b
        k = np.rint(np.sqrt(d.astype(np.float64))).astype(np.int64)
        n = int(((k * k == d) & (b != 0)).sum() + (np.abs(k * k - d) == 1).sum())
        if n > best_n:
            best, best_n = im, n
    return best


@functools.lru_cache(maxsize=None)
def disagreeing_seeds(cx, cy, md, want=3):
    """float32 seeds on the circle of radius md around the pixel (cx, cy) which the float32 rule of the walk calls NOT closer than md (the
    sum rounds up to md^2) while the same expression in double calls them closer: `want` of them, from one batch of 65536 tries"""
    rng = np.random.default_rng(11)
    md2 = float(md * md)
    ang = rng.uniform(0, 2 * np.pi, 1 << 16)
    sx = (F(cx) - (md * np.cos(ang)).astype(F)).astype(F)
    fx64 = float(cx) - sx.astype(np.float64)
    sy = (cy - np.sqrt(np.maximum(md2 - fx64 * fx64, 0.0))).astype(F)
    fx, fy = F(cx) - sx, F(cy) - sy
    r32 = (fx * fx + fy * fy) < F(md2)
    d64 = fx64 ** 2 + (float(cy) - sy.astype(np.float64)) ** 2 < md2
    idx = np.flatnonzero(~r32 & d64)[:want]
    assert len(idx) == want
    return [(float(sx[i]), float(sy[i])) for i in idx]


def chain_row():
    """70 dots of descending strength 4 pixels apart in a row, min_distance 5: the walk accepts every second one, and each decision waits
    for the one before it"""
    pts = [(20 + 4 * k, 120) for k in range(70)]
    return dots(321, 243, pts, [250 - k for k in range(70)]), pts


def chain_diagonal():
    """50 dots of descending strength (4, 4) apart, min_distance 6 (cells of 6 pixels): the chain crosses cell borders in both axes"""
    pts = [(12 + 4 * k, 10 + 4 * k) for k in range(50)]
    return dots(321, 243, pts, [250 - 2 * k for k in range(50)]), pts


def lattice():
    """a dot every 4 pixels, 79 x 59 of one strength: 9185 candidates (the dots, and plateau pixels between them)"""
    pts = [(x, y) for y in range(4, 240, 4) for x in range(4, 320, 4)]
    return dots(321, 243, pts, [200] * len(pts))


def _build():
    S = []
    # ---- tile seams: last tiles of 1 pixel (97 = 3 * 32 + 1, 65 = 64 + 1 = 16 * 4 + 1) and of tile - 1 (95, 63, 127), 8 x 8, the full size
    for block in (3, 5, 7):
        for (w, h) in ((97, 65), (95, 63), (127, 33), (65, 97), (321, 243)):
            S.append(_single("seams_%dx%d_b%d" % (w, h, block), seam_image(w, h, w + block), block=block, min_distance=3))
        S.append(_single("tiny_8x8_b%d" % block, blocks(8, 8, 3, 5), block=block, min_distance=1))
    # ---- the arithmetic of the response
    quad = np.zeros((48, 64), np.uint8); quad[:24, :32] = 255; quad[24:, 32:] = 255
    chk2 = ((np.indices((48, 64)) // 2).sum(0) % 2 * 255).astype(np.uint8)
    for block in (3, 5, 7):
        S.append(_single("saturated_quadrants_b%d" % block, quad, block=block))
        S.append(_single("saturated_checker2_b%d" % block, chk2, block=block, min_distance=2))
        S.append(_single("perfect_square_b%d" % block, _psq(), block=block, min_distance=2, quality=0.05))
        S.append(_single("flat_b%d" % block, np.full((40, 72), 77, np.uint8), block=block))
    ring = np.full((24, 32), 77, np.uint8); ring[5, 0] = 255             # the one corner lies in the border ring: it sets m, nothing is a candidate
    S.append(_single("border_ring_only", ring))
    # ---- threshold: 12 * 200^2 * 0.25 = 12 * 100^2 exactly
    S.append(_single("threshold_equal_dropped", dots(96, 64, [(30, 30), (60, 30)], [200, 100]), quality=0.25, min_distance=5))
    S.append(_single("threshold_one_level_stronger_kept", dots(96, 64, [(30, 30), (60, 30)], [200, 101]), quality=0.25, min_distance=5))
    # ---- plateaus and ties
    pair = dots(96, 64, [(40, 30), (41, 30)], [180, 180])
    S.append(_single("plateau_adjacent_pair", pair))                                       # both candidates, the second too close
    S.append(_single("plateau_adjacent_pair_md0", pair, min_distance=0))                   # ... and both kept
    ties = dots(128, 96, [(100, 20), (30, 20), (90, 70), (20, 70)], [150] * 4)
    S.append(_single("ties_raster_order", ties))
    S.append(_single("ties_cut_by_max_corners", ties, max_corners=2))
    S.append(_single("ties_cut_by_cap", ties, cap=3))
    # ---- distance: (12, 16) is exactly 20 away, (12, 15) is closer
    S.append(_single("distance_exact_kept", dots(128, 96, [(40, 30), (52, 46), (90, 60), (78, 44)], [200, 190, 180, 170])))
    S.append(_single("distance_inside_dropped", dots(128, 96, [(40, 30), (52, 45), (90, 60), (78, 45)], [200, 190, 180, 170])))
    tex = blocks(321, 243, 5, 3)
    for md in (0, 1, 255):
        S.append(_single("min_distance_%d" % md, tex, min_distance=md))
    S.append(_single("defaults_on_blocks", blocks(321, 243, 9, 4)))
    # ---- decision chains
    S.append(_single("chain_row", chain_row()[0], min_distance=5))
    S.append(_single("chain_diagonal", chain_diagonal()[0], min_distance=6))
    # ---- seeds
    cand = [(50, 50), (100, 50), (150, 50), (200, 50), (50, 120), (100, 120), (150, 120), (200, 120), (250, 120), (250, 50)]
    img = dots(321, 243, cand, [240 - 5 * k for k in range(len(cand))])
    S.append(_single("seeds_exact_and_inside", img, seeds=[(70, 50), (100, 69.5), (150, 50), (200.25, 30.5), (30, 120.0)]))
    S.append(_single("seeds_float32_rule", img, seeds=disagreeing_seeds(100, 120, 20) + disagreeing_seeds(150, 120, 20) + [(50 + 12, 120 + 16)]))
    nan, inf = float("nan"), float("inf")
    S.append(_single("seeds_not_finite", img, seeds=[(nan, 50), (50, nan), (inf, 50), (100, -inf), (nan, nan), (150, 51)]))
    S.append(_single("seeds_outside", img, seeds=[(-0.5, 50), (321, 50), (320.75, 50), (50, -0.001), (50, 243), (250, 242.5), (0, 0),
                                                  (-10, 120), (340, 120), (250, 130)]))
    S.append(_single("seeds_none_but_a_pointer", img, seeds=np.zeros((0, 2), F)))
    S.append(_single("seeds_many_on_blocks", tex, seeds=np.random.default_rng(9).uniform(-5, 326, (400, 2)).astype(F), min_distance=12))
    S.append(_single("seeds_md0_ignored", img, seeds=[(50, 50), (100, 50)], min_distance=0))
    # ---- overflow: 9185 candidates against a capacity of max(1024, 256), and with room
    S.append(_single("overflow_lattice", lattice(), max_cand=256))
    S.append(_single("lattice_with_room", lattice()))
    # ---- one call of jobs that differ in everything
    S.append(Scene("mixed_call", [
        (blocks(321, 243, 7, 21), np.random.default_rng(2).uniform(0, 240, (30, 2)).astype(F), MAX_KPS),
        (np.full((16, 40), 9, np.uint8), None, 8),                                      # nothing to find
        (seam_image(95, 63, 1), None, 0),                                               # no room: counts only
        (blocks(64, 200, 4, 22), np.zeros((0, 2), F), 17),
        (blocks(8, 8, 2, 23), None, MAX_KPS),
    ], min_distance=9, quality=0.02))
    return S


@functools.lru_cache(maxsize=None)
def _scenes():
    return tuple(_build())


def scenes():
    return list(_scenes())


def scene(name):
    for s in _scenes():
        if s.name == name:
            return s
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the walk's answer for every job of the scene: [(pts, response, info, response map)]; computed once, shared, read only"""
    s = scene(name)
    out = []
    for img, seeds, cap in s.jobs:
        res = gftt_ref.detect(img, seeds, cap, s.ref_params(), cand_cap=s.cand_cap())
        for a in (res[0], res[1], res[3]):
            a.setflags(write=False)
        out.append(res)
    return out
