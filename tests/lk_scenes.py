"""Hand-built inputs for svo_lk_track: deterministic, numpy and scipy only.  Every scene is named after the property it is built for;
tests/test_lk_scenes_cpu.py pins that the walk (tests/lk_ref.py) takes that branch, tests/test_gpu_lk.py holds the device to the walk on
all of them."""
import functools
import numpy as np
from scipy import ndimage

import lk_ref

MAX_KPS = 512          # the context the GPU tests create: max_kps 512 (point count 257 and one job at n = max_kps)


@functools.lru_cache(maxsize=None)
def texture_f(w, h, seed=0):
    """multi-octave texture as float in 0 .. 255: bicubic zooms of random grids at 4, 16 and 64 px, summed, Gaussian sigma 1"""
    rng = np.random.default_rng(seed)
    acc = np.zeros((h, w))
    for cell in (4, 16, 64):
        grid = rng.random((h // cell + 3, w // cell + 3))
        acc += ndimage.zoom(grid, cell, order=3)[:h, :w]
    acc = ndimage.gaussian_filter(acc, 1.0)
    acc -= acc.min()
    return acc * (255.0 / acc.max())


def to_u8(f):
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def texture(w, h, seed=0):
    return to_u8(texture_f(w, h, seed))


def shifted(w, h, dx, dy, seed=0):
    """the texture moved by (dx, dy): next(x + dx, y + dy) = prev(x, y)"""
    return to_u8(ndimage.shift(texture_f(w, h, seed), (dy, dx), order=3, mode="nearest"))


def grid_points(w, h, n, margin, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1).astype(np.float32)


class Scene:
    """one svo_lk_track call: jobs = [(prev, next, pts, init or None)], params = LkParams keyword arguments"""
    def __init__(self, name, jobs, **params):
        self.name, self.jobs, self.params = name, jobs, params

    def ref_params(self):
        return lk_ref.LkParams(**self.params)


def _single(name, prev, nxt, pts, init=None, **params):
    return Scene(name, [(prev, nxt, np.asarray(pts, np.float32).reshape(-1, 2), None if init is None else np.asarray(init, np.float32).reshape(-1, 2))], **params)


def _build():
    S = []
    small, small_n = texture(96, 80), shifted(96, 80, 0.6, 0.4)
    big = texture(321, 243)
    # window sizes: 25 pixels on 64 lanes, 7 per lane, 16 per lane
    for win in (5, 21, 31):
        S.append(_single("win_%d" % win, big, shifted(321, 243, 1.3, -0.7), grid_points(321, 243, 12, 45, seed=win), win=win))
    # point counts: the wave, block and grid edges
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        S.append(_single("count_%d" % n, small, small_n, grid_points(96, 80, n, 20, seed=100 + n), win=21))
    # the inside limit at level 0 (win 21 on 96 x 80: 11 <= x < 84, 11 <= y < 68): on it the point lives, one step beyond it is lost
    S.append(_single("inside_level0", small, small,
                     [(11, 40), (10.99, 40), (83.5, 40), (84, 40), (40, 11), (40, 10.5), (40, 67.75), (40, 68)], win=21, max_level=0))
    # ... and at coarse levels only: skipped there, tracked below
    S.append(_single("inside_coarse", big, shifted(321, 243, 0.5, 0.25), [(30, 120), (290, 120), (160, 30), (160, 212)], win=21, max_level=3))
    # weight rounding: integer coordinates (w00 = 16384), fractions 2^-20 and 1 - 2^-20 (a weight rounds to 0 or 16384)
    e = 2.0 ** -20
    S.append(_single("weights", small, small_n, [(40, 40), (12 + e, 12 + e), (13 - e, 13 - e), (12 + e, 13 - e), (41, 12 + e)], win=21, max_level=0))
    # textureless and one-dimensional
    S.append(_single("flat", np.full((80, 96), 128, np.uint8), np.full((80, 96), 128, np.uint8), grid_points(96, 80, 5, 20), win=21, max_level=1))
    edge = np.full((80, 96), 50, np.uint8); edge[:, 48:] = 200
    S.append(_single("vertical_edge", edge, edge, [(48, 40), (47.5, 30.25), (50, 50)], win=21, max_level=1))
    # saturated: the 0 / 255 checkerboard of 1 px period under win 31 (its Scharr response is zero: lost by min_eig), and 2 x 2 blocks
    # against their negative, where |J - I| is as large as it gets (8160) beside derivatives of 10 * 255
    yy, xx = np.mgrid[0:80, 0:96]
    chk = (((xx + yy) & 1) * 255).astype(np.uint8)
    S.append(_single("checker_1px", chk, chk, [(48, 40), (47.5, 39.5), (40.25, 41.75)], win=31, max_level=0))
    blk = ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)
    S.append(_single("blocks_2px_negative", blk, 255 - blk, [(48, 40), (47, 41), (47.5, 39.5), (40.25, 41.75)], win=31, max_level=0, max_iters=5))
    # ... and 2 px stripes, upright above row 40 and lying below it, against their negative: derivatives of 16 * 255 on both axes
    stp = np.where(yy < 40, (xx >> 1) & 1, (yy >> 1) & 1).astype(np.uint8) * 255
    S.append(_single("stripes_2px_negative", stp, 255 - stp, [(48, 40), (47.5, 39.5)], win=31, max_level=0, max_iters=5))
    # the window leaves the next image during the iterations: at level 0 (lost) and at level 2 (the level ends, the point survives)
    S.append(_single("leaves_level0", small, shifted(96, 80, 4.0, 0.0), [(82, 40), (60, 40)], win=21, max_level=0))
    S.append(_single("leaves_level2", big, shifted(321, 243, -12.0, 0.0), [(46, 120), (160, 120)], win=21, max_level=2))
    # iteration limits
    for it in (1, 2):
        S.append(_single("max_iters_%d" % it, big, shifted(321, 243, 2.3, 1.1), grid_points(321, 243, 6, 45, seed=7), win=21, max_iters=it))
    S.append(_single("oscillation", *OSCILLATION[:3], **OSCILLATION[3]))
    # first guesses: on the answer and 3 px off
    p = grid_points(321, 243, 6, 60, seed=9)
    mv = np.array([5.5, -3.25], np.float32)
    S.append(_single("init_on_answer", big, shifted(321, 243, 5.5, -3.25), p, p + mv, win=21, max_level=1))
    S.append(_single("init_3px_off", big, shifted(321, 243, 5.5, -3.25), p, p + mv + np.array([3, 0], np.float32), win=21, max_level=1))
    # forward-backward: the right half of the next image is other texture
    other = shifted(321, 243, 1.5, 0.5).copy()
    other[:, 160:] = texture(321, 243, seed=5)[:, 160:]
    fbp = np.array([(60, 60), (100, 180), (80, 120), (230, 60), (260, 180), (240, 120)], np.float32)
    S.append(_single("fb_half_replaced", big, other, fbp, win=21, fb_max=0.5))
    S.append(_single("fb_off", big, other, fbp, win=21, fb_max=0.0))
    # levels: none below the image, and more asked for than the image gives (96 x 80 at win 21: 48 x 40, then 24 x 20 is too small)
    S.append(_single("max_level_0", small, small_n, grid_points(96, 80, 5, 20, seed=3), win=21, max_level=0))
    S.append(_single("max_level_5_stops_early", small, small_n, grid_points(96, 80, 5, 20, seed=3), win=21, max_level=5))
    # bad coordinates, in pts and in init
    bad = np.array([(np.nan, 40), (40, np.inf), (-np.inf, 40), (40, 40), (40, 40), (40, 40)], np.float32)
    bad_init = np.array([(40, 40), (40, 40), (40, 40), (np.nan, 40), (40, -np.inf), (40.5, 40.25)], np.float32)
    S.append(_single("bad_coordinates", small, small_n, bad, bad_init, win=21))
    S.append(mixed_call())
    return S


def mixed_call():
    """five jobs of different sizes and strides: an odd width held contiguously, a crop of a larger frame, prev and next with different
    strides, an empty job and one at n = max_kps"""
    big, big_n = texture(321, 243), shifted(321, 243, 1.3, -0.7)
    frame, frame_n = texture(200, 150, seed=2), shifted(200, 150, -0.8, 0.6, seed=2)
    crop, crop_n = frame[30:110, 50:146], frame_n[30:110, 50:146]                   # 96 x 80 views, stride 200
    wide = np.zeros((80, 128), np.uint8); wide[:, :96] = texture(96, 80)
    pn = np.zeros((80, 160), np.uint8); pn[:, :96] = shifted(96, 80, 0.6, 0.4)
    jobs = [(big, big_n, grid_points(321, 243, 9, 45, seed=21), None),
            (crop, crop_n, grid_points(96, 80, 7, 20, seed=22), None),
            (wide[:, :96], pn[:, :96], grid_points(96, 80, 5, 20, seed=23), grid_points(96, 80, 5, 20, seed=23) + np.float32(0.5)),
            (texture(96, 80), shifted(96, 80, 0.6, 0.4), np.zeros((0, 2), np.float32), None),
            (texture(96, 80), shifted(96, 80, 0.6, 0.4), grid_points(96, 80, MAX_KPS, 12, seed=24), None)]
    return Scene("mixed_call", jobs, win=21)


def _oscillation():
    """a point that ends in the oscillation half-step: found by searching the walk once; pinned by tests/test_lk_scenes_cpu.py"""
    prev, nxt = texture(96, 80, seed=11), shifted(96, 80, 2.6, -1.7, seed=11)
    return prev, nxt, OSC_POINTS, dict(win=5, max_level=0, max_iters=30)


OSC_POINTS = [(17.640865325927734, 33.116336822509766), (40.0, 40.0)]      # the first oscillates, the second converges
OSCILLATION = _oscillation()


@functools.lru_cache(maxsize=None)
def scenes():
    return tuple(_build())


def scene(name):
    return next(s for s in scenes() if s.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the walk's results of a scene, computed once per process and shared: [(next_pts, status, err, traces, Prepared)] per job"""
    s = scene(name)
    P = s.ref_params()
    out = []
    for prev, nxt, pts, init in s.jobs:
        pre = lk_ref.Prepared(np.ascontiguousarray(prev), np.ascontiguousarray(nxt), P)
        o, st, e, tr = lk_ref.track(prev, nxt, pts, init, P, prepared=pre)
        for a in (o, st, e):
            a.setflags(write=False)
        out.append((o, st, e, tr, pre))
    return tuple(out)
