"""Hand-built inputs for svo_lk_track_rows: deterministic, numpy and scipy only.  Every scene is named after the branch of the row walk
(tests/lk_row_ref.py) it is built for; tests/test_lk_row_scenes_cpu.py pins that the walk takes that branch, tests/test_gpu_lk_rows.py
holds the device to the walk on all of them.  The texture and its shifts are tests/lk_scenes.py's."""
import functools
import numpy as np
from scipy import ndimage

import lk_ref
import lk_row_ref
from lk_scenes import MAX_KPS, Scene, grid_points, shifted, texture, texture_f, to_u8      # noqa: F401

F = np.float32

# the tolerances the CPU test asserts, each taken from what the walk attains on its scene on the CPU (measured: see the scene)
EDGE_SHIFT = 1.75          # vertical_step_edge: next(x + 1.75) = prev(x)
EDGE_TOL = 0.005           # measured: the walk's largest |recovered - 1.75| over the scene's four points is 0.0031 px
STEREO_DISP = 7.3          # stereo_shift: right(x - 7.3) = left(x)
STEREO_TOL = 0.02          # measured: the walk's largest |recovered - 7.3| over the 24 points (all tracked) is 0.0100 px, median 0.0046


def _single(name, prev, nxt, pts, init=None, **params):
    return Scene(name, [(prev, nxt, np.asarray(pts, np.float32).reshape(-1, 2), None if init is None else np.asarray(init, np.float32).reshape(-1, 2))], **params)


def step_edge(w, h, x_edge):
    """a vertical step from 50 to 200 at x_edge (float), constant along y, softened by a Gaussian of sigma 1.5 so that a fractional
    shift is a different image"""
    from scipy.special import erf
    x = np.arange(w, dtype=np.float64)
    row = 50.0 + 150.0 * 0.5 * (1.0 + erf((x - x_edge) / (1.5 * np.sqrt(2.0))))
    return to_u8(np.tile(row, (h, 1)))


def a11_over_win2(prev, pt, win):
    """A11 / win^2 of the template at pt on level 0, as the walk computes it"""
    h, w = prev.shape
    half = F((win - 1) // 2)
    wd = lk_ref._window(F(F(pt[0]) - half), F(F(pt[1]) - half), w, h, win)
    Ix = lk_ref._sample(lk_ref.scharr(prev)[0], win, wd, 8192, 14)
    return float(int((Ix * Ix).sum())) * lk_ref.TWO_M20 / float(win * win)


def faint(w, h):
    """a texture of a few grey levels: its A11 / win^2 is small enough to put min_eig on either side of it"""
    return to_u8(126.0 + texture_f(w, h, seed=4) * (6.0 / 255.0))


A11_POINT = (48.25, 40.5)


def _build():
    S = []
    small, small_n = texture(96, 80), shifted(96, 80, 0.6, 0.0)
    big = texture(321, 243)
    # window sizes: 2, 7 and 16 pixels per lane; the strip is 22, 38 and 36 columns wide
    for win in (5, 21, 31):
        S.append(_single("win_%d" % win, big, shifted(321, 243, 1.3, 0.0), grid_points(321, 243, 12, 45, seed=win), win=win))
    # point counts: the wave, block and grid edges
    for n in (0, 1, 3, 4, 5, 63, 64, 65, 257):
        S.append(_single("count_%d" % n, small, small_n, grid_points(96, 80, n, 20, seed=100 + n), win=21))
    # a vertical step edge: the 2-D tracker loses every point on it (min_eig is 0), the row tracker follows it
    ep = [(48, 40), (47.5, 30.25), (50, 50), (46.25, 22.5)]
    S.append(_single("vertical_step_edge", step_edge(96, 80, 48.0), step_edge(96, 80, 48.0 + EDGE_SHIFT), ep, win=21, max_level=1))
    # a horizontal edge: Ix = 0 everywhere, lost by the A11 rule at level 0
    S.append(_single("horizontal_edge", step_edge(80, 96, 40.0).T.copy(), step_edge(80, 96, 41.0).T.copy(), [(48, 40), (47.5, 39.25), (50, 42)], win=21, max_level=1))
    # A11 / win^2 on both sides of min_eig: the largest float32 not above it keeps the point, the next one loses it
    f = faint(96, 80)
    v = a11_over_win2(f, A11_POINT, 21)
    lo = F(v) if float(F(v)) <= v else np.nextafter(F(v), F(0))
    S.append(_single("a11_at_min_eig", f, f, [A11_POINT], win=21, max_level=0, min_eig=lo))
    S.append(_single("a11_below_min_eig", f, f, [A11_POINT], win=21, max_level=0, min_eig=np.nextafter(lo, F(1))))
    # the row of the search is the guess's: init.y != pt.y, the result's y is init.y's bit pattern
    p = grid_points(321, 243, 6, 60, seed=9)
    gi = p + np.array([5.5, 0], F)
    gi[:, 1] = (p[:, 1] + np.array([0.3, -0.7, 1.25, 0.0, 2.0 ** -12, -3.0], F)).astype(F)
    S.append(_single("init_y_differs", big, shifted(321, 243, 5.5, 0.0), p, gi, win=21, max_level=2))
    S.append(_single("init_on_answer", big, shifted(321, 243, 5.5, 0.0), p, p + np.array([5.5, 0], F), win=21, max_level=1))
    # a level skipped at the top (the template is not inside there) and tracked below
    S.append(_single("inside_coarse", big, shifted(321, 243, 0.5, 0.0), [(30, 120), (290, 120), (160, 30), (160, 212)], win=21, max_level=3))
    # the inside limit at level 0 (win 21 on 96 x 80: 11 <= x < 84, 11 <= y < 68): on it the point lives, one step beyond it is lost
    S.append(_single("inside_level0", small, small,
                     [(11, 40), (10.99, 40), (83.5, 40), (84, 40), (40, 11), (40, 10.5), (40, 67.75), (40, 68)], win=21, max_level=0))
    # a guess that walks out of the next image during the iterations at level 0: the "outside" loss
    S.append(_single("leaves_level0", small, shifted(96, 80, 4.0, 0.0), [(82, 40), (60, 40)], win=21, max_level=0))
    # a window that leaves the strip: at win 31 the strip holds the first window and 2 columns on either side; 9 px at level 0
    S.append(_single("leaves_strip", big, shifted(321, 243, 9.0, 0.0), grid_points(321, 243, 6, 60, seed=31), win=31, max_level=0))
    S.append(_single("leaves_strip_left", big, shifted(321, 243, -6.5, 0.0), grid_points(321, 243, 6, 60, seed=32), win=31, max_level=0, max_iters=40))
    # the stops: eps (the scenes above), max (max_iters = 1), osc
    for it in (1, 2):
        S.append(_single("max_iters_%d" % it, big, shifted(321, 243, 2.3, 0.0), grid_points(321, 243, 6, 45, seed=7), win=21, max_iters=it))
    S.append(_single("oscillation", *OSCILLATION[:3], **OSCILLATION[3]))
    # bad coordinates, in pts and in init
    bad = np.array([(np.nan, 40), (40, np.inf), (-np.inf, 40), (40, 40), (40, 40), (40, 40)], np.float32)
    bad_init = np.array([(40, 40), (40, 40), (40, 40), (np.nan, 40), (40, -np.inf), (40.5, 40.25)], np.float32)
    S.append(_single("bad_coordinates", small, small_n, bad, bad_init, win=21))
    # forward-backward along the row: the right half of the next image is other texture (points there do not return), and a flat patch
    # in it takes the gradient from the way back (lost there by the A11 rule)
    other = shifted(321, 243, 1.5, 0.0).copy()
    other[:, 160:] = texture(321, 243, seed=5)[:, 160:]
    other[150:243, 0:110] = 128
    fbp = np.array([(60, 60), (100, 120), (80, 100), (230, 60), (260, 180), (240, 120), (50, 200), (60, 190)], np.float32)
    S.append(_single("fb_rows", big, other, fbp, win=21, fb_max=0.5))
    S.append(_single("fb_off", big, other, fbp, win=21, fb_max=0.0))
    # a rectified pair: the right image is the left one moved by a fractional disparity
    S.append(_single("stereo_shift", big, shifted(321, 243, -STEREO_DISP, 0.0), grid_points(321, 243, 24, 60, seed=41), win=21))
    S.append(mixed_call())
    return S


def mixed_call():
    """four jobs in one call: two image sizes, a crop with a stride, an empty job and one at n = max_kps"""
    big, big_n = texture(321, 243), shifted(321, 243, 1.3, 0.0)
    frame, frame_n = texture(200, 150, seed=2), shifted(200, 150, -0.8, 0.0, seed=2)
    crop, crop_n = frame[30:110, 50:146], frame_n[30:110, 50:146]                   # 96 x 80 views, stride 200
    jobs = [(big, big_n, grid_points(321, 243, 9, 45, seed=21), None),
            (crop, crop_n, grid_points(96, 80, 7, 20, seed=22), grid_points(96, 80, 7, 20, seed=22) + np.float32(0.5)),
            (texture(96, 80), shifted(96, 80, 0.6, 0.0), np.zeros((0, 2), np.float32), None),
            (texture(96, 80), shifted(96, 80, 0.6, 0.0), grid_points(96, 80, MAX_KPS, 12, seed=24), None)]
    return Scene("mixed_call", jobs, win=21)


def _oscillation():
    """a point that ends in the oscillation half-step of the row rule (with eps = 0.001 two steps that cancel to within 0.01 come before
    one below eps): found by searching the walk once; pinned by the CPU test"""
    prev, nxt = texture(96, 80, seed=11), shifted(96, 80, 2.6, 0.0, seed=11)
    return prev, nxt, OSC_POINTS, dict(win=5, max_level=0, max_iters=30, eps=0.001)


OSC_POINTS = [(54.24431610107422, 25.997730255126953), (40.0, 40.0)]      # both end in the half-step, after five iterations
OSCILLATION = _oscillation()


@functools.lru_cache(maxsize=None)
def scenes():
    return tuple(_build())


def scene(name):
    return next(s for s in scenes() if s.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the row walk's results of a scene, computed once per process and shared: [(next_pts, status, err, traces, Prepared)] per job"""
    s = scene(name)
    P = s.ref_params()
    out = []
    for prev, nxt, pts, init in s.jobs:
        pre = lk_ref.Prepared(np.ascontiguousarray(prev), np.ascontiguousarray(nxt), P)
        o, st, e, tr = lk_row_ref.track(prev, nxt, pts, init, P, prepared=pre)
        for a in (o, st, e):
            a.setflags(write=False)
        out.append((o, st, e, tr, pre))
    return tuple(out)
