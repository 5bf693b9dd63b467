"""Hand-built inputs for the trackers under svo_lk_set_photometric(ctx, 1): deterministic, numpy alone.  Every scene is named after what
it is built to reach in the compensated walks (tests/lk_photo_ref.py); tests/test_lk_photo_cpu.py pins that the walks reach it, and
tests/test_gpu_lk_photo.py holds the device to BOTH walks (svo_lk_track and svo_lk_track_rows) on all of them, bit for bit.

The texture is a sum of plane waves, so a shift is exact: next(x + dx, y + dy) = prev(x, y) before rounding to 8 bits.  Its grey range
is 42 .. 158, so that 1.4 J + 20, 0.6 J - 15 and J + 40 do not clip."""
import functools

import numpy as np

import lk_ref
import lk_photo_ref

F = np.float32
MAX_KPS = 512          # the context the GPU tests create

SHIFT = (3.4, -2.0)    # the recovery scenes: true motion of the 2-D pairs
ROW_SHIFT = (3.4, 0.0)  # ... and of the row pairs
# (name, gain, offset) of the recovery scenes; "unchanged" is the pair with its photometry left alone
PHOTOMETRY = (("gain_1.4_p20", 1.4, 20.0), ("gain_0.6_m15", 0.6, -15.0), ("offset_p40", 1.0, 40.0))


class Scene:
    """one tracker call: jobs = [(prev, next, pts, init or None)], params = LkParams keyword arguments"""
    def __init__(self, name, jobs, **params):
        self.name, self.jobs, self.params = name, jobs, params

    def ref_params(self):
        return lk_ref.LkParams(**self.params)


def to_u8(f):
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def texture_f(w, h, dx=0.0, dy=0.0, seed=0, mean=100.0, amp=58.0):
    """six plane waves with wavelengths of 9 .. 90 px, |f - mean| <= amp, moved by (dx, dy)"""
    rng = np.random.default_rng(1000 + seed)
    lam = np.array([9.0, 14.0, 22.0, 35.0, 56.0, 90.0])
    th, ph = rng.uniform(0, np.pi, 6), rng.uniform(0, 2 * np.pi, 6)
    a = np.array([0.8, 1.0, 1.2, 1.2, 1.0, 0.8]); a = a / a.sum() * amp
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    f = np.full((h, w), mean)
    for k in range(6):
        f += a[k] * np.sin(2 * np.pi / lam[k] * (np.cos(th[k]) * x + np.sin(th[k]) * y) + ph[k])
    return f


def pair(w, h, dx, dy, gain=1.0, offset=0.0, seed=0, **kw):
    """(prev, next): next is prev moved by (dx, dy) with gain * grey + offset applied before the rounding"""
    return to_u8(texture_f(w, h, seed=seed, **kw)), to_u8(gain * texture_f(w, h, dx, dy, seed=seed, **kw) + offset)


def grid_points(w, h, n, margin, seed=1):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1).astype(np.float32)


def step_edge(w, h, x_edge, lo=50.0, hi=200.0):
    """a vertical edge from lo to hi at x_edge (float), constant along y, tanh profile 3 px wide"""
    x = np.arange(w, dtype=np.float64)
    return np.tile(lo + (hi - lo) * 0.5 * (1.0 + np.tanh((x - x_edge) / 1.5)), (h, 1))


def _single(name, prev, nxt, pts, init=None, **params):
    return Scene(name, [(prev, nxt, np.asarray(pts, np.float32).reshape(-1, 2), None if init is None else np.asarray(init, np.float32).reshape(-1, 2))], **params)


def ramp(w=64, h=40):
    """grey = 30 + 2 x + (y - 20)^2 / 8: Ix is the same everywhere, so the x direction cannot be told from an offset, while Iy varies
    and the plain gradient matrix is regular"""
    y, x = np.mgrid[0:h, 0:w]
    return (30 + 2 * x + ((y - 20) ** 2) // 8).astype(np.uint8)


EDGE_SHIFT = 1.75


def _build():
    S = []
    W, H = 321, 243
    # 1. recovery: the known shift under a gain and an offset, and with the photometry left alone
    pts = grid_points(W, H, 40, 45, seed=3)
    rpts = grid_points(W, H, 24, 45, seed=4)
    S.append(_single("unchanged", *pair(W, H, *SHIFT), pts))
    S.append(_single("row_unchanged", *pair(W, H, *ROW_SHIFT), rpts))
    for name, g, b in PHOTOMETRY:
        S.append(_single(name, *pair(W, H, *SHIFT, gain=g, offset=b), pts))
        S.append(_single("row_" + name, *pair(W, H, *ROW_SHIFT, gain=g, offset=b), rpts))
    # 2. the window sizes at both edges of the three instantiations (2, 7 and 16 pixels per lane), under a gain; fb_max on for half
    for win in (5, 11, 13, 21, 23, 31):
        S.append(_single("win_%d" % win, *pair(W, H, 1.3, -0.7, gain=1.25, offset=-12.0, seed=win), grid_points(W, H, 8, 45, seed=win),
                         win=win, fb_max=(0.5 if win in (11, 13, 31) else 0.0)))
    # 3. reach
    # a template flat to 1/32 grey level: CII == 0 at level 0 (the first two points), and a point on texture beside it
    p, n = pair(96, 80, 0.6, 0.4, gain=1.2, offset=5.0)
    p = p.copy(); n = n.copy(); p[20:60, 4:50] = 77; n[20:60, 4:50] = 97
    S.append(_single("flat_template", p, n, [(26, 40), (27.5, 39.25), (70, 40)], win=21, max_level=0))
    # ... and flat at the coarse level only is not what skips there: these templates are not inside at the top levels and tracked below
    S.append(_single("inside_coarse", *pair(W, H, 0.5, 0.25, gain=0.8, offset=9.0), [(30, 120), (290, 120), (160, 30), (160, 212)], win=21, max_level=3))
    # an exact ramp in x: the plain walks track it, the compensated walks lose it on the reduced matrix
    r = ramp()
    S.append(_single("ramp", r, r, [(30, 20), (31.5, 18.25), (28, 24)], win=11, max_level=0))
    # pixel 0 of the window is 255 on a dark template: the indices behind the window sit on it and must count for nothing
    for win in (5, 13):
        p, n = pair(96, 80, 1.0, 0.0, gain=1.5, offset=4.0, seed=6, mean=30.0, amp=18.0)
        p = p.copy(); n = n.copy()
        half = (win - 1) // 2
        for cx, cy in ((40, 40), (60, 30)):
            p[cy - half, cx - half] = 255; n[cy - half, cx - half + 1] = 255
        S.append(_single("pad_pixel0_win_%d" % win, p, n, [(40, 40), (60, 30), (60.25, 30.5)], win=win, max_level=0))
    # win 31, a bright template against a dark target: a lane's 16 pixels of I I and of d I pass 2^29
    p, n = pair(W, H, 1.0, 0.5, gain=0.15, offset=0.0, seed=8, mean=228.0, amp=27.0)
    S.append(_single("lane_sums_win_31", p, n, grid_points(W, H, 6, 60, seed=8), win=31, max_level=1))
    # the target clips at 255
    S.append(_single("target_clips", *pair(W, H, 1.3, -0.7, gain=1.8, offset=20.0), grid_points(W, H, 10, 45, seed=12), win=21))
    # a gain that changes over the image, an offset that changes down it
    p = texture_f(W, H); n = texture_f(W, H, 1.3, -0.7)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    S.append(_single("vignette", to_u8(p), to_u8(n * (0.6 + 0.8 * x / W) + 10.0 * y / H), grid_points(W, H, 10, 45, seed=13), win=21))
    # the stops: eps (most scenes), max_iters, the oscillation half-step (2-D and along the row)
    for it in (1, 2):
        S.append(_single("max_iters_%d" % it, *pair(W, H, 2.3, -1.1, gain=1.3, offset=10.0), grid_points(W, H, 6, 45, seed=7), win=21, max_iters=it))
    S.append(_single("oscillation", *pair(96, 80, 2.6, -1.7, gain=1.3, offset=-8.0, seed=11), OSC_POINTS, win=5, max_level=0, max_iters=30, eps=0.001))
    S.append(_single("row_oscillation", *pair(96, 80, 2.6, 0.0, gain=1.3, offset=-8.0, seed=11), ROW_OSC_POINTS, win=5, max_level=0, max_iters=30, eps=0.001))
    # forward-backward: the right half of the target is other texture
    p, n = pair(W, H, 1.5, 0.0, gain=0.7, offset=12.0)
    n = n.copy(); n[:, 160:] = to_u8(texture_f(W, H, seed=5))[:, 160:]
    fbp = np.array([(60, 60), (100, 120), (80, 100), (230, 60), (260, 180), (240, 120), (50, 200), (60, 190)], np.float32)
    S.append(_single("fb_on", p, n, fbp, win=21, fb_max=0.5))
    S.append(_single("fb_off", p, n, fbp, win=21, fb_max=0.0))
    # init given, with a y of its own; a NaN and an infinity in pts and in init
    q = grid_points(W, H, 6, 60, seed=9)
    gi = (q + np.array([5.0, 0.3], F)).astype(F)
    S.append(_single("init_given", *pair(W, H, 5.5, 0.0, gain=1.2, offset=-6.0), q, gi, win=21, max_level=2))
    bad = np.array([(np.nan, 40), (40, np.inf), (40, 40), (40, 40), (40, 40)], np.float32)
    bad_init = np.array([(40, 40), (40, 40), (np.nan, 40), (40, -np.inf), (40.5, 40.25)], np.float32)
    S.append(_single("bad_coordinates", *pair(96, 80, 0.6, 0.4, gain=1.2, offset=5.0), bad, bad_init, win=21))
    # a vertical edge under a gain change: the row walk follows it, the 2-D walk has nothing along y
    S.append(_single("row_vertical_edge", to_u8(step_edge(96, 80, 48.0)), to_u8(0.7 * step_edge(96, 80, 48.0 + EDGE_SHIFT) + 10.0),
                     [(48, 40), (47.5, 30.25), (50, 50), (46.25, 22.5)], win=21, max_level=1))
    # point counts at the wave, block and grid edges
    for cnt in (1, 5, 65):
        S.append(_single("count_%d" % cnt, *pair(96, 80, 0.6, 0.4, gain=1.2, offset=5.0), grid_points(96, 80, cnt, 20, seed=100 + cnt), win=21))
    S.append(mixed_call())
    return S


def mixed_call():
    """four jobs in one call: two image sizes, a crop with an odd stride, an empty job, init on one job only"""
    big, big_n = pair(321, 243, 1.3, -0.7, gain=1.4, offset=20.0)
    frame, frame_n = pair(201, 150, -0.8, 0.6, gain=0.6, offset=-15.0, seed=2)
    crop, crop_n = frame[30:110, 50:146], frame_n[30:110, 50:146]                   # 96 x 80 views, stride 201
    small, small_n = pair(96, 80, 0.6, 0.4, gain=1.0, offset=40.0)
    g = grid_points(96, 80, 7, 20, seed=22)
    jobs = [(big, big_n, grid_points(321, 243, 9, 45, seed=21), None),
            (crop, crop_n, g, (g + np.float32(0.5)).astype(np.float32)),
            (small, small_n, np.zeros((0, 2), np.float32), None),
            (small, small_n, grid_points(96, 80, 70, 12, seed=24), None)]
    return Scene("mixed_call", jobs, win=13, fb_max=1.0)


# with eps = 0.001 these end in the oscillation half-step (two steps that cancel to within 0.01 come before one below eps); pinned by
# tests/test_lk_photo_cpu.py
OSC_POINTS = [(40.0, 40.0), (52.5, 31.25)]
ROW_OSC_POINTS = [(40.0, 40.0), (52.5, 31.25)]


@functools.lru_cache(maxsize=None)
def scenes():
    return tuple(_build())


def scene(name):
    return next(s for s in scenes() if s.name == name)


@functools.lru_cache(maxsize=None)
def prepared(name):
    s = scene(name)
    P = s.ref_params()
    return tuple(lk_ref.Prepared(np.ascontiguousarray(prev), np.ascontiguousarray(nxt), P) for prev, nxt, _, _ in s.jobs)


@functools.lru_cache(maxsize=None)
def reference(name, rows=False):
    """the compensated walk's results of a scene (rows: the row walk), computed once per process and shared, read-only:
    [(next_pts, status, err, traces, Prepared)] per job"""
    s = scene(name)
    P = s.ref_params()
    walk = lk_photo_ref.track_rows if rows else lk_photo_ref.track
    out = []
    for (prev, nxt, pts, init), pre in zip(s.jobs, prepared(name)):
        o, st, e, tr = walk(prev, nxt, pts, init, P, prepared=pre)
        for a in (o, st, e):
            a.setflags(write=False)
        out.append((o, st, e, tr, pre))
    return tuple(out)
