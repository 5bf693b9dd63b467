"""Hand-built keypoint lists for svo_adaptive_nms (TEST INFRASTRUCTURE), after the pattern of ransac_scenes.py / match_scenes.py: every
scene is a list of (name, keypoints in strictly ascending raster order, num_out_points, img_w, img_h).  The expected order of a case
is oracle.anms_copy(kps, num_out_points).  tests/test_anms_scenes_cpu.py pins, on the oracle and the plain walk below alone, that
every scene reaches what it is built for; tests/test_gpu_faster_anms.py holds the kernel to the oracle on all of them.

radii() is m_adaptive_non_max_sup (S2:141-215) once more, in numpy, because the oracle returns the order only: rank = (response desc,
index asc) through the oracle's ord32, radius of rank 0 = +inf, of rank k1 >= 1 the minimum over rank 0 and the ranks k2 in [1, k1)
with (double)r_k1 < 0.9 (double)r_k2 of the FLOAT dx * dx + dy * dy (exact = True: the same in exact integers, which the reference
does not compute -- scene (g) shows the difference)."""
import numpy as np

from stereo_vo_amd.abi import keypoint_dtype

# the sizes at which the kernel changes its path: a wave's segment of a radix pass grows by 64 keys at every multiple of 1024, the
# waves' ballots are 64 wide, one pass of the block's loops covers 1024 ranks; 2048 is the chunk of the neighbouring kernels
EDGE_N = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
DIRECT_L = 96        # prefixes up to this length are scanned directly, longer ones through the cell grid


def make(xs, ys, resp):
    """keypoint records as dmFASTER leaves them, sorted into raster order; positions must be unique"""
    xs, ys, resp = np.asarray(xs, np.int64), np.asarray(ys, np.int64), np.asarray(resp, np.float32)
    order = np.lexsort((xs, ys))
    k = np.zeros(len(xs), keypoint_dtype)
    k["x"], k["y"], k["response"] = xs[order], ys[order], resp[order]
    k["size"], k["angle"], k["octave"], k["class_id"] = 0.0, -1.0, 0, -1
    assert len(set(zip(k["x"].tolist(), k["y"].tolist()))) == len(k)
    return k


def ord32(resp):
    u = np.asarray(resp, np.float32).view(np.uint32).astype(np.int64)
    return np.where(u & 0x80000000, 0xFFFFFFFF - u, u | 0x80000000)


def rank_order(kps):
    return np.lexsort((np.arange(len(kps)), -ord32(kps["response"])))


def radii(kps, exact=False):
    """radius^2 of every keypoint, by input index: float32 as the reference computes it, or float64 of the exact integer (exact)"""
    n = len(kps)
    order = rank_order(kps)
    x, y = kps["x"][order].astype(np.float32), kps["y"][order].astype(np.float32)
    xi, yi = kps["x"][order].astype(np.int64), kps["y"][order].astype(np.int64)
    r = kps["response"][order].astype(np.float64)
    out = np.full(n, np.inf, np.float64 if exact else np.float32)
    for k1 in range(1, n):
        if exact:
            d2 = ((xi[k1] - xi[:k1]) ** 2 + (yi[k1] - yi[:k1]) ** 2).astype(np.float64)
        else:
            dx, dy = x[k1] - x[:k1], y[k1] - y[:k1]
            d2 = dx * dx + dy * dy
        m = r[k1] < 0.9 * r[:k1]
        m[0] = True
        out[order[k1]] = d2[m].min()
    return out


def order_of(rad, num_out):
    """(radius desc, index asc), the first min(num_out, n)"""
    n = len(rad)
    return np.lexsort((np.arange(n), -rad.astype(np.float64)))[:max(0, min(num_out, n))].astype(np.int32)


def prefix_lengths(kps):
    """L of every rank: min(rank, #{ j : (double)r < 0.9 (double)r_j })"""
    r = kps["response"][rank_order(kps)].astype(np.float64)
    return np.array([min(i, int((r[i] < 0.9 * r).sum())) for i in range(len(r))], np.int64)


def random_positions(rng, n, w, h, x0=0, y0=0):
    pos = rng.choice(w * h, size=n, replace=False)
    return x0 + pos % w, y0 + pos // w


def scene_a():
    """n = 0, 1, 2; num_out_points = 0, 1, n, n + 5"""
    out = []
    for n in (0, 1, 2):
        k = make([5, 40][:n], [7, 30][:n], [2.0, 3.0][:n])
        for num in sorted({0, 1, n, n + 5}):
            out.append(("a n=%d out=%d" % (n, num), k, num, 64, 48))
    return out


def boundary_pair(r2=np.float32(100.0)):
    """(r1, next): the largest float with (double)r1 < 0.9 (double)r2, and the float after it"""
    r1 = np.float32(0.9 * float(r2))
    while not float(r1) < 0.9 * float(r2):
        r1 = np.nextafter(r1, np.float32(-np.inf))
    while float(np.nextafter(r1, np.float32(np.inf))) < 0.9 * float(r2):
        r1 = np.nextafter(r1, np.float32(np.inf))
    return r1, np.nextafter(r1, np.float32(np.inf))


def scene_b():
    """A (10, 10) beside B (12, 10) with response r2, the strongest S far away: A's response just below / just not below 0.9 r2"""
    r2 = np.float32(100.0)
    lo, hi = boundary_pair(r2)
    return [("b %s" % t, make([10, 12, 60], [10, 10, 40], [r1, r2, 1000.0]), 3, 64, 48) for t, r1 in (("below", lo), ("at", hi))]


def scene_c():
    rng = np.random.default_rng(3)
    xs, ys = random_positions(rng, 40, 64, 48)
    mix = np.where(rng.integers(0, 2, 40) == 1, np.float32(0.0), np.float32(-0.0))
    return [("c %s" % t, make(xs, ys, r), 25, 64, 48) for t, r in
            (("equal positive", np.full(40, 5.0)), ("zero", np.zeros(40)), ("equal negative", np.full(40, -3.0)), ("signed zeros", mix))]


def scene_d():
    """a 32 x 32 lattice at pitch 4, five response values: many equal radii; the cut falls inside a tie group"""
    rng = np.random.default_rng(4)
    gx, gy = np.meshgrid(np.arange(32) * 4 + 1, np.arange(32) * 4 + 1)
    k = make(gx.ravel(), gy.ravel(), rng.choice(np.array([1.0, 1.05, 2.0, 4.0, 8.0], np.float32), 1024))
    rad = radii(k)
    o = order_of(rad, 1024)
    cut = next(c for c in range(100, 1024) if rad[o[c - 1]] == rad[o[c]] and rad[o[c - 2]] == rad[o[c]])
    return [("d lattice cut %d" % cut, k, cut, 128, 128)]


def scene_e():
    """64 strong corners in an 8 x 8 block at the origin of 1024 x 768, 4000 weak ones over the rest: every weak corner's prefix is
    exactly the 64 strong ones... or longer, and its nearest robustly stronger corner may be the whole image away"""
    rng = np.random.default_rng(5)
    sx, sy = np.meshgrid(np.arange(8), np.arange(8))
    pos = rng.choice(1024 * 768, size=6000, replace=False)
    wx, wy = pos % 1024, pos // 1024
    keep = (wx >= 8) | (wy >= 8)
    wx, wy = wx[keep][:4000], wy[keep][:4000]
    resp = np.concatenate([100.0 + np.arange(64), rng.uniform(1.0, 50.0, 4000)]).astype(np.float32)
    return [("e cluster", make(np.concatenate([sx.ravel(), wx]), np.concatenate([sy.ravel(), wy]), resp), 1000, 1024, 768)]


def scene_f():
    out = []
    for n in EDGE_N:
        rng = np.random.default_rng(600 + n)
        xs, ys = random_positions(rng, n, 320, 240)
        out.append(("f n=%d" % n, make(xs, ys, rng.normal(1.0, 1.0, n)), n // 3 + 1, 320, 240))
    return out


def far_list(seed):
    """16 000 x 1000: the strongest corner at the origin; 40 corners of nearly equal response (none robustly stronger than another, and
    nothing else robustly stronger than them) in a 16 x 8 patch 15 900 pixels away, whose radii are the distance to the origin --
    integers near 2.5e8, where a float has a spacing of 16 --; 260 weaker corners spread over the image"""
    rng = np.random.default_rng(seed)
    bx, by = random_positions(rng, 40, 16, 8, 15900, 0)
    fx, fy = random_positions(rng, 260, 11000, 900, 4000, 100)
    resp = np.concatenate([[1000.0], rng.uniform(45.0, 50.0, 40), rng.uniform(1.0, 40.0, 260)]).astype(np.float32)
    return make(np.concatenate([[0], bx, fx]), np.concatenate([[0], by, fy]), resp)


def scene_g():
    """the first seed whose float order differs from the order under exact integer distances"""
    for seed in range(64):
        k = far_list(seed)
        if not np.array_equal(order_of(radii(k), 150), order_of(radii(k, exact=True), 150)):
            return [("g far seed %d" % seed, k, 150, 16000, 1000)]
    raise AssertionError("no seed below 64 separates float from integer distances")


def scene_h():
    """every pixel of 256 x 128 a corner: 32 768 of them, sixteen response values"""
    rng = np.random.default_rng(8)
    gx, gy = np.meshgrid(np.arange(256), np.arange(128))
    return [("h full lattice", make(gx.ravel(), gy.ravel(), rng.integers(1, 17, 256 * 128).astype(np.float32)), 2000, 256, 128)]


SCENES = {"a": scene_a, "b": scene_b, "c": scene_c, "d": scene_d, "e": scene_e, "f": scene_f, "g": scene_g, "h": scene_h}
_cache = {}


def cases(letter):
    """the cases of a scene, built once"""
    if letter not in _cache:
        _cache[letter] = SCENES[letter]()
    return _cache[letter]


_expected = {}


def expected(letter, i):
    """oracle.anms_copy of case i of a scene, computed once and shared"""
    from oracle import oracle as O
    if (letter, i) not in _expected:
        _, k, num, _, _ = cases(letter)[i]
        _expected[(letter, i)] = O.anms_copy(k, num) if len(k) else np.zeros(0, np.int32)
    return _expected[(letter, i)]
