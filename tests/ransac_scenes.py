"""Stage-4 input lists built by hand for the F-matrix RANSAC (numpy only: no GPU, and the oracle is imported by the functions that need it).

Every scene is a dict of the lists stage 4 takes -- previous / current keypoints and descriptors of both sides, previous / current pairings
(pkl pkr pdl pdr pm, ckl ckr cdl cdr cm), the image size they are PUT with (W, H) -- plus, for the hand-built ones, `p1` / `p2`: the left
pixel pairs in the order the brute-force tracker hands them to findFundamentalMat (every keypoint has a random descriptor of its own, so
pairing k of the previous frame is continued by its own copy: every pairing is a candidate, in the previous list's order).

All coordinates are small integers or exact binary fractions (exact in binary32 and far beyond), the motions are exact epipolar geometries whose F has small integer
entries, so that a model fitted to seven inliers is the true F up to rounding: pairs placed at distance exactly 1 from their epipolar line
then have a symmetric error of 1 +- a few ulp -- inside the band in which the matrix-core count (k_ransac_count_mfma16) may not decide for
itself -- and pairs placed ON the epipole have a line of length ~0: the count's guards must fail for them and the oracle's own
expression (inf, or 0 * inf = NaN: "outlier") must be replayed.  tests/test_ransac_scenes_cpu.py asserts, on the oracle alone, that the scenes
do reach those paths; tests/test_gpu_ransac_forms.py runs them through every form of the RANSAC kernels."""
import functools
import os

import numpy as np

from stereo_vo_amd.abi import keypoint_dtype, dmatch_dtype


def _kps(xy):
    k = np.zeros(len(xy), keypoint_dtype)
    k["x"], k["y"], k["size"], k["response"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, 1.0, -1
    return k


def line_scene(n, ys, d, outlier_frac, seed, W=640, H=480, disp=20, off_line=True):
    """Stage-4 input lists built by hand: n pairings whose keypoints sit on the rows `ys` at INTEGER x; the current frame is the previous
    one shifted by d pixels in x (pure translation: every correspondence satisfies F = [t]_x exactly); a fraction of the pairings is
    moved somewhere else in the current frame (outliers).  Every keypoint has a random descriptor of its own, so the brute-force tracker
    pairs pairing k of the previous frame with its own continuation."""
    rng = np.random.RandomState(seed)
    per = max(1, n // len(ys))
    pts = []
    for y in ys:
        xs = rng.choice(np.arange(60, W - 60), per, replace=False)
        pts += [(float(x), float(y)) for x in np.sort(xs)]
    pts = np.array(pts, np.float32)
    n = len(pts)

    def kps(xy):
        k = np.zeros(len(xy), keypoint_dtype)
        k["x"], k["y"], k["size"], k["response"], k["class_id"] = xy[:, 0], xy[:, 1], 31.0, 1.0, -1
        return k
    desc, descr = rng.randint(0, 256, (n, 32)).astype(np.uint8), rng.randint(0, 256, (n, 32)).astype(np.uint8)
    m = np.zeros(n, dmatch_dtype); m["queryIdx"] = np.arange(n); m["trainIdx"] = np.arange(n); m["distance"] = 10.0
    cur = pts + np.array([d, 0], np.float32)
    out = rng.rand(n) < outlier_frac
    if off_line:
        cur[out, 1] = rng.randint(40, H - 40, int(out.sum())).astype(np.float32); cur[out, 0] = rng.randint(60, W - 60, int(out.sum())).astype(np.float32)
    else:
        yi = np.searchsorted(np.array(ys, np.float32), pts[:, 1])
        cur[out, 1] = np.array(ys, np.float32)[(yi[out] + 1) % len(ys)]
    order = np.lexsort((cur[:, 0], cur[:, 1]))                             # the current lists are row-sorted too
    curL = cur[order]
    sh = np.array([disp, 0], np.float32)
    return dict(pkl=kps(pts), pkr=kps(pts - sh), pdl=desc, pdr=descr, pm=m, ckl=kps(curL), ckr=kps(curL - sh), cdl=desc[order], cdr=descr[order], cm=m.copy(), W=W, H=H)


def _scene(rng, prev, cur, W, H, disp):
    """the lists of a scene from its pixel pairs (n x 2 arrays): previous list row-sorted, current list row-sorted, right = left - disp"""
    o = np.lexsort((prev[:, 0], prev[:, 1]))
    prev, cur, exact = prev[o].astype(np.float32), cur[o].astype(np.float32), (prev[o], cur[o])
    n = len(prev)
    assert (prev == exact[0]).all() and (cur == exact[1]).all() and ((cur[:, 0] - disp) + disp == cur[:, 0]).all()                         # exact in binary32, right lists too
    desc, descr = rng.randint(0, 256, (n, 32)).astype(np.uint8), rng.randint(0, 256, (n, 32)).astype(np.uint8)
    m = np.zeros(n, dmatch_dtype); m["queryIdx"] = np.arange(n); m["trainIdx"] = np.arange(n); m["distance"] = 10.0
    order = np.lexsort((cur[:, 0], cur[:, 1]))
    curL = cur[order]
    sh = np.array([disp, 0], np.float32)
    return dict(pkl=_kps(prev), pkr=_kps(prev - sh), pdl=desc, pdr=descr, pm=m, ckl=_kps(curL), ckr=_kps(curL - sh), cdl=desc[order], cdr=descr[order], cm=m.copy(),
                W=W, H=H, p1=prev.copy(), p2=cur.copy())


def _roles(rng, n, border_share, outlier_share):
    perm = rng.permutation(n)
    nb, no = int(round(border_share * n)), int(round(outlier_share * n))
    return perm[:nb], perm[nb:nb + no]


HAIR = 1.0 + 2.0 ** -22        # a binary32 number: a pair this far from its line has the error (1 + 2^-22)^2 = 1 + 2^-21 + 2^-44, exactly


def sideways_scene(n, seed, border_share, outlier_share, n_hair=0, W=640, H=480, disp=20, xr=(64, 560), yr=(40, 440), step=8):
    """Sideways motion: previous keypoints on an integer grid, current = previous + (d_i, 0) with an integer d_i in 2..40 of its own per
    point (depth varies: no homography explains the pairs, the 7-point solve is not degenerate).  The exact F is [(1,0,0)]_x: every
    epipolar line is the point's own row.  `border_share` of the pairs is moved by exactly +-1 px in y (symmetric error exactly 1 on the
    exact model: "inlier", by the `<=`), `outlier_share` by +-7 px.  `n_hair` of the n pairs sit on the row y = 0 with the current point at
    y = 1 + 2^-22: an OUTLIER by 2^-21, just beyond the band -- a screen whose lower edge were misplaced by a few 2^-22 would let it in.
    Right lists = left lists shifted by the integer disparity."""
    rng = np.random.RandomState(seed)
    xs, ys = np.arange(xr[0], xr[1] + 1, step), np.arange(yr[0], yr[1] + 1, step)
    ys = ys[ys != 0]
    n_grid = n - n_hair
    cell = rng.choice(len(xs) * len(ys), n_grid, replace=False)
    prev = np.stack([xs[cell % len(xs)], ys[cell // len(xs)]], 1).astype(np.float64)
    cur = prev + np.stack([rng.randint(2, 41, n_grid), np.zeros(n_grid, np.int64)], 1)
    border, outl = _roles(rng, n_grid, border_share, outlier_share)
    cur[border, 1] += rng.choice([-1, 1], len(border))
    cur[outl, 1] += 7 * rng.choice([-1, 1], len(outl))
    hx = rng.choice(xs, n_hair, replace=False).astype(np.float64)
    hprev = np.stack([hx, np.zeros(n_hair)], 1)
    hcur = np.stack([hx + rng.randint(2, 41, n_hair), np.full(n_hair, HAIR)], 1)
    return _scene(rng, np.concatenate([prev, hprev]), np.concatenate([cur, hcur]), W, H, disp)


# (offset of the previous point from c along the row y = 240, current point): exact in binary32, whose ulp at 320 is 2^-15
NEAR = ((2.0 ** -14, 321.0, 241.0), (-2.0 ** -13, 318.0, 239.0), (2.0 ** -12, 323.0, 241.0), (-2.0 ** -14, 317.0, 239.0))


def forward_scene(n, seed, n_epipole, border_share, outlier_share, n_near=0, n_ray=0, W=640, H=480, disp=20):
    """Forward motion: expansion about the integer centre c = (320, 240), current = c + s_i (previous - c) with previous - c a multiple of 4
    in both coordinates and s_i from {1.25, 1.5, 1.75, 2} per point (again no homography).  The exact F is [(320, 240, 1)]_x: the
    epipolar lines are the rays through c, the epipole of both frames.  `n_epipole` pairs sit AT c in both frames: l = F x is 0 on the exact
    model (1 / |l|^2 = inf, the error infinite, NaN where d is 0 too) and tiny on a fitted one.  Border pairs lie on the row y = 240 with the current point moved to
    y = 241: distance exactly 1 from the ray on one side, less on the other.  Outliers are moved 7 px across their ray.
    `n_near` (<= 4) further border pairs have their previous point on the row y = 240 a few 2^-14 px beside c (exact in binary32) and their
    current point one row off: an error of 1 again, but on a line only 2^-12 .. 2^-14 long, whose d the matrix cores get to 1e-7
    relatively at best -- only the guards keep the screen from deciding such a pair.  `n_ray` pairs lie on the row and the column
    through c (two exact rays of the motion): samples drawn mostly from them give models with nearly vanishing rows, whose lines are
    short for EVERY pair -- the case the guards are there for (a count kernel built without them gets forward-64 and forward-120 wrong)."""
    rng = np.random.RandomState(seed)
    c = np.array([320, 240], np.int64)
    n_rest = n - n_epipole - n_near - n_ray
    border, outl = _roles(rng, n_rest, border_share, outlier_share)
    ii, jj = np.arange(-37, 38), np.arange(-27, 28)
    jj = jj[jj != 0]                                                       # row 240 belongs to the border pairs
    cell = rng.choice(len(ii) * len(jj), n_rest, replace=False)
    off = 4 * np.stack([ii[cell % len(ii)], jj[cell // len(ii)]], 1).astype(np.int64)
    bi = rng.choice(ii[ii != 0], len(border), replace=False)
    off[border] = np.stack([4 * bi, np.zeros(len(border), np.int64)], 1)
    s4 = rng.randint(5, 9, n_rest)                                         # 4 s_i
    prev, cur = c + off, c + (off // 4) * s4[:, None]
    cur[border, 1] += 1
    across_y = np.abs(off[outl, 0]) >= np.abs(off[outl, 1])                  # a ray closer to horizontal: move in y
    sign = 7 * rng.choice([-1, 1], len(outl))
    cur[outl, 1] += np.where(across_y, sign, 0)
    cur[outl, 0] += np.where(across_y, 0, sign)
    if n_ray:                                                              # (drawn last: the scenes without them keep their points)
        nr, nc = (n_ray + 1) // 2, n_ray // 2                              # on the row y = 240 / on the column x = 320: exact rays of the motion
        tr = rng.choice(np.concatenate([np.arange(-37, 0), np.arange(1, 38)]), nr, replace=False)
        tc = rng.choice(np.concatenate([np.arange(-27, 0), np.arange(1, 28)]), nc, replace=False)
        t = np.concatenate([np.stack([tr, 0 * tr], 1), np.stack([0 * tc, tc], 1)])
        prev = np.concatenate([prev, c + 4 * t]); cur = np.concatenate([cur, c + t * rng.randint(5, 9, n_ray)[:, None]])
    near = np.array(NEAR[:n_near]).reshape(-1, 3)
    prev = np.concatenate([prev, np.tile(c, (n_epipole, 1)), np.stack([320.0 + near[:, 0], np.full(n_near, 240.0)], 1)])
    cur = np.concatenate([cur, np.tile(c, (n_epipole, 1)), near[:, 1:]])
    return _scene(rng, prev, cur, W, H, disp)


def far_scene(n, seed, border_share, outlier_share, n_hair=0, W=640, H=480):
    """A sideways_scene whose coordinates run from negative values to four times the image size the lists are put with (W x H): still exact
    in binary32, but outside the premise under which store_model bounds the matrix cores' rounding ("coordinates inside the image")."""
    return sideways_scene(n, seed, border_share, outlier_share, n_hair, W=W, H=H, disp=20, xr=(-640, 4 * W - 64), yr=(-480, 4 * H), step=16)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the scene set of tests/test_ransac_scenes_cpu.py (preconditions) and tests/test_gpu_ransac_forms.py: (name, generator, arguments).
# The list lengths are the candidate counts the kernels have edges at: below / at / above the direct 7-point path and LMedS (6, 7, 8, 14),
# the first RANSAC sizes and one 16-pair tile +- 1 (15, 16, 17, 31, 32, 33), the 256-pair super-tile +- 1 (255, 256, 257), a whole number
# of tiles past it (272) and three super-tiles (530: no multiple of 16, and of no 16 * nsplit).
# ---------------------------------------------------------------------------------------------------------------------------------------
SCENES = [
    # name, generator, (n, seed, [n_epipole,] border share, outlier share[, n_hair | n_near[, n_ray]]): the seeds were picked so that the oracle meets the
    # preconditions of tests/test_ransac_scenes_cpu.py (not every seed does: most fitted models are a few 1e-14 off the exact one,
    # and |l|^2 == 0 with d == 0 -- the NaN -- needs one that is exact to the last place)
    ("sideways-6", sideways_scene, (6, 1, 0.0, 0.0)),
    ("sideways-7", sideways_scene, (7, 1, 0.0, 0.0)),
    ("sideways-8", sideways_scene, (8, 3, 0.125, 0.0)),
    ("sideways-15", sideways_scene, (15, 3, 0.2, 0.07, 1)),
    ("sideways-17", sideways_scene, (17, 6, 0.2, 0.12, 1)),
    ("sideways-31", sideways_scene, (31, 2, 0.15, 0.15, 2)),
    ("sideways-33", sideways_scene, (33, 5, 0.15, 0.25, 2)),
    ("sideways-255", sideways_scene, (255, 2, 0.1, 0.3, 4)),
    ("sideways-257", sideways_scene, (257, 2, 0.06, 0.42, 4)),
    ("sideways-530", sideways_scene, (530, 2, 0.05, 0.45, 6)),
    ("forward-11", forward_scene, (11, 56, 2, 0.2, 0.0)),
    ("forward-14", forward_scene, (14, 237, 2, 0.15, 0.0)),
    ("forward-16", forward_scene, (16, 47, 1, 0.2, 0.1)),
    ("forward-24", forward_scene, (24, 42, 1, 0.1, 0.1, 4)),
    ("forward-32", forward_scene, (32, 89, 2, 0.1, 0.1)),
    ("forward-48", forward_scene, (48, 29, 2, 0.1, 0.15, 4)),
    ("forward-64", forward_scene, (64, 16, 2, 0.1, 0.1, 4, 36)),
    ("forward-120", forward_scene, (120, 8, 2, 0.05, 0.3, 4, 60)),
    ("forward-150", forward_scene, (150, 7, 4, 0.1, 0.15)),
    ("forward-256", forward_scene, (256, 86, 5, 0.1, 0.2)),
    ("forward-272", forward_scene, (272, 92, 3, 0.08, 0.3)),
    ("far-33", far_scene, (33, 1, 0.2, 0.15, 2)),
    ("far-257", far_scene, (257, 1, 0.1, 0.3, 4)),
]
CANDIDATE_COUNTS = (6, 7, 8, 14, 15, 16, 17, 31, 32, 33, 255, 256, 257, 272)      # ... and one above 512


@functools.lru_cache(maxsize=None)
def scene(name):
    for nm, gen, args in SCENES:
        if nm == name:
            return gen(*args)
    raise KeyError(name)


def scene_names(kind=None):
    return [nm for nm, _, _ in SCENES if kind is None or nm.startswith(kind)]


# the eleven line_scene cases of test_collinear_point_sets_continue_the_sampler_past_its_table (rows, pairings, outlier share, outliers off the rows)
LINE_CASES = [([100, 300], 120, 0.5, True), ([100, 200, 300], 120, 0.5, True), ([100, 300], 80, 0.7, True), ([100, 300], 200, 0.3, True), ([100], 100, 0.5, True),
              ([100, 300], 120, 0.5, False), ([100, 300], 14, 0.0, True), ([100, 300], 12, 0.2, True), ([100, 300], 10, 0.0, False), ([60, 100, 300, 420], 200, 0.6, True),
              ([90, 91, 92, 93, 94, 95, 96, 97, 98, 99, 100, 101], 96, 0.2, True)]
THINNED_KEEP = (6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 24, 32, 48, 64)


def pairings_row_index(m, kl, H):
    """matches_lr_row_index (S3:425-445) of a pairing list over its left keypoints"""
    ri, idx = np.zeros(H + 1, np.int64), 0
    for y in range(H):
        ri[y] = idx
        while idx < len(m) and kl[m[idx]["queryIdx"]]["y"] <= np.float32(y):
            idx += 1
    ri[H] = len(m)
    return ri


@functools.lru_cache(maxsize=None)
def thinned_cases(golden_dir, reps=6):
    """the thinned golden lists of test_few_candidates_reach_the_sampler_edge_cases: frame 1's pairings cut down to `keep`, frame 2 whole;
    `pri` / `cri` = the row indices of the two pairing lists (what the windowed tracker, ifm_method 1, reads)"""
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    rng = np.random.RandomState(23)
    pm_all, cm = g["matches1"], np.ascontiguousarray(g["matches2"])
    cri = np.ascontiguousarray(g["mrow2"], np.int64)
    out = []
    for keep in THINNED_KEEP:
        for rep in range(reps):
            sel = np.sort(rng.choice(len(pm_all), min(keep, len(pm_all)), replace=False))
            pm = np.ascontiguousarray(pm_all[sel])
            out.append(("thinned-%d-%d" % (keep, rep), dict(pkl=g["kps0_1"], pkr=g["kps1_1"], pdl=g["desc0_1"], pdr=g["desc1_1"], pm=pm, ckl=g["kps0_2"], ckr=g["kps1_2"],
                                                             cdl=g["desc0_2"], cdr=g["desc1_2"], cm=cm, W=W, H=H, pri=pairings_row_index(pm, g["kps0_1"], H), cri=cri)))
    return out


@functools.lru_cache(maxsize=None)
def line_cases():
    return [("line-%d-%d" % (i, seed), line_scene(n, ys, 4.0, of, seed, off_line=off)) for i, (ys, n, of, off) in enumerate(LINE_CASES) for seed in (0, 1, 2)]


def all_cases(golden_dir):
    """every case the forced-form tests run: the hand-built scenes, the thinned golden lists, the line scenes"""
    return [(nm, scene(nm)) for nm in scene_names()] + list(thinned_cases(golden_dir)) + list(line_cases())


def put_scene(ctx, lane, s):
    """a scene's lists into lane `lane` of a stereo_vo_amd.hip.Context: previous frame (which = 1) and current frame (which = 0)"""
    for side, (k1, d1, k0, d0) in enumerate(((s["pkl"], s["pdl"], s["ckl"], s["cdl"]), (s["pkr"], s["pdr"], s["ckr"], s["cdr"]))):
        ctx.put_features(lane, 1, side, k1, d1, s["W"], s["H"])
        ctx.put_features(lane, 0, side, k0, d0, s["W"], s["H"])
    ctx.put_matches(lane, 1, s["pm"]); ctx.put_matches(lane, 0, s["cm"])


def run_case(ctx, s, params=None):
    """stage 4 alone on a scene, in lane 0 of a one-lane context: (tracked pairs, the eight counters, the lane's status word)"""
    from stereo_vo_amd import hip
    if params is not None:
        ctx.set_params(params)
    put_scene(ctx, 0, s)
    ctx.run_stages(hip.RUN_TRACK)
    return ctx.tracked(0), [int(v) for v in ctx.result(0).track_stats[:8]], ctx.status_word(0)


def check_case(name, got, want):
    """tracked pairs byte for byte, all eight counters, SVO_ST_INTERNAL (status bit 8) down"""
    (trk, ts, status), (want_trk, want_ts) = got, want
    assert list(ts) == [int(v) for v in want_ts], (name, "stage-4 counters", list(ts), [int(v) for v in want_ts])
    assert trk.tobytes() == want_trk.tobytes(), (name, "tracked pairs", len(trk), len(want_trk))
    assert not (int(status) & 8), (name, "SVO_ST_INTERNAL")


_WANT = {}


def oracle_track(p, s, key=None):
    """the oracle's stage 4 on a scene: (tracked pairs, the eight track_stats counters).  Computed once per `key` and kept."""
    k = None if key is None else (key, int(p.ifm_method))
    if k is not None and k in _WANT:
        return _WANT[k]
    from oracle import oracle
    zeros = np.zeros(s["H"] + 1, np.int64)
    win = int(p.ifm_method) != 0
    want = oracle.track(p, p.orb_max_distance, s["pkl"], s["pdl"], s["pkr"], s["pdr"], s["pm"], s["pri"] if win else zeros,
                        s["ckl"], s["cdl"], s["ckr"], s["cdr"], s["cm"], s["cri"] if win else zeros, s["W"], s["H"], stats=True)
    if k is not None:
        _WANT[k] = want
    return want


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle's error in float64 numpy, operation for operation (svo_oracle.c: fm_error), and the guards of the matrix-core count
# ---------------------------------------------------------------------------------------------------------------------------------------
def fm_error_terms(F, p1, p2):
    """(error as a float32, |l'|^2 = denA, |l|^2 = denB) of every pair under model F (3x3), in the operation order of fm_error"""
    F = np.asarray(F, np.float64).reshape(9)
    x1, y1, x2, y2 = (np.asarray(v, np.float64) for v in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]))
    with np.errstate(all="ignore"):
        a = (F[0] * x1 + F[1] * y1) + F[2]; b = (F[3] * x1 + F[4] * y1) + F[5]; c = (F[6] * x1 + F[7] * y1) + F[8]
        denB = a * a + b * b
        sB = 1.0 / denB; dB = (x2 * a + y2 * b) + c
        a = (F[0] * x2 + F[3] * y2) + F[6]; b = (F[1] * x2 + F[4] * y2) + F[7]; c = (F[2] * x2 + F[5] * y2) + F[8]
        denA = a * a + b * b
        sA = 1.0 / denA; dA = (x1 * a + y1 * b) + c
        eA, eB = (dA * dA) * sA, (dB * dB) * sB
        e = np.where(eA < eB, eB, eA)                                     # std::max(eA, eB): a NaN first operand stays
        return e.astype(np.float32), denA, denB


def count_guards(F, W, H):
    """(dminA, dminB) = ((2^28 EA)^2, (2^28 EB)^2) as store_model (k_match.hip) computes them for the image size W x H"""
    aF = np.abs(np.asarray(F, np.float64).reshape(9))
    X, Y, u = float(W), float(H), 2.0 ** -47
    EB = u * (X * (aF[0] * X + aF[1] * Y + aF[2]) + Y * (aF[3] * X + aF[4] * Y + aF[5]) + (aF[6] * X + aF[7] * Y + aF[8]))
    EA = u * (X * (aF[0] * X + aF[3] * Y + aF[6]) + Y * (aF[1] * X + aF[4] * Y + aF[7]) + (aF[2] * X + aF[5] * Y + aF[8]))
    gA, gB = 268435456.0 * EA, 268435456.0 * EB
    return gA * gA, gB * gB


def sample_models(p1, p2, count):
    """the models of the first `count` samples findFundamentalMat's RANSAC draws for these pairs: [(sample number, F 3x3), ...]"""
    from oracle import oracle
    out = []
    for k, s in enumerate(oracle.ransac_samples(p1, p2, count)):
        for F in oracle.seven_point(p1[s], p2[s]):
            out.append((k, F))
    return out


BAND = 2.0 ** -22


def scene_facts(p, s):
    """What the oracle alone says about a hand-built scene -- the preconditions of the GPU tests (tests/test_ransac_scenes_cpu.py):
      ts          the eight stage counters of the oracle's stage 4 ([1] = candidates reaching the RANSAC, [4], [5] = samples visited)
      near        (model, pair) tests whose error is within 2^-22 of 1, over the models of the first 160 samples
      win_near    ... on the winning model (-1: no model)
      nan, inf    tests whose error is NaN (|l|^2 == 0 and d == 0) / infinite (|l|^2 == 0 alone), over the models of the first 320 samples
                  (8..14 candidates: of LMedS's 300) -- every one of them is scored by the one-lane forms' first chunk
      small       tests of an epipole pair (both points at (320, 240)) with 0 < |l|^2 < the guard of store_model, same models as `near`
      hair        tests with 1 + 2^-24 < error <= 1 + 2^-20 (an outlier the screen's own `lo` must not reach), same models as `near`
      guarded     tests with the error within 2^-20 of 1 on a line whose |l|^2 is positive but below the guard, same models as `near`:
                  pairs whose verdict the guards, not the band, keep away from the matrix cores' rounding"""
    from oracle import oracle
    _, ts = oracle_track(p, s)
    p1, p2 = s["p1"], s["p2"]
    n = len(p1)
    f = dict(ts=[int(v) for v in ts], near=0, win_near=-1, nan=0, inf=0, small=0, hair=0, guarded=0)
    if n < 8:
        return f
    ep = (p1 == (320, 240)).all(1) & (p2 == (320, 240)).all(1)
    for k, F in sample_models(p1, p2, 300 if n <= 14 else 320):
        e, denA, denB = fm_error_terms(F, p1, p2)
        f["nan"] += int(np.isnan(e).sum()); f["inf"] += int(np.isinf(e).sum())
        if k >= 160:
            continue
        e64 = e.astype(np.float64)
        f["near"] += int((np.abs(e64 - 1.0) <= BAND).sum())
        gA, gB = count_guards(F, s["W"], s["H"])
        f["small"] += int((((denA > 0) & (denA < gA)) | ((denB > 0) & (denB < gB)))[ep].sum())
        f["hair"] += int(((e64 > 1.0 + 2.0 ** -24) & (e64 <= 1.0 + 2.0 ** -20)).sum())
        f["guarded"] += int(((np.abs(e64 - 1.0) <= 2.0 ** -20) & (((denA > 0) & (denA < gA)) | ((denB > 0) & (denB < gB)))).sum())
    cnt, mask, Fw, best, visited = oracle.ransac_fundamental(p1, p2)
    if best >= 0:
        e, _, _ = fm_error_terms(Fw, p1, p2)
        f["win_near"] = int((np.abs(e.astype(np.float64) - 1.0) <= BAND).sum())
    return f
