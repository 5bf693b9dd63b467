"""The scenes of tests/gftt_scenes.py really reach what they are named for, on the walk (tests/gftt_ref.py); the walk's response is held
to numpy.linalg.eigvalsh on the same integer tensors, and its selection to a brute-force greedy and to the round-based form the device
runs.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gftt_ref as G                                                                   # noqa: E402
import gftt_scenes as GS                                                               # noqa: E402

F = np.float32


def one(name):
    s = GS.scene(name)
    (pts, resp, info, rmap), = GS.reference(name)
    return s, pts, resp, info, rmap


def test_sizes_and_names():
    names = [s.name for s in GS.scenes()]
    assert len(set(names)) == len(names)
    for s in GS.scenes():
        assert 1 <= len(s.jobs) <= 8
        for img, seeds, cap in s.jobs:
            assert img.dtype == np.uint8 and 8 <= img.shape[1] <= 321 and 8 <= img.shape[0] <= 243 and 0 <= cap <= GS.MAX_KPS
            assert seeds is None or len(seeds) <= GS.MAX_KPS


def test_seam_scenes_have_candidates_on_the_seams():
    sizes = ((97, 65), (95, 63), (127, 33), (65, 97), (321, 243))
    # last tiles of 1 pixel and of tile - 1: 32 x 32 (response), 64 x 4 (candidates)
    assert {1, 31} <= {w % 32 for w, h in sizes} and {1, 31} <= {h % 32 for w, h in sizes}
    assert {1, 63} <= {w % 64 for w, h in sizes} and {1, 3} <= {h % 4 for w, h in sizes}
    for w, h in sizes:
        s, pts, resp, info, rmap = one("seams_%dx%d_b3" % (w, h))
        m, thr, ys, xs = G.candidates(rmap, s.ref_params().quality)
        near = lambda v, t: ((v % t) <= 1) | ((v % t) >= t - 2)                           # noqa: E731
        assert (near(xs, 32) & near(ys, 32)).sum() >= 1 or min(w, h) < 64
        assert near(xs, 32).sum() >= 4 and near(ys, 4).sum() >= 4 and info[0] >= 8
    assert one("tiny_8x8_b3")[0].jobs[0][0].shape == (8, 8)


def test_saturated_scenes_carry_the_largest_sums():
    for block in (3, 5, 7):
        for name in ("saturated_quadrants_b%d", "saturated_checker2_b%d"):
            img = GS.scene(name % block).jobs[0][0]
            assert set(np.unique(img)) == {0, 255}
            a, b, c = G.tensor(img, block)
            assert (a + c).max() >= block * block * 300000 and (a + c).max() <= block * block * 1300500 < 2 ** 31
    a, b, c = G.tensor(GS.scene("saturated_checker2_b7").jobs[0][0], 7)
    assert ((a - c) ** 2 + 4 * b * b).max() < 2 ** 53


def test_perfect_square_scene():
    a, b, c = G.tensor(GS.scene("perfect_square_b3").jobs[0][0], 3)
    d = (a - c) ** 2 + 4 * b * b
    k = np.rint(np.sqrt(d.astype(np.float64))).astype(np.int64)
    assert ((k * k == d) & (b != 0)).sum() >= 10 and (np.abs(k * k - d) == 1).sum() >= 5


def test_flat_and_border_ring():
    for block in (3, 5, 7):
        s, pts, resp, info, rmap = one("flat_b%d" % block)
        assert rmap.max() == 0 and info == (0, 0, 0)
    s, pts, resp, info, rmap = one("border_ring_only")
    y, x = np.unravel_index(rmap.argmax(), rmap.shape)
    assert rmap.max() > 0 and x == 0 and info == (0, 0, 0)
    assert (rmap[1:-1, 1:-1] > F(0.01) * rmap.max()).any()                                # pixels above thr exist, none is a maximum


def test_threshold_scenes():
    s, pts, resp, info, rmap = one("threshold_equal_dropped")
    thr = F(F(0.25) * rmap.max())
    assert rmap[30, 30] == 12 * 200 * 200 and rmap[30, 60] == thr == 12 * 100 * 100 and info == (1, 1, 0)
    s, pts, resp, info, rmap = one("threshold_one_level_stronger_kept")
    assert rmap[30, 60] == 12 * 101 * 101 > thr and info == (2, 2, 0) and pts.tolist() == [[30, 30], [60, 30]]


def test_plateaus_and_ties():
    s, pts, resp, info, rmap = one("plateau_adjacent_pair")
    assert rmap[30, 40] == rmap[30, 41] == rmap.max() and info == (1, 2, 0) and pts.tolist() == [[40, 30]]
    assert one("plateau_adjacent_pair_md0")[1].tolist() == [[40, 30], [41, 30]]
    s, pts, resp, info, rmap = one("ties_raster_order")
    assert len(set(resp.tolist())) == 1 and pts.tolist() == [[30, 20], [100, 20], [20, 70], [90, 70]]
    assert one("ties_cut_by_max_corners")[1].tolist() == [[30, 20], [100, 20]] and one("ties_cut_by_max_corners")[3] == (2, 4, 0)
    assert one("ties_cut_by_cap")[1].tolist() == [[30, 20], [100, 20], [20, 70]]


def test_distance_scenes():
    assert 12 * 12 + 16 * 16 == 20 * 20 and 12 * 12 + 15 * 15 < 20 * 20
    assert one("distance_exact_kept")[1].tolist() == [[40, 30], [52, 46], [90, 60], [78, 44]]
    assert one("distance_inside_dropped")[1].tolist() == [[40, 30], [90, 60]] and one("distance_inside_dropped")[3][1] == 4
    n = one("min_distance_0")[3][1]
    assert n > GS.MAX_KPS and one("min_distance_0")[3][0] == GS.MAX_KPS == one("min_distance_1")[3][0]
    assert 1 <= one("min_distance_255")[3][0] <= 4


def rounds_greedy(xs, ys, md, cell, pre_rejected=None):
    """the device's form of the walk: candidates by rank in a cell grid; rounds in which an undecided candidate is rejected by an accepted
    stronger one within reach and accepted when no stronger one within reach is undecided.  -> (accepted mask, rounds)"""
    n = len(xs)
    state = np.zeros(n, np.int8) if pre_rejected is None else np.where(pre_rejected, 2, 0).astype(np.int8)
    grid = {}
    for i in range(n):
        grid.setdefault((xs[i] // cell, ys[i] // cell), []).append(i)
    near = []
    for i in range(n):
        cx, cy = xs[i] // cell, ys[i] // cell
        near.append([j for yy in (cy - 1, cy, cy + 1) for xx in (cx - 1, cx, cx + 1) for j in grid.get((xx, yy), ())
                     if j < i and (xs[i] - xs[j]) ** 2 + (ys[i] - ys[j]) ** 2 < md * md])
    rounds = 0
    while (state == 0).any():
        rounds += 1
        assert rounds <= n
        old = state.copy()                                                                # the slowest schedule: nobody sees this round's writes
        for i in np.flatnonzero(old == 0):
            if any(old[j] == 1 for j in near[i]):
                state[i] = 2
            elif not any(old[j] == 0 for j in near[i]):
                state[i] = 1
        assert old[np.flatnonzero(old == 0)[0]] != state[np.flatnonzero(old == 0)[0]]     # the strongest undecided one was decided
    return state == 1, rounds


def brute_greedy(xs, ys, md):
    acc = []
    for i in range(len(xs)):
        if all((xs[i] - xs[j]) ** 2 + (ys[i] - ys[j]) ** 2 >= md * md for j in acc):
            acc.append(i)
    return acc


def test_decision_chains_are_deep():
    for name, depth in (("chain_row", 64), ("chain_diagonal", 40)):
        s, pts, resp, info, rmap = one(name)
        p = s.ref_params()
        m, thr, ys, xs = G.candidates(rmap, p.quality)
        want = (GS.chain_row if name == "chain_row" else GS.chain_diagonal)()[1]
        assert list(zip(xs.tolist(), ys.tolist())) == want                               # the dots, strongest first, nothing else
        cell = max(p.min_distance, (321 + 63) // 64)
        acc, rounds = rounds_greedy(xs.tolist(), ys.tolist(), p.min_distance, cell)
        assert rounds >= depth and acc.tolist() == [k % 2 == 0 for k in range(len(want))]
        assert pts.tolist() == [list(want[k]) for k in range(0, len(want), 2)]
    cells = {(x // 6, y // 6) for x, y in GS.chain_diagonal()[1]}
    assert len({c[0] for c in cells}) > 10 and len({c[1] for c in cells}) > 10


def test_seed_scenes():
    s, pts, resp, info, rmap = one("seeds_exact_and_inside")
    kept = {tuple(p) for p in pts.tolist()}
    assert (50, 50) in kept and (100, 50) not in kept and (150, 50) not in kept and (200, 50) not in kept and (50, 120) in kept and info[1] == 10
    s, pts, resp, info, rmap = one("seeds_float32_rule")
    seeds = s.jobs[0][1]
    for (cx, cy), rows in (((100, 120), seeds[0:3]), ((150, 120), seeds[3:6])):
        for sx, sy in rows:
            fx, fy = F(cx) - sx, F(cy) - sy
            assert not (fx * fx + fy * fy < F(400)) and (float(cx) - float(sx)) ** 2 + (float(cy) - float(sy)) ** 2 < 400.0
    assert info == (10, 10, 0)
    s, pts, resp, info, rmap = one("seeds_not_finite")
    assert info == (9, 10, 0) and [150, 50] not in pts.tolist()
    s, pts, resp, info, rmap = one("seeds_outside")
    assert len(G.valid_seeds(s.jobs[0][1], 321, 243)) == 4 and info == (9, 10, 0) and [250, 120] not in pts.tolist()
    assert one("seeds_none_but_a_pointer")[3] == (10, 10, 0) and one("seeds_md0_ignored")[3] == (10, 10, 0)


def test_overflow_scene():
    s, pts, resp, info, rmap = one("overflow_lattice")
    assert s.cand_cap() == 1024 and info[1] > 1024 and info == (0, info[1], 1) and len(pts) == 0
    s2, pts2, resp2, info2, _ = one("lattice_with_room")
    assert info2[1] == info[1] <= s2.cand_cap() and info2[2] == 0 and info2[0] > 100


def test_mixed_call():
    s = GS.scene("mixed_call")
    infos = [r[2] for r in GS.reference("mixed_call")]
    assert len({j[0].shape for j in s.jobs}) == 5 and infos[1] == (0, 0, 0) and s.jobs[2][2] == 0 and infos[2][0] == 0 and infos[2][1] > 0
    assert infos[3][0] == 17 and infos[0][0] > 100


def test_response_against_eigvalsh():
    """lambda_min of [[a, b], [b, c]].  The walk: s and D are exact; the correctly rounded sqrt errs by at most 2^-53 sqrt(D) <= 2^-53 s,
    the subtraction and the halving by at most 2^-53 s more in all, so |lambda_walk - lambda| <= 2^-52 s before the float32 rounding,
    which adds half a float32 ulp of the result.  eigvalsh (LAPACK, backward stable): |lambda_eig - lambda| <= p(n) eps ||A||_2 with
    eps = 2^-52, ||A||_2 <= s and p(2) taken as 10, the 'modest' constant of the LAPACK Users' Guide's error bounds."""
    rng = np.random.default_rng(1)
    imgs = [GS.blocks(96, 80, 5, 31), rng.integers(0, 256, (64, 64), dtype=np.uint8), GS.scene("saturated_checker2_b7").jobs[0][0], GS._psq()]
    for img in imgs:
        for block in (3, 5, 7):
            a, b, c = G.tensor(img, block)
            walk = G.response_map(img, block)
            mats = np.stack([np.stack([a, b], -1), np.stack([b, c], -1)], -2).astype(np.float64)
            lam = np.maximum(np.linalg.eigvalsh(mats)[..., 0], 0.0)
            s = (a + c).astype(np.float64)
            tol = 0.5 * np.spacing(walk).astype(np.float64) + 2.0 ** -52 * s + 10 * 2.0 ** -52 * s
            assert (np.abs(walk.astype(np.float64) - lam) <= tol).all()


def test_selection_against_brute_force_and_rounds():
    rng = np.random.default_rng(3)
    for t in range(6):
        w, h = int(rng.integers(40, 160)), int(rng.integers(40, 120))
        img = GS.blocks(w, h, int(rng.integers(3, 7)), 100 + t)
        md = int(rng.integers(1, 25))
        p = G.GfttParams(min_distance=md, block=(3, 5, 7)[t % 3])
        seeds = rng.uniform(-3, max(w, h), (12, 2)).astype(F) if t % 2 else None
        pts, resp, info, rmap = G.detect(img, seeds, 1 << 20, p)
        m, thr, ys, xs = G.candidates(rmap, p.quality)
        xs, ys = xs.tolist(), ys.tolist()
        sd = G.valid_seeds(seeds, w, h)
        hit = np.array([bool(len(sd)) and bool((((F(x) - sd[:, 0]) ** 2 + (F(y) - sd[:, 1]) ** 2) < F(md * md)).any()) for x, y in zip(xs, ys)], bool)
        keep = [i for i in range(len(xs)) if not hit[i]]
        acc = [keep[i] for i in brute_greedy([xs[i] for i in keep], [ys[i] for i in keep], md)]
        assert pts.tolist() == [[xs[i], ys[i]] for i in acc] and info[1] == len(xs)
        mask, rounds = rounds_greedy(xs, ys, md, max(md, (max(w, h) + 63) // 64), pre_rejected=hit)
        assert np.flatnonzero(mask).tolist() == acc
