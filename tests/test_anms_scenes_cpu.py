"""What every scene of tests/anms_scenes.py reaches, pinned on the oracle and the plain numpy walk alone (no GPU): a scene that stopped
reaching its case would let the GPU test pass for nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anms_scenes as A                                         # noqa: E402


def check_walk_is_the_oracle(letter):
    """radii() + order_of() give the oracle's order, so what the walk says about a scene holds for the oracle"""
    for i, (name, k, num, w, h) in enumerate(A.cases(letter)):
        assert np.array_equal(A.order_of(A.radii(k), num), A.expected(letter, i)), name


def test_lists_are_valid_inputs():
    for letter in A.SCENES:
        for name, k, num, w, h in A.cases(letter):
            pos = k["y"].astype(np.int64) * w + k["x"].astype(np.int64)
            assert w * h < 1 << 24 and (np.diff(pos) > 0).all() and not np.isnan(k["response"]).any(), name
            assert len(k) == 0 or (k["x"].min() >= 0 and k["x"].max() < w and k["y"].min() >= 0 and k["y"].max() < h), name


def test_a_tiny_lists():
    got = [(len(k), num, len(A.expected("a", i))) for i, (_, k, num, _, _) in enumerate(A.cases("a"))]
    assert got == [(0, 0, 0), (0, 1, 0), (0, 5, 0), (1, 0, 0), (1, 1, 1), (1, 6, 1), (2, 0, 0), (2, 1, 1), (2, 2, 2), (2, 7, 2)]
    check_walk_is_the_oracle("a")


def test_b_the_boundary_of_the_comparison():
    lo, hi = A.boundary_pair(np.float32(100.0))
    assert float(lo) < 0.9 * 100.0 and not float(hi) < 0.9 * 100.0 and np.nextafter(lo, np.float32(np.inf)) == hi
    (_, below, _, _, _), (_, at, _, _, _) = A.cases("b")
    ra, rb = A.radii(below), A.radii(at)
    assert ra[0] == 4.0 and rb[0] == np.float32(50 * 50 + 30 * 30) and ra[1] == rb[1] and np.isinf(ra[2])       # A's radius: to B, or to S
    assert A.expected("b", 0).tolist() == [2, 1, 0] and A.expected("b", 1).tolist() == [2, 0, 1]
    check_walk_is_the_oracle("b")


def test_c_ties_and_zeros():
    by = {name[2:]: (k, A.radii(k)) for name, k, _, _, _ in A.cases("c")}
    for tag in ("equal positive", "zero", "signed zeros"):
        k, rad = by[tag]
        first = A.rank_order(k)[0]
        d0 = ((k["x"] - k["x"][first]) ** 2 + (k["y"] - k["y"][first]) ** 2).astype(np.float32)
        assert (np.delete(rad, first) == np.delete(d0, first)).all(), tag      # nothing is robustly stronger: the distance to rank 0
    k, _ = by["signed zeros"]
    assert np.signbit(k["response"]).any() and not np.signbit(k["response"]).all()
    assert not np.signbit(k["response"][A.rank_order(k)[0]])                  # +0 ranks above -0
    k, rad = by["equal negative"]
    assert A.prefix_lengths(k).tolist() == list(range(len(k)))                # every corner sees all earlier indices
    for i in range(1, len(k)):
        assert rad[i] == ((k["x"][:i] - k["x"][i]) ** 2 + (k["y"][:i] - k["y"][i]) ** 2).min()
    check_walk_is_the_oracle("c")


def test_d_the_cut_inside_a_tie_group():
    (name, k, cut, _, _), = A.cases("d")
    rad = A.radii(k)
    full = A.order_of(rad, len(k))
    assert len(k) == 1024 and len(np.unique(k["response"])) == 5 and 4 * len(np.unique(rad)) < len(k)      # many radii are equal
    assert rad[full[cut - 1]] == rad[full[cut]] and len(A.expected("d", 0)) == cut
    check_walk_is_the_oracle("d")


def test_e_the_far_cluster():
    (name, k, num, w, h), = A.cases("e")
    strong = (k["x"] < 8) & (k["y"] < 8)
    assert strong.sum() == 64 and len(k) == 4064 and (k["response"][~strong].astype(np.float64) < 0.9 * float(k["response"][strong].min())).all()
    L = A.prefix_lengths(k)
    assert (L[64:] >= 64).all() and (L[64:] > A.DIRECT_L).sum() >= 2000 and (L[64:] <= A.DIRECT_L).sum() >= 50      # both search paths
    rad = A.radii(k)
    assert (rad[~strong] >= 500.0 ** 2).sum() >= 50              # nearest robustly stronger corner: hundreds of pixels away
    check_walk_is_the_oracle("e")


def test_f_the_edge_sizes():
    assert [len(k) for _, k, _, _, _ in A.cases("f")] == list(A.EDGE_N)
    assert {63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049} <= set(A.EDGE_N)
    for i, (name, k, num, _, _) in enumerate(A.cases("f")):
        assert (k["response"] < 0).any() and 0 < num < len(k) and len(A.expected("f", i)) == num, name
        if len(k) >= 1023:
            L = A.prefix_lengths(k)
            assert (L > A.DIRECT_L).any() and ((L > 1) & (L <= A.DIRECT_L)).any(), name
    for i in (0, 1, 2, 4):
        name, k, num, _, _ = A.cases("f")[i]
        assert np.array_equal(A.order_of(A.radii(k), num), A.expected("f", i)), name


def test_g_float_distances_are_not_integer_distances():
    (name, k, num, w, h), = A.cases("g")
    assert (w, h) == (16000, 1000)
    rf, re = A.radii(k), A.radii(k, exact=True)
    finite = np.isfinite(rf)
    assert (rf[finite].astype(np.float64) != re[finite]).sum() >= 20          # rounded distances
    assert not np.array_equal(A.order_of(rf, num), A.order_of(re, num))
    assert np.array_equal(A.order_of(rf, num), A.expected("g", 0))            # the oracle computes in float
    assert (A.prefix_lengths(k) > A.DIRECT_L).sum() >= 50


def test_h_the_full_lattice():
    (name, k, num, w, h), = A.cases("h")
    assert len(k) == w * h == 32768 and len(np.unique(k["response"])) == 16 and len(A.expected("h", 0)) == num == 2000
