"""Preconditions of tests/test_gpu_faster_scenes.py, on tests/faster_ref.py and the oracle alone (no GPU): where a scene of
tests/faster_scenes.py predicts its answer from its construction, the reference gives exactly that answer; and every scene has what it
is named for -- arcs on both sides of 12 and of the threshold, negative radicands, computed zeros, sums beyond 2^24, corners on the
columns of the border rule and on both sides of the tile seams, cells of the NMS grid with several corners, decisions that cross the
chunk boundary -- counted from the reference's lists and the geometry constants.  Every count is printed (pytest -s)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                                               # noqa: E402
import faster_scenes as FS                                                           # noqa: E402


def O():
    from oracle import oracle
    return oracle


def raw(s, o=0):
    """the reference's corners of octave o before the NMS, raster order"""
    return F.corners(FS.pyramid(s["name"])[o], s["t"], s["win"])


def xy(k):
    return list(zip(k["x"].astype(int).tolist(), k["y"].astype(int).tolist()))


def walk(s, k):
    return FS.grid_walk(list(zip(k["x"].tolist(), k["y"].tolist(), k["response"].tolist())), s["md"], s["w"], s["h"], F.kps_to_detect(s["nfeats"], s["n_oct"])[0])


def test_generators_are_deterministic_and_small():
    names = []
    for f, gen in FS.FAMILIES.items():
        a, b = FS.scenes(f), gen()
        assert [s["name"] for s in a] == [s["name"] for s in b], f
        for s, t in zip(a, b):
            assert s["img"].tobytes() == t["img"].tobytes() and s["expect"] == t["expect"], s["name"]
            assert s["w"] <= 385 and s["h"] <= 241 and 1 <= s["win"] <= 15 and s["family"] == f, s["name"]
            assert max(F.kps_to_detect(s["nfeats"], s["n_oct"])) <= 4096, s["name"]           # far from the unguarded hash bound of the chunked NMS
        names += [s["name"] for s in a]
    assert len(set(names)) == len(names)
    counts = {f: len(FS.scenes(f)) for f in FS.FAMILIES}
    print("scenes per family:", counts)
    assert counts == {"rings": 14, "response": 16, "sizes": 12, "nms": 16}


def test_every_scene_has_corners_unless_named_empty():
    """no GPU case compares empty against empty: every octave of every scene has a corner, and its lists fit the slots of a 4096-entry
    context without the NMS -- unless the scene is marked as having none"""
    for f in FS.FAMILIES:
        for s in FS.scenes(f):
            n = [len(raw(s, o)) for o in range(s["n_oct"])]
            if s.get("none"):
                assert n == [0] * s["n_oct"], (s["name"], n)
            else:
                assert all(0 < c <= 4096 >> o for o, c in enumerate(n)), (s["name"], n)
                assert all(len(r[0]) > 0 for r in FS.reference(s["name"], True)), s["name"]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. rings
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_rings_reference_gives_the_predicted_verdicts():
    cells, corners, by_t = 0, 0, {}
    xs_seen, ys_seen = set(), set()
    for s in FS.scenes("rings"):
        got = set(xy(raw(s)))
        for x, y, want in s["expect"]["centres"]:
            assert ((x, y) in got) == want, (s["name"], x, y, want)
            if want:
                xs_seen.add(x); ys_seen.add(y)
        assert all(3 <= x < s["w"] - 3 and 3 <= y < s["h"] - 3 for x, y in got), s["name"]        # x = w - 3, y = h - 3: never listed
        cells += len(s["expect"]["centres"]); corners += sum(c for _, _, c in s["expect"]["centres"])
        by_t[s["t"]] = by_t.get(s["t"], 0) + len(s["expect"]["centres"])
    print("ring cells:", cells, "of them corners:", corners, "per threshold:", by_t)
    assert (cells, corners) == RING_CELLS
    assert sorted(by_t) == [1, 20, 254]
    # the cases: every start of arcs of 11, 12, 13, both signs, on and beyond the threshold
    for t, c in ((20, 100), (1, 100)):
        cases = FS.ring_cases(t, c)
        for length in (11, 12, 13):
            for sgn in (1, -1):
                for d in (t, t + 1):
                    v = c + sgn * d
                    arcs = {tuple(r) for cc, r, _ in cases if cc == c and r.count(v) == length and r.count(c) == 16 - length and is_one_arc(r, v)}
                    assert len(arcs) == 16, (t, length, sgn, d, len(arcs))
    # a corner stands on every special column and row, and on every row a thread owns first and last in its tile
    assert {3, 66, 67, 130, 131, FS.W0 - 4} <= xs_seen and {3, 34, 35, 66, 67, FS.H0 - 4} <= ys_seen, (sorted(xs_seen), sorted(ys_seen))
    assert {(y - 3) % 32 for y in ys_seen} >= {0, 1, 2, 3, 28, 29, 30, 31}


def is_one_arc(ring, v):
    return sum(1 for i in range(16) if ring[i] == v and ring[i - 1] != v) == 1


RING_CELLS = (2562, 793)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. response
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_response_dots_and_computed_zeros():
    n = 0
    for s in FS.scenes("response"):
        if "resp" not in s["expect"]:
            continue
        k = raw(s)
        got = {p: r for p, r in zip(xy(k), k["response"])}
        for p, want in s["expect"]["resp"].items():
            assert p in got and got[p].tobytes() == np.float32(want).tobytes(), (s["name"], p, got.get(p), want)          # (bits: +0.0 is not -0.0)
            assert F.in_klt_border(p[0], p[1], s["w"], s["h"], s["win"])
        if "dots" in s["name"]:
            assert len(k) == len(s["expect"]["resp"]) == 255 - int(s["img"].min()) - s["t"], s["name"]      # every amplitude from t + 1 up, nothing else is a corner
        n += len(s["expect"]["resp"])
    z = FS.scene("response-zero-rings")
    k = raw(z)
    zeros = k[k["response"] == 0]
    print("predicted responses:", n, "computed zeros:", len(zeros))
    assert n == 235 + 215 + 54 + 1 + 10 and len(zeros) >= 6 and not np.signbit(zeros["response"]).any()
    kept = FS.reference(z["name"], True)[0][0]
    assert len(kept) == F.kps_to_detect(z["nfeats"], 1)[0] < len(k) and 2 <= (kept["response"] == 0).sum() < len(zeros)      # the cap cuts among equal computed zeros: by position


def test_response_clamp_scenes_have_negative_radicands():
    n = 0
    for win in (2, 4):
        s = FS.scene("response-clamp-win%d" % win)
        k = raw(s)
        got = {p: r for p, r in zip(xy(k), k["response"])}
        for x, y in s["centres"]:
            sums = F.klt_sums(s["img"], x, y, win)
            rad = FS.klt_rad(*sums, win)
            assert rad < 0 and (x, y) in got, (s["name"], x, y, sums, rad)
            f = np.float32
            K = f(0.5) / f((2 * win + 1) ** 2)
            assert got[x, y] == f(0.5) * (f(sums[0]) * K + f(sums[2]) * K)       # the clamp: sqrt(0), the response is half the trace
            n += 1
    print("corners with a negative radicand:", n)
    assert n == 8


def test_response_negative_scene_orders_negative_keys():
    """ten corners whose response is below zero with the sign bit set, of five values, equal ones on both sides of the seams; they rank
    behind the computed zeros, and the cap cuts among them: value, then position, decide which of them stay"""
    s = FS.scene("response-negative")
    k = raw(s)
    pos = xy(k)
    neg = np.flatnonzero(k["response"] < 0)
    assert sorted(pos[i] for i in neg) == sorted(s["centres"]) and len(neg) == 10 and np.signbit(k["response"][neg]).all()
    values = sorted(set(k["response"][neg].tolist()), reverse=True)
    assert values == [-2.0 ** -22, -2.0 ** -21, -2.0 ** -20, -2.0 ** -19, -2.0 ** -18], values
    for x, y, p, q, amps in FS.NEGATIVE_CELLS:
        B = sum(a * a for a in amps)
        assert F.klt_sums(s["img"], x, y, 1) == (p * p * B, p * q * B, q * q * B), (x, y)
    assert any(x <= 66 for x, _ in s["centres"]) and any(x >= 67 for x, _ in s["centres"]) and {66, 67, 130, 131} <= {x for x, _ in s["centres"]}
    zeros = [i for i in range(len(k)) if k["response"][i] == 0]
    assert sorted(pos[i] for i in zeros) == sorted(s["zeros"]) and not np.signbit(k["response"][zeros]).any() and (k["response"] > 0).sum() >= 3
    cap = F.kps_to_detect(s["nfeats"], 1)[0]
    order = [int(i) for i in O().nms_copy(k, s["md"], s["w"], s["h"], cap)]
    everything = [int(i) for i in O().nms_copy(k, s["md"], s["w"], s["h"], len(k))]
    assert len(everything) == len(k) and len(order) == cap and everything[-10:] == sorted(neg, key=lambda i: (-float(k["response"][i]), i))      # cells of one pixel: nothing is suppressed
    kept_neg = [i for i in order if k["response"][i] < 0]
    print("negative responses:", len(neg), "kept under the cap:", len(kept_neg), "of", cap)
    assert 3 < len(kept_neg) < 10 and k["response"][kept_neg[-1]] == k["response"][everything[cap]]          # the cut falls inside a group of equal negative values


def test_response_largest_sums_round_in_float():
    for name in ("response-blocks2-win15", "response-stripes2-win15"):
        s = FS.scene(name)
        k = raw(s)
        inside = [(x, y) for x, y in xy(k) if F.in_klt_border(x, y, s["w"], s["h"], 15)]
        big = [max(F.klt_sums(s["img"], x, y, 15)) for x, y in inside]
        print(name, "corners with a response:", len(inside), "largest sum:", max(big))
        assert len(inside) >= 20 and max(big) > 1 << 24 and max(big) < 1 << 31
        assert any(v > 1 << 24 and int(np.float32(v)) != v for v in big)        # the int -> float conversion does round


def test_response_border_and_seams():
    for win in (1, 4, 15):
        s = FS.scene("response-border-win%d" % win)
        k = raw(s)
        pos = xy(k)
        for c in FS.border_columns(s["w"], win):
            assert any(x == c for x, _ in pos), (win, "column", c)
        for c in FS.border_columns(s["h"], win):
            assert any(y == c for _, y in pos), (win, "row", c)
        zero = sum(1 for (x, y), r in zip(pos, k["response"]) if not F.in_klt_border(x, y, s["w"], s["h"], win))
        assert (zero > 0) == (win > 1) and (k["response"] > 0).sum() > 100, (win, zero)      # at win 1 the rule never bites: 3 >= win + 1
        assert s["img"][:, 0].max() - s["img"][:, 0].min() > 200 and s["img"][-1].max() - s["img"][-1].min() > 200      # texture up to the edge
    s = FS.scene("response-seams-win15")
    pos = [p for p in xy(raw(s)) if F.in_klt_border(p[0], p[1], s["w"], s["h"], 15)]
    for qx in ((59, 66), (67, 74)):
        for qy in ((27, 34), (35, 42)):                                        # a response window over four tiles from each of the four
            assert any(qx[0] <= x <= qx[1] and qy[0] <= y <= qy[1] for x, y in pos), (qx, qy)
    assert all(any(x == c for x, _ in pos) for c in (66, 67)) and all(any(y == c for _, y in pos) for c in (34, 35))


def test_response_equal_patches_tie():
    s = FS.scene("response-equal-md3")
    k = raw(s)
    n = len(FS.equal_patch_positions())
    vals, cnt = np.unique(k["response"].view(np.uint32), return_counts=True)
    assert len(k) >= 2 * n and (cnt % n == 0).all(), cnt                          # every response n times: once per copy of the patch
    x0, y0 = FS.equal_patch_positions()[1]
    assert x0 < 66 < 67 < x0 + 9 and y0 < 34 < 35 < y0 + 9
    for md in (3, 7):                                                            # the cap cuts inside a group of equal responses: position decides
        s = FS.scene("response-equal-md%d" % md)
        cap = F.kps_to_detect(s["nfeats"], 1)[0]
        order = [int(i) for i in O().nms_copy(k, md, s["w"], s["h"], len(k))]
        assert cap < len(order) and k["response"][order[cap - 1]] == k["response"][order[cap]] and xy(k)[order[cap - 1]] != xy(k)[order[cap]], (md, cap)
        assert len(FS.reference(s["name"], True)[0][0]) == cap


# ---------------------------------------------------------------------------------------------------------------------------------------
# 3. sizes
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_sizes_reach_their_edges():
    shapes = {(w, h): [im.shape[::-1] for im in FS.pyramid("sizes-%dx%d-noise" % (w, h))] for w, h, _, _ in FS.SIZES}
    assert shapes == {(198, 102): [(198, 102), (99, 51), (49, 25)], (199, 103): [(199, 103), (99, 51), (49, 25)], (135, 135): [(135, 135), (67, 67), (33, 33)],
                      (135, 71): [(135, 71), (67, 35), (33, 17)], (104, 72): [(104, 72), (52, 36), (26, 18), (13, 9)]}
    s = FS.scene("sizes-199x103-noise")                                          # the last tile: one column wide (x = 195), one row high (y = 99)
    pos = xy(raw(s))
    assert (199 - 4 - 3) % FS.FK_W == 0 and (103 - 4 - 3) % FS.FK_H == 0 and any(x == 195 for x, _ in pos) and any(y == 99 for _, y in pos)
    s = FS.scene("sizes-198x102-noise")                                          # whole tiles only
    pos = xy(raw(s))
    assert (198 - 6) % FS.FK_W == 0 and (102 - 6) % FS.FK_H == 0 and any(x == 194 for x, _ in pos) and any(y == 98 for _, y in pos)
    s = FS.scene("sizes-135x135-noise")                                          # octave 2 is 33 x 33: (16, 16) alone can carry a response
    k = raw(s, 2)
    carry = [p for p in xy(k) if F.in_klt_border(p[0], p[1], 33, 33, 15)]
    assert carry == [(16, 16)] and k["response"][xy(k).index((16, 16))] > 0 and (k["response"] != 0).sum() == 1
    s = FS.scene("sizes-135x71-noise")                                           # octave 2 is 33 x 17: no response exists
    k = raw(s, 2)
    assert len(k) > 0 and not k["response"].any()
    k = raw(FS.scene("sizes-104x72-noise"), 3)                                   # octave 3 is 13 x 9: an interior of 7 x 3, no response
    assert len(k) > 0 and not k["response"].any() and all(3 <= x < 10 and 3 <= y < 6 for x, y in xy(k))
    for w, h in FS.RING2_SIZES:                                                  # octave 1 keeps corners on its first and last valid column and row
        s = FS.scene("sizes-%dx%d-rings2" % (w, h))
        pos = set(xy(raw(s, 1)))
        assert {(3, 3), (95, 3), (3, 47), (95, 47)} <= pos, sorted(pos)[:8]


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. nms
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_nms_reference_keeps_the_predicted_dots():
    total = 0
    for s in FS.scenes("nms"):
        if "kept" not in s["expect"]:
            continue
        k = raw(s)
        plan = s.get("plan", [])
        assert xy(k) == [(x, y) for x, y, _ in plan], s["name"]                    # the dots and nothing else, in raster order
        assert all(r.tobytes() == FS.dot_response(a).tobytes() for r, (_, _, a) in zip(k["response"], plan)), s["name"]
        cap = F.kps_to_detect(s["nfeats"], s["n_oct"])[0]
        order = O().nms_copy(k, s["md"], s["w"], s["h"], cap) if len(k) else []
        assert [xy(k)[i] for i in order] == s["expect"]["kept"], s["name"]
        total += len(s["expect"]["kept"])
    print("dots kept over the family:", total)
    row = [(9 + 6 * i, 9) for i in range(60)]
    kept = {n: FS.scene("nms-" + n)["expect"]["kept"] for n in ("row-falling", "row-rising", "row-equal", "md2", "md3", "cap-equal-10", "cap-falling-14", "cap-1")}
    assert kept["row-falling"] == row[0::2] and kept["row-equal"] == row[0::2]      # accept, reject, accept, ...: 59 decisions deep
    assert kept["row-rising"] == row[::-1][0::2]
    assert kept["md2"] == kept["md3"] == row                                       # cells of one pixel either way
    assert kept["cap-equal-10"] == row[0::2][:10] and kept["cap-falling-14"] == row[0::2][:14] and kept["cap-1"] == [row[0]]
    assert [len(r[0]) for r in FS.reference("nms-cap-1", True)] == [1, 1]
    assert FS.reference("nms-md2", True)[0][0].tobytes() == FS.reference("nms-md3", True)[0][0].tobytes()
    ys = {y for _, y in FS.scene("nms-rows-first-last")["expect"]["kept"]}
    assert ys == {3, FS.H0 - 4} and {y for _, y in kept["row-falling"]} == {9}
    assert total == NMS_KEPT


NMS_KEPT = 3831


def test_nms_chunks_cross_the_boundary():
    """from the plan alone: a corner of chunk 2 rejected only by corners accepted in chunk 1, and a corner accepted in chunk 2 beside a
    cell whose only chunk-1 corner was rejected"""
    for name, n in (("nms-chunks-2560", 2560), ("nms-chunks-2048", 2048), ("nms-chunks-2049", 2049)):
        s = FS.scene(name)
        plan = s["plan"]
        assert len(plan) == n
        kept, order, blockers = FS.grid_walk([(x, y, float(FS.dot_response(a))) for x, y, a in plan], s["md"], s["w"], s["h"], 4000)
        rank = {i: r for r, i in enumerate(order)}
        assert len(order) == n and len(kept) < 4000
        if n <= FS.CHUNK:
            continue
        late_rejected = [i for i in blockers if rank[i] >= FS.CHUNK and all(rank[j] < FS.CHUNK for j in blockers[i])]
        cell = lambda i: (plan[i][0] // 6, plan[i][1] // 6)
        by_cell = {cell(i): i for i in range(n)}                                 # every dot has a cell of its own
        assert len(by_cell) == n
        late_accepted = [i for i in kept if rank[i] >= FS.CHUNK and
                         any(rank.get(by_cell.get((cell(i)[0] + dx, cell(i)[1] + dy)), n) < FS.CHUNK and by_cell[cell(i)[0] + dx, cell(i)[1] + dy] in blockers
                             for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)))]
        print(name, "kept", len(kept), "chunk-2 rejects by chunk 1:", len(late_rejected), "chunk-2 accepts beside a rejected chunk-1 cell:", len(late_accepted))
        assert late_rejected and (late_accepted or n == 2049)                     # (2049: the one corner of chunk 2 is rejected by chunk 1)
        if n == 2560:                                                            # the boundary falls inside a row whose amplitudes fall
            y = plan[order[FS.CHUNK]][1]
            in_row = [i for i in range(n) if plan[i][1] == y]
            assert {rank[i] < FS.CHUNK for i in in_row} == {True, False} and all(plan[i][2] > plan[j][2] for i, j in zip(in_row, in_row[1:])) and late_accepted


def test_nms_dense_cells():
    """cells of 3 and 2 pixels: several corners per cell, the representative accepted, the representative rejected by a neighbour cell
    with a lower corner of the same cell behind it, every phase of the grid"""
    for md in (7, 4):
        s = FS.scene("nms-dense-md%d" % md)
        k = raw(s)
        kept, order, blockers = walk(s, k)
        assert [int(i) for i in O().nms_copy(k, md, s["w"], s["h"], 4000)] == kept
        c = md // 2
        cells = {}
        for i in order:
            cells.setdefault((int(k["x"][i]) // c, int(k["y"][i]) // c), []).append(i)
        multi = [v for v in cells.values() if len(v) >= 2]
        rep_acc = sum(1 for v in multi if v[0] in set(kept))
        rep_rej = sum(1 for v in multi if v[0] in blockers)
        sizes = sorted({len(v) for v in multi})
        phases = {(int(x) % c, int(y) % c) for x, y in zip(k["x"], k["y"])}
        print("md", md, "corners", len(k), "kept", len(kept), "cells with several:", len(multi), "sizes", sizes, "representative accepted / rejected:", rep_acc, rep_rej)
        assert rep_acc >= 20 and rep_rej >= 5 and len(phases) == c * c and sizes == [2, 3, 4], sizes
