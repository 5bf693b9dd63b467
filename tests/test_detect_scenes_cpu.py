"""Preconditions of tests/test_gpu_detect_scenes.py, on the oracle alone (no GPU): where a scene of tests/detect_scenes.py predicts its
answer from its construction, the oracle gives exactly that answer; and the scenes do reach the edges the detect chain is built around --
tile seams, group and row-block residues, octants and quadrants, saturated and empty blur windows, last tiles of every width, interiors of
one row -- counted from the oracle's lists and the geometry constants alone.  Every count is printed (pytest -s) and asserted nonzero."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_scenes as DS                                                           # noqa: E402


def O():
    from oracle import oracle
    return oracle


def test_generators_are_deterministic_and_small():
    names = []
    for f, gen in DS.FAMILIES.items():
        a, b = DS.scenes(f), gen()
        assert [s["name"] for s in a] == [s["name"] for s in b], f
        for s, t in zip(a, b):
            assert all(i.tobytes() == j.tobytes() for i, j in zip(s["imgs"], t["imgs"])) and s["expect"] == t["expect"], s["name"]
            assert s["w"] <= 384 and s["h"] <= 288 and s["initial_FAST_threshold"] == DS.TH and s["orb_nlevels"] == (8 if f == "levels" else 1), s["name"]
            assert s["nms"] == (f == "spacing"), s["name"]
        names += [s["name"] for s in a]
    assert len(set(names)) == len(names)
    print("scenes per family:", {f: len(DS.scenes(f)) for f in DS.FAMILIES})


# ---------------------------------------------------------------------------------------------------------------------------------------
# the oracle against construction
# ---------------------------------------------------------------------------------------------------------------------------------------
def fast_maxima(img, th):
    """oracle.fast_score_map plus the strict 3x3 maxima inside the border, in raster order"""
    sm = O().fast_score_map(img, th).astype(np.int32)
    h, w = sm.shape
    c = sm[1:-1, 1:-1]
    keep = c > 0
    for i, j in DS.NBR8:
        keep &= c > sm[1 + j:h - 1 + j, 1 + i:w - 1 + i]
    ys, xs = np.nonzero(keep)
    return [(int(x) + 1, int(y) + 1, int(sm[y + 1, x + 1])) for y, x in zip(ys, xs) if DS.interior(x + 1, y + 1, w, h)]


def test_dots_oracle_gives_the_predicted_corners():
    total = 0
    for s in DS.scenes("dots"):
        got = fast_maxima(s["imgs"][0], DS.TH)
        assert got == s["expect"]["fast"], (s["name"], sorted(set(got) ^ set(s["expect"]["fast"]))[:6])
        k, _ = DS.oracle_raw(s["name"])                              # ... and the detector keeps every one of them, nothing else
        assert sorted((int(y), int(x)) for x, y in zip(k["x"], k["y"])) == [(y, x) for x, y, _ in got], s["name"]
        total += len(got)
    assert total > 300
    th_scenes = [s for s in DS.scenes("dots") if s["kind"] == "thbytes"]
    assert len(th_scenes) == 2 and all(len(s["expect"]["fast"]) == 12 and {sc for _, _, sc in s["expect"]["fast"]} == {DS.TH} for s in th_scenes)
    assert all({(x - 30) % 4 for x, _, _ in s["expect"]["fast"]} == {0, 1, 2, 3} for s in th_scenes)


def test_cuts_oracle_keeps_the_predicted_dots():
    for s in DS.scenes("cuts"):
        k, _ = DS.oracle_raw(s["name"])
        assert [(int(x), int(y)) for x, y in zip(k["x"], k["y"])] == s["expect"]["kept"], s["name"]
        assert len(k) == s["orb_nfeats"]
    for n in (10, 24, 47, 48, 49):
        k, _ = DS.oracle_raw("cuts-equal-%d" % n)
        assert len(set(k["response"].tolist())) == 1                                  # one Harris response: position alone decides
    # the raised dots: a cut inside their tie group (10, 15 of 20) and outside it (30 = 20 + the first ten of the others)
    for n, inside in ((10, True), (15, True), (30, False)):
        kept = DS.scene("cuts-raised-%d" % n)["expect"]["kept"]
        raised = [DS.CUT_GRID[i] for i in DS.RAISED]
        assert (kept == raised[:n]) if inside else (kept == raised + [p for p in DS.CUT_GRID if p not in raised][:n - 20])
    # the redo scene: the first image leaves 3 * 10 + 32 candidates at score 59, the second has five there: fewer than 2 * 10
    s = DS.scene("cuts-redo-10")
    assert len(s["imgs"]) == 2 and s["redo"]
    a, b = (O().fast_score_map(i, DS.TH) for i in s["imgs"])
    assert (a == 59).sum() == 96 >= 3 * 10 + 32 and (b >= 59).sum() == 5 < 2 * 10 and (b == 39).sum() == 91


def octant_and_quadrant(angle):
    """the octant of an orientation and k & 3 of the oracle's sincosf for it (its argument reduction, in float32 as it computes it)"""
    x = np.float32(angle) * np.float32(0.017453292)
    k = int(x * np.float32(0.63661977) + np.float32(0.5))
    return int(angle // 45.0) % 8, k & 3


def test_orient_oracle_angles():
    octants, quads, exact, d45 = set(), set(), 0, []
    for s in DS.scenes("orient"):
        k, _ = DS.oracle_raw(s["name"])
        got = {(int(x), int(y)): float(a) for x, y, a in zip(k["x"], k["y"], k["angle"])}
        assert set(got) == set(s["expect"]["angle"]), (s["name"], sorted(set(got) ^ set(s["expect"]["angle"])))      # the cells' dots, no other corner
        for pos, want in s["expect"]["angle"].items():
            a = got[pos]
            assert a == O().orb_angle(s["imgs"][0], *pos)
            if not s["weighted"] or want % 90.0 == 0.0:
                assert a == want, (s["name"], pos, a, want)            # no weight: 0; edges and axes: 0, 90, 180, 270 to the bit
                exact += 1
            else:
                assert abs((a - want + 180.0) % 360.0 - 180.0) <= 0.3, (s["name"], pos, a, want)        # fastAtan2's documented accuracy
            o, q = octant_and_quadrant(a)
            octants.add(o); quads.add(q)
            d45 += [a] if want == 45.0 else []
    assert d45 and all(abs(a - 44.990456) < 1e-5 for a in d45), d45            # 45 degrees through the oracle's polynomial
    print("orient: octants", sorted(octants), "quadrants k & 3", sorted(quads), "exact angles", exact)
    assert octants == set(range(8)) and quads == {0, 1, 2, 3} and exact >= 3 * 5 + 4


def test_orient_quadrant_tie_decides_a_descriptor_bit():
    """orient-tie-225: its argument of sincosf sits within 0.01 of the tie between two quadrants, and the other quadrant would change the
    descriptor -- shown with a float32 model of the oracle's sincosf and steering that is first held to the oracle bit for bit"""
    rng = np.random.RandomState(5)
    for a in list(rng.uniform(0.0, 360.0, 2000).astype(np.float32)) + [np.float32(v) for v in (0, 45, 90, 135, 180, 225, 270, 315, 360)]:
        x = np.float32(a * np.float32(0.017453292))
        assert DS.sincos_model(x)[:2] == tuple(np.float32(v) for v in O().sincosf(float(x))), a
    s = DS.scene("orient-tie-225")
    k, d = DS.oracle_raw(s["name"])
    assert len(k) == 1 and (int(k["x"][0]), int(k["y"][0])) == DS.TIE_AT and float(k["angle"][0]) == 225.1514892578125
    x = np.float32(k["angle"][0] * np.float32(0.017453292))
    t = float(np.float32(x * np.float32(0.63661977)))
    assert 2.5 <= t < 2.51 and DS.sincos_model(x)[2] == 3 and DS.sincos_model(x, 0.49)[2] == 2, t
    bl = DS.gauss_blur(s["imgs"][0])
    cx, cy = DS.TIE_AT
    assert (int(bl[cy + 3, cx - 13]), int(bl[cy + 4, cx - 13]), int(bl[cy - 4, cx - 1])) == (0, 1, 0)
    right, other = DS.steer_model(bl, cx, cy, k["angle"][0]), DS.steer_model(bl, cx, cy, k["angle"][0], 0.49)
    assert (right == d[0]).all() and (right == O().steered_brief(bl, cx, cy, k["angle"][0])).all()
    flipped = np.flatnonzero(np.unpackbits(right ^ other, bitorder="little"))
    print("orient-tie-225: sincosf argument * 2 / pi = %.6f, tests that the other quadrant flips: %s" % (t, flipped.tolist()))
    assert flipped.tolist() == [1]
    # ... and the model on the (a) scenes of `blur`: every descriptor of the oracle, so gauss_blur and steer_model ARE its blur and steering
    for nm in ("blur-texture-100", "blur-blocks-0"):
        kk, dd = DS.oracle_raw(nm)
        bb = DS.gauss_blur(DS.scene(nm)["imgs"][0])
        assert all((DS.steer_model(bb, int(kk["x"][i]), int(kk["y"][i]), kk["angle"][i]) == dd[i]).all() for i in range(len(kk))), nm


def blurred_windows(s):
    """per raw keypoint of a one-level scene the 37 x 37 blurred window its 256 tests read from"""
    k, d = DS.oracle_raw(s["name"])
    bl = DS.gauss_blur(s["imgs"][0])
    return k, d, bl, [bl[int(y) - 18:int(y) + 19, int(x) - 18:int(x) + 19] for x, y in zip(k["x"], k["y"])]


def test_blur_reach():
    has255 = has0 = 0
    bits = []
    xres = set()
    for s in DS.scenes("blur"):
        k, d, bl, wins = blurred_windows(s)
        assert sorted((int(x), int(y)) for x, y in zip(k["x"], k["y"])) == sorted(DS.blur_positions()), s["name"]      # the dots, and the texture adds no corner
        # gauss_blur IS the oracle's blur: its steering on this blurred level gives the detector's descriptors
        for i in range(0, len(k), 7):
            assert (O().steered_brief(bl, int(k["x"][i]), int(k["y"][i]), k["angle"][i]) == d[i]).all(), (s["name"], i)
        has255 += sum(bool((w == 255).any()) for w in wins); has0 += sum(bool((w == 0).any()) for w in wins)
        xres |= {int(x) % 16 for x in k["x"]}
        if s["part"] == "a":
            bits.append(np.unpackbits(d, axis=1))
            assert len(np.unique(np.concatenate([w.reshape(-1) for w in wins]))) > 8, s["name"]      # non-trivial sums
    bits = np.concatenate(bits)
    ones = float(bits.mean())
    pos = set(DS.blur_positions())
    print("blur: windows holding 255: %d, holding 0: %d; tests that are 1 in the (a) scenes: %.3f; x residues mod 16: %d" % (has255, has0, ones, len(xres)))
    assert has255 > 0 and has0 > 0 and 0.25 <= ones <= 0.75
    assert xres == set(range(16)) and {(31, 31), (DS.W0 - 32, 31), (31, DS.H0 - 32), (DS.W0 - 32, DS.H0 - 32)} <= pos
    flat = {s["name"]: blurred_windows(s)[2] for s in DS.scenes("blur") if s["part"] == "b"}
    assert (flat["blur-flat-255"] == 255).mean() > 0.5 and (flat["blur-flat-0"] == 0).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------------------------------
# reach
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_dots_reach():
    kept = [(x, y) for s in DS.scenes("dots") for x, y, _ in s["expect"]["fast"]]
    on_x = {v: sum(x == v for x, _ in kept) for v in (31, 92, 93, 128)}
    on_y = {v: sum(y == v for _, y in kept) for v in (31, 92, 93, 96)}
    groups = {r: sum((x - 30) % 4 == r for x, _ in kept) for r in range(4)}
    blocks = {r: sum((y - 30) % 8 == r for _, y in kept) for r in (0, 7)}
    never = sum(1 for s in DS.scenes("dots") if s["kind"] == "pairs" for g in s["groups"] for x, y, _ in g if not DS.interior(x, y, s["w"], s["h"]))
    seam = {"x": 0, "y": 0}
    for s in DS.scenes("dots"):
        if s["kind"] != "pairs":
            continue
        alive = {(x, y) for x, y, _ in s["expect"]["fast"]}
        for (xa, ya, _), (xb, yb, _) in s["groups"]:
            if max(abs(xa - xb), abs(ya - yb)) == 1 and not ((xa, ya) in alive and (xb, yb) in alive):
                seam["x"] += {xa, xb} == {92, 93}
                seam["y"] += {ya, yb} == {92, 93}
    at_th = sum(1 for s in DS.scenes("dots") if s["kind"] == "single" for y, x in zip(*np.nonzero(s["imgs"][0] != s["background"]))
                if abs(int(s["imgs"][0][y, x]) - s["background"]) == DS.TH and DS.interior(x, y, s["w"], s["h"]))
    print("dots: kept corners on x", on_x, "on y", on_y, "group residues", groups, "row-block residues", blocks, "suppressed pairs across the seams", seam,
          "dots outside the border in pairs", never, "dots of exactly th inside", at_th)
    assert all(on_x.values()) and all(on_y.values()) and all(groups.values()) and all(blocks.values()) and seam["x"] and seam["y"] and never and at_th
    assert {s["background"] for s in DS.scenes("dots") if s["kind"] == "single"} == set(DS.BACKGROUNDS)
    scores = {sc for s in DS.scenes("dots") for _, _, sc in s["expect"]["fast"]}
    assert {DS.TH, 59, 254} <= scores and min(scores) == DS.TH


def test_levels_reach():
    lw1 = {}
    for w, h in DS.LEVEL_SIZES:
        levels, lw, lh, sc = DS.levels_with_interior(w, h)
        lw1[w, h] = (lw[1], lh[1])
        k, _ = DS.oracle_raw("levels-%dx%d-blobs" % (w, h))
        hit = {l: DS.on_border(k, l, lw, lh, sc) for l in levels}
        print("levels %dx%d: levels with an interior %s, keypoints per level %s, on a border (column, row) %s" % (w, h, levels, np.bincount(k["octave"], minlength=8).tolist(), hit))
        assert all(c and r for c, r in hit.values()), (w, h, hit)
        assert all((k["octave"] == l).any() for l in levels)
    assert lw1 == {(152, 76): (127, 63), (154, 77): (128, 64), (155, 78): (129, 65), (157, 78): (131, 65), (186, 116): (155, 97)}
    assert O().pyramid_sizes(186, 116, 8)[0][2] == 129 and O().pyramid_sizes(186, 116, 8)[1][2] == 81
    # k_resize: last tiles of 127, 128, 1 and 3 columns, last row bands of 31, 0 (a full one) and 1 rows, widths that are no multiple of 4
    cols = {lw % DS.RZ_W for lw, _ in lw1.values()} | {129 % DS.RZ_W}
    rows = {lh % DS.RZ_H for _, lh in lw1.values()}
    widths = {lw % 4 for w, h in DS.LEVEL_SIZES for lw in O().pyramid_sizes(w, h, 8)[0][1:]}
    print("levels: last-tile columns", sorted(cols), "last-band rows", sorted(rows), "width residues mod 4", sorted(widths))
    assert {127, 0, 1, 3} <= cols and {31, 0, 1} <= rows and widths == {0, 1, 2, 3}
    # 152x76: a level whose interior is exactly one row, and levels with none
    levels, lw, lh, _ = DS.levels_with_interior(152, 76)
    assert levels == [0, 1] and lh[1] - 2 * DS.EDGE == 1
    assert {s["content"] for s in DS.scenes("levels")} == {"blobs", "noise", "white", "columns", "rows", "checker", "lastline"}


def test_spacing_reach():
    """min_distance 7 (cells of 3 pixels): the NMS removes a dot of some pairs and keeps both of others.  min_distance 3 (cells of one
    pixel): keypoints of one level are never 4-neighbours after the strict 3x3 maxima, so the NMS has to keep every dot, two apart included"""
    for md in (3, 7):
        lost = kept = 0
        for s in DS.scenes("spacing"):
            if s["min_distance"] != md:
                continue
            raw, _ = DS.oracle_raw(s["name"])
            fin, _ = DS.oracle_final(s["name"])
            assert len(raw) == int((s["imgs"][0] > 0).sum()) and len(raw) % 2 == 0, s["name"]              # every dot is a raw keypoint
            lost += len(raw) - len(fin); kept += len(fin)
        print("spacing %d: dots the NMS removed %d, kept %d" % (md, lost, kept))
        assert (lost > 0 and kept - lost > 0) if md == 7 else (lost == 0 and kept == 2 * 27)
