"""What the compensated walks (tests/lk_photo_ref.py) mean and what the scenes of tests/lk_photo_scenes.py reach, on the CPU alone.
The GPU tests hold the device to these walks bit for bit; here the walks are held to what they are for (a known shift is recovered under
a gain and an offset, where the plain walks of lk_ref / lk_row_ref are not) and every scene is pinned to the branch it is named after."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_photo_ref as PR                                                              # noqa: E402
import lk_photo_scenes as PS                                                           # noqa: E402
import lk_ref                                                                          # noqa: E402
import lk_row_ref                                                                      # noqa: E402

WALKS = {False: ("", PS.SHIFT, lk_ref.track), True: ("row_", PS.ROW_SHIFT, lk_row_ref.track)}


def endpoint_errors(out, pts, shift):
    return np.hypot(out[:, 0] - pts[:, 0] - shift[0], out[:, 1] - pts[:, 1] - shift[1])


def plain_on(name, rows):
    s = PS.scene(name)
    prev, nxt, pts, init = s.jobs[0]
    return WALKS[rows][2](prev, nxt, pts, init, s.ref_params(), prepared=PS.prepared(name)[0])


def bound(rows):
    """twice the largest endpoint error the unchanged plain walk makes on the pair with the photometry left alone (the factor 2 covers the
    re-quantisation of a rescaled image to 8 bits)"""
    pre, shift, _ = WALKS[rows]
    o, st, _, _ = plain_on(pre + "unchanged", rows)
    assert st.all()
    return 2.0 * float(endpoint_errors(o, PS.scene(pre + "unchanged").jobs[0][2], shift).max())


@pytest.mark.parametrize("rows", [False, True], ids=["2d", "rows"])
@pytest.mark.parametrize("name", [p[0] for p in PS.PHOTOMETRY])
def test_a_gain_and_an_offset_are_removed(name, rows):
    """Measured with this arithmetic (40 points 2-D, 24 along the row, shift (3.4, -2.0) / (3.4, 0), win 21, 4 levels).  Bound = twice the
    plain walk's largest error on the unchanged pair: 0.0672 px (2-D), 0.0582 px (rows).  Largest error of the compensated walk, all
    points tracked:   1.4 J + 20: 0.0309 / 0.0225;   0.6 J - 15: 0.0490 / 0.0496;   J + 40: 0.0400 / 0.0295 px.
    The plain walk on the changed pair: 13 / 12, 6 / 7 and 17 / 13 points still reported tracked, NONE of them inside the bound (median
    error 50 .. 150 px)."""
    pre, shift, _ = WALKS[rows]
    pts = PS.scene(pre + name).jobs[0][2]
    o, st, e, _, _ = PS.reference(pre + name, rows)[0]
    b = bound(rows)
    worst = float(endpoint_errors(o, pts, shift).max())
    po, pst, _, _ = plain_on(pre + name, rows)
    inside = int(((endpoint_errors(po, pts, shift) <= b) & (pst == 1)).sum())
    print("%s%s: bound %.4f, compensated tracked %d of %d, largest error %.4f; plain tracked %d, inside the bound %d" % (pre, name, b, st.sum(), len(st), worst, pst.sum(), inside))
    assert st.all()
    assert worst <= b
    assert inside < len(pts) / 2                     # the scene needs the feature


@pytest.mark.parametrize("rows", [False, True], ids=["2d", "rows"])
def test_unchanged_photometry_stays_with_the_plain_walk(rows):
    """measured: the compensated walk ends at most 0.0175 px (2-D) / 0.0146 px (rows) from the plain walk on the unchanged pair"""
    pre, shift, _ = WALKS[rows]
    o, st, _, _, _ = PS.reference(pre + "unchanged", rows)[0]
    po, pst, _, _ = plain_on(pre + "unchanged", rows)
    d = float(np.hypot(*(o - po).T).max())
    print("%sunchanged: compensated against plain, largest distance %.4f, bound %.4f" % (pre, d, bound(rows)))
    assert st.all() and pst.all() and d <= bound(rows)
    # an offset alone changes nothing at all: d keeps its centred moments, bit for bit
    oo, so, eo, _, _ = PS.reference(pre + "offset_p40", rows)[0]
    assert oo.tobytes() == o.tobytes() and so.tobytes() == st.tobytes()


def traces(name, rows):
    return [t for job in PS.reference(name, rows) for t in job[3]]


def stops(name, rows):
    return {lv[3] for t in traces(name, rows) for lv in t["levels"] if lv[1] == "run"}


@pytest.mark.parametrize("rows", [False, True], ids=["2d", "rows"])
def test_reach(rows):
    # CII == 0: lost at level 0 as "flat", nothing divided
    tr = traces("flat_template", rows)
    assert [t["lost"] for t in tr] == ["flat0", "flat0", None]
    assert all(t["sums"][-1][3] == 0 and t["levels"][-1][1] == "skip_flat" for t in tr[:2]) and tr[2]["sums"][-1][3] > 0
    # an exact ramp: the plain walk tracks every point, the compensated walk loses every point on the reduced matrix
    assert [t["lost"] for t in traces("ramp", rows)] == ["eig0"] * 3
    assert plain_on("ramp", rows)[1].all()
    # the pad-index trap: pixel 0 of the window is 255, the rest of the template is dark, and the instantiation has indices behind the window
    for win, per_lane in ((5, 2), (13, 7)):
        s = PS.scene("pad_pixel0_win_%d" % win)
        prev, _, pts, _ = s.jobs[0]
        half = (win - 1) // 2
        for x, y in pts[:2].astype(int):
            w = prev[y - half:y + half + 1, x - half:x + half + 1].astype(int).ravel()
            assert w[0] == 255 and w[1:].max() < 60
        assert per_lane * 64 > win * win
        # the sums the walk took are the window's: one bright pixel, not 1 + the pad count of them
        SI = traces(s.name, rows)[0]["sums"][-1][1]
        x, y = pts[0].astype(int)
        assert SI == 32 * int(prev[y - half:y + half + 1, x - half:x + half + 1].astype(int).sum())
        assert all(t["lost"] is None for t in traces(s.name, rows))
    # win 31: a lane's 16 pixels of I I and of d I pass 2^29 and stay below 2^30
    tr = traces("lane_sums_win_31", rows)
    assert max(t["lane_II"] for t in tr) > 1 << 29 and max(t["lane_dI"] for t in tr) > 1 << 29
    assert max(max(t["lane_II"], t["lane_dI"]) for t in tr) < 1 << 30
    # the target clips at 255
    assert max(t["max_J"] for t in traces("target_clips", rows)) == 255 * 32
    # the stops
    assert "osc" in stops("row_oscillation" if rows else "oscillation", rows)
    assert "eps" in stops("unchanged", rows)
    assert stops("max_iters_1", rows) == {"max"} and "max" in stops("max_iters_2", rows)
    # a forward-backward rejection, and none with the check off
    assert sum(t["lost"] in ("fb_dist", "fb_lost") for t in traces("fb_on", rows)) >= 2
    assert all(t["lost"] is None and "back" not in t for t in traces("fb_off", rows))
    assert all("back" in t for t in traces("fb_on", rows))
    # a level skipped above level 0, the point tracked below it
    tr = traces("inside_coarse", rows)
    assert all(t["lost"] is None and any(lv[0] > 0 and lv[1].startswith("skip_") for lv in t["levels"]) for t in tr)
    # NaN and infinite coordinates copy the guess through
    assert [t["lost"] for t in traces("bad_coordinates", rows)] == ["nan"] * 4 + [None]


def test_the_row_walk_follows_a_vertical_edge_under_a_gain_change():
    """measured: the plain row walk on the edge pair with the photometry left alone recovers 1.75 px to within 0.0119 px (bound 0.0238);
    under 0.7 J + 10 the compensated row walk recovers it to within 0.0154 px on all four points; the plain row walk reports all four
    tracked, each off by 1.41 .. 1.47 px; the compensated 2-D walk has nothing along y and loses all four"""
    s = PS.scene("row_vertical_edge")
    prev, nxt, pts, _ = s.jobs[0]
    same = PS.to_u8(PS.step_edge(96, 80, 48.0 + PS.EDGE_SHIFT))
    o0, s0, _, _ = lk_row_ref.track(prev, same, pts, None, s.ref_params())
    assert s0.all()
    b = 2.0 * float(np.abs(o0[:, 0] - pts[:, 0] - PS.EDGE_SHIFT).max())
    o, st, _, _, _ = PS.reference(s.name, True)[0]
    worst = float(np.abs(o[:, 0] - pts[:, 0] - PS.EDGE_SHIFT).max())
    po, pst, _, _ = lk_row_ref.track(prev, nxt, pts, None, s.ref_params())
    pe = np.abs(po[:, 0] - pts[:, 0] - PS.EDGE_SHIFT)
    print("row_vertical_edge: bound %.4f, compensated largest error %.4f, plain tracked %d errors %s" % (b, worst, pst.sum(), pe))
    assert st.all() and worst <= b and (o[:, 1] == pts[:, 1]).all()
    assert int(((pe <= b) & (pst == 1)).sum()) < len(pts) / 2
    assert not PS.reference(s.name, False)[0][1].any()


def test_the_walks_import_what_does_not_change():
    assert PR._window is lk_ref._window and PR._sample is lk_ref._sample and PR.Prepared is lk_ref.Prepared and PR.LkParams is lk_ref.LkParams
    assert PR.RR is lk_row_ref and PR.TWO_M20 == lk_ref.TWO_M20
    names = [s.name for s in PS.scenes()]
    assert len(names) == len(set(names))
    assert {s.params.get("win", 21) for s in PS.scenes()} >= {5, 11, 13, 21, 23, 31}
    assert all(len(s.jobs) <= 8 and all(len(j[2]) <= PS.MAX_KPS for j in s.jobs) for s in PS.scenes())
