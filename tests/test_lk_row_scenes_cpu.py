"""The reach of tests/lk_row_scenes.py on the row walk (tests/lk_row_ref.py): every named scene takes the branch it was built for, the
walk follows a vertical edge the two-dimensional tracker loses, and it recovers a fractional disparity.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_ref                                                                          # noqa: E402
import lk_row_ref                                                                      # noqa: E402
import lk_row_scenes as RS                                                             # noqa: E402


def _one(name):
    (out, status, err, traces, pre), = RS.reference(name)
    return out, status, err, traces, pre


def _levels(tr):
    return [(l[0], l[1]) for l in tr["levels"]]


def _pts(name, job=0):
    return RS.scene(name).jobs[job][2]


def test_every_case_of_the_issue_has_a_scene():
    names = {s.name for s in RS.scenes()}
    want = {"win_5", "win_21", "win_31", "vertical_step_edge", "horizontal_edge", "a11_at_min_eig", "a11_below_min_eig", "init_y_differs",
            "inside_coarse", "inside_level0", "leaves_level0", "leaves_strip", "leaves_strip_left", "max_iters_1", "oscillation",
            "bad_coordinates", "fb_rows", "fb_off", "stereo_shift", "mixed_call"}
    want |= {"count_%d" % n for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)}
    assert want <= names, want - names


def test_the_walk_shares_everything_but_the_point_loop_with_lk_ref():
    for name in ("LkParams", "Prepared", "build_pyramid", "scharr", "_window", "_sample", "_finite"):
        assert getattr(lk_row_ref, name) is getattr(lk_ref, name), name


@pytest.mark.parametrize("win,per_lane", [(5, 1), (21, 7), (31, 16)])
def test_window_sizes(win, per_lane):
    out, status, err, traces, pre = _one("win_%d" % win)
    assert (win * win + 63) // 64 == per_lane
    assert status.all() and all(t["levels"][-1][1:] == ("run", t["levels"][-1][2], "eps") for t in traces)
    pts = _pts("win_%d" % win)
    assert out[:, 1].tobytes() == pts[:, 1].tobytes()                     # y is carried, never moved
    assert np.abs(out[:, 0] - pts[:, 0] - 1.3).max() < (0.3 if win == 5 else 0.05)       # the small window is there for its lane layout


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257])
def test_point_counts(n):
    out, status, err, traces, pre = _one("count_%d" % n)
    assert len(out) == len(status) == len(err) == len(traces) == n
    assert status.all()


def test_vertical_step_edge_is_lost_in_two_dimensions_and_followed_along_the_row():
    s = RS.scene("vertical_step_edge")
    prev, nxt, pts, init = s.jobs[0]
    assert (prev == prev[0]).all() and (nxt == nxt[0]).all()              # constant along y
    _, st2, _, tr2 = lk_ref.track(prev, nxt, pts, init, s.ref_params())
    assert not st2.any() and all(t["lost"] == "eig0" for t in tr2)
    out, status, err, traces, pre = _one("vertical_step_edge")
    assert status.all() and all(_levels(t) == [(1, "run"), (0, "run")] for t in traces)
    got = out[:, 0] - pts[:, 0]
    print("vertical_step_edge: recovered shifts", got, "largest error", np.abs(got - RS.EDGE_SHIFT).max())
    assert np.abs(got - RS.EDGE_SHIFT).max() <= RS.EDGE_TOL


def test_horizontal_edge_is_lost_by_the_a11_rule():
    out, status, err, traces, pre = _one("horizontal_edge")
    prev = RS.scene("horizontal_edge").jobs[0][0]
    assert (lk_ref.scharr(prev)[0] == 0).all()
    assert not status.any() and not err.any()
    for tr in traces:
        assert tr["lost"] == "eig0" and _levels(tr) == [(1, "skip_eig"), (0, "skip_eig")]
    assert out.tobytes() == _pts("horizontal_edge").tobytes()


def test_a11_on_both_sides_of_min_eig():
    s_at, s_below = RS.scene("a11_at_min_eig"), RS.scene("a11_below_min_eig")
    v = RS.a11_over_win2(s_at.jobs[0][0], RS.A11_POINT, 21)
    lo, hi = s_at.ref_params().min_eig, s_below.ref_params().min_eig
    assert float(lo) <= v < float(hi) and hi == np.nextafter(lo, np.float32(1)) and v >= 2.0 ** -23
    assert list(_one("a11_at_min_eig")[1]) == [1] and _one("a11_at_min_eig")[3][0]["lost"] is None
    assert list(_one("a11_below_min_eig")[1]) == [0] and _one("a11_below_min_eig")[3][0]["lost"] == "eig0"


def test_the_row_is_the_guesses():
    out, status, err, traces, pre = _one("init_y_differs")
    pts, init = RS.scene("init_y_differs").jobs[0][2:4]
    assert status.all()
    assert (init[:, 1] != pts[:, 1]).sum() == 5
    assert out[:, 1].tobytes() == init[:, 1].tobytes()
    same = init[:, 1] == pts[:, 1]                                        # the one point on its own row lands on the answer
    assert np.abs(out[same, 0] - pts[same, 0] - 5.5).max() < 0.05


def test_a_level_skipped_at_the_top_and_tracked_below():
    out, status, err, traces, pre = _one("inside_coarse")
    assert status.all()
    for tr in traces:
        assert _levels(tr) == [(3, "skip_inside"), (2, "skip_inside"), (1, "run"), (0, "run")]


def test_inside_limit_at_level0():
    out, status, err, traces, pre = _one("inside_level0")
    assert list(status) == [1, 0, 1, 0, 1, 0, 1, 0]
    for i, tr in enumerate(traces):
        assert tr["lost"] == (None if i % 2 == 0 else "inside0")
        assert _levels(tr) == [(0, "run" if i % 2 == 0 else "skip_inside")]


def test_a_guess_that_walks_out_is_lost_outside():
    out, status, err, traces, pre = _one("leaves_level0")
    assert list(status) == [0, 1]
    assert traces[0]["lost"] == "outside0" and traces[0]["levels"][-1][3] == "outside" and err[0] == 0
    assert out[0, 0] > 84 and out[0, 1] == 40                             # the guess it had when it was lost


@pytest.mark.parametrize("name,shift", [("leaves_strip", 9.0), ("leaves_strip_left", -6.5)])
def test_windows_that_travel_farther_than_a_strip_is_wide(name, shift):
    """at win 31 a strip holds the first window and two columns on either side: these points travel farther at one level"""
    out, status, err, traces, pre = _one(name)
    moved = out[:, 0] - _pts(name)[:, 0]
    far = np.abs(moved - shift) < 0.05
    assert status.all() and far.sum() >= 4
    assert all(t["levels"] == [(0, "run", t["levels"][0][2], "eps")] and t["levels"][0][2] >= 5 for t, f in zip(traces, far) if f)


def test_the_stops():
    out, status, err, traces, pre = _one("max_iters_1")
    assert status.all() and all(l[2] == 1 for t in traces for l in t["levels"] if l[1] == "run")
    assert sum(l[3] == "max" for t in traces for l in t["levels"] if l[1] == "run") == 19        # all but one level of one point (it meets eps)
    out, status, err, traces, pre = _one("oscillation")
    assert list(status) == [1, 1]
    assert [t["levels"] for t in traces] == [[(0, "run", 5, "osc")], [(0, "run", 5, "osc")]]
    out, status, err, traces, pre = _one("win_21")
    assert all(l[3] == "eps" for t in traces for l in t["levels"] if l[1] == "run")


def test_bad_coordinates_are_copied_through():
    out, status, err, traces, pre = _one("bad_coordinates")
    pts, init = RS.scene("bad_coordinates").jobs[0][2:4]
    assert list(status) == [0, 0, 0, 0, 0, 1]
    assert out[:5].tobytes() == init[:5].tobytes() and all(t["lost"] == "nan" and not t["levels"] for t in traces[:5])
    assert out[5, 1].tobytes() == init[5, 1].tobytes()


def test_forward_backward_along_the_row():
    out, status, err, traces, pre = _one("fb_rows")
    off = _one("fb_off")
    lost = [t["lost"] for t in traces]
    assert lost == [None, None, None, "fb_dist", "outside0", "fb_dist", "fb_lost", "fb_lost"]
    assert list(status) == [1, 1, 1, 0, 0, 0, 0, 0] and list(off[1]) == [1, 1, 1, 1, 0, 1, 1, 1]
    assert out.tobytes() == off[0].tobytes() and err.tobytes() == off[2].tobytes()         # only status changes
    assert all(traces[i]["back"]["lost"] == "eig0" for i in (6, 7))                        # the flat patch has no gradient for the way back
    assert all(traces[i]["back"]["lost"] is None for i in (0, 1, 2, 3, 5))
    pts = _pts("fb_rows")
    assert np.abs(out[:3, 0] - pts[:3, 0] - 1.5).max() < 0.05


def test_the_calls_jobs():
    ref = RS.reference("mixed_call")
    s = RS.scene("mixed_call")
    assert [len(j[2]) for j in s.jobs] == [9, 7, 0, RS.MAX_KPS]
    assert {j[0].shape for j in s.jobs} == {(243, 321), (80, 96)} and s.jobs[1][0].strides[0] == 200
    assert ref[1][0][:, 1].tobytes() == s.jobs[1][3][:, 1].tobytes()
    assert ref[3][1].sum() >= 500


def test_a_fractional_disparity_is_recovered():
    out, status, err, traces, pre = _one("stereo_shift")
    pts = _pts("stereo_shift")
    assert status.all() and out[:, 1].tobytes() == pts[:, 1].tobytes()
    d = pts[:, 0] - out[:, 0]
    print("stereo_shift: largest |disparity error|", np.abs(d - RS.STEREO_DISP).max(), "median", np.median(np.abs(d - RS.STEREO_DISP)))
    assert np.abs(d - RS.STEREO_DISP).max() <= RS.STEREO_TOL
