"""The reach of tests/lk_scenes.py on the walk (tests/lk_ref.py): every named scene takes the branch it was built for, the walk meets
ground truth on the textured pair, and its pyramid is the [1 4 6 4 1] filter.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_ref                                                                          # noqa: E402
import lk_scenes as LS                                                                 # noqa: E402


def _one(name):
    (out, status, err, traces, pre), = LS.reference(name)
    return out, status, err, traces, pre


def _levels(tr):
    return [(l[0], l[1]) for l in tr["levels"]]


def test_every_hard_case_of_the_issue_has_a_scene():
    names = {s.name for s in LS.scenes()}
    want = {"win_5", "win_21", "win_31", "inside_level0", "inside_coarse", "weights", "flat", "vertical_edge", "checker_1px",
            "blocks_2px_negative", "stripes_2px_negative", "leaves_level0", "leaves_level2", "max_iters_1", "max_iters_2", "oscillation", "init_on_answer",
            "init_3px_off", "fb_half_replaced", "fb_off", "mixed_call", "max_level_0", "max_level_5_stops_early", "bad_coordinates"}
    want |= {"count_%d" % n for n in (0, 1, 3, 4, 5, 63, 64, 65, 257)}
    assert want <= names, want - names


@pytest.mark.parametrize("win,per_lane", [(5, 1), (21, 7), (31, 16)])
def test_window_sizes(win, per_lane):
    out, status, err, traces, pre = _one("win_%d" % win)
    assert (win * win + 63) // 64 == per_lane
    assert status.all() and all(t["levels"][-1][1] == "run" for t in traces)
    truth = LS.scene("win_%d" % win).jobs[0][2] + np.array([1.3, -0.7], np.float32)
    assert np.abs(out - truth).max() < (0.3 if win == 5 else 0.05)       # the small window is there for its lane layout, not its accuracy


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257])
def test_point_counts(n):
    out, status, err, traces, pre = _one("count_%d" % n)
    assert len(out) == len(status) == len(err) == len(traces) == n
    assert status.all()


def test_inside_limit_at_level0():
    out, status, err, traces, pre = _one("inside_level0")
    assert list(status) == [1, 0, 1, 0, 1, 0, 1, 0]
    for i, tr in enumerate(traces):
        assert tr["lost"] == (None if i % 2 == 0 else "inside0")
        assert _levels(tr) == [(0, "run" if i % 2 == 0 else "skip_inside")]


def test_inside_limit_at_coarse_levels_only():
    out, status, err, traces, pre = _one("inside_coarse")
    assert len(pre.pyr[0]) == 4 and [l.shape for l in pre.pyr[0]] == [(243, 321), (122, 161), (61, 81), (31, 41)]
    assert status.all()
    for tr in traces:
        assert _levels(tr) == [(3, "skip_inside"), (2, "skip_inside"), (1, "run"), (0, "run")]


def test_weight_rounding():
    s = LS.scene("weights")
    pts = s.jobs[0][2]
    half = np.float32(10)
    ws = [lk_ref._window(np.float32(p[0] - half), np.float32(p[1] - half), 96, 80, 21)[2:] for p in pts]
    assert ws[0] == (16384, 0, 0, 0)                                  # integer coordinates
    assert ws[1] == (16384, 0, 0, 0)                                  # both fractions 2^-20: every other weight rounds to 0
    assert ws[2] == (0, 0, 0, 16384)                                  # both 1 - 2^-20
    assert ws[3] == (0, 0, 16384, 0) and ws[4] == (16384, 0, 0, 0)
    assert float(pts[1, 0]) == 12 + 2.0 ** -20 and float(pts[2, 0]) == 13 - 2.0 ** -20      # float32 holds them exactly
    assert _one("weights")[1].all()


def test_textureless_and_one_dimensional():
    for name in ("flat", "vertical_edge", "checker_1px"):
        out, status, err, traces, pre = _one(name)
        assert not status.any() and (err == 0).all()
        assert all(tr["lost"] == "eig0" and tr["levels"][-1][:2] == (0, "skip_eig") for tr in traces), name
    # the straight edge has A22 = 0 exactly: D = 0 loses it, whatever min_eig says
    out, status, err, traces, pre = _one("vertical_edge")
    wd = lk_ref._window(np.float32(38), np.float32(30), 96, 80, 21)
    assert not lk_ref._sample(pre.der[0][0][1], 21, wd, 8192, 14).any() and lk_ref._sample(pre.der[0][0][0], 21, wd, 8192, 14).any()


def test_saturated():
    out, status, err, traces, pre = _one("blocks_2px_negative")
    assert status.all() and all(tr["levels"][-1][1] == "run" for tr in traces)
    # integer coordinates on 0 / 255: the template holds 8160 = 255 * 32 beside derivatives of 2550 = 255 * 10
    wd = lk_ref._window(np.float32(33), np.float32(25), 96, 80, 31)
    assert lk_ref._sample(pre.pyr[0][0].astype(np.int64), 31, wd, 256, 9).max() == 8160
    assert np.abs(lk_ref._sample(pre.der[0][0][0], 31, wd, 8192, 14)).max() == 2550
    assert err.max() > 100                                             # against its negative |J - I| is about half of 255 on average
    # the stripes reach the largest derivative there is, 4080 = 255 * 16, on both axes inside one window, and |J - I| = 8160 with it
    out, status, err, traces, pre = _one("stripes_2px_negative")
    assert all(tr["levels"][-1][1] == "run" for tr in traces)
    assert np.abs(lk_ref._sample(pre.der[0][0][0], 31, wd, 8192, 14)).max() == 4080
    assert np.abs(lk_ref._sample(pre.der[0][0][1], 31, wd, 8192, 14)).max() == 4080
    diff = lk_ref._sample(pre.pyr[1][0].astype(np.int64), 31, wd, 256, 9) - lk_ref._sample(pre.pyr[0][0].astype(np.int64), 31, wd, 256, 9)
    assert np.abs(diff).max() == 8160


def test_window_leaves_the_image():
    out, status, err, traces, pre = _one("leaves_level0")
    assert list(status) == [0, 1] and traces[0]["lost"] == "outside0" and traces[0]["levels"][-1][1:] == ("run", 2, "outside")
    out, status, err, traces, pre = _one("leaves_level2")
    assert status.all() and traces[0]["levels"][0][:2] == (2, "run") and traces[0]["levels"][0][3] == "outside"
    assert traces[1]["levels"][0][3] == "eps"
    assert np.abs(out - LS.scene("leaves_level2").jobs[0][2] - np.array([-12, 0], np.float32)).max() < 0.05


def test_iteration_limits():
    for it in (1, 2):
        out, status, err, traces, pre = _one("max_iters_%d" % it)
        assert status.all() and all(l[2] <= it for tr in traces for l in tr["levels"])
        assert any(l[3] == "max" for tr in traces for l in tr["levels"])
    out, status, err, traces, pre = _one("oscillation")
    assert traces[0]["levels"][-1][3] == "osc" and traces[0]["levels"][-1][2] > 1 and status[0] == 1
    assert traces[1]["levels"][-1][3] == "eps"


def test_initial_guesses():
    on, off = _one("init_on_answer"), _one("init_3px_off")
    truth = LS.scene("init_on_answer").jobs[0][2] + np.array([5.5, -3.25], np.float32)
    for out, status, err, traces, pre in (on, off):
        assert status.all() and np.abs(out - truth).max() < 0.05
    # a guess on the answer needs fewer iterations than one 3 px off
    its = [sum(l[2] for tr in r[3] for l in tr["levels"]) for r in (on, off)]
    assert its[0] < its[1]


def test_forward_backward():
    out, status, err, traces, pre = _one("fb_half_replaced")
    assert list(status) == [1, 1, 1, 0, 0, 0]                           # the right half of the next image is other texture
    assert {tr["lost"] for tr in traces[3:]} & {"fb_dist", "fb_lost"}
    o0, s0, e0, t0, _ = _one("fb_off")
    assert s0.sum() > status.sum() and all(tr["lost"] not in ("fb_dist", "fb_lost") for tr in t0)
    assert o0.tobytes() == out.tobytes()                                # the check changes status alone
    assert e0.tobytes() == err.tobytes()


def test_levels():
    assert len(_one("max_level_0")[4].pyr[0]) == 1
    pre = _one("max_level_5_stops_early")[4]
    assert [l.shape for l in pre.pyr[0]] == [(80, 96), (40, 48)]       # 24 x 20 would be smaller than win + 4 = 25


def test_bad_coordinates():
    out, status, err, traces, pre = _one("bad_coordinates")
    assert list(status) == [0, 0, 0, 0, 0, 1] and [tr["lost"] for tr in traces] == ["nan"] * 5 + [None]
    init = LS.scene("bad_coordinates").jobs[0][3]
    assert out[:5].tobytes() == init[:5].tobytes() and not any(tr["levels"] for tr in traces[:5])


def test_mixed_call():
    s = LS.scene("mixed_call")
    assert len(s.jobs) == 5
    assert s.jobs[0][0].shape == (243, 321) and s.jobs[0][0].strides[0] == 321            # odd width, contiguous
    assert s.jobs[1][0].shape == (80, 96) and s.jobs[1][0].strides[0] == 200              # a crop of a larger frame
    assert s.jobs[2][0].strides[0] == 128 and s.jobs[2][1].strides[0] == 160              # prev and next with different strides
    assert len(s.jobs[3][2]) == 0 and len(s.jobs[4][2]) == LS.MAX_KPS
    assert s.jobs[2][3] is not None


@pytest.mark.parametrize("shift", [(0.5, -0.25), (3.3, -2.6), (9.4, 6.2)])
def test_walk_against_ground_truth(shift):
    """The multi-octave texture at 320 x 240, 128 points at least 40 px from the border, default parameters: every point is tracked to
    within 0.05 px of the true shift.  Measured with this walk: largest coordinate error 0.0176 px at (0.5, -0.25), 0.0207 px at
    (3.3, -2.6), 0.0157 px at (9.4, 6.2); 7.7, 8.8 and 11.0 iterations per point on average over all levels, at most 10, 13 and 25."""
    prev, nxt = LS.texture(320, 240, seed=3), LS.shifted(320, 240, shift[0], shift[1], seed=3)
    pts = LS.grid_points(320, 240, 128, 40, seed=5)
    out, status, err, traces = lk_ref.track(prev, nxt, pts, None, lk_ref.LkParams())
    worst = float(np.abs(out - pts - np.array(shift, np.float32)).max())
    its = [sum(l[2] for l in tr["levels"]) for tr in traces]
    print("shift %s: %d of 128 tracked, largest coordinate error %.4f px, %.1f iterations per point, at most %d" % (shift, status.sum(), worst, np.mean(its), max(its)))
    assert status.all()
    assert worst <= 0.05


def test_pyramid_of_a_constant_image_is_constant():
    for v in (0, 1, 127, 255):
        for lvl in lk_ref.build_pyramid(np.full((243, 321), v, np.uint8), 21, 5):
            assert (lvl == v).all()


def test_one_pyramid_level_against_the_float_filter():
    img = LS.texture(321, 243)
    k = np.array([1, 4, 6, 4, 1], np.float64) / 16
    f = np.pad(img.astype(np.float64), 2, mode="reflect")                # numpy's "reflect" is BORDER_REFLECT_101
    f = sum(k[i] * f[i:i + 243, :] for i in range(5))
    f = sum(k[j] * f[:, j:j + 321] for j in range(5))
    want = f[::2, ::2]
    got = lk_ref.pyr_down(img)
    assert got.shape == (122, 161) == want.shape
    assert np.abs(got.astype(np.float64) - want).max() <= 0.5
