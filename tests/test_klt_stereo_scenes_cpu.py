"""The recipe of svo_klt_set_stereo(1) through the walks alone (tests/klt_stereo_ref.walk_sequence: tests/lk_ref.py for the left list
through time, tests/lk_row_ref.py for the right partner along the row) on the five-frame sequence of tests/klt_scenes.py.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import klt_stereo_ref as SR                                                            # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def runs():
    frames, points = KS.sequence_frames(), KS.sequence_points()
    g = KR.Gate(win=KS.WIN, **KS.SEQ_GATE)
    return {mode: SR.walk_sequence(frames, points, KS.SEQ_LK, g, KS.SEQ_CAP, KS.H, mode) for mode in (0, 1)}


def disparity_errors(table, f):
    w = KS.sequence_world()
    d_gt = w.f * w.B / KS.gt_depth(w, f, table.left)
    return np.abs((table.left[:, 0] - table.right[:, 0]) - d_gt)


def test_mode_0_of_the_walk_is_the_sequence_walk_of_klt_scenes(runs):
    for (lists, table, init, _), (rl, rt, _) in zip(runs[0], KS.sequence_walk()):
        assert init is None
        assert table.left.tobytes() == rt.left.tobytes() and table.right.tobytes() == rt.right.tobytes() and np.array_equal(table.ids, rt.ids)


def test_every_surviving_pair_lies_on_one_row(runs):
    for f, (lists, table, init, _) in enumerate(runs[1]):
        assert len(table) > 0
        assert table.right[:, 1].tobytes() == table.left[:, 1].tobytes(), f
        assert lists.kps[1]["y"].tobytes() == lists.kps[0]["y"].tobytes(), f
    assert any((t.left[:, 1] != t.right[:, 1]).any() for _, t, _, _ in runs[0][1:])          # through time the halves drift apart


def test_the_first_guesses_are_held_in_float32_as_written(runs):
    frames, points = KS.sequence_frames(), KS.sequence_points()
    t = KR.add_points(KR.Table(), points[0], points[1], KS.SEQ_CAP)[0]
    for f, (lists, table, init, (ol, or_)) in enumerate(runs[1]):
        assert init.dtype == np.float32 and len(init) == len(t)
        for s in range(len(t)):
            d = F(t.left[s, 0] - t.right[s, 0])
            assert init[s, 0].tobytes() == F(ol[s, 0] - d).tobytes() and init[s, 1].tobytes() == ol[s, 1].tobytes(), (f, s)
        t = table
    # "as written" is two float32 roundings, not the double expression rounded once: on random points the two differ somewhere
    rng = np.random.default_rng(0)
    xl, xr, nl = (rng.uniform(0, 160, (1000, 2)).astype(F) for _ in range(3))
    g = SR.row_init(xl, xr, nl)
    assert g[:, 0].tobytes() == (nl[:, 0] - (xl[:, 0] - xr[:, 0]).astype(F)).astype(F).tobytes() and g[:, 1].tobytes() == nl[:, 1].tobytes()
    once = (nl[:, 0].astype(np.float64) - (xl[:, 0].astype(np.float64) - xr[:, 0].astype(np.float64))).astype(F)
    assert (g[:, 0] != once).any()
    # a lane without a last pair: its left points stand and are the guesses' rows
    assert runs[1][0][3][0].tobytes() == points[0].tobytes() and runs[1][0][2][:, 1].tobytes() == points[0][:, 1].tobytes()


def test_mode_1_keeps_at_least_as_many_tracks_and_a_smaller_disparity_error(runs):
    """two CPU walks against each other at the last frame; the figures on this sequence: 27 tracks against 25, median |disparity error|
    0.111 px against 0.243 px"""
    last = KS.SEQ_FRAMES - 1
    t0, t1 = runs[0][last][1], runs[1][last][1]
    e0, e1 = disparity_errors(t0, last), disparity_errors(t1, last)
    print("tracks alive at frame %d: mode 0 %d, mode 1 %d; median |disparity error| %.4f, %.4f px; p90 %.4f, %.4f" % (
        last, len(t0), len(t1), np.median(e0), np.median(e1), np.percentile(e0, 90), np.percentile(e1, 90)))
    assert len(t1) >= len(t0)
    assert np.median(e1) <= np.median(e0)
