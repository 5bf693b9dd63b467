"""The reach of tests/klt_scenes.py, pinned on the walk of tests/klt_ref.py alone (no GPU, no library): every scene hits the rule it
names, the two row-table formulae equal the sequential loops of svo_put_features_oct / svo_put_matches_oct transcribed here, and the
image sequence loses tracks to each cause the GPU tests want exercised while keeping enough of them alive."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402

F = np.float32
NAMES = [s.name for s in KS.scenes()]


# ---- the loops of svo_api.hip, transcribed ------------------------------------------------------------------------------------------
def put_features_row_index(ys, H):
    """svo_put_features_oct: cnt per clamped row, a running sum, kept for first_row <= r < last_row"""
    n = len(ys)
    ri = [0] * H
    if n > 0 and H > 0:
        cnt = [0] * (H + 1)
        for i in range(n):
            r = KR.row_of(ys[i])
            cnt[0 if r < 0 else (H if r > H else r)] += 1
        first_row, last_row = KR.row_of(ys[0]), KR.row_of(ys[n - 1])
        acc = 0
        for r in range(H):
            acc += cnt[r]
            if first_row <= r < last_row:
                ri[r] = acc
    return np.array(ri, np.int32)


def put_matches_row_index(ys, query, H):
    """svo_put_matches_oct: the sequential walk over the pairings (S3:441), ri[H] = n"""
    n = len(query)
    ri = [0] * (H + 1)
    idx = 0
    for y in range(H):
        ri[y] = idx
        while idx < n and F(ys[query[idx]]) <= F(y):
            idx += 1
    ri[H] = n
    return np.array(ri, np.int32)


def test_the_scenes_cover_what_the_issue_lists():
    assert set("count_%d" % n for n in (0, 1, 63, 64, 65, 255, 256, 257, KS.CAP)) <= set(NAMES)
    assert set("survivors_" + k for k in ("all", "none", "first_only", "last_only", "alternating", "one_per_wave")) <= set(NAMES)
    assert {"gate_boundaries", "nonfinite", "status_combinations", "rows_unsorted", "with_and_without_p", "held_lane"} <= set(NAMES)
    assert KS.CAP > 256 and KS.CAP <= KS.MAX_KPS


@pytest.mark.parametrize("name", NAMES)
def test_scene_hits_its_rule(name):
    sc = KS.scene(name)
    assert sc.rule
    lists, table, reasons, every = KS.walk(sc)
    last = sc.ops[-1]
    assert last[0] == "select" and len(reasons) == len(last[1])
    for slot, why in sc.expect.items():
        assert reasons[slot] == why, (name, slot, reasons[slot], why)
    if sc.survivors is not None:
        assert len(lists.matches) == sc.survivors == len(table)
    if sc.tracked is not None:
        assert len(lists.tracked) == sc.tracked
    if sc.check is not None:
        assert sc.check(lists), name
    # the order is the slot order, the table is the compacted one
    keep = [s for s, w in enumerate(reasons) if w is None]
    assert np.array_equal(lists.kps[0]["x"].view(np.uint32), np.asarray(last[1], F).reshape(-1, 2)[keep, 0].view(np.uint32))
    assert np.array_equal(table.idx, np.arange(len(keep))) and np.array_equal(table.left, np.asarray(last[1], F).reshape(-1, 2)[keep])
    assert np.array_equal(lists.tracked["second"], np.flatnonzero(table.pidx >= 0))


@pytest.mark.parametrize("name", NAMES)
def test_row_table_formulae_equal_the_loops_of_the_puts(name):
    for lists in KS.walk(KS.scene(name))[3]:
        for side in (0, 1):
            assert np.array_equal(lists.row_index[side], put_features_row_index(lists.kps[side]["y"], KS.H)), (name, side)
        assert np.array_equal(lists.mrow_index, put_matches_row_index(lists.kps[0]["y"], lists.matches["queryIdx"], KS.H)), name


def test_row_table_formulae_on_random_lists():
    rng = np.random.RandomState(5)
    for trial in range(40):
        n = int(rng.randint(0, 90))
        ys = (rng.uniform(-20, 150, n)).astype(F)
        if trial % 4 == 0:
            ys = np.round(ys)                                                            # rows hit exactly: the <= of the walk on its boundary
        assert np.array_equal(KR.feats_row_index(ys, KS.H), put_features_row_index(ys, KS.H))
        assert np.array_equal(KR.matches_row_index(ys, KS.H), put_matches_row_index(ys, np.arange(n), KS.H))


def test_gate_compares_are_float32():
    """one ulp of a float32 coordinate decides: the same numbers in double would all pass or all fail together"""
    sc = KS.scene("gate_boundaries")
    _, _, reasons, _ = KS.walk(sc)
    assert reasons[0] is None and reasons[1] == "max_dy" and reasons[4] is None and reasons[5] == "min_disp" and reasons[6] is None and reasons[7] == "max_disp"


def test_held_lane_keeps_p_and_shifted_lane_moves_it():
    held, shifted = KS.walk(KS.scene("held_lane"))[0], KS.walk(KS.scene("shifted_lane"))[0]
    assert np.array_equal(held.kps[0], shifted.kps[0]) and not np.array_equal(held.tracked, shifted.tracked)
    assert np.array_equal(shifted.tracked["first"], np.arange(60))
    want = np.array([s for s in range(90) if s % 3 != 0], np.int32)                     # the indices the survivors of the second list had in the first
    assert np.array_equal(held.tracked["first"], want)


def test_add_points_respects_cap_and_numbers_ids():
    t, m = KR.add_points(KR.Table(), *KS.good(10), cap=16)
    assert m == 10 and list(t.ids) == list(range(10)) and (t.idx == -1).all() and (t.pidx == -1).all() and (t.age == 0).all()
    t, m = KR.add_points(t, *KS.good(10, 1), cap=16)
    assert m == 6 and len(t) == 16 and list(t.ids[10:]) == list(range(10, 16)) and t.next_id == 16
    assert KR.add_points(t, *KS.good(3), cap=16)[1] == 0
    assert t.cleared().next_id == 0 and len(t.cleared()) == 0


# ---- the sequence -------------------------------------------------------------------------------------------------------------------
def test_sequence_keeps_enough_tracks_and_loses_some_to_every_cause():
    walk = KS.sequence_walk()
    assert len(walk) == KS.SEQ_FRAMES == 5
    left, right = KS.sequence_points()
    assert len(left) == 48 and np.isfinite(right).all() and ((left[:, 0] - right[:, 0]) > 0.5).all()
    causes = set()
    for f, (lists, table, loss) in enumerate(walk):
        assert len(lists.matches) >= 12, (f, len(lists.matches))
        causes |= set(w for w in loss if w)
    assert {"status", "max_dy", "left_image"} <= causes, causes
    # frame 0 takes the points as they are; from frame 1 on every survivor has a previous index
    assert len(walk[0][0].tracked) == 0
    for f in range(1, 5):
        assert len(walk[f][0].tracked) == len(walk[f][0].matches)
