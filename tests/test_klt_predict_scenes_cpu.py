"""The reach of tests/klt_predict_scenes.py, pinned on the reference walk alone (tests/klt_predict_ref.py; no GPU): every branch of the
prediction rule is taken on both sides of its compare, the walk's projection is the oracle's getProjectedCoords, a first guess equal
to the point is no first guess, and the fast-motion sequence meets its condition under tests/lk_ref.py before any GPU run."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_predict_ref as PR                                                           # noqa: E402
import klt_predict_scenes as PS                                                        # noqa: E402
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import lk_ref as LR                                                                    # noqa: E402

F = np.float32
SCENES = PS.scenes()


@pytest.fixture(scope="module")
def walked():
    return {s.name: PS.walk(s) for s in SCENES}


@pytest.mark.parametrize("sc", SCENES, ids=[s.name for s in SCENES])
def test_scene_reaches_its_rule(walked, sc):
    o = walked[sc.name]
    n = len(sc.left)
    assert len(o.gl) == len(o.gr) == len(o.used) == len(o.reasons) == n and n <= PS.CAP
    for s, why in sc.expect.items():
        assert o.reasons[s] == why, (sc.name, s, o.reasons[s], why)
    if sc.predicted is not None:
        assert int(o.used.sum()) == sc.predicted, (sc.name, int(o.used.sum()))
    if sc.check is not None:
        assert sc.check(o), sc.name
    # what the rule promises of every slot
    for s in range(n):
        if o.reasons[s] is None:
            assert o.used[s] == 1 and np.isfinite(o.gl[s]).all() and np.isfinite(o.gr[s]).all()
            assert 0 <= o.gl[s, 0] <= PS.W - 1 and 0 <= o.gr[s, 0] <= PS.W - 1 and 0 <= o.gl[s, 1] <= PS.H - 1 and 0 <= o.gr[s, 1] <= PS.H - 1
        else:
            assert o.used[s] == 0 and o.gl[s].tobytes() == sc.left[s].tobytes() and o.gr[s].tobytes() == sc.right[s].tobytes()


def test_every_branch_of_item_4_is_taken_on_both_sides(walked):
    seen = {}
    for name, o in walked.items():
        for why in o.reasons:
            seen.setdefault(why, set()).add(name)
    for why in (None,) + PR.REASONS:
        assert seen.get(why), "no scene reaches '%s'" % why
    # each compare, on the side that passes it AND on the side that fails it, inside one scene where the neighbours differ only there
    o = walked["disparity"]
    assert o.reasons[2] is None and o.reasons[3] == "disparity" and o.reasons[0] == "disparity"                        # > 0, < 0, == 0
    assert walked["depth_zero"].reasons[0] == walked["depth_below"].reasons[0] == "depth" and walked["depth_above"].reasons[0] != "depth"
    o = walked["edges_left"]
    assert [o.reasons[s] for s in range(4)] == [None, "outside_left", None, "outside_left"]
    for name, why, col in (("edge_left_zero", "outside_left", lambda o: o.gl[:, 1]), ("edge_right_zero", "outside_right", lambda o: o.gr[:, 0])):
        o = walked[name]
        inside = [s for s, w in enumerate(o.reasons) if w is None]
        assert inside and any(w == why for w in o.reasons) and all(col(o)[s] >= 0 for s in inside), name
    assert walked["nonfinite_pixel"].reasons[0] == "nonfinite"
    # item 1 on both sides of each of its conditions
    assert all(w == "lane" for w in walked["not_valid"].reasons) and all(w is None for w in walked["valid_other_than_1"].reasons)
    for k in (0, 4):
        for tag in ("nan", "inf", "minus_inf"):
            assert all(w == "lane" for w in walked["delta_%s_%d" % (tag, k)].reasons)
    # both branches of the rotation, and they meet at the threshold to within the second-order term
    a, b = walked["small_angle_below"], walked["small_angle_above"]
    assert PR.rotation_row3(PS.scene("small_angle_below").delta)[2] == 1.0 and PR.rotation_row3(PS.scene("small_angle_above").delta)[2] < 1.0
    assert np.abs(a.gl - b.gl).max() < 1e-3 and a.gl.tobytes() != walked["delta_zero"].gl.tobytes()


def test_item_5_pads_the_block_with_nan():
    sc = PS.scene("count_257")
    gl, gr, used = PR.predict_slots(sc.left, sc.right, PS.CAP, PS.camera(), sc.delta, sc.valid, PS.W, PS.H)
    assert len(gl) == len(gr) == len(used) == PS.CAP
    assert np.isnan(gl[257:]).all() and np.isnan(gr[257:]).all() and not used[257:].any() and used[:257].all()
    # a lane outside the mask or without a last pair: its own points
    gl, gr, used, why = PR.predict(sc.left, sc.right, PS.camera(), sc.delta, 1, PS.W, PS.H, tracks=False)
    assert gl.tobytes() == sc.left.tobytes() and gr.tobytes() == sc.right.tobytes() and not used.any() and set(why) == {"lane"}


def test_the_walk_projects_as_get_projected_coords_does():
    """the walk's triangulation + oracle.project against oracle.projected_coords on the same points with delta = pose_to_delta(pose):
    the path the device's k_project_points is already held to"""
    from oracle import oracle as O
    l, r = KS.good(120, 11)
    cam = PS.camera()
    kl = np.zeros(len(l), KR.keypoint_dtype); kr = np.zeros(len(l), KR.keypoint_dtype)
    kl["x"], kl["y"], kr["x"], kr["y"] = l[:, 0], l[:, 1], r[:, 0], r[:, 1]
    m = np.zeros(len(l), KR.dmatch_dtype); m["queryIdx"] = m["trainIdx"] = np.arange(len(l))
    first = np.full(len(l), -1, np.int32)
    for pose in ([0.15, -0.02, 0.01, 0.03, -0.004, 0.002], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0], [-0.3, 0.05, 0.02, -0.2, 0.01, 0.1]):
        delta = O.pose_to_delta(pose)
        want = O.projected_coords(m, kl, kr, first, cam, pose)
        _, X = PR.triangulate(l, r, cam)
        got, _ = O.project(X, cam, delta)
        assert got.tobytes() == want.tobytes()
        gl, gr, used, _ = PR.predict(l, r, cam, delta, 1, 1 << 20, 1 << 20)         # an image that holds every guess
        ok = used == 1
        assert ok.sum() > 100 and gl[ok].tobytes() == want[ok][:, 0:2].tobytes() and gr[ok].tobytes() == want[ok][:, 2:4].tobytes()
        # the depth the walk restates beside the oracle agrees with the pixels the oracle returns: a positive Z1c keeps the pixel on
        # the side of the principal point that X1c is on
        r3 = PR.rotation_row3(delta)
        assert abs(np.linalg.norm(r3) - 1.0) < 1e-12


def test_a_first_guess_equal_to_the_point_is_no_first_guess():
    """k_lk_track with init == pts is the tracker without init (k_lk.hip: the guess only replaces the start): pinned on tests/lk_ref.py
    over the five-frame sequence of tests/klt_scenes.py.  A step in mode 1 relies on it for every slot that is not predicted."""
    frames, (l0, r0) = KS.sequence_frames(), KS.sequence_points()
    P = LR.LkParams(**KS.SEQ_LK)
    for f in range(1, KS.SEQ_FRAMES):
        for sd, pts in ((0, l0), (1, r0)):
            pre = LR.Prepared(frames[f - 1][sd], frames[f][sd], P)
            a = LR.track(frames[f - 1][sd], frames[f][sd], pts, params=P, prepared=pre)
            b = LR.track(frames[f - 1][sd], frames[f][sd], pts, init=pts.copy(), params=P, prepared=pre)
            for x, y in zip(a[:3], b[:3]):
                assert x.tobytes() == y.tobytes(), (f, sd)
            assert a[1].any()


INSIDE_LOSSES = ("eig0", "fb_lost", "fb_dist")        # status 0 with the window inside the image ('inside0' / 'outside0': it left the image)


def test_the_fast_sequence_needs_the_prediction():
    """under tests/lk_ref.py, before any GPU run: the yaw ramps up, the shallow tracker follows the first pair and loses the later
    ones, and with the last increment applied it keeps them"""
    plain, pred = PS.fast_walk(False), PS.fast_walk(True)
    last = PS.FAST_FRAMES - 1
    n_plain, n_pred = [len(w[0]) for w in plain], [len(w[0]) for w in pred]
    assert n_plain[0] == n_pred[0] == 48
    assert n_plain[1] == n_pred[1] >= 40                                  # the first tracked pair: within reach, nothing predicted yet
    assert not pred[1][3].any() and all(pred[f][3].any() for f in range(2, PS.FAST_FRAMES))
    assert n_pred[last] > n_plain[last], (n_plain, n_pred)
    # a track the predicted walk keeps to the end, whose unpredicted counterpart the tracker gave up inside the image
    kept = set(int(i) for i in pred[last][0].ids)
    rescued = set()
    for f in range(1, PS.FAST_FRAMES):
        _, status, traces, _, ids = plain[f]
        for s, i in enumerate(ids):
            for sd in (0, 1):
                if status[sd][s] == 0 and traces[sd][s]["lost"] in INSIDE_LOSSES and int(i) in kept:
                    rescued.add(int(i))
    assert rescued, (n_plain, n_pred)
    # the ramp is what does it: the per-frame image motion grows beyond the reach, the residual after the prediction does not
    f = PS.fast_world().f
    shift = [f * np.tan(np.radians(a)) for a in PS.FAST_YAW_DEG]
    assert shift[1] < 5 < shift[2] and all(abs((shift[t] - shift[t - 1]) - shift[1]) < 0.1 for t in range(2, PS.FAST_FRAMES))
