"""The resident top-up of the KLT front end on the GPU (svo_klt_topup and its companions), held byte for byte to the host recipe it
replaces.

Every comparison is between two contexts whose front ends step alike (svo_klt_step): on one the top-up is resident, on the other it is
tests/klt_topup_ref.KltTopupRecipe -- svo_klt_get_tracks, svo_gftt_detect, svo_lk_track, svo_klt_add_points, lane by lane.  After
every top-up the tables (points, IDs, ages, counts) of every lane and the info records must be equal; after the step that follows,
every public getter of the lane must be equal as bytes (`snapshot`)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import abi, hip
from stereo_vo_amd.abi import north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402
import klt_topup_scenes as TS                                                          # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SVO_ERR_ARG, SVO_ERR_CAPACITY, SVO_ERR_STATE = -2, -5, -6
SCENE_NAMES = [s.name for s in TS.scenes()]


def params():
    p = north_star_params(hip.default_params())
    p.orb_nlevels, p.orb_nfeats = 2, 300
    return p


def klt_params(cap, lk, gate):
    p = hip.default_klt_params()
    p.cap = cap
    for k, v in lk.items():
        setattr(p.lk, k, v)
    for k, v in gate.items():
        setattr(p, k, v)
    return p


def gftt_params(d):
    return abi.GfttParams(d["max_corners"], d["block"], d["min_distance"], d["quality"])


def make_ctx(n_lanes, w, h, max_cand=TS.MAX_CAND, **kw):
    c = hip.Context(n_lanes=n_lanes, max_w=w, max_h=h, max_kps=TS.MAX_KPS, max_cand=max_cand, **kw)
    c.set_params(params())
    c.set_camera(KS.sequence_world().camera())
    return c


def snapshot(c, lane=0):
    out = {}
    for which in (0, 1):
        for side in (0, 1):
            k, d = c.keypoints(lane, which, side)
            out["kps%d%d" % (which, side)] = k.tobytes() + d.tobytes()
            out["row%d%d" % (which, side)] = c.row_index(lane, which, side).tobytes() if which == 0 or len(k) else b""
        out["matches%d" % which] = c.matches(lane, which).tobytes()
        out["ids%d" % which] = c.match_ids(lane, which).tobytes()
        out["mrow%d" % which] = c.matches_row_index(lane, which).tobytes() if which == 0 or len(k) else b""
        out["values%d" % which] = b"|".join(a.tobytes() for a in c.values(lane, which))
    out["tracked"] = c.tracked(lane).tobytes()
    out["result"] = bytes(c.result(lane))
    out["residuals"] = c.residuals(lane).tobytes()
    out["outliers"] = c.outliers(lane).tobytes()
    return out


def assert_same(a, b, tag):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] == b[k], "%s: getter '%s' differs (%d vs %d bytes)" % (tag, k, len(a[k]), len(b[k]))


def tracks_bytes(c, lane):
    return tuple(a.tobytes() for a in c.klt_tracks(lane))


class Pair:
    """A: the resident top-up; B: the recipe.  Both front ends are enabled alike and are given the same calls."""

    def __init__(self, A, B):
        self.A, self.B, self.recipe = A, B, None

    def configure(self, kp, gftt, **topup):
        for c in (self.A, self.B):
            c.reset()
            if self.recipe is not None:            # enabled before: empty tables accept other parameters
                c.klt_reset()
            c.klt_enable(kp)
        self.kp = kp
        self.A.klt_topup_enable(None, **dict(gftt, **topup))
        tp = self.A.klt_topup_default_params()
        for k, v in topup.items():
            setattr(tp, k, v)
        self.recipe = TR.KltTopupRecipe(self.B, kp, TR.TopupParams(kp.cap, tp.below, tp.target, tp.init_disp), gftt_params(gftt))

    def add(self, lane, left, right):
        m = self.A.klt_add_points(lane, left, right)
        assert m == self.B.klt_add_points(lane, left, right)
        return m

    def step(self, frames, flags=0, active=None):
        for c in (self.A, self.B):
            c.klt_step(frames, flags=flags, active=active)
        self.recipe.note_step(frames, active)

    def reset(self, lanes):
        for c in (self.A, self.B):
            c.klt_reset(lanes)
        self.recipe.note_reset(lanes)

    def topup(self, active=None):
        self.A.klt_topup(active)
        self.recipe.topup(active)

    def same_tables(self, tag):
        for l in range(self.A.n_lanes):
            assert tracks_bytes(self.A, l) == tracks_bytes(self.B, l), (tag, l)
            assert self.A.klt_topup_info(l) == self.recipe.info[l], (tag, l, self.A.klt_topup_info(l), self.recipe.info[l])

    def same_getters(self, tag):
        for l in range(self.A.n_lanes):
            assert_same(snapshot(self.A, l), snapshot(self.B, l), "%s lane %d" % (tag, l))

    def close(self):
        self.A.close(); self.B.close()


@pytest.fixture(scope="module")
def small():
    """one lane each, the size of the small scenes"""
    p = Pair(make_ctx(1, TS.W, TS.H), make_ctx(1, TS.W, TS.H))
    yield p
    p.close()


def run_scene(p, s, lane=0, n_lanes=1):
    kp = klt_params(s.cap, s.lk, s.gate)
    p.configure(kp, s.gftt, **s.topup)
    if len(s.tracks[0]):
        assert p.add(lane, *s.tracks) == len(s.tracks[0])
    frames = [(s.left, s.right) if l == lane else None for l in range(n_lanes)]
    p.step(frames, active=[lane])
    p.topup()
    p.same_tables(s.name)
    info = p.A.klt_topup_info(lane)
    e = s.expect
    assert (info[0], info[2], info[3]) == (e["corners"], e["appended"], e["reason"]), (s.name, info)
    tracks = p.A.klt_tracks(lane)
    assert len(tracks[2]) == e.get("n_after", len(s.tracks[0]) + e["appended"])
    # the step after: the new tracks enter the lists, and every getter equals the recipe context's
    p.step(frames, flags=hip.RUN_OPTIMIZE, active=[lane])
    p.same_getters(s.name + ", the step after")
    p.same_tables(s.name + ", the step after")
    return info, tracks


# ---- 1. the scenes: how many are wanted, the seeds, the gate --------------------------------------------------------------------------
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_scene_equals_the_recipe(small, name):
    s = TS.scene(name)
    info, _ = run_scene(small, s)
    # the device against the numpy walk as well: the same corners survive
    _, t1, winfo, _ = TS.walk(name)
    assert info == winfo, (name, info, winfo)


def test_seam_scene_equals_the_recipe():
    s = TS.seam()
    w, h = s.size
    p = Pair(make_ctx(1, w, h, max_cand=4096), make_ctx(1, w, h, max_cand=4096))
    try:
        info, (left, right, ids, age) = run_scene(p, s)
        assert info[0] > 512 and info[2] == s.expect["appended"]
        # the survivors are the corners the scene keeps, in walk order, behind the 8 tracks that were there
        _, t1, _, det = TS.walk("seam")
        assert left[TS.SEAM_TRACKS:].tobytes() == det["corners"][det["keep"]].tobytes()
        assert np.array_equal(ids, np.arange(len(ids)))
    finally:
        p.close()


# ---- 2. five lanes in one call -------------------------------------------------------------------------------------------------------
def test_five_lanes_each_with_its_reason():
    s = TS.scene("want_exceeds_corners")
    pts = TS.grid(TS.W, TS.H, 16)
    p = Pair(make_ctx(5, TS.W, TS.H), make_ctx(5, TS.W, TS.H))
    try:
        p.configure(klt_params(s.cap, s.lk, s.gate), s.gftt, below=10)
        for lane, n in ((0, 2), (1, 10), (2, 2), (4, 3)):
            assert p.add(lane, *TS.tracks_on(pts[:n])) == n
        fr = (s.left, s.right)
        p.step([fr, fr, fr, None, fr], active=[0, 1, 2, 4])          # lane 3 is never fed
        p.reset([4])                                                  # lane 4: reset since its step
        before = [tracks_bytes(p.A, l) for l in range(5)]
        p.topup(active=[0, 1, 3, 4])                                  # lane 2 is out of the mask
        p.same_tables("five lanes")
        reasons = [p.A.klt_topup_info(l)[3] for l in range(5)]
        assert reasons == [abi.TOPUP_OK, abi.TOPUP_ENOUGH, abi.TOPUP_NOT_ASKED, abi.TOPUP_NO_PAIR, abi.TOPUP_NO_PAIR]
        assert p.A.klt_topup_info(0)[2] == 22 and len(p.A.klt_tracks(0)[2]) == 24
        for l in (1, 2, 3, 4):
            assert tracks_bytes(p.A, l) == before[l] and p.A.klt_topup_info(l)[:3] == (0, 0, 0), l
        p.step([fr, fr, fr, None, fr], flags=hip.RUN_OPTIMIZE, active=[0, 1, 2, 4])
        p.same_getters("five lanes, the step after")
        p.same_tables("five lanes, the step after")
        # a second call with another mask: the records are those of the LAST call
        p.topup(active=[2])
        p.same_tables("five lanes, second call")
        assert [p.A.klt_topup_info(l)[3] for l in range(5)] == [abi.TOPUP_NOT_ASKED, abi.TOPUP_NOT_ASKED, abi.TOPUP_OK, abi.TOPUP_NOT_ASKED, abi.TOPUP_NOT_ASKED]
    finally:
        p.close()


# ---- 3. the gate and the append alone, on arrays no image could produce ----------------------------------------------------------------
def test_debug_append_on_hand_built_arrays(small):
    p = small
    s = TS.scene("shifted")
    left, right, status, ok = TS.append_arrays()
    gate = KR.Gate(win=TS.WIN, **TS.GATE)
    full = TS.tracks_on([(10 + k, 10) for k in range(TS.CAP)])
    room_minus_one = TS.tracks_on([(10 + k, 10) for k in range(TS.CAP - int(ok.sum()) + 1)])
    many = TS.tracks_on([(8 + k, 9 + (k % 5)) for k in range(TS.CAP)])     # n = cap, every pair passes
    for tag, start, arrays in (("empty", None, (left, right, status)), ("full", full, (left, right, status)),
                               ("one past cap", room_minus_one, (left, right, status)),
                               ("n = 0", full[0][:5], (left[:0], right[:0], status[:0])),
                               ("n = cap into an empty table", None, many + (np.ones(TS.CAP, np.uint8),)),
                               ("n = cap into a full table", full, many + (np.ones(TS.CAP, np.uint8),))):
        p.configure(klt_params(s.cap, s.lk, s.gate), s.gftt)
        table = KR.Table()
        if start is not None:
            start = start if isinstance(start, tuple) else TS.tracks_on(start)
            p.add(0, *start)
            table, _ = KR.add_points(table, start[0], start[1], TS.CAP)
        p.A.klt_debug_topup_append(0, *arrays)
        want, m, keep = TR.append(table, arrays[0], arrays[1], arrays[2], gate, TS.CAP)
        l, r, ids, age = p.A.klt_tracks(0)
        assert l.tobytes() == want.left.tobytes() and r.tobytes() == want.right.tobytes(), tag
        assert np.array_equal(ids, want.ids) and np.array_equal(age, want.age), tag
        assert p.A.klt_topup_info(0) == (len(arrays[0]), len(arrays[0]), m, abi.TOPUP_OK), tag
        # the recipe's last call on the other context, and a step on both: the appended tracks enter the lists alike
        assert p.B.klt_add_points(0, arrays[0][keep], arrays[1][keep]) == m, tag
        p.step([(s.left, s.right)], flags=hip.RUN_OPTIMIZE)
        p.same_getters(tag)
        assert tracks_bytes(p.A, 0) == tracks_bytes(p.B, 0), tag


# ---- 4. candidate overflow on one lane ------------------------------------------------------------------------------------------------
def test_candidate_overflow_on_one_lane_leaves_the_others_alone():
    w = h = 128
    pts = TS.grid(w, h, 16)
    good = (TS.blobs(w, h, pts), TS.blobs(w, h, pts, dx=1))
    dots = TS.overflow_image(w, h)
    p = Pair(make_ctx(3, w, h), make_ctx(3, w, h))
    try:
        p.configure(klt_params(TS.CAP, TS.LK, TS.GATE), TS.GFTT)
        for lane in range(3):
            assert p.add(lane, *TS.tracks_on(pts[:3])) == 3
        frames = [good, (dots, dots.copy()), good]
        p.step(frames)
        before = tracks_bytes(p.A, 1)
        p.topup()
        p.same_tables("overflow")
        info = p.A.klt_topup_info(1)
        assert info[0] == 0 and info[1] > max(1024, TS.MAX_CAND) and info[2] == 0 and info[3] == abi.TOPUP_OVERFLOW
        assert tracks_bytes(p.A, 1) == before
        for lane in (0, 2):
            assert p.A.klt_topup_info(lane)[3] == abi.TOPUP_OK and p.A.klt_topup_info(lane)[2] == len(pts) - 3
        p.step(frames, flags=hip.RUN_OPTIMIZE)
        p.same_getters("overflow, the step after")
    finally:
        p.close()


# ---- 5. a sequence: step, top up, step, ... -------------------------------------------------------------------------------------------
SEQ_GFTT = dict(max_corners=0, block=3, min_distance=8, quality=0.02)


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "pose_covariance_and_landmarks"])
def test_sequence_step_topup_step(extras):
    frames = KS.sequence_frames()
    lk = dict(KS.SEQ_LK); lk["win"] = 9
    kp = klt_params(KS.SEQ_CAP, lk, KS.SEQ_GATE)
    p = Pair(make_ctx(1, KS.W, KS.H, max_cand=1 << 15), make_ctx(1, KS.W, KS.H, max_cand=1 << 15))
    try:
        if extras:
            for c in (p.A, p.B):
                c.set_pose_covariance(True); c.set_landmarks(True)
        p.configure(kp, SEQ_GFTT, below=KS.SEQ_CAP, init_disp=4.0)
        assert p.add(0, *KS.sequence_points()) == 48
        appended, new_tracked = [], 0
        for f in range(KS.SEQ_FRAMES):
            p.step([frames[f]], flags=hip.RUN_OPTIMIZE)
            p.same_getters("frame %d" % f)
            p.same_tables("frame %d, before the top-up" % f)
            assert bytes(p.A.result(0)) == bytes(p.B.result(0))
            if extras:
                assert bytes(p.A.pose_covariance(0)) == bytes(p.B.pose_covariance(0)), f
                (ia, ra), (ib, rb) = p.A.landmarks(0), p.B.landmarks(0)
                assert bytes(ia) == bytes(ib) and ra.tobytes() == rb.tobytes(), f
            ids, trk = p.A.match_ids(0, 0), p.A.tracked(0)
            new_tracked += int((ids[trk["second"]] >= 48).sum()) if len(trk) else 0
            p.topup()
            p.same_tables("frame %d" % f)
            appended.append(p.A.klt_topup_info(0)[2])
        # tracks really were replaced, and the replaced ones were followed: first without a previous index, then with one
        assert sum(appended) > 0 and new_tracked > 0, (appended, new_tracked)
    finally:
        p.close()


# ---- 6. the primitives in between keep their own buffers -------------------------------------------------------------------------------
def test_primitive_calls_between_topups_are_undisturbed(small):
    import gftt_scenes as GS
    import lk_scenes as LS
    p = small
    s = TS.scene("shifted")
    img = GS.blocks(TS.W, TS.H, 8, 3)
    prev, nxt = LS.texture(TS.W, TS.H, 1), LS.shifted(TS.W, TS.H, 1.25, -0.5, 1)
    pts = LS.grid_points(TS.W, TS.H, 20, 12)
    lkp = hip.default_lk_params(); lkp.win = 9; lkp.max_level = 1
    alone = hip.Context(n_lanes=1, max_w=TS.W, max_h=TS.H, max_kps=TS.MAX_KPS, max_cand=TS.MAX_CAND)
    try:
        g0 = alone.gftt_detect([(img, None, 100)])
        r0 = alone.gftt_response(0)
        l0 = alone.lk_track([(prev, nxt, pts)], lkp)
        lvl0 = alone.lk_level(0, 1, 1)
    finally:
        alone.close()
    p.configure(klt_params(s.cap, s.lk, s.gate), s.gftt)
    p.step([(s.left, s.right)])
    p.A.klt_topup()
    g1 = p.A.gftt_detect([(img, None, 100)])
    l1 = p.A.lk_track([(prev, nxt, pts)], lkp)
    p.A.klt_reset(); p.A.klt_step([(s.left, s.right)]); p.A.klt_topup()      # a top-up AFTER the caller's calls
    assert p.A.klt_topup_info(0)[2] == 24
    # the debug getters still answer for the caller's call, not for the top-up's detector and tracker
    assert p.A.gftt_response(0).tobytes() == r0.tobytes()
    assert p.A.lk_level(0, 1, 1).tobytes() == lvl0.tobytes()
    for a, b in zip(g0[0][:2] + l0[0], g1[0][:2] + l1[0]):
        assert a.tobytes() == b.tobytes()
    assert g0[0][2:] == g1[0][2:]
    # ... and the caller's calls did not disturb the top-up: the recipe's context agrees
    p.B.klt_reset(); p.B.klt_step([(s.left, s.right)]); p.recipe.note_step([(s.left, s.right)]); p.recipe.topup()
    p.same_tables("after the primitives")


# ---- 7. refusals, kernel-time names, a context that never tops up --------------------------------------------------------------------
def test_refusals_leave_the_tables_untouched(small):
    p = small
    s = TS.scene("lands_on_cap")
    L = hip.lib()
    A = p.A
    p.configure(klt_params(s.cap, s.lk, s.gate), s.gftt, target=40)
    p.add(0, *s.tracks)
    p.step([(s.left, s.right)])
    before, info = tracks_bytes(A, 0), A.klt_topup_info(0)
    err = lambda: L.svo_last_error(A.h)
    # the mask
    assert L.svo_klt_topup(A.h, (C.c_uint64 * 2)(2, 0)) == SVO_ERR_ARG and err()
    assert L.svo_klt_topup(A.h, (C.c_uint64 * 2)(0, 1)) == SVO_ERR_ARG and err()
    # the lane calls
    buf = (C.c_int32 * 4)()
    assert L.svo_klt_topup_info(A.h, 1, buf) == SVO_ERR_ARG and b"lane 1 of 1" in err()
    assert L.svo_klt_topup_info(A.h, 0, None) == SVO_ERR_ARG and b"NULL" in err()
    assert L.svo_debug_klt_topup_append(A.h, 0, None, None, None, 3) == SVO_ERR_ARG and b"NULL" in err()
    assert L.svo_debug_klt_topup_append(A.h, 0, None, None, None, -1) == SVO_ERR_ARG
    big = np.zeros((TS.CAP + 1, 2), F)
    assert L.svo_debug_klt_topup_append(A.h, 0, hip._vp(big), hip._vp(big), hip._vp(np.ones(TS.CAP + 1, np.uint8)), TS.CAP + 1) == SVO_ERR_ARG and b"cap = 64" in err()
    # the parameters
    for change, want, text in ((dict(below=0), SVO_ERR_ARG, b"below"), (dict(below=TS.CAP + 1), SVO_ERR_ARG, b"below"), (dict(target=0), SVO_ERR_ARG, b"target"),
                               (dict(target=TS.CAP + 1), SVO_ERR_ARG, b"target"), (dict(init_disp=float("nan")), SVO_ERR_ARG, b"init_disp"),
                               (dict(init_disp=float("inf")), SVO_ERR_ARG, b"init_disp"), (dict(block=4), SVO_ERR_ARG, b"block"),
                               (dict(min_distance=256), SVO_ERR_ARG, b"min_distance"), (dict(quality=0.0), SVO_ERR_ARG, b"quality"),
                               (dict(max_corners=-1), SVO_ERR_ARG, b"max_corners"), (dict(max_corners=TS.MAX_KPS + 1), SVO_ERR_CAPACITY, b"max_kps")):
        tp = A.klt_topup_default_params()
        for k, v in change.items():
            setattr(tp.gftt if k in ("max_corners", "block", "min_distance", "quality") else tp, k, v)
        assert L.svo_klt_topup_enable(A.h, C.byref(tp)) == want and text in err(), change
    assert tracks_bytes(A, 0) == before and A.klt_topup_info(0) == info
    # other parameters: refused after a top-up has run while the table holds tracks, accepted again once it is empty
    tp = A.klt_topup_default_params(); tp.gftt = gftt_params(s.gftt)
    A.klt_topup(); p.recipe.topup()
    p.same_tables("after the refusals")                               # the top-up is what it would have been
    assert A.klt_topup_info(0)[2] == 32
    after = tracks_bytes(A, 0)
    tp.target = 50
    assert L.svo_klt_topup_enable(A.h, C.byref(tp)) == SVO_ERR_STATE and b"svo_klt_reset" in err()
    tp.target = 40
    assert L.svo_klt_topup_enable(A.h, C.byref(tp)) == 0              # the parameters in force: nothing happens
    assert tracks_bytes(A, 0) == after
    A.klt_reset()
    tp.target = 50
    assert L.svo_klt_topup_enable(A.h, C.byref(tp)) == 0
    # contexts in the wrong state
    c = hip.Context(n_lanes=1, max_w=TS.W, max_h=TS.H, max_kps=TS.MAX_KPS, max_cand=TS.MAX_CAND)
    try:
        for rc in (L.svo_klt_topup_enable(c.h, None), L.svo_klt_topup(c.h, None), L.svo_klt_topup_info(c.h, 0, buf), L.svo_debug_klt_topup_append(c.h, 0, None, None, None, 0)):
            assert rc == SVO_ERR_STATE and b"svo_klt_enable" in L.svo_last_error(c.h)
        c.klt_enable(klt_params(s.cap, s.lk, s.gate))
        for rc in (L.svo_klt_topup(c.h, None), L.svo_klt_topup_info(c.h, 0, buf), L.svo_debug_klt_topup_append(c.h, 0, None, None, None, 0)):
            assert rc == SVO_ERR_STATE and b"svo_klt_topup_enable" in L.svo_last_error(c.h)
        assert L.svo_klt_topup_enable(c.h, None) == 0                 # the defaults; no svo_set_params is needed
        d = c.klt_topup_default_params()
        assert (d.below, d.target) == (32, 64)
        assert L.svo_klt_topup(c.h, None) == 0 and c.klt_topup_info(0) == (0, 0, 0, abi.TOPUP_NO_PAIR)
    finally:
        c.close()
    # (a context whose max_cand exceeds 2^24 and a response-map buffer the device cannot provide would each need gigabytes of device
    #  memory to set up: tools/klt_topup_check.cpp holds the first refusal, the second is svo_gftt_detect's, allocation for allocation)


def test_kernel_time_names_and_a_context_that_never_tops_up():
    s = TS.scene("shifted")
    c = make_ctx(1, TS.W, TS.H, kernel_times=True)
    try:
        names0 = list(c.kernel_times(appended=True))
        c.klt_enable(klt_params(s.cap, s.lk, s.gate))
        c.klt_step([(s.left, s.right)], flags=0); c.klt_step([(s.left, s.right)], flags=0)
        stepped = c.kernel_times(appended=True)
        assert list(stepped)[len(names0):] == ["lk_pyrdown", "lk_track", "klt_select"]          # as before this feature
        c.klt_topup_enable(None, **s.gftt)
        assert list(c.kernel_times(appended=True)) == list(stepped)                               # enabling alone lists and launches nothing
        assert {k: v[1] for k, v in c.kernel_times(appended=True).items()} == {k: v[1] for k, v in stepped.items()}
        c.klt_topup()
        kt = c.kernel_times(appended=True)
        assert list(kt)[len(names0):] == ["gftt_response", "gftt_candidates", "gftt_select", "lk_pyrdown", "lk_track", "klt_select", "klt_topup"]
        assert kt["klt_topup"][1] == 3 and kt["gftt_response"][1] == kt["gftt_candidates"][1] == kt["gftt_select"][1] == 1
        assert kt["lk_track"][1] == stepped["lk_track"][1] + 1 and kt["klt_select"][1] == 2
        assert list(c.kernel_times()) == names0[:c.FRAME_KERNEL_NAMES]
        c.kernel_times_select("klt_topup"); c.kernel_times_select(None)
    finally:
        c.close()
