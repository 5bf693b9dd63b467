"""The RANSAC gate of the resident KLT front end (svo_klt_set_ransac) on the GPU, held byte for byte to its recipe.

Every comparison is between two contexts: A steps with the gate resident, B is driven by tests/ransac_tracked_ref.KltRansacHostFrontEnd
-- the recipe of tests/klt_ref.py up to its puts, the public svo_ransac_tracked, for mode 2 svo_get_tracked and the removal from the
host's table, then stage 5.  After every step all getters (`snapshot` of tests/test_gpu_klt.py) and svo_klt_get_tracks must be equal."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import abi, hip
from stereo_vo_amd.abi import VOEC_BAD_TRACKING

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402
import ransac_tracked_ref as RR                                                        # noqa: E402
import ransac_tracked_scenes as RS                                                     # noqa: E402
from test_gpu_klt import assert_same, assert_tracks, klt_params, make_ctx, snapshot    # noqa: E402

pytestmark = pytest.mark.gpu


def same(A, B, fe, lane, tag):
    assert_same(snapshot(A, lane), snapshot(B, lane), tag)
    assert_tracks(A, lane, fe.tables[lane], tag)


# ---- 1. hand-built steps ---------------------------------------------------------------------------------------------------------
class Pair:
    """A: the resident gate; B with fe: the recipe"""
    def __init__(self, n_lanes, mode):
        kp = klt_params(KS.CAP, dict(win=KS.WIN), KS.GATE)
        self.A, self.B = make_ctx(n_lanes), make_ctx(n_lanes)
        self.A.klt_enable(kp)
        self.A.klt_step([(np.zeros((KS.H, KS.W), np.uint8),) * 2] * n_lanes, flags=0)     # a step gives the context the geometry of the scenes' image size
        self.A.reset(); self.A.klt_reset()
        self.A.klt_set_ransac(mode)
        assert self.A.klt_ransac() == mode
        self.fe = RR.KltRansacHostFrontEnd(self.B, kp, KS.H, mode)

    def add(self, lane, l, r):
        assert self.A.klt_add_points(lane, l, r) == self.fe.add_points(lane, l, r)

    def select(self, lane, l, r, tag):
        n = len(l)
        self.A.klt_debug_select(lane, l, r, KS.ones(n), KS.ones(n))
        self.fe.debug_select(lane, l, r, KS.ones(n), KS.ones(n), KS.W, KS.H)
        same(self.A, self.B, self.fe, lane, tag)
        (_, lost), = self.fe.rejected
        return lost

    def hold(self, lane):
        """stage 4 on the put lists ends in voecBadTracking (bad_tracking_th of test_gpu_klt.params): the lane keeps its previous frame"""
        for c in (self.A, self.B):
            c.run_stages(hip.RUN_TRACK, [lane] if c.n_lanes > 1 else None)
            assert c.result(lane).error_code == VOEC_BAD_TRACKING

    def close(self):
        self.A.close(); self.B.close()


def run_steps(p, lane, world, mode, hold_before_third=False, slide=True):
    """add, then three selections; the second and third with slid tracks at the seams.  Returns the rejected list indices per step"""
    ids = np.arange(world.n)
    p.add(lane, *world.arrays(0, ids)[:2])
    out = []
    for k in range(3):
        ids = p.fe.tables[lane].ids
        l, r, slid = world.arrays(k, ids, RS.SEAMS if (k and slide) else ())
        if k == 2 and hold_before_third:
            p.hold(lane)
        lost = p.select(lane, l, r, "lane %d step %d mode %d" % (lane, k, mode))
        out.append((lost, slid))
    return out


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_built_steps_one_lane(mode):
    p = Pair(1, mode)
    try:
        world = RS.StepWorld(KS.CAP)
        steps = run_steps(p, 0, world, mode)
        assert len(steps[0][0]) == 0                                      # no p yet: nothing to verify, nothing leaves
        for k in (1, 2):                                                  # asserted on the RECIPE: the slid tracks at the seams are rejected
            lost, slid = steps[k]
            hit = set(int(v) for v in np.intersect1d(lost, slid))
            assert len(hit) >= len(slid) - 2 and hit & {63, 64} and hit & {255, 256}, (k, sorted(hit))
        n_live = len(p.A.klt_tracks(0)[2])
        if mode == 2:                                                     # the dropped tracks are gone, and p indexes the previous list, not the table
            assert n_live == KS.CAP - len(steps[1][0]) - len(steps[2][0]) < KS.CAP
            trk = p.A.tracked(0)
            assert (trk["first"] != trk["second"]).any() and len(trk) >= 0.9 * n_live
            assert "klt_prune" in p.A.kernel_times(appended=True)
        else:
            assert n_live == KS.CAP and "klt_prune" not in p.A.kernel_times(appended=True)
        assert "ransac_feed" in p.A.kernel_times(appended=True)
        ts = p.A.result(0).track_stats
        assert ts[RR.TS_THRESHOLD] == ts[RR.TS_COLLISION] > 0 and ts[RR.TS_TRACKED] == len(p.A.tracked(0))
    finally:
        p.close()


@pytest.mark.parametrize("mode", [1, 2])
def test_hand_built_steps_ten_lanes(mode):
    """lane 1: the full table; lane 4: a lane that holds its previous frame before its third step; lane 6: ten tracks (the LMedS path);
    lane 9: nothing slides, nothing leaves; the other lanes are never fed"""
    p = Pair(10, mode)
    try:
        full = run_steps(p, 1, RS.StepWorld(KS.CAP, 1), mode)
        held = run_steps(p, 4, RS.StepWorld(90, 2), mode, hold_before_third=True)
        run_steps(p, 6, RS.StepWorld(10, 3), mode)
        clean = run_steps(p, 9, RS.StepWorld(70, 4), mode, slide=False)
        assert len(np.intersect1d(*full[1])) >= len(full[1][1]) - 2 and len(np.intersect1d(*held[2])) >= 1
        assert all(len(lost) == 0 for lost, _ in clean) and len(p.A.klt_tracks(9)[2]) == 70
        trk = p.A.tracked(4)                                              # the held lane's pairs go back two selections
        assert len(trk) and (mode == 1 or (trk["first"] != trk["second"]).any())
        for lane in (1, 4, 6, 9):                                         # the later lanes' steps left the earlier lanes alone
            same(p.A, p.B, p.fe, lane, "lane %d at the end" % lane)
        for lane in (0, 2, 3, 5, 7, 8):
            assert len(p.A.klt_tracks(lane)[2]) == 0 and len(p.A.tracked(lane)) == 0
    finally:
        p.close()


# ---- 2. the image sequence: steps with stage 5, a top-up in between, mode 2 -----------------------------------------------------------
SEQ_GFTT = dict(max_corners=0, block=3, min_distance=8, quality=0.02)


def host_topup(B, fe, lane, pair, kp, tp, gp):
    """the recipe of svo_klt_topup on the HOST's table (tests/klt_topup_ref.py): detect, track left to right, gate, append"""
    t = fe.tables[lane]
    want = TR.want_of(len(t), kp.cap, tp)
    if want is None:
        return 0
    (corners, _, _, status), = B.gftt_detect([(pair[0], t.left, want)], gp)
    assert status == 0
    (out, st, _), = B.lk_track([(pair[0], pair[1], corners, TR.first_guess(corners, tp.init_disp))], kp.lk)
    fe.tables[lane], m, _ = TR.append(t, corners, out, st, fe.gate, kp.cap)
    return m


def test_sequence_with_stage5_and_topups_mode_2():
    lanes = {0: RS.gate_sequence_frames(), 1: KS.sequence_frames()}      # lane 0 carries the moving patch
    points = {0: RS.gate_sequence_points(), 1: KS.sequence_points()}
    kp = klt_params(KS.SEQ_CAP, KS.SEQ_LK, KS.SEQ_GATE)
    A, B = make_ctx(2, max_cand=1 << 15), make_ctx(2, max_cand=1 << 15)
    try:
        A.klt_enable(kp)
        A.klt_set_ransac(abi.KLT_RANSAC_PRUNE)
        A.klt_topup_enable(None, below=KS.SEQ_CAP, init_disp=4.0, **SEQ_GFTT)
        fe = RR.KltRansacHostFrontEnd(B, kp, KS.H, 2)
        tp, gp = TR.TopupParams(kp.cap, KS.SEQ_CAP, KS.SEQ_CAP, 4.0), abi.GfttParams(SEQ_GFTT["max_corners"], SEQ_GFTT["block"], SEQ_GFTT["min_distance"], SEQ_GFTT["quality"])
        for l in lanes:
            assert A.klt_add_points(l, *points[l]) == fe.add_points(l, *points[l]) == len(points[l][0])
        rejected, appended, valid = {0: 0, 1: 0}, 0, 0
        for f in range(KS.SEQ_FRAMES):
            frames = [lanes[0][f], lanes[1][f]]
            A.klt_step(frames)
            fe.step(frames)
            for l, lost in fe.rejected:
                rejected[l] += len(lost)
            for l in lanes:
                same(A, B, fe, l, "frame %d lane %d" % (f, l))
            valid += int(B.result(0).valid == 1)
            A.klt_topup()
            for l in lanes:
                appended += host_topup(B, fe, l, frames[l], kp, tp, gp)
                assert_tracks(A, l, fe.tables[l], "frame %d lane %d after the top-up" % (f, l))
        # asserted on the RECIPE's side: the gate rejected tracks, the top-up refilled the tables, stage 5 ran on the filtered pairs
        assert rejected[0] >= 1 and appended > 0 and valid >= 1, (rejected, appended, valid)
    finally:
        A.close(); B.close()


# ---- 3. mode 0 is the front end as it was ---------------------------------------------------------------------------------------------
def test_mode_0_equals_a_context_that_never_called_the_setter():
    kp = klt_params(KS.SEQ_CAP, KS.SEQ_LK, KS.SEQ_GATE)
    A, B = make_ctx(), make_ctx()
    try:
        for c in (A, B):
            c.klt_enable(kp)
        A.klt_set_ransac(2); A.klt_set_ransac(0)
        assert A.klt_ransac() == 0 and B.klt_ransac() == 0
        for c in (A, B):
            assert c.klt_add_points(0, *RS.gate_sequence_points()) == 52
        for f, fr in enumerate(RS.gate_sequence_frames()[:3]):
            for c in (A, B):
                c.klt_step([fr])
            assert_same(snapshot(A), snapshot(B), "frame %d" % f)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(A.klt_tracks(0), B.klt_tracks(0)))
        ka, kb = A.kernel_times(appended=True), B.kernel_times(appended=True)
        assert list(ka) == list(kb) and "ransac_feed" not in ka and "klt_prune" not in ka
        assert [v[1] for v in ka.values()] == [v[1] for v in kb.values()]             # the same launches were counted
    finally:
        A.close(); B.close()
