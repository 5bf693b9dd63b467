"""The resident KLT front end under svo_lk_set_photometric(ctx, 1) on the GPU.

The contracts of the front end are recipes of public calls.  They hold verbatim in mode 1 because the recipe's svo_lk_track /
svo_lk_track_rows calls run on a context in the same mode: two contexts in one mode, A stepping resident, B driven by the host recipe
(tests/klt_ref.py, tests/klt_stereo_ref.py, tests/klt_topup_ref.py); after every step all getters and svo_klt_get_tracks are equal as
bytes.  The sequence is tests/klt_scenes.py's five frames with a gain and an offset of its own on every frame and the right camera at
0.8 x the left one's gain."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import abi, hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klt_predict_scenes as PS                                                        # noqa: E402
import klt_ref as KR                                                                   # noqa: E402
import klt_scenes as KS                                                                # noqa: E402
import klt_stereo_ref as SR                                                            # noqa: E402
import klt_topup_ref as TR                                                             # noqa: E402
from test_gpu_klt_predict import (SEQ_GFTT, assert_runs_equal, assert_tracks, drive, host_topup, make_ctx, recipe_run, same,      # noqa: E402
                                  seq_klt_params)

pytestmark = pytest.mark.gpu

EXPOSURE = ((1.0, 0.0), (1.25, 10.0), (0.8, -6.0), (1.1, 18.0), (0.7, 4.0))      # (gain, offset) of each frame
RIGHT_GAIN = 0.8
_frames = {}


def photo_frames():
    """the sequence's frames as two cameras under auto-exposure would deliver them"""
    if not _frames:
        u8 = lambda f: np.clip(np.rint(f), 0, 255).astype(np.uint8)
        _frames["f"] = [(u8(g * l.astype(np.float64) + b), u8(RIGHT_GAIN * (g * r.astype(np.float64) + b)))
                        for (l, r), (g, b) in zip(KS.sequence_frames(), EXPOSURE)]
    return _frames["f"]


def pair_in_mode(mode):
    A, B = make_ctx(), make_ctx()
    for c in (A, B):
        c.lk_set_photometric(mode)
    return A, B


def survivors(ref):
    return [len(table) for _, table, _ in ref]


@pytest.mark.parametrize("stereo", [0, 1])
def test_a_sequence_in_mode_1_equals_the_recipe_in_mode_1(stereo):
    kp = seq_klt_params()
    A, B = pair_in_mode(1)
    try:
        A.klt_enable(kp); A.klt_set_stereo(stereo)
        assert A.lk_get_photometric() == 1                                  # svo_klt_enable does not reset the tracker's mode
        fe = (SR.KltStereoHostFrontEnd if stereo else KR.KltHostFrontEnd)(B, kp, KS.H)
        got = drive(A, photo_frames(), KS.sequence_points())
        ref = recipe_run(B, fe, photo_frames(), KS.sequence_points())
        assert_runs_equal(got, ref, "photometric mode 1, stereo %d" % stereo)
        # asserted on the RECIPE: tracks live to the last frame, and the mode matters on this sequence (mode 0 leaves other bytes)
        B.lk_set_photometric(0)
        fe0 = (SR.KltStereoHostFrontEnd if stereo else KR.KltHostFrontEnd)(B, kp, KS.H)
        ref0 = recipe_run(B, fe0, photo_frames(), KS.sequence_points())
        print("stereo %d: tracks per frame, mode 1 %s, mode 0 %s" % (stereo, survivors(ref), survivors(ref0)))
        assert survivors(ref)[-1] > 0
        assert any(r[0] != r0[0] for r, r0 in zip(ref, ref0))
    finally:
        A.close(); B.close()


def test_a_topup_between_the_steps_equals_its_recipe_in_mode_1():
    kp = seq_klt_params(fb_max=0.5)
    frames, points = photo_frames(), KS.sequence_points()
    A, B = pair_in_mode(1)
    try:
        A.klt_enable(kp)
        fe = KR.KltHostFrontEnd(B, kp, KS.H)
        A.klt_topup_enable(None, below=KS.SEQ_CAP, init_disp=4.0, **SEQ_GFTT)
        tp, gp = TR.TopupParams(kp.cap, KS.SEQ_CAP, KS.SEQ_CAP, 4.0), abi.GfttParams(SEQ_GFTT["max_corners"], SEQ_GFTT["block"], SEQ_GFTT["min_distance"], SEQ_GFTT["quality"])
        assert A.klt_add_points(0, *points) == fe.add_points(0, *points) == 48
        appended = 0
        for f in range(KS.SEQ_FRAMES):
            A.klt_step([frames[f]]); fe.step([frames[f]])
            same(A, B, fe, 0, "frame %d" % f)
            A.klt_topup()
            appended += host_topup(B, fe, 0, frames[f], kp, tp, gp)
            assert_tracks(A, 0, fe.tables[0], "frame %d after the top-up" % f)
        assert appended > 0 and len(fe.tables[0]) > 0                       # asserted on the RECIPE
        assert A.lk_get_photometric() == 1
    finally:
        A.close(); B.close()


def test_both_contexts_in_mode_0_reproduce_the_bytes_of_a_context_that_never_set_the_mode():
    kp = seq_klt_params()
    A, B = pair_in_mode(1)
    C = make_ctx(kernel_times=True)
    try:
        for c in (A, B):
            c.lk_set_photometric(0)
        A.klt_enable(kp); C.klt_enable(kp)
        fe = KR.KltHostFrontEnd(B, kp, KS.H)
        got = drive(A, photo_frames(), KS.sequence_points())
        assert_runs_equal(got, recipe_run(B, fe, photo_frames(), KS.sequence_points()), "mode 0 after mode 1")
        never = drive(C, photo_frames(), KS.sequence_points())
        for f, ((s, t), (s0, t0)) in enumerate(zip(got, never)):
            assert s == s0 and all(x.tobytes() == y.tobytes() for x, y in zip(t, t0)), f
        # ... and the same launches under the same names in both modes
        names0 = {k: v[1] for k, v in C.kernel_times(appended=True).items()}
        C.lk_set_photometric(1)
        drive(C, photo_frames(), KS.sequence_points())
        names1 = {k: v[1] for k, v in C.kernel_times(appended=True).items()}
        assert list(names1) == list(names0) and all(names1[k] == 2 * names0[k] for k in names0 if k.startswith(("lk_", "klt_")))
    finally:
        A.close(); B.close(); C.close()
