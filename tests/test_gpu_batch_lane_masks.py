"""svo_batch_step_lanes: ragged streams through the batched scheduler.  Two contexts of three lanes, the pipelined detect-ahead
schedule and the free one; every stream is held against an oracle of its own that sees a frame only on the stream's active steps,
through the contexts' getters, through svo_batch_results and through the caller-owned records buffer."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import Result, north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import O, POSE_TOL_M, POSE_TOL_RAD        # noqa: E402
from test_gpu_lane_masks import W, H, assert_fresh, assert_lane, lane_frames       # noqa: E402

pytestmark = pytest.mark.gpu

# global lanes 0-2: context 0, 3-5: context 1.  Step 1: context 1 wholly idle.  Step 2: one idle lane in each context.
# Step 4: context 0 wholly idle.
MASKS = ([0, 1, 2, 3, 4, 5], [0, 1, 2], [0, 2, 3, 4], [1, 2, 3, 5], [3, 5], [0, 1, 2, 3, 4, 5])


def streams():
    """six streams out of the four rendered worlds (read only): two of them mirrored, one the second half of the longest"""
    f, cam = lane_frames()
    mirror = lambda seq: [(np.ascontiguousarray(r[:, ::-1]), np.ascontiguousarray(l[:, ::-1])) for l, r in seq]
    return [f[0][:4], f[1], mirror(f[0][:5]), mirror(f[1]), f[2], f[0][4:]], cam


def assert_record(r, ro, tag):
    assert (r.valid, r.error_code, r.detected_left[0], r.detected_right[0], r.stereo_matches[0], r.tracked_feats_from_last_frame, r.n_residual, r.n_outliers) == \
           (ro.valid, ro.error_code, ro.detected_left[0], ro.detected_right[0], ro.stereo_matches[0], ro.tracked_feats_from_last_frame, ro.n_residual, ro.n_outliers), tag
    assert list(r.track_stats) == list(ro.track_stats), tag
    if ro.valid:
        dp = np.abs(np.array(r.outPose) - np.array(ro.outPose))
        assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (tag, dp)


@pytest.mark.parametrize("schedule", ["pipelined", "free"])
def test_ragged_streams_through_the_batch(schedule):
    import torch
    from stereo_vo_amd.pipeline import StreamBatch
    src, cam = streams()
    p = north_star_params(hip.default_params(), orb_nfeats=400)
    batch = StreamBatch(p, cam, W, H, 6, 2, schedule=schedule, max_kps=1024, max_cand=1 << 15)
    assert batch.pipelined == (schedule == "pipelined")
    dev = [[(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in s] for s in src]
    torch.cuda.synchronize()
    orcs, last, k = [O().Oracle(p) for _ in range(6)], [None] * 6, [0] * 6
    for step, act in enumerate(MASKS):
        if step in (1, 4):
            batch.flip_records()          # a context that sits the step out must still leave its records in the buffer now in use
        batch.step([(dev[g][k[g]][0].data_ptr(), dev[g][k[g]][1].data_ptr()) if g in act else None for g in range(6)], active=act)
        for g in act:
            last[g] = orcs[g].process(src[g][k[g]][0], src[g][k[g]][1], cam)
            k[g] += 1
        batch.synchronize()
        res = batch.results()
        own = batch.rec.cpu().numpy()
        for g in range(6):
            c, lane = batch.lane(g)
            tag = "%s step %d stream %d (%s)" % (schedule, step, g, "active" if g in act else "idle")
            mine = Result.from_buffer_copy(own[g].tobytes())
            assert bytes(mine) == bytes(res[g]), (tag, "records buffer against svo_batch_results")
            if last[g] is None:
                assert_fresh(c, lane, 1, tag)
                continue
            assert_lane(c, lane, orcs[g], last[g], 1, False, tag)
            assert_record(res[g], last[g], tag)
    assert k == [4, 4, 5, 5, 3, 4] and sum(1 for r in res if r.valid) == 6
    batch.close()
    # a stream at or above svo_batch_lanes is refused before anything is enqueued
    batch = StreamBatch(p, cam, W, H, 6, 2, schedule=schedule, max_kps=1024, max_cand=1 << 15)
    rc = batch.L.svo_batch_step_lanes(batch.h, (hip.Frame * 6)(), C.c_uint32(hip.FLAG_DEVICE_IMAGES), (C.c_uint64 * 1)(1 << 6))
    assert rc == -2 and b"svo_batch_lanes" in batch.L.svo_batch_last_error(batch.h)
    batch.close()
