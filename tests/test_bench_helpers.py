"""CPU checks of bench.py's host-side helpers that need no GPU: the sweep of the in-kernel launch timeline (SVO_TIMELINE=1, `--timeline`),
the frame schedules and the --dump-outputs writer."""
import os

import numpy as np

import bench
from stereo_vo_amd.abi import Result, dmatch_dtype, index_pair_dtype, keypoint_dtype


class _FakeCtx:
    """what hip.Context.timeline() returns: (frame counter, [16 frames][32 kinds][8 aux][2] ticks of 10 ns, t0 = 2**64 - 1 where nothing ran)"""
    def __init__(self, launches):
        self.a = np.full((16, 32, 8, 2), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
        self.a[..., 1] = 0
        for frame, kind, aux, t0_us, t1_us in launches:
            self.a[frame % 16, bench.TIMELINE_KINDS.index(kind), aux] = (int(t0_us * 100), int(t1_us * 100))

    def timeline(self, reset=False):
        return 1, self.a


def test_timeline_sweep_counts_queues_gaps_and_lonely_kernels():
    """Two contexts.  Detect stream (queue 0): ctx 0 runs fast 0-100 us and select 110-120 us (a 10 us gap), ctx 1 runs fast 120-220 us.
    Stage 3-5 streams: ctx 0's describe 100-200 us (queue 1), ctx 1's gauss_newton 150-250 us (queue 2).
    Busy 0-250 us:  [0,100) fast alone | [100,110) describe alone | [110,120) select + describe | [120,150) fast + describe |
    [150,200) fast + describe + gn | [200,220) fast + gn | [220,250) gn alone."""
    c0 = _FakeCtx([(1, "fast", 0, 0, 100), (1, "select", 0, 110, 120), (1, "describe", 1, 100, 200)])
    c1 = _FakeCtx([(1, "fast", 0, 120, 220), (1, "gauss_newton", 0, 150, 250)])
    r = bench.timeline_report([c0, c1], True)
    assert r["launches"] == 5 and abs(r["span_ms"] - 0.25) < 1e-9 and r["idle_frac"] == 0
    q = r["queues_executing_frac_of_busy"]
    assert abs(q["1"] - 140 / 250) < 1e-3 and abs(q["2"] - 60 / 250) < 1e-3 and abs(q["3"] - 50 / 250) < 1e-3
    assert abs(r["mean_queues_executing"] - (140 + 120 + 150) / 250) < 2e-3
    alone = r["alone_on_chip_by_kernel_frac_of_busy"]
    assert abs(alone["fast"] - 0.4) < 1e-3 and abs(alone["describe"] - 0.04) < 1e-3 and abs(alone["gauss_newton"] - 0.12) < 1e-3
    pairs = r["two_in_flight_pairs_frac_of_busy"]
    assert abs(pairs["describe + fast"] - 30 / 250) < 1e-3 and abs(pairs["describe + select"] - 10 / 250) < 1e-3 and abs(pairs["fast + gauss_newton"] - 20 / 250) < 1e-3
    det = r["per_queue"]["detect"]
    assert det["launches"] == 3 and abs(det["executing_frac_of_span"] - 210 / 250) < 1e-3 and abs(det["gap_us_mean"] - 10.0) < 1e-6      # one gap of 10 us (back-to-back launches are not gaps)
    assert r["per_queue"]["rest0"]["launches"] == 1 and r["per_queue"]["rest1"]["launches"] == 1
    assert r["hull_us_mean"]["describe"] == 100.0 and r["hull_us_mean"]["fast[0]"] == 100.0
    # with the NMS / description kept on the detect stream (post_on_rest = False) describe belongs to queue 0
    r0 = bench.timeline_report([c0, c1], False)
    assert r0["per_queue"]["detect"]["launches"] == 4 and r0["per_queue"]["rest0"]["launches"] == 0


def test_timeline_sweep_without_records_says_so():
    assert "error" in bench.timeline_report([_FakeCtx([])], True)


def test_frames_needed_and_lane_frame_never_repeat_a_frame():
    T, B, steps = 8, 192, 105
    F = bench.frames_needed(B, T, steps)
    for lane in (0, 7, 8, 100, 191):
        seen = [bench.lane_frame(lane, i, T, F) for i in range(steps)]
        assert len(set(seen)) == steps and all(j == lane % T for j, _ in seen)
        assert all(b[1] == a[1] + 1 for a, b in zip(seen, seen[1:]))            # consecutive frames of one trajectory


def test_plain_run_pool_never_shows_two_streams_one_frame_and_keeps_poses_consecutive():
    """The plain run's pool: a size that does not depend on the number of steps; at every step the 192 streams read 192 different
    frames of it (no stream reads a frame another one reads in the same step), and every stream moves one frame per step."""
    T, B = 8, 192
    F = bench.pool_frames(B, T)
    assert F == B // T - 1 + bench.POOL_SWING
    prev = None
    for i in range(3 * bench.POOL_SWING):
        now = [bench.pool_frame(lane, i, T) for lane in range(B)]
        assert len(set(now)) == B and all(0 <= t < F and j == lane % T for lane, (j, t) in enumerate(now))
        if prev is not None:
            assert all(abs(a[1] - b[1]) == 1 for a, b in zip(prev, now))
        prev = now


class _ListsCtx:
    """what hip.Context's list getters return for one lane: n keypoints per side, n // 2 pairings, n // 4 tracked pairs"""
    def __init__(self, n):
        self.n = n

    def keypoints(self, lane, which, side, octave):
        assert all(type(v) is int for v in (lane, which, side, octave))         # what ctypes converts
        k = np.zeros(self.n, keypoint_dtype)
        k["x"] = np.arange(self.n) + 0.25 + lane; k["y"] = side + 0.5; k["octave"] = octave
        return k, np.full((self.n, 32), 200 + side, np.uint8)

    def matches(self, lane, which, octave):
        m = np.zeros(self.n // 2, dmatch_dtype)
        m["queryIdx"] = np.arange(self.n // 2); m["distance"] = 7.0
        return m

    def tracked(self, lane, octave):
        return np.zeros(self.n // 4, index_pair_dtype)

    def residuals(self, lane):
        return np.linspace(0.0, 1.0, self.n // 4)


class _Batch:
    def __init__(self, B, n):
        self.B, self.ctx = B, _ListsCtx(n)

    def lane(self, g):
        return self.ctx, g


def test_dump_outputs_writes_every_record_field_and_a_fixed_sample_of_lists(tmp_path):
    B = 24
    recs = (Result * B)()
    for g in range(B):
        recs[g].outPose[0] = 0.125 * g; recs[g].valid = g % 2; recs[g].n_octaves = 1; recs[g].track_stats[7] = g
    raw = np.frombuffer(bytes(recs), np.uint8).reshape(B, -1)
    d1, d2 = str(tmp_path / "a"), str(tmp_path / "b")
    n1 = bench.dump_outputs(d1, _Batch(B, 40), raw, 4096)
    n2 = bench.dump_outputs(d2, _Batch(B, 40), raw, 4096)
    names = sorted(os.listdir(d1))
    assert names == sorted(os.listdir(d2)) and n1 == n2 and n1 < 64 << 20
    arrs = {f[:-4]: np.load(os.path.join(d1, f)) for f in names}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert arrs["result_outPose"].shape == (B, 6) and arrs["result_outPose"][5, 0] == 0.625
    assert list(arrs["result_valid"]) == [g % 2 for g in range(B)] and arrs["result_track_stats"][9, 7] == 9
    lanes = sorted({int(f[4:7]) for f in arrs if f.startswith("lane")})
    assert len(lanes) == bench.DUMP_LANES and all(0 <= g < B for g in lanes)
    g = lanes[0]
    k = arrs["lane%03d_o0_keypoints_right" % g]
    assert k.shape == (40, 7) and k[3, 0] == 3.25 + g and k[0, 1] == 1.5
    assert arrs["lane%03d_o0_descriptors_left" % g].shape == (40, 32) and arrs["lane%03d_o0_descriptors_left" % g].max() == 200
    assert arrs["lane%03d_o0_pairings" % g].shape == (20, 4) and arrs["lane%03d_o0_tracked" % g].shape == (10, 2)
    assert arrs["lane%03d_residuals" % g].shape == (10,)
    for f in names:
        assert np.array_equal(np.load(os.path.join(d1, f)), np.load(os.path.join(d2, f)))
