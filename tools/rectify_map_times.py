#!/usr/bin/env python3
"""What it costs to give every lane of a context its rectification maps, the old way and from a calibration, at the benchmarked context
shape: ONE context of `lanes` streams at 1280x960.
  (a) the float maps of the calibration (tests/rectify_ref.py computes them on the host, outside the timed span) through
      svo_set_rectify_map(lane = -1), both sides: one host conversion and one 9.8 MB upload per lane and side, one table per lane;
  (b) svo_set_stereo_calibration(lane = -1) for the same maps: one k_rectify_map launch, one table per side shared by every lane;
  (c) stage 1 per frame with either: the `begin_frame` span of svo_kernel_times, which brackets k_begin_frame AND k_prepare (k_prepare
      has no span of its own), per launch, on device frames with SVO_RUN_DETECT alone -- per-lane copies against the shared table.
Each setter is timed twice: the first call of a context allocates the tables, the second only fills them.  The two contexts' tables
are compared entry for entry on the first and the last lane.
Prints one JSON line (profiles/rectify_map_times.json).  No threshold hangs on these figures."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params
import rectify_ref as RR

W, H = 1280, 960


def frames_pass(ctx, lanes, L, R, warm, timed):
    def step():
        ctx.process_device([(L.data_ptr(), R.data_ptr())] * lanes, W, H, W, hip.RUN_DETECT)
    for _ in range(warm):
        step()
    ctx.wait(); ctx.kernel_times_reset()
    for _ in range(timed):
        step()
    kt = ctx.kernel_times()
    return {"begin_frame_plus_prepare_us_per_launch": round(1e3 * kt["begin_frame"][0] / kt["begin_frame"][1], 2), "launches": kt["begin_frame"][1]}


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return round(1e3 * (time.perf_counter() - t0), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=96)
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cal = RR.calibration_mild(0, W, H, 600.0)
    _, sides = RR.walk(cal)
    calib = RR.to_ctypes(cal)
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (H, W)).astype(np.uint16)
    img = ((img + np.roll(img, 1, 1) + np.roll(img, 1, 0) + np.roll(img, (1, 1), (0, 1))) // 4).astype(np.uint8)
    L = torch.from_numpy(img).to(dev); R = torch.from_numpy(np.roll(img, -6, axis=1).copy()).to(dev)
    p = north_star_params(hip.default_params(), orb_nfeats=a.orb_nfeats)
    out = {"shape": "%dx%d, one context of %d lanes, maps of the mild test calibration at f = 600; wall times of the setter calls in ms (first call allocates, second refills); begin_frame span = k_begin_frame + k_prepare, %d timed detect-only frames on device images" % (W, H, a.lanes, a.steps)}
    tables = {}
    for name in ("float_maps_per_lane", "calibration_shared"):
        ctx = hip.Context(n_lanes=a.lanes, max_w=W, max_h=H, max_kps=4096, kernel_times=True)
        ctx.set_params(p)

        def old():
            for side in range(2):
                ctx.set_rectify_map(-1, side, sides[side]["mx"], sides[side]["my"])

        def new():
            ctx.set_stereo_calibration(calib, lane=-1, set_camera=True)
        fn = old if name == "float_maps_per_lane" else new
        entry = {"first_call_ms": timed_ms(fn), "second_call_ms": timed_ms(fn)}
        if name == "float_maps_per_lane":
            ctx.set_camera(hip.stereo_rectify(calib).cam)
        entry["map_bytes_on_device"] = (2 * a.lanes if name == "float_maps_per_lane" else 2) * W * H * 8
        entry.update(frames_pass(ctx, a.lanes, L, R, a.warmup, a.steps))
        tables[name] = [ctx.rectify_map_fixed(lane, side) for lane in (0, a.lanes - 1) for side in range(2)]
        ctx.close()
        out[name] = entry
    out["tables_equal"] = bool(all((x[0] == y[0]).all() and (x[1] == y[1]).all() for x, y in zip(tables["float_maps_per_lane"], tables["calibration_shared"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
