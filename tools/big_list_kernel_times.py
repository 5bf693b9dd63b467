#!/usr/bin/env python3
"""Per-launch HIP-event times (svo_config.kernel_times) of one stream on lists above 8192 entries: FAST+ORB, one octave, no NMS, FAST
threshold 5 on the 2048x1536 synthetic street (14.4 k keypoints per image, 9.3 k row-by-row pairings, brute-force tracker), once in a
context with max_kps 16384 and once with max_kps 8192, where the lists are cut at 8192 and status bit 2 is raised -- the nearest
figures the smaller instantiations can give for the same frames.  Prints one JSON line (profiles/r08_kernel_times_16384.json).
No speed is claimed for 16384-entry contexts; these are the baseline for the next change to their kernels."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from stereo_vo_amd import hip
from stereo_vo_amd.abi import DM_FAST_ORB
from stereo_vo_amd.synth import SyntheticStereoWorld

W, H = 2048, 1536


def params():
    p = hip.default_params()
    p.detect_method, p.nOctaves, p.non_maximal_suppression = DM_FAST_ORB, 1, 0
    p.initial_FAST_threshold, p.fast_min_th = 5, 1
    p.match_method, p.enable_robust_1to1_match, p.max_y_diff = 1, 0, 8.0
    p.orb_max_distance, p.orb_max_th = 120.0, 256
    p.ifm_method = 0
    return p


def run(max_kps, frames, cam, passes):
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=max_kps, max_cand=1 << 18, kernel_times=True)
    ctx.set_params(params()); ctx.set_camera(cam)
    for rep in range(passes + 1):                              # the first pass warms up
        ctx.reset()
        if rep == 1:
            ctx.kernel_times_reset()
        for f in frames:
            ctx.process_host([f])
            r = ctx.result(0)
    kt = ctx.kernel_times()
    out = {"us_per_launch": {k: round(1e3 * v[0] / v[1], 1) for k, v in kt.items() if v[1]}, "launches": {k: v[1] for k, v in kt.items() if v[1]},
           "last_frame": {"keypoints_left": r.detected_left[0], "pairings": r.stereo_matches[0], "track_stats": [int(v) for v in r.track_stats],
                          "tracked": r.tracked_feats_from_last_frame, "valid": int(r.valid), "status": r.status}}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3, help="timed passes over the three frames")
    a = ap.parse_args()
    w = SyntheticStereoWorld(W, H, 1280.0, 0.12, seed=51, n_frames=3)
    frames = [tuple(np.ascontiguousarray(x.numpy()) for x in w.render(t)) for t in range(3)]
    out = {"shape": "%dx%d, one stream, FAST+ORB x 1 octave, no NMS, FAST threshold 5, RbR pairing (max_y_diff 8, no 1-to-1), BF tracker; %d timed passes over 3 frames" % (W, H, a.passes),
           "max_kps 16384": run(16384, frames, w.camera(), a.passes), "max_kps 8192 (lists cut at 8192, status bit 2)": run(8192, frames, w.camera(), a.passes)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
