#!/usr/bin/env python3
"""HIP-event time of the window gather of svo_gather_windows (k_sad_patch_slot, "gather_windows") beside stage 2's own gather
(k_sad_patch, "sad_patch") on THE SAME lists and images: one context of `lanes` streams at 1280x960 under dmFASTER + smSAD on three
octaves, svo_config.kernel_times on.  Each timed step detects a frame (sad_patch gathers the windows of the lists it has just made)
and then hands the same images to svo_gather_windows for those lists (gather_windows gathers them again): same grid, same body.
Three alternating runs per lane count give the spread.  Writes one JSON record (profiles/put_windows_times.json).
No threshold hangs on these figures: the yardstick of the new launch is sad_patch itself."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import DM_FASTER, SM_SAD, IFM_SAD
from stereo_vo_amd.synth import SyntheticStereoWorld


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "put_windows_times.json"))
    a = ap.parse_args()
    W, H = 1280, 960
    dev = torch.device("cuda", 0)
    p = hip.default_params()
    p.detect_method, p.match_method, p.ifm_method, p.nOctaves = DM_FASTER, SM_SAD, IFM_SAD, 3
    p.orb_nfeats, p.initial_FAST_threshold, p.non_maximal_suppression, p.nmsMethod, p.min_distance, p.max_y_diff = a.orb_nfeats, 20, 1, 0, 3, 2.0
    out = {"shape": "%dx%d, dmFASTER + smSAD, three octaves, orb_nfeats %d, one context; %d runs of %d (detect, gather) steps" % (W, H, a.orb_nfeats, a.runs, a.steps),
           "us_per_launch": {}}
    for lanes in a.lanes:
        worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=2, device=dev, scene="street", noise_on_device=True) for g in range(lanes)]
        frames = [w.render(1) for w in worlds]
        torch.cuda.synchronize()
        ptrs = [(f[0].data_ptr(), f[1].data_ptr()) for f in frames]
        ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=4096, max_octaves=3, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(worlds[0].camera())
        ctx.process_device(ptrs, W, H, W, hip.RUN_DETECT | hip.RUN_MATCH)       # warm-up of both launches
        ctx.gather_windows_device(ptrs, W, H, W, which=0)
        ctx.wait()
        runs = []
        for _ in range(a.runs):
            ctx.kernel_times_reset()
            for _ in range(a.steps):
                ctx.process_device(ptrs, W, H, W, hip.RUN_DETECT | hip.RUN_MATCH)
                ctx.gather_windows_device(ptrs, W, H, W, which=0)
            kt = ctx.kernel_times(appended=True)
            assert kt["sad_patch"][1] == a.steps and kt["gather_windows"][1] == a.steps, (kt["sad_patch"], kt["gather_windows"])
            runs.append({k: round(1e3 * kt[k][0] / kt[k][1], 2) for k in ("sad_patch", "gather_windows")})
        res = ctx.results()
        out["us_per_launch"]["%d lanes" % lanes] = {"runs": runs, "mean_keypoints_left_per_octave": [round(sum(r.detected_left[o] for r in res) / lanes, 1) for o in range(3)]}
        ctx.close()
        del frames, worlds
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
