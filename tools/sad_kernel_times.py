#!/usr/bin/env python3
"""Per-launch HIP-event times of the SAD kernels (k_sad_patch, k_match_lr_rbr<true>, k_track_win<true>) beside the Hamming forms of
the same loops (k_match_lr_rbr<false>, k_track_win<false>) from the same run: ONE context of `lanes` streams at 1280x960, every
lane its own trajectory through one synthetic street, svo_config.kernel_times on.  Prints one JSON line (profiles/sad_kernel_times.json).
No threshold hangs on these figures: they are the baseline for the next change to these kernels."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params
from stereo_vo_amd.synth import SyntheticStereoWorld


def run(lanes, W, H, nfe, frames, cam, match_method, ifm_method, sad, warm, timed):
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.match_method, p.ifm_method, p.max_y_diff = match_method, ifm_method, 2.0
    p.sad_max_distance = p.ifm_sad_max_distance = sad
    ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=4096, kernel_times=True)
    ctx.set_params(p); ctx.set_camera(cam)

    def step(t):
        ctx.process_device([(frames[g][t][0].data_ptr(), frames[g][t][1].data_ptr()) for g in range(lanes)], W, H, W)
    for t in range(warm):
        step(t)
    ctx.wait(); ctx.kernel_times_reset()
    for t in range(warm, warm + timed):
        step(t)
    kt = ctx.kernel_times()
    res = ctx.results()
    out = {"us_per_launch": {k: round(1e3 * v[0] / v[1], 2) for k, v in kt.items() if v[1]},
           "launches": {k: v[1] for k, v in kt.items() if v[1]},
           "mean_keypoints_left": round(sum(r.detected_left[0] for r in res) / lanes, 1),
           "mean_pairings": round(sum(r.stereo_matches[0] for r in res) / lanes, 1),
           "mean_candidates": round(sum(r.track_stats[1] for r in res) / lanes, 1),
           "mean_tracked": round(sum(r.tracked_feats_from_last_frame for r in res) / lanes, 1),
           "valid": sum(int(r.valid) for r in res)}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--sad", type=int, default=800, help="sad_max_distance of both groups")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    W, H = 1280, 960
    dev = torch.device("cuda", 0)
    nf = a.warmup + a.steps
    out = {"shape": "%dx%d, one context, orb_nfeats %d, max_y_diff 2, windows 16/16, sad_max_distance %d (both groups), %d timed frames" % (W, H, a.orb_nfeats, a.sad, a.steps), "runs": {}}
    for lanes in a.lanes:
        worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=nf, device=dev, scene="street", noise_on_device=True) for g in range(lanes)]
        frames = [[w.render(t) for t in range(nf)] for w in worlds]
        torch.cuda.synchronize()
        cam = worlds[0].camera()
        out["runs"]["%d lanes" % lanes] = {
            "hamming (match_method 1 = k_match_lr_rbr<false> under match_lr_filter, ifm_method 1 = k_track_win<false> under track_filter)":
                run(lanes, W, H, a.orb_nfeats, frames, cam, 1, 1, a.sad, a.warmup, a.steps),
            "sad (match_method 2 = match_lr_sad, ifm_method 2 = track_sad, sad_patch)":
                run(lanes, W, H, a.orb_nfeats, frames, cam, 2, 2, a.sad, a.warmup, a.steps)}
        del frames, worlds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
