#!/usr/bin/env python3
"""Per-launch HIP-event times of the dmFASTER kernels (k_faster under `faster`, k_faster_nms under `faster_nms`) beside those of `fast`,
`select` and `describe` from a FAST+ORB run on the same frames (`select` there is k_fastorb_nms: it and k_faster_nms are the two
instantiations of chunked_grid_nms in k_detect.hip, over 32-bit and 64-bit keys): ONE context of `lanes` streams at 1280x960 on three x1/2 octaves,
every lane its own trajectory through one synthetic street, svo_config.kernel_times on.  Both runs share `resize` (k_half) and
`nms_rowsort`.  Prints one JSON line (profiles/faster_kernel_times.json).  No threshold hangs on these figures: they are the
baseline for the next change to these kernels."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, DM_FAST_ORB, DM_FASTER
from stereo_vo_amd.synth import SyntheticStereoWorld

N_OCT = 3


def run(lanes, W, H, nfe, frames, cam, faster, sad, warm, timed):
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.detect_method, p.nOctaves, p.max_y_diff = (DM_FASTER if faster else DM_FAST_ORB), N_OCT, 2.0
    if faster:                                                  # no descriptors: the SAD stages
        p.match_method, p.ifm_method = 2, 2
        p.sad_max_distance = p.ifm_sad_max_distance = sad
    ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=4096, max_cand=1 << 18, max_octaves=N_OCT, kernel_times=True)
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
           "mean_keypoints_left": [round(sum(r.detected_left[o] for r in res) / lanes, 1) for o in range(N_OCT)],
           "mean_pairings": [round(sum(r.stereo_matches[o] for r in res) / lanes, 1) for o in range(N_OCT)],
           "mean_tracked": round(sum(r.tracked_feats_from_last_frame for r in res) / lanes, 1),
           "valid": sum(int(r.valid) for r in res),
           "status_bits": sorted(set(int(r.status) for r in res))}
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--sad", type=int, default=800, help="sad_max_distance of both groups (dmFASTER run)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    W, H = 1280, 960
    dev = torch.device("cuda", 0)
    nf = a.warmup + a.steps
    out = {"shape": "%dx%d, one context, %d octaves, orb_nfeats %d, grid NMS, FAST threshold 20, KLT_win 4, max_cand 2^18, %d timed frames" % (W, H, N_OCT, a.orb_nfeats, a.steps), "runs": {}}
    for lanes in a.lanes:
        worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=nf, device=dev, scene="street", noise_on_device=True) for g in range(lanes)]
        frames = [[w.render(t) for t in range(nf)] for w in worlds]
        torch.cuda.synchronize()
        cam = worlds[0].camera()
        out["runs"]["%d lanes" % lanes] = {
            "fast_orb (detect_method 1: fast, select = k_fastorb_nms, describe; brute-force Hamming stages)": run(lanes, W, H, a.orb_nfeats, frames, cam, False, a.sad, a.warmup, a.steps),
            "faster (detect_method 2: faster, faster_nms; smSAD + ifmSAD)": run(lanes, W, H, a.orb_nfeats, frames, cam, True, a.sad, a.warmup, a.steps)}
        del frames, worlds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
