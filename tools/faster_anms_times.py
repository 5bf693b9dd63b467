#!/usr/bin/env python3
"""Per-launch HIP-event times of dmFASTER's selection kernel (`faster_nms` in svo_kernel_times) with the grid NMS (k_faster_nms) and with
the adaptive NMS (k_faster_anms, svo_set_faster_adaptive_nms) on the same frames: ONE context of `lanes` streams at 1280x960 on three
x1/2 octaves, every lane its own trajectory through one synthetic street, svo_config.kernel_times on.  Then one DENSE frame in a
one-lane context: lightly smoothed noise at the lowest FAST threshold whose level-0 candidate list still fits max_cand = 2^17.

Beside each time: N, the level-0 corner count of lane 0's left image (read through the statistics of svo_set_dyn_fast_threshold in a
context of its own, at the same threshold), and what a brute-force scan of every prefix would have cost, N * mean L, with
L(i) = min(i, #{ j : r_i < 0.9 r_j }) computed on the host from the corner responses of tests/faster_ref.py.  The point of the table:
the dense frame has about 12 x the corners of the street frame and about 100 x its N * mean L; the kernel's time must follow the first,
not the second (DESIGN.md section 4 quotes the figures).
Prints one JSON line (profiles/faster_anms_times.json).  No threshold hangs on these figures."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, DM_FASTER
from stereo_vo_amd.synth import SyntheticStereoWorld

N_OCT, W, H, MAX_CAND = 3, 1280, 960, 1 << 17


def params(nfe, t, adaptive, sad=800):
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.detect_method, p.nOctaves, p.max_y_diff, p.initial_FAST_threshold = DM_FASTER, N_OCT, 2.0, t
    p.match_method, p.ifm_method = 2, 2
    p.sad_max_distance = p.ifm_sad_max_distance = sad
    p.non_maximal_suppression, p.nmsMethod = 1, (1 if adaptive else 0)
    return p


def run(lanes, frames, cam, p, adaptive, warm, timed, flags=hip.RUN_ALL):
    ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=4096, max_cand=MAX_CAND, max_octaves=N_OCT, kernel_times=True)
    ctx.set_params(p); ctx.set_camera(cam)
    ctx.set_faster_adaptive_nms(adaptive)

    def step(t):
        ctx.process_device([(frames[g][t][0].data_ptr(), frames[g][t][1].data_ptr()) for g in range(lanes)], W, H, W, flags)
    for t in range(warm):
        step(t)
    ctx.wait(); ctx.kernel_times_reset()
    for t in range(warm, warm + timed):
        step(t)
    kt = ctx.kernel_times()
    res = ctx.results()
    out = {"us_per_launch": {k: round(1e3 * kt[k][0] / kt[k][1], 2) for k in ("faster", "faster_nms", "nms_rowsort") if kt[k][1]},
           "launches": kt["faster_nms"][1],
           "mean_keypoints_left": [round(sum(r.detected_left[o] for r in res) / lanes, 1) for o in range(N_OCT)],
           "status_bits": sorted(set(int(r.status) for r in res))}
    ctx.close()
    return out


def corner_counts(frame, cam, p):
    """level-0 .. level-2 corner counts of one left image at p.initial_FAST_threshold"""
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=4096, max_cand=MAX_CAND, max_octaves=N_OCT)
    ctx.set_params(p); ctx.set_camera(cam)
    ctx.set_dyn_fast_threshold(True, 0.01)
    ctx.process_device([(frame[0].data_ptr(), frame[1].data_ptr())], W, H, W, hip.RUN_DETECT)
    n = list(ctx.faster_stats(0).corners_left)[:N_OCT]
    ctx.close()
    return n


def brute_force(img, t):
    """(N, mean L, N * mean L) of a level-0 image: what scanning every prefix would cost"""
    import faster_ref as F
    r = np.sort(F.corners(img, t, 4)["response"].astype(np.float64))[::-1]
    n = len(r)
    if not n:
        return 0, 0.0, 0
    bigger = n - np.searchsorted((0.9 * r)[::-1], r, side="right")        # #{ j : 0.9 r_j > r_i }
    L = np.minimum(np.arange(n), bigger)
    return n, round(float(L.mean()), 1), int(L.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[1, 64])
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=6)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nf = a.warmup + a.steps
    out = {"shape": "%dx%d, one context, %d octaves, orb_nfeats %d, FAST threshold 20 (street), KLT_win 4, max_cand 2^17, %d timed frames; faster_nms = k_faster_nms (grid) or k_faster_anms (adaptive)" % (W, H, N_OCT, a.orb_nfeats, a.steps), "street": {}}
    for lanes in a.lanes:
        worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=nf, device=dev, scene="street", noise_on_device=True) for g in range(lanes)]
        frames = [[w.render(t) for t in range(nf)] for w in worlds]
        torch.cuda.synchronize()
        cam = worlds[0].camera()
        entry = {"grid": run(lanes, frames, cam, params(a.orb_nfeats, 20, False), False, a.warmup, a.steps),
                 "adaptive": run(lanes, frames, cam, params(a.orb_nfeats, 20, True), True, a.warmup, a.steps)}
        if lanes == a.lanes[0]:
            entry["corners_lane0_left_last_frame"] = corner_counts(frames[0][nf - 1], cam, params(a.orb_nfeats, 20, False))
            n, ml, tot = brute_force(frames[0][nf - 1][0].cpu().numpy(), 20)
            entry["level0_brute_force"] = {"N": n, "mean_L": ml, "N_x_mean_L": tot}
        out["street"]["%d lanes" % lanes] = entry
        del frames, worlds
    # the dense frame
    rng = np.random.default_rng(7)
    noise = rng.integers(0, 256, (H, W)).astype(np.uint16)
    img = ((noise + np.roll(noise, 1, axis=1)) // 2).astype(np.uint8)
    L = torch.from_numpy(img).to(dev); R = torch.from_numpy(np.roll(img, -6, axis=1).copy()).to(dev)
    cam = SyntheticStereoWorld(W, H, 800.0, 0.12, seed=0, scene_seed=0, n_frames=1, device=dev, scene="street", noise_on_device=True).camera()
    t_dense, counts = None, None
    for t in range(10, 80, 2):
        counts = corner_counts((L, R), cam, params(a.orb_nfeats, t, False))
        if counts[0] <= MAX_CAND:
            t_dense = t
            break
    frames = [[(L, R)] * nf]
    dense = {"fast_threshold": t_dense, "corners_left": counts,
             "grid": run(1, frames, cam, params(a.orb_nfeats, t_dense, False), False, a.warmup, a.steps, hip.RUN_DETECT),
             "adaptive": run(1, frames, cam, params(a.orb_nfeats, t_dense, True), True, a.warmup, a.steps, hip.RUN_DETECT)}
    n, ml, tot = brute_force(img, t_dense)
    dense["level0_brute_force"] = {"N": n, "mean_L": ml, "N_x_mean_L": tot}
    out["dense (smoothed noise, detect only, 1 lane)"] = dense
    print(json.dumps(out))


if __name__ == "__main__":
    main()
