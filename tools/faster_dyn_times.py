#!/usr/bin/env python3
"""What dmFASTER's dynamic threshold costs: HIP-event times of `faster` (k_faster: one launch with the feature off, two k_faster_dyn
launches -- left images, then right images -- with it on) and `faster_nms` per step, feature OFF and ON ALTERNATED in one job on ONE
context: `rounds` x (`block` steps off, `block` steps on), 40 steps of each by default, the first step after every switch left out
(it is the one that meets a cold instruction cache).  ONE context of `lanes` streams at 1280x960 on three x1/2 octaves, every lane
its own trajectory through one synthetic street, svo_config.kernel_times on, detection only (stage 2 is all the feature touches).

EVERY step starts from svo_reset, on both sides, so that an ON step detects its left images at the initial threshold 20 -- the threshold of
the OFF side -- and its right images at most one step away from it (19, 20 or 21: the target is the density lane 0 measures at 20;
what lane 0 used is printed): the corner load of the two sides is the same to within that step.  Without the reset the thresholds of an
ON block drift -- the octaves differ in density, so no single target holds them all -- and the two sides would time different images.

A library of another commit, loaded through SVO_HIP_LIB, has no svo_set_dyn_fast_threshold: the tool then times the off side only,
in the same alternation ("off_a" / "off_b" blocks), which gives that commit's own spread.  Prints one JSON line
(profiles/faster_dyn_times.json holds the runs).  No threshold hangs on these figures."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, DM_FASTER
from stereo_vo_amd.synth import SyntheticStereoWorld

N_OCT, W, H = 3, 1280, 960
NAMES = ("faster", "faster_nms")


def summary(v):
    v = sorted(v)
    return {"n": len(v), "median_us": round(statistics.median(v), 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2),
            "p10_us": round(v[len(v) // 10], 2), "p90_us": round(v[(9 * len(v)) // 10], 2)}


def run(lanes, nfe, n_frames, rounds, block, dev):
    worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=n_frames, device=dev, scene="street", noise_on_device=True) for g in range(lanes)]
    frames = [[w.render(t) for t in range(n_frames)] for w in worlds]
    torch.cuda.synchronize()
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.detect_method, p.nOctaves, p.max_y_diff, p.match_method, p.ifm_method = DM_FASTER, N_OCT, 2.0, 2, 2
    ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=4096, max_cand=1 << 18, max_octaves=N_OCT, kernel_times=True)
    ctx.set_params(p); ctx.set_camera(worlds[0].camera())
    has_dyn = hasattr(ctx.L, "svo_set_dyn_fast_threshold")
    step_no = [0]

    def step():
        t = step_no[0] % n_frames
        step_no[0] += 1
        ctx.reset()
        ctx.kernel_times_reset()
        ctx.process_device([(frames[g][t][0].data_ptr(), frames[g][t][1].data_ptr()) for g in range(lanes)], W, H, W, hip.RUN_DETECT)
        ctx.wait()
        kt = ctx.kernel_times()
        return {k: 1e3 * kt[k][0] for k in NAMES}, {k: kt[k][1] for k in NAMES}

    for _ in range(3):
        step()
    target = None
    if has_dyn:                                                 # the density at threshold 20: what keeps the thresholds near 20
        ctx.set_dyn_fast_threshold(True, 1.0)
        step()
        s = ctx.faster_stats(0)
        target = s.corners_left[0] / float(W * H)
        ctx.set_dyn_fast_threshold(False, target)
    sides = ("off", "on") if has_dyn else ("off_a", "off_b")
    times = {s: {k: [] for k in NAMES} for s in sides}
    launches = {}
    for r in range(rounds):
        for side in sides:
            if has_dyn:
                ctx.set_dyn_fast_threshold(side == "on", target)
            for i in range(block + 1):
                us, calls = step()
                if i:                                           # the first step after a switch is left out
                    for k in NAMES:
                        times[side][k].append(us[k])
                    launches[side] = calls
    out = {"spans_per_step": launches, "target_feats_per_pixel": target,
           "us_per_step": {s: {k: summary(times[s][k]) for k in NAMES} for s in sides}}
    if has_dyn:
        ctx.set_dyn_fast_threshold(True, target)
        step()
        st = ctx.faster_stats(0)
        out["lane0_last_on_step"] = {"used_left": list(st.used_left)[:N_OCT], "used_right": list(st.used_right)[:N_OCT], "next": list(st.next)[:N_OCT]}
        out["median_on_minus_off_us"] = {k: round(out["us_per_step"]["on"][k]["median_us"] - out["us_per_step"]["off"][k]["median_us"], 2) for k in NAMES}
    ctx.close()
    del frames, worlds
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, nargs="+", default=[96, 1])
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--frames", type=int, default=6, help="distinct frames per lane, cycled")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--block", type=int, default=10, help="timed steps per side and round (rounds x block = 40 per side)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    out = {"library": os.environ.get("SVO_HIP_LIB", "this tree"),
           "shape": "%dx%d, one context, %d octaves, orb_nfeats %d, grid NMS, initial FAST threshold 20, KLT_win 4, max_cand 2^18, detection only; %d rounds x %d timed steps per side"
                    % (W, H, N_OCT, a.orb_nfeats, a.rounds, a.block), "runs": {}}
    for lanes in a.lanes:
        out["runs"]["%d lanes" % lanes] = run(lanes, a.orb_nfeats, a.frames, a.rounds, a.block, dev)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
