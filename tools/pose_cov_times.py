#!/usr/bin/env python3
"""What the covariance of every pose increment costs (svo_set_pose_covariance): the time of k_pose_covariance beside k_gauss_newton's,
both from the context's own kernel_times (HIP events around each launch), in one call.  One JSON line, also written to
profiles/pose_cov_times.json:

  lanes96   one 96-lane context, 1280x960, north-star parameters, device-resident frames (the benchmark's shape: ~380 tracked pairs
            per lane): ms per step of "gauss_newton" and "pose_covariance", the feature off and on, and the mean iteration count
  lane1     one lane, 1025 tracked pairs through svo_change_in_pose (the first list size whose mask lives in global scratch)

The expectation to read the figure against: about ONE Gauss-Newton iteration -- the kernel is one more pass of the per-track loop and
one 6 x 6 factorisation, where k_gauss_newton runs its set-up (gather, NMS mask, triangulation) and some ten iterations.
gn_ms_per_iteration = gauss_newton ms / iterations overstates an iteration by the set-up's share.  An expectation, not a gate: no
threshold hangs on these figures."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params
from stereo_vo_amd.synth import SyntheticStereoWorld

W, H, LANES = 1280, 960, 96


def ping_pong(step, F):
    period = 2 * (F - 1); k = step % period
    return k if k < F else period - k


def per_step(ctx, steps):
    kt = ctx.kernel_times(appended=True)
    return {k: round(kt[k][0] / steps, 5) for k in ("gauss_newton", "pose_covariance") if k in kt and kt[k][1]}          # "pose_covariance" is listed only while the feature is on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--orb-nfeats", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_cov_times.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=100 + s, n_frames=a.frames, device=dev, scene_seed=s % 4) for s in range(a.worlds)]
    imgs = [[w.render(t) for t in range(a.frames)] for w in worlds]
    torch.cuda.synchronize()
    cam = worlds[0].camera()
    p = north_star_params(hip.default_params(), orb_nfeats=a.orb_nfeats)
    tb = []
    for t in range(a.frames):
        fr = (hip.Frame * LANES)()
        for l in range(LANES):
            L, R = imgs[l % a.worlds][t]
            fr[l].left = hip.Image(L.data_ptr(), W, H, W); fr[l].right = hip.Image(R.data_ptr(), W, H, W)
        tb.append(fr)
    out = {"shape": "lanes96: one context of %d lanes, %dx%d, north-star ORB + brute force, orb_nfeats %d, max_kps 4096, device frames, %d timed steps after %d; "
                    "lane1: svo_change_in_pose on 1025 tracked pairs (0.3 px noise, 10 %% outliers), max_kps 2048, %d timed calls" % (LANES, W, H, a.orb_nfeats, a.steps, a.warmup, a.steps),
           "expectation": "pose_covariance costs about one Gauss-Newton iteration"}
    out["lanes96"] = {}
    for on in (False, True):
        ctx = hip.Context(n_lanes=LANES, max_w=W, max_h=H, max_kps=4096, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam); ctx.set_pose_covariance(on)
        for i in range(a.warmup):
            ctx._process(tb[ping_pong(i, a.frames)], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, None)
        ctx.wait(); ctx.kernel_times_reset()
        iters = []
        for i in range(a.steps):
            ctx._process(tb[ping_pong(a.warmup + i, a.frames)], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, None)
            if i % 10 == 0: iters += [r.num_it + r.num_it_final for r in ctx.results() if r.valid]
        ctx.wait()
        res = ctx.results()
        e = per_step(ctx, a.steps)
        e["tracked_per_lane"] = round(float(np.mean([r.tracked_feats_from_last_frame for r in res])), 1)
        e["iterations"] = round(float(np.mean(iters)), 2) if iters else 0
        e["gn_ms_per_iteration"] = round(e["gauss_newton"] / max(e["iterations"], 1), 5)
        if on: e["states"] = sorted(set(c.state for c in ctx.pose_covariances()))
        out["lanes96"]["on" if on else "off"] = e
        ctx.close()
    import stage5_ref as S
    lists = S.permuted(S.camera(), S.BASE_TRUE, 1025, seed=22, noise=0.3, n_out=102)
    out["lane1"] = {}
    for on in (False, True):
        ctx = hip.Context(n_lanes=1, max_w=S.W, max_h=S.H, max_kps=2048, max_cand=1 << 15, kernel_times=True)
        ctx.set_params(north_star_params(hip.default_params(), orb_nfeats=40)); ctx.set_pose_covariance(on)
        for i in range(a.warmup): ctx.change_in_pose(*lists, S.camera())
        ctx.kernel_times_reset()
        for i in range(a.steps): v, r, _, _ = ctx.change_in_pose(*lists, S.camera())
        e = per_step(ctx, a.steps)
        e["iterations"] = r.num_it + r.num_it_final
        e["gn_ms_per_iteration"] = round(e["gauss_newton"] / max(e["iterations"], 1), 5)
        if on: e["state"] = ctx.pose_covariance(0).state
        out["lane1"]["on" if on else "off"] = e
        ctx.close()
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f: f.write(line + "\n")


if __name__ == "__main__":
    main()
