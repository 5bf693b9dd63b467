#!/usr/bin/env python3
"""What the landmark records cost (svo_set_landmarks), and what they cost everyone who leaves them off.  One JSON line, also written
to profiles/landmarks_times.json:

  kernel    one 96-lane context, 1280x960, north-star parameters, device-resident frames of the benchmark's scene (a few hundred
            tracked pairs per lane): ms per step of "landmarks" beside "gauss_newton" and "pose_covariance", from the context's own
            kernel_times (HIP events around each launch), with the pose covariance off and on
  step      the same context without kernel_times: the wall clock around --steps enqueued steps and the wait behind them, the feature
            off and on, alternating, --rounds times each (ms per step; min and all values)
  bench     with --parent-lib: `bench.py --gpus 1 --steps K --warmup W` (the plain run, the feature off) as a child process per run,
            this tree's library and the parent commit's (SVO_HIP_LIB) alternating, --bench-runs each.  The criterion for "off costs
            nothing": this tree's mean within the spread of the parent's own runs.

No time is fixed anywhere.  The expectation from arithmetic, to read the figures against: about 400 tracked pairs x 176 bytes x 96 lanes
is some 7 MB per step against about 3.5 GB of step traffic, and one launch of a few microseconds behind stage 5 on each context's own
stream."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, LMK_OK
from stereo_vo_amd.synth import SyntheticStereoWorld

W, H, LANES = 1280, 960, 96


def ping_pong(step, F):
    period = 2 * (F - 1); k = step % period
    return k if k < F else period - k


def bench_value(lib, steps, warmup):
    env = dict(os.environ)
    if lib: env["SVO_HIP_LIB"] = lib
    else: env.pop("SVO_HIP_LIB", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)],
                         env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0: raise RuntimeError("bench.py failed: " + out.stderr[-2000:])
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    return float(json.loads(line)["value"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--orb-nfeats", type=int, default=2000)
    ap.add_argument("--parent-lib", default="", help="libsvo_hip.so built from the parent commit: adds the `bench` leg")
    ap.add_argument("--bench-runs", type=int, default=2)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "landmarks_times.json"))
    a = ap.parse_args()
    out = {"shape": "one context of %d lanes, %dx%d, north-star ORB + brute force, orb_nfeats %d, max_kps 4096, device frames of the benchmark's scene, %d timed steps after %d"
                    % (LANES, W, H, a.orb_nfeats, a.steps, a.warmup),
           "expectation": "unmeasured arithmetic: ~400 pairings x 176 B x 96 lanes = ~7 MB per step against ~3.5 GB of step traffic; one launch of a few microseconds"}
    if a.parent_lib:      # first, before this process opens the GPU: every run is a process of its own
        tree, parent = [], []
        for _ in range(a.bench_runs):
            parent.append(bench_value(a.parent_lib, a.bench_steps, a.warmup)); tree.append(bench_value("", a.bench_steps, a.warmup))
        spread = max(parent) - min(parent)
        out["bench"] = {"what": "bench.py --gpus 1 --steps %d --warmup %d (plain run, the landmarks off), the parent commit's libsvo_hip.so and this tree's alternating in one call, %d runs each" % (a.bench_steps, a.warmup, a.bench_runs),
                        "parent_pairs_per_s": parent, "tree_pairs_per_s": tree, "parent_mean": round(float(np.mean(parent)), 1), "tree_mean": round(float(np.mean(tree)), 1),
                        "parent_spread": round(spread, 1), "difference_of_means": round(float(np.mean(tree) - np.mean(parent)), 1),
                        "within_parent_spread": bool(abs(np.mean(tree) - np.mean(parent)) <= spread)}
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
    run = lambda ctx, i: ctx._process(tb[ping_pong(i, a.frames)], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, None)
    out["kernel"] = {}
    for cov in (False, True):
        ctx = hip.Context(n_lanes=LANES, max_w=W, max_h=H, max_kps=4096, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam); ctx.set_pose_covariance(cov); ctx.set_landmarks(True)
        for i in range(a.warmup): run(ctx, i)
        ctx.wait(); ctx.kernel_times_reset()
        for i in range(a.steps): run(ctx, a.warmup + i)
        ctx.wait()
        kt = ctx.kernel_times(appended=True)
        e = {k: round(kt[k][0] / a.steps, 5) for k in ("gauss_newton", "pose_covariance", "landmarks") if k in kt and kt[k][1]}
        infos = [ctx.landmarks_info(l) for l in range(LANES)]
        e["records_per_lane"] = round(float(np.mean([i.n for i in infos])), 1)
        e["inliers_per_lane"] = round(float(np.mean([i.n_inliers for i in infos])), 1)
        e["lanes_ok"] = int(sum(i.state == LMK_OK for i in infos))
        e["record_bytes_per_step"] = int(sum(i.n for i in infos)) * 176
        out["kernel"]["pose_cov_on" if cov else "pose_cov_off"] = e
        ctx.close()
    ctx = hip.Context(n_lanes=LANES, max_w=W, max_h=H, max_kps=4096)
    ctx.set_params(p); ctx.set_camera(cam)
    times = {"off": [], "on": []}
    for rnd in range(a.rounds):
        for on in (False, True):
            ctx.set_landmarks(on)
            for i in range(a.warmup): run(ctx, i)
            ctx.wait()
            t0 = time.perf_counter()
            for i in range(a.steps): run(ctx, a.warmup + i)
            ctx.wait()
            times["on" if on else "off"].append(round((time.perf_counter() - t0) * 1e3 / a.steps, 4))
    ctx.close()
    out["step"] = {"what": "ms per step of the whole frame on one 96-lane context (wall clock around %d enqueued steps and the wait), the feature off and on alternating, %d rounds" % (a.steps, a.rounds),
                   "off_ms": times["off"], "on_ms": times["on"], "off_min": min(times["off"]), "on_min": min(times["on"])}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f: f.write(line + "\n")


if __name__ == "__main__":
    main()
