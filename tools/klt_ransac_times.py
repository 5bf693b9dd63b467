#!/usr/bin/env python3
"""What the RANSAC gate of the resident KLT front end (svo_klt_set_ransac) adds to a step: ONE context of `lanes` streams at 1280x960,
1024 tracks per lane from a 32 x 32 grid with ground-truth disparity, device images, default tracker parameters -- the shape of
tools/klt_times.py.

  modes      wall time per step of svo_klt_step(SVO_RUN_OPTIMIZE) in mode 0, 1 and 2 over the timed frames, one synchronisation at the end
             of a leg; every leg is a process of its own (one process has the GPU open at a time), `--reps` legs per mode, alternating
  parent     with --parent-lib: mode 0 of this tree against the same step of another libsvo_hip.so (the parent commit's, loaded through
             SVO_HIP_LIB), alternating in the same call, with the spread of each
  kernels    per step from svo_kernel_times, in legs of their own (events cost a few percent): the two new kernels, the RANSAC launches
             under their names of a frame, and the rest of the step
Prints one JSON line (profiles/klt_ransac_times.json).  No threshold hangs on these figures."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, CAP = 1280, 960, 1024
RANSAC_NAMES = ("ransac_feed", "ransac_hyp", "ransac_count", "ransac_hyp_1", "ransac_count_1", "ransac_hyp_2", "ransac_count_2", "track_finalize", "klt_prune")
STEP_NAMES = ("begin_frame", "lk_pyrdown", "lk_track", "klt_select", "gauss_newton")


def leg(a):
    """one leg in this process: a JSON line with the step time (or the kernel times) of one mode"""
    import numpy as np
    import torch
    from stereo_vo_amd import hip
    from stereo_vo_amd.abi import north_star_params
    from stereo_vo_amd.synth import SyntheticStereoWorld
    import klt_scenes as KS
    dev = torch.device("cuda", 0)
    nf = a.warmup + a.steps + 1                            # the last frame is stepped untimed and without stage 5: the gate's counters stand
    worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=nf, device=dev, noise_on_device=True) for g in range(a.worlds)]
    rendered = [[w.render(t) for t in range(nf)] for w in worlds]
    torch.cuda.synchronize()

    def grid_points(world):
        xs = np.linspace(40.0, W - 41.0, 32); ys = np.linspace(40.0, H - 41.0, 32)
        left = np.array([(x, y) for y in ys for x in xs], np.float32)
        right = left.copy()
        right[:, 0] = (left[:, 0] - world.f * world.B / KS.gt_depth(world, 0, left)).astype(np.float32)
        return left, right
    wpts = [grid_points(w) for w in worlds]

    def frames_of(t):
        return [tuple((im.data_ptr(), W, H, W) for im in rendered[g % a.worlds][t]) for g in range(a.lanes)]
    c = hip.Context(n_lanes=a.lanes, max_w=W, max_h=H, max_kps=CAP, max_cand=1 << 15, kernel_times=bool(a.kernel_times))
    c.set_params(north_star_params(hip.default_params(), orb_nfeats=600))      # (the detector is never run; its list capacity must fit max_kps)
    c.set_camera(worlds[0].camera())
    kp = hip.default_klt_params()
    kp.cap = CAP
    c.klt_enable(kp)
    if a.mode:                                             # (mode 0 never calls the setter: a library without it runs the same leg)
        c.klt_set_ransac(a.mode)
    for g in range(a.lanes):
        assert c.klt_add_points(g, *wpts[g % a.worlds]) == CAP
    for t in range(a.warmup):
        c.klt_step(frames_of(t), device=True)
    c.wait()
    if a.kernel_times:
        c.kernel_times_reset()
    t0 = time.perf_counter()
    for t in range(a.warmup, nf - 1):
        c.klt_step(frames_of(t), device=True)
    c.wait()
    ms = 1e3 * (time.perf_counter() - t0) / a.steps
    valid = sum(int(r.valid) for r in c.results())
    kt = c.kernel_times(appended=True) if a.kernel_times else None
    c.klt_step(frames_of(nf - 1), flags=0, device=True)
    res = c.results()
    live = [len(c.klt_tracks(g)[2]) for g in range(a.lanes)]
    out = {"mode": a.mode, "ms_per_step": round(ms, 4), "lanes_valid_last_timed_frame": valid,
           "live_tracks_after": {"min": min(live), "mean": round(sum(live) / len(live), 1), "max": max(live)},
           "candidates_mean": round(sum(r.track_stats[1] for r in res) / len(res), 1),
           "survivors_mean": round(sum(r.track_stats[7] for r in res) / len(res), 1),
           "hypotheses_left_mean": round(sum(r.track_stats[4] for r in res) / len(res), 1)}
    if a.kernel_times:
        out["kernel_us_per_step"] = {k: round(1e3 * kt[k][0] / a.steps, 2) for k in STEP_NAMES + RANSAC_NAMES if k in kt}
    c.close()
    print("LEG " + json.dumps(out))


def run_leg(a, mode, lib=None, kernel_times=False):
    env = dict(os.environ)
    if lib:
        env["SVO_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--mode", str(mode), "--lanes", str(a.lanes), "--worlds", str(a.worlds),
           "--warmup", str(a.warmup), "--steps", str(a.steps)] + (["--kernel-times"] if kernel_times else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.leg_timeout)
    if p.returncode != 0:                                  # a leg that failed ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("leg mode %d (%s) ended with %d" % (mode, lib or "this tree", p.returncode))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")][-1]
    sys.stderr.write("leg mode %d%s%s: %s\n" % (mode, " (other library)" if lib else "", " with kernel times" if kernel_times else "", line[4:])); sys.stderr.flush()
    return json.loads(line[4:])


def spread(v):
    v = sorted(v)
    return {"runs": v, "median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=96)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="another libsvo_hip.so whose mode-0 step is timed beside this tree's")
    ap.add_argument("--leg", action="store_true", help="(internal) run one leg in this process")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--kernel-times", action="store_true")
    ap.add_argument("--leg-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    ms = {0: [], 1: [], 2: []}
    parent, info = [], {}
    for _ in range(a.reps):
        if a.parent_lib:
            parent.append(run_leg(a, 0, a.parent_lib)["ms_per_step"])
        for mode in (0, 1, 2):
            r = run_leg(a, mode)
            ms[mode].append(r["ms_per_step"]); info[mode] = r
    kernels = {m: run_leg(a, m, kernel_times=True)["kernel_us_per_step"] for m in (0, 1, 2)}
    out = {"shape": "%d lanes of %dx%d in one context, %d tracks per lane at the start, default tracker parameters (win 21, 4 levels), device images, "
                    "%d warm-up + %d timed frames, %d rendered trajectories shared by the lanes; %d legs per mode, a process each, alternating"
                    % (a.lanes, W, H, CAP, a.warmup, a.steps, a.worlds, a.reps),
           "ms_per_step": {"mode_%d" % m: spread(ms[m]) for m in (0, 1, 2)},
           "mode_0_against_parent": ({"parent_library": spread(parent), "this_tree": spread(ms[0])} if parent else None),
           "last_leg": {"mode_%d" % m: {k: v for k, v in info[m].items() if k not in ("mode", "ms_per_step")} for m in (0, 1, 2)},
           "kernel_us_per_step": {"mode_%d" % m: kernels[m] for m in (0, 1, 2)}}
    for m in (1, 2):
        k = kernels[m]
        new = sum(k.get(n, 0.0) for n in ("ransac_feed", "klt_prune"))
        gate = sum(k.get(n, 0.0) for n in RANSAC_NAMES)
        out["kernel_us_per_step"]["mode_%d_gate_total" % m] = round(gate, 2)
        out["kernel_us_per_step"]["mode_%d_new_kernels" % m] = round(new, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
