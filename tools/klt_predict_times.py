#!/usr/bin/env python3
"""What the pose prediction of the resident KLT front end (svo_klt_set_prediction) costs and what a shallower pyramid under it buys:
ONE context of `lanes` streams at 1280x960, 1024 tracks per lane from a 32 x 32 grid with ground-truth disparity, device images -- the
shape of tools/klt_times.py and tools/klt_ransac_times.py.

  configurations   wall time per step of svo_klt_step(SVO_RUN_OPTIMIZE) over the timed frames, one synchronisation at the end of a leg:
                   mode 0 (and, with --parent-lib, mode 0 of another libsvo_hip.so -- the parent commit's, loaded through SVO_HIP_LIB),
                   mode 1 at the default max_level 3, mode 1 at max_level 1, and mode 0 at max_level 1 beside it.  Every leg is a
                   process of its own (one process has the GPU open at a time), `--reps` legs per configuration, alternating
  kernels          per step from svo_kernel_times, in legs of their own (events cost a few percent): klt_predict, lk_track and the
                   rest of the step
  survivors        live tracks per lane after the last frame, and the lanes whose last timed step ended valid
Prints one JSON line (profiles/klt_predict_times.json).  No threshold hangs on these figures."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, CAP = 1280, 960, 1024
STEP_NAMES = ("klt_predict", "begin_frame", "lk_pyrdown", "lk_track", "klt_select", "gauss_newton")
# name -> (mode, max_level); "parent" is mode_0 on the other library
CONFIGS = {"mode_0": (0, 3), "mode_1": (1, 3), "mode_1_level_1": (1, 1), "mode_0_level_1": (0, 1)}


def leg(a):
    """one leg in this process: a JSON line with the step time (or the kernel times) of one configuration"""
    import numpy as np
    import torch
    from stereo_vo_amd import hip
    from stereo_vo_amd.abi import north_star_params
    from stereo_vo_amd.synth import SyntheticStereoWorld
    import klt_scenes as KS
    dev = torch.device("cuda", 0)
    nf = a.warmup + a.steps
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
    kp.lk.max_level = a.max_level
    c.klt_enable(kp)
    if a.mode:                                             # (mode 0 never calls the setter: a library without it runs the same leg)
        c.klt_set_prediction(a.mode)
    for g in range(a.lanes):
        assert c.klt_add_points(g, *wpts[g % a.worlds]) == CAP
    for t in range(a.warmup):
        c.klt_step(frames_of(t), device=True)
    c.wait()
    if a.kernel_times:
        c.kernel_times_reset()
    t0 = time.perf_counter()
    for t in range(a.warmup, nf):
        c.klt_step(frames_of(t), device=True)
    c.wait()
    ms = 1e3 * (time.perf_counter() - t0) / a.steps
    valid = sum(int(r.valid) for r in c.results())
    kt = c.kernel_times(appended=True) if a.kernel_times else None
    live = [len(c.klt_tracks(g)[2]) for g in range(a.lanes)]
    out = {"mode": a.mode, "max_level": a.max_level, "ms_per_step": round(ms, 4), "lanes_valid_last_frame": valid,
           "survivors_per_lane_last_frame": {"min": min(live), "mean": round(sum(live) / len(live), 1), "max": max(live)}}
    if a.mode:
        used = [int(c.klt_predicted(g)[2].sum()) for g in range(a.lanes)]
        out["slots_the_next_step_would_predict"] = {"min": min(used), "mean": round(sum(used) / len(used), 1), "max": max(used)}
    if a.kernel_times:
        out["kernel_us_per_step"] = {k: round(1e3 * kt[k][0] / a.steps, 2) for k in STEP_NAMES if k in kt}
    c.close()
    print("LEG " + json.dumps(out))


def run_leg(a, name, lib=None, kernel_times=False):
    mode, level = CONFIGS[name]
    env = dict(os.environ)
    if lib:
        env["SVO_HIP_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--mode", str(mode), "--max-level", str(level), "--lanes", str(a.lanes), "--worlds", str(a.worlds),
           "--warmup", str(a.warmup), "--steps", str(a.steps)] + (["--kernel-times"] if kernel_times else [])
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.leg_timeout)
    if p.returncode != 0:                                  # a leg that failed ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("leg %s (%s) ended with %d" % (name, lib or "this tree", p.returncode))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")][-1]
    sys.stderr.write("leg %s%s%s: %s\n" % (name, " (other library)" if lib else "", " with kernel times" if kernel_times else "", line[4:])); sys.stderr.flush()
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
    ap.add_argument("--max-level", type=int, default=3)
    ap.add_argument("--kernel-times", action="store_true")
    ap.add_argument("--leg-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    ms = {name: [] for name in CONFIGS}
    parent, info = [], {}
    for _ in range(a.reps):
        if a.parent_lib:
            parent.append(run_leg(a, "mode_0", a.parent_lib)["ms_per_step"])
        for name in CONFIGS:
            r = run_leg(a, name)
            ms[name].append(r["ms_per_step"]); info[name] = r
    kernels = {name: run_leg(a, name, kernel_times=True)["kernel_us_per_step"] for name in CONFIGS}
    out = {"shape": "%d lanes of %dx%d in one context, %d tracks per lane at the start, default tracker parameters but max_level (win 21), device images, "
                    "%d warm-up + %d timed frames, %d rendered trajectories shared by the lanes; %d legs per configuration, a process each, alternating"
                    % (a.lanes, W, H, CAP, a.warmup, a.steps, a.worlds, a.reps),
           "configurations": {name: {"mode": m, "max_level": lv} for name, (m, lv) in CONFIGS.items()},
           "ms_per_step": {name: spread(ms[name]) for name in CONFIGS},
           "mode_0_against_parent": ({"parent_library": spread(parent), "this_tree": spread(ms["mode_0"])} if parent else None),
           "last_leg": {name: {k: v for k, v in info[name].items() if k not in ("mode", "max_level", "ms_per_step")} for name in CONFIGS},
           "kernel_us_per_step": kernels}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
