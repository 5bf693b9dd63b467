#!/usr/bin/env python3
"""What the stereo re-association of the resident KLT front end (svo_klt_set_stereo) costs: ONE context of `lanes` streams at 1280x960,
1024 tracks per lane from a 32 x 32 grid with ground-truth disparity, device images -- the shape of tools/klt_times.py and
tools/klt_predict_times.py.

  configurations   wall time per step of svo_klt_step(SVO_RUN_OPTIMIZE) over the timed frames, one synchronisation at the end of a leg:
                   mode 0 and mode 1, each with fb_max 0 and 0.5.  Mode 0 of the same tree is the baseline (the launch census shows it
                   is the parent's step).  Every leg is a process of its own (one process has the GPU open at a time), `--reps` legs per
                   configuration, alternating
  kernels          per step from svo_kernel_times, in legs of their own (events cost a few percent): lk_track, lk_track_row and the
                   rest of the step
  survivors        live tracks per lane after the last frame, and the lanes whose last timed step ended valid
Also, as information: the rotation / translation error of both modes against SyntheticStereoWorld.gt_delta on the 160x120 sequence of
tests/klt_scenes.py, as profiles/klt_times.json has it for mode 0.
Prints one JSON line (profiles/klt_stereo_times.json).  No threshold hangs on these figures.
  --photometric   every leg runs under svo_lk_set_photometric(ctx, 1); --configs a,b restricts the run to those configurations and
                  --no-accuracy leaves the 160x120 sequence out (profiles/lk_photo_times.json holds mode_0 and mode_1 both ways)."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, CAP = 1280, 960, 1024
STEP_NAMES = ("begin_frame", "lk_pyrdown", "lk_track", "lk_track_row", "klt_select", "gauss_newton")
# name -> (mode, fb_max)
CONFIGS = {"mode_0": (0, 0.0), "mode_1": (1, 0.0), "mode_0_fb": (0, 0.5), "mode_1_fb": (1, 0.5)}


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
    kp.lk.fb_max = a.fb_max
    if a.photometric:                                      # (the tracker's mode: before or after svo_klt_enable alike)
        c.lk_set_photometric(1)
    c.klt_enable(kp)
    if a.mode:                                             # (mode 0 never calls the setter)
        c.klt_set_stereo(a.mode)
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
    out = {"mode": a.mode, "fb_max": a.fb_max, "photometric": c.lk_get_photometric(), "ms_per_step": round(ms, 4), "lanes_valid_last_frame": valid,
           "survivors_per_lane_last_frame": {"min": min(live), "mean": round(sum(live) / len(live), 1), "max": max(live)}}
    if a.kernel_times:
        out["kernel_us_per_step"] = {k: round(1e3 * kt[k][0] / a.steps, 2) for k in STEP_NAMES if k in kt}
    c.close()
    print("LEG " + json.dumps(out))


def accuracy_leg(photometric=False):
    """both modes on the 160x120 sequence: per frame 1 .. 4 [valid, rotation error rad, translation error m, live tracks]"""
    from stereo_vo_amd import hip
    from stereo_vo_amd.abi import north_star_params
    from stereo_vo_amd.synth import pose6_to_matrix, pose_error
    import klt_scenes as KS
    world, frames = KS.sequence_world(), KS.sequence_frames()
    kp = hip.default_klt_params()
    kp.cap = KS.SEQ_CAP
    for k, v in KS.SEQ_LK.items():
        setattr(kp.lk, k, v)
    kp.max_dy, kp.min_disp, kp.max_disp = KS.SEQ_GATE["max_dy"], KS.SEQ_GATE["min_disp"], KS.SEQ_GATE["max_disp"]
    out = {}
    for mode in (0, 1):
        c = hip.Context(n_lanes=1, max_w=KS.W, max_h=KS.H, max_kps=512, max_cand=1 << 15)
        p = north_star_params(hip.default_params()); p.orb_nlevels, p.orb_nfeats = 2, 300      # (the detector is never run; its list capacity must fit max_kps)
        c.set_params(p); c.set_camera(world.camera())
        c.klt_enable(kp); c.klt_set_stereo(mode); c.klt_add_points(0, *KS.sequence_points())
        if photometric:
            c.lk_set_photometric(1)
        rows = []
        for t in range(KS.SEQ_FRAMES):
            c.klt_step([frames[t]])
            r = c.result(0)
            if t:
                er, et = pose_error(pose6_to_matrix(list(r.outPose)), world.gt_delta(t))
                rows.append([int(r.valid), round(er, 5), round(et, 4), len(c.klt_tracks(0)[2])])
        c.close()
        out["mode_%d" % mode] = rows
    print("LEG " + json.dumps(out))


def run_leg(a, name, kernel_times=False):
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--lanes", str(a.lanes), "--worlds", str(a.worlds), "--warmup", str(a.warmup), "--steps", str(a.steps)]
    if a.photometric:
        cmd.append("--photometric")
    if name == "accuracy":
        cmd.append("--accuracy")
    else:
        mode, fb = CONFIGS[name]
        cmd += ["--mode", str(mode), "--fb-max", str(fb)] + (["--kernel-times"] if kernel_times else [])
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
    if p.returncode != 0:                                  # a leg that failed ends the run: nothing more is started on the GPU
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit("leg %s ended with %d" % (name, p.returncode))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")][-1]
    sys.stderr.write("leg %s%s: %s\n" % (name, " with kernel times" if kernel_times else "", line[4:])); sys.stderr.flush()
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
    ap.add_argument("--leg", action="store_true", help="(internal) run one leg in this process")
    ap.add_argument("--accuracy", action="store_true", help="(internal) the leg is the 160x120 sequence in both modes")
    ap.add_argument("--mode", type=int, default=0)
    ap.add_argument("--fb-max", type=float, default=0.0)
    ap.add_argument("--kernel-times", action="store_true")
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--photometric", action="store_true", help="every leg under svo_lk_set_photometric(ctx, 1)")
    ap.add_argument("--configs", default=",".join(CONFIGS), help="the configurations to run, comma separated")
    ap.add_argument("--no-accuracy", action="store_true")
    a = ap.parse_args()
    if a.leg:
        return accuracy_leg(a.photometric) if a.accuracy else leg(a)
    configs = {name: CONFIGS[name] for name in a.configs.split(",")}
    ms = {name: [] for name in configs}
    info = {}
    for _ in range(a.reps):
        for name in configs:
            r = run_leg(a, name)
            ms[name].append(r["ms_per_step"]); info[name] = r
    kernels = {name: run_leg(a, name, kernel_times=True)["kernel_us_per_step"] for name in configs}
    acc = {} if a.no_accuracy else run_leg(a, "accuracy")
    out = {"shape": "%d lanes of %dx%d in one context, %d tracks per lane at the start, default tracker parameters but fb_max (win 21, 4 levels), device images, "
                    "%d warm-up + %d timed frames, %d rendered trajectories shared by the lanes; %d legs per configuration, a process each, alternating"
                    % (a.lanes, W, H, CAP, a.warmup, a.steps, a.worlds, a.reps),
           "photometric": int(a.photometric),
           "configurations": {name: {"mode": m, "fb_max": fb} for name, (m, fb) in configs.items()},
           "ms_per_step": {name: spread(ms[name]) for name in configs},
           "last_leg": {name: {k: v for k, v in info[name].items() if k not in ("mode", "fb_max", "ms_per_step")} for name in configs},
           "kernel_us_per_step": kernels,
           "accuracy_160x120": {"columns": "per frame 1..4: [valid, rotation error rad, translation error m, live tracks] against gt_delta", **acc}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
