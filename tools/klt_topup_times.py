#!/usr/bin/env python3
"""Time of the resident top-up of the KLT front end (svo_klt_topup) beside the host round trip it replaces (svo_klt_get_tracks,
svo_gftt_detect, svo_lk_track, svo_klt_add_points: four synchronising calls per lane), on the leg of tools/klt_times.py: ONE context
of `lanes` streams at 1280x960, cap 1024, device images, default tracker and detector parameters.

Before every timed top-up each lane's table is thinned to half (every second track is dropped through svo_debug_klt_select, outside
the timed region), so that every lane is below the default threshold and wants its table filled.

  topup      wall time of one top-up of all lanes with the synchronisation behind it: resident (svo_klt_topup, svo_wait) and
             round trip (the four calls, lane by lane; its gate is vectorised numpy)
  step+topup wall time of svo_klt_step(SVO_RUN_OPTIMIZE) followed by the top-up, one synchronisation at the end (resident); the same
             step followed by the round trip
  kernels    per top-up, from svo_kernel_times in a run of its own: "klt_topup" is the SUM of the three new kernels (jobs, prepare,
             append), beside the detector's and the tracker's launches between them
After the timed top-ups the two contexts must hold the same tables: a figure for different work would mean nothing.
Prints one JSON line (profiles/klt_topup_times.json).  No threshold hangs on these figures."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params
from stereo_vo_amd.synth import SyntheticStereoWorld
import klt_scenes as KS

W, H, CAP = 1280, 960, 1024


def grid_points(world):
    xs = np.linspace(40.0, W - 41.0, 32); ys = np.linspace(40.0, H - 41.0, 32)
    left = np.array([(x, y) for y in ys for x in xs], np.float32)
    right = left.copy()
    right[:, 0] = (left[:, 0] - world.f * world.B / KS.gt_depth(world, 0, left)).astype(np.float32)
    return left, right


def make_ctx(lanes, cam, kp, pts, kernel_times=False):
    c = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=CAP, max_cand=1 << 17, kernel_times=kernel_times)
    c.set_params(north_star_params(hip.default_params(), orb_nfeats=600))
    c.set_camera(cam)
    c.klt_enable(kp)
    for g in range(lanes):
        assert c.klt_add_points(g, *pts[g]) == CAP
    return c


def thin(c):
    """drops every second track of every lane (a selection with hand-made statuses: the lane's last pair stays)"""
    for g in range(c.n_lanes):
        l, r, _, _ = c.klt_tracks(g)
        st = (np.arange(len(l)) % 2 == 0).astype(np.uint8)
        c.klt_debug_select(g, l, r, st, np.ones(len(l), np.uint8))


def round_trip(c, kp, tp, frames):
    """the four calls, lane by lane"""
    out = []
    for g in range(c.n_lanes):
        left = c.klt_tracks(g)[0]
        if len(left) >= tp.below:
            continue
        want = max(min(tp.target, kp.cap) - len(left), 0)
        (corners, _, _, status), = c.gftt_detect([(frames[g][0], left, want)], tp.gftt, device=True)
        if status:
            continue
        init = corners.copy(); init[:, 0] -= np.float32(tp.init_disp)
        (o, st, _), = c.lk_track([(frames[g][0], frames[g][1], corners, init)], kp.lk, device=True)
        with np.errstate(invalid="ignore", over="ignore"):
            d = corners[:, 0] - o[:, 0]
            ok = (st == 1) & np.isfinite(o).all(axis=1) & (np.abs(corners[:, 1] - o[:, 1]) <= np.float32(kp.max_dy)) \
                & (d >= np.float32(kp.min_disp)) & (d <= np.float32(kp.max_disp))
        out.append(c.klt_add_points(g, corners[ok], o[ok]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=96)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=4)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nf = 2 * (a.warmup + a.steps) + 1
    worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=g, scene_seed=0, n_frames=nf, device=dev, noise_on_device=True) for g in range(a.worlds)]
    rendered = [[w.render(t) for t in range(nf)] for w in worlds]
    torch.cuda.synchronize()
    cam = worlds[0].camera()
    wpts = [grid_points(w) for w in worlds]
    pts = [wpts[g % a.worlds] for g in range(a.lanes)]

    def frames_of(t):
        return [tuple((im.data_ptr(), W, H, W) for im in rendered[g % a.worlds][t]) for g in range(a.lanes)]
    kp = hip.default_klt_params()
    kp.cap = CAP
    ca, cb = make_ctx(a.lanes, cam, kp, pts), make_ctx(a.lanes, cam, kp, pts)
    tp = ca.klt_topup_enable()
    t_res, t_rt, t_sres, t_srt, appended = [], [], [], [], []
    t = 0
    for c in (ca, cb):
        c.klt_step(frames_of(0), device=True); c.wait()
    # leg 1: the top-up alone
    for k in range(a.warmup + a.steps):
        t += 1
        fr = frames_of(t)
        for c in (ca, cb):
            c.klt_step(fr, device=True); thin(c); c.wait()
        t0 = time.perf_counter(); ca.klt_topup(); ca.wait(); t1 = time.perf_counter()
        got = round_trip(cb, kp, tp, fr); cb.wait(); t2 = time.perf_counter()
        if k >= a.warmup:
            t_res.append(1e3 * (t1 - t0)); t_rt.append(1e3 * (t2 - t1)); appended += got
    # leg 2: a step and the top-up behind it
    for k in range(a.warmup + a.steps):
        t += 1
        fr = frames_of(t)
        for c in (ca, cb):
            thin(c); c.wait()
        t0 = time.perf_counter(); ca.klt_step(fr, device=True); ca.klt_topup(); ca.wait(); t1 = time.perf_counter()
        cb.klt_step(fr, device=True); round_trip(cb, kp, tp, fr); cb.wait(); t2 = time.perf_counter()
        if k >= a.warmup:
            t_sres.append(1e3 * (t1 - t0)); t_srt.append(1e3 * (t2 - t1))
    same = all(all(x.tobytes() == y.tobytes() for x, y in zip(ca.klt_tracks(g), cb.klt_tracks(g))) for g in range(a.lanes))
    reasons = [ca.klt_topup_info(g)[3] for g in range(a.lanes)]
    live = [len(ca.klt_tracks(g)[2]) for g in range(a.lanes)]
    ca.close(); cb.close()
    # the kernels, in a run of their own
    ck = make_ctx(a.lanes, cam, kp, pts, kernel_times=True)
    ck.klt_topup_enable()
    ck.klt_step(frames_of(0), device=True)
    n_k = 3
    names = ("klt_topup", "gftt_response", "gftt_candidates", "gftt_select", "lk_track")
    kt = {k: 0.0 for k in names}
    for k in range(n_k + 1):
        ck.klt_step(frames_of(k + 1), device=True); thin(ck)
        before = ck.kernel_times(appended=True)                  # (waits)
        ck.klt_topup()
        after = ck.kernel_times(appended=True)
        for name in names:
            if k and name in after:
                kt[name] += after[name][0] - before.get(name, (0.0, 0))[0]
    ck.close()
    med = lambda v: round(float(np.median(v)), 3)
    out = {"shape": "%d lanes of %dx%d in one context, cap %d, tables thinned to half before each top-up, default tracker (win 21, 4 levels) and detector "
                    "(block 3, min_distance 20, quality 0.01) parameters, below = %d, target = %d, device images, %d warm-up + %d timed rounds per leg, "
                    "%d rendered trajectories shared by the lanes" % (a.lanes, W, H, CAP, tp.below, tp.target, a.warmup, a.steps, a.worlds),
           "topup_ms": {"resident": med(t_res), "round_trip": med(t_rt), "resident_all": [round(v, 3) for v in t_res], "round_trip_all": [round(v, 3) for v in t_rt]},
           "step_plus_topup_ms": {"resident": med(t_sres), "round_trip": med(t_srt)},
           "same_tables": bool(same), "reasons_last_topup": {str(r): reasons.count(r) for r in sorted(set(reasons))},
           "appended_per_lane_round_trip": {"min": int(min(appended)) if appended else 0, "mean": round(float(np.mean(appended)), 1) if appended else 0.0, "max": int(max(appended)) if appended else 0},
           "live_tracks_at_the_end": {"min": min(live), "mean": round(sum(live) / len(live), 1), "max": max(live)},
           "kernel_us_per_topup": {k: round(1e3 * kt[k] / n_k, 2) for k in names},
           "kernel_note": "klt_topup is the sum of k_klt_topup_jobs, k_klt_topup_prepare and k_klt_topup_append (three launches per top-up)"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
