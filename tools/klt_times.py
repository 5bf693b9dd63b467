#!/usr/bin/env python3
"""Step time of the resident KLT front end (svo_klt_step) beside the host recipe it replaces (a shift-only call,
svo_lk_track, the gate in numpy, the svo_put_* calls, stage 5) on the same frames: ONE context of `lanes` streams at 1280x960, 1024
tracks per lane from a 32 x 32 grid with ground-truth disparity, device images, default tracker parameters.

  resident   wall time per step of svo_klt_step(SVO_RUN_OPTIMIZE) over the timed frames, ONE synchronisation at the end of the leg
  recipe     wall time per step of the recipe on a second context (every step synchronises by itself: svo_lk_track and the puts do);
             its gate is vectorised numpy, not the per-slot walk of tests/klt_ref.py, so that the figure is the calls' and not Python's
  kernels    lk_pyrdown (the job records and the level launches) / lk_track / klt_select per step from svo_kernel_times, in a run of its
             own (events cost a few percent)
After the timed frames the two contexts must agree in every lane's result record and current lists: a figure for different work would
mean nothing.  Lanes share `worlds` rendered trajectories (lane g follows world g % worlds): rendering is not what is measured.

Also, as information: the translation / rotation error of the resident front end against SyntheticStereoWorld.gt_delta on the 160x120
sequence of tests/klt_scenes.py, beside the library's detect-match-track path on the same frames.
Prints one JSON line (profiles/klt_times.json).  No threshold hangs on these figures."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, keypoint_dtype, dmatch_dtype, index_pair_dtype, VOEC_BAD_TRACKING, VOEC_BAD_COND_NUMBER
from stereo_vo_amd.synth import SyntheticStereoWorld, pose6_to_matrix, pose_error
import klt_scenes as KS

W, H, CAP = 1280, 960, 1024


def grid_points(world):
    xs = np.linspace(40.0, W - 41.0, 32); ys = np.linspace(40.0, H - 41.0, 32)
    left = np.array([(x, y) for y in ys for x in xs], np.float32)
    right = left.copy()
    right[:, 0] = (left[:, 0] - world.f * world.B / KS.gt_depth(world, 0, left)).astype(np.float32)
    return left, right


def make_ctx(lanes, cam, kernel_times=False):
    c = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=CAP, max_cand=1 << 15, kernel_times=kernel_times)
    c.set_params(north_star_params(hip.default_params(), orb_nfeats=600))      # (the detector is never run; its list capacity must fit max_kps)
    c.set_camera(cam)
    return c


def resident(lanes, frames_of, pts, cam, kp, warm, timed, kernel_times=False):
    c = make_ctx(lanes, cam, kernel_times)
    c.klt_enable(kp)
    for g in range(lanes):
        assert c.klt_add_points(g, *pts[g]) == CAP
    for t in range(warm):
        c.klt_step(frames_of(t), device=True)
    c.wait()
    if kernel_times:
        c.kernel_times_reset()
    t0 = time.perf_counter()
    for t in range(warm, warm + timed):
        c.klt_step(frames_of(t), device=True)
    c.wait()
    ms = 1e3 * (time.perf_counter() - t0) / timed
    return c, ms


class Recipe:
    """the recipe of INTEGRATION.md 3d with a vectorised gate"""
    def __init__(self, ctx, kp, pts):
        self.c, self.kp = ctx, kp
        n = ctx.n_lanes
        self.left = [p[0].copy() for p in pts]; self.right = [p[1].copy() for p in pts]
        self.ids = [np.arange(CAP, dtype=np.int32) for _ in range(n)]
        self.idx = [np.full(CAP, -1, np.int32) for _ in range(n)]; self.pidx = [np.full(CAP, -1, np.int32) for _ in range(n)]
        self.prev, self.stepped = None, False

    def step(self, frames):
        c, kp, n = self.c, self.kp, self.c.n_lanes
        held = [False] * n
        if self.stepped:
            held = [r.error_code in (VOEC_BAD_TRACKING, VOEC_BAD_COND_NUMBER) for r in c.results()]
        c._process(None, 0, None)
        if self.prev is not None:
            jobs = []
            for g in range(n):
                for s in (0, 1):
                    jobs.append((self.prev[g][s], frames[g][s], self.left[g] if s == 0 else self.right[g]))
            res = c.lk_track(jobs, kp.lk, device=True)
        for g in range(n):
            if self.prev is not None:
                (L, sl, _), (R, sr, _) = res[2 * g], res[2 * g + 1]
                ok = (sl == 1) & (sr == 1)
            else:
                L, R, ok = self.left[g], self.right[g], np.ones(len(self.left[g]), bool)
            with np.errstate(invalid="ignore", over="ignore"):
                d = L[:, 0] - R[:, 0]
                ok &= np.isfinite(L).all(axis=1) & np.isfinite(R).all(axis=1) & (np.abs(L[:, 1] - R[:, 1]) <= np.float32(kp.max_dy)) \
                    & (d >= np.float32(kp.min_disp)) & (d <= np.float32(kp.max_disp))
            keep = np.flatnonzero(ok)
            m = len(keep)
            p = (self.pidx[g] if held[g] or not self.stepped else self.idx[g])[keep]
            kps = []
            for pts in (L, R):
                k = np.zeros(m, keypoint_dtype)
                k["x"], k["y"], k["size"], k["angle"], k["class_id"] = pts[keep, 0], pts[keep, 1], kp.lk.win, -1.0, self.ids[g][keep]
                kps.append(k)
            mm = np.zeros(m, dmatch_dtype); mm["queryIdx"] = mm["trainIdx"] = np.arange(m)
            has = np.flatnonzero(p >= 0)
            tr = np.zeros(len(has), index_pair_dtype); tr["first"], tr["second"] = p[has], has
            c.put_features(g, 0, 0, kps[0], None, W, H); c.put_features(g, 0, 1, kps[1], None, W, H)
            c.put_matches(g, 0, mm); c.put_match_ids(g, 0, self.ids[g][keep]); c.put_tracked(g, tr, octave=0)
            self.left[g], self.right[g], self.ids[g] = L[keep].copy(), R[keep].copy(), self.ids[g][keep].copy()
            self.idx[g], self.pidx[g] = np.arange(m, dtype=np.int32), p.astype(np.int32)
        c.run_stages(hip.RUN_OPTIMIZE)
        self.prev, self.stepped = frames, True


def accuracy():
    """(resident, detect-match-track): per frame 1 .. 4 of the 160x120 sequence [valid, rotation error rad, translation error m]"""
    world, frames = KS.sequence_world(), KS.sequence_frames()
    kp = hip.default_klt_params()
    kp.cap = KS.SEQ_CAP
    for k, v in KS.SEQ_LK.items():
        setattr(kp.lk, k, v)
    kp.max_dy, kp.min_disp, kp.max_disp = KS.SEQ_GATE["max_dy"], KS.SEQ_GATE["min_disp"], KS.SEQ_GATE["max_disp"]
    p = north_star_params(hip.default_params()); p.orb_nlevels, p.orb_nfeats = 2, 300
    out = []
    for klt in (True, False):
        c = hip.Context(n_lanes=1, max_w=KS.W, max_h=KS.H, max_kps=512, max_cand=1 << 15)
        c.set_params(p); c.set_camera(world.camera())
        if klt:
            c.klt_enable(kp); c.klt_add_points(0, *KS.sequence_points())
        rows = []
        for t in range(KS.SEQ_FRAMES):
            if klt: c.klt_step([frames[t]])
            else: c.process_host([frames[t]])
            r = c.result(0)
            if t:
                er, et = pose_error(pose6_to_matrix(list(r.outPose)), world.gt_delta(t))
                rows.append([int(r.valid), round(er, 5), round(et, 4)])
        c.close()
        out.append(rows)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=96)
    ap.add_argument("--worlds", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    nf = a.warmup + a.steps
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
    ca, ms_res = resident(a.lanes, frames_of, pts, cam, kp, a.warmup, a.steps)
    cb = make_ctx(a.lanes, cam)
    rec = Recipe(cb, kp, pts)
    for t in range(a.warmup):
        rec.step(frames_of(t))
    cb.wait()
    t0 = time.perf_counter()
    for t in range(a.warmup, nf):
        rec.step(frames_of(t))
    cb.wait()
    ms_rec = 1e3 * (time.perf_counter() - t0) / a.steps
    # the same work: every lane's record and current lists
    ra, rb = ca.results(), cb.results()
    same = all(bytes(x) == bytes(y) for x, y in zip(ra, rb)) and all(
        ca.keypoints(g, 0, s)[0].tobytes() == cb.keypoints(g, 0, s)[0].tobytes() for g in range(a.lanes) for s in (0, 1)) and all(
        ca.tracked(g).tobytes() == cb.tracked(g).tobytes() for g in range(a.lanes))
    live = [len(ca.klt_tracks(g)[2]) for g in range(a.lanes)]
    valid = sum(int(r.valid) for r in ra)
    ca.close(); cb.close()
    ck, _ = resident(a.lanes, frames_of, pts, cam, kp, a.warmup, a.steps, kernel_times=True)
    kt = ck.kernel_times(appended=True)
    ck.close()
    acc = accuracy()
    out = {"shape": "%d lanes of %dx%d in one context, %d tracks per lane at the start, default tracker parameters (win 21, 4 levels), device images, "
                    "%d warm-up + %d timed frames, %d rendered trajectories shared by the lanes" % (a.lanes, W, H, CAP, a.warmup, a.steps, a.worlds),
           "resident_ms_per_step": round(ms_res, 3), "recipe_ms_per_step": round(ms_rec, 3),
           "same_results_and_lists": bool(same), "lanes_valid_last_frame": valid,
           "live_tracks_last_frame": {"min": min(live), "mean": round(sum(live) / len(live), 1), "max": max(live)},
           "kernel_us_per_step": {k: round(1e3 * kt[k][0] / a.steps, 2) for k in ("begin_frame", "lk_pyrdown", "lk_track", "klt_select", "gauss_newton") if k in kt},
           "accuracy_160x120": {"columns": "per frame 1..4: [valid, rotation error rad, translation error m] against gt_delta",
                                "resident_klt": acc[0], "detect_match_track (ORB, 2 levels, 300 features)": acc[1]}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
