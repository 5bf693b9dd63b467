#!/usr/bin/env python3
"""What a svo_lk_track call costs at the size a many-stream user runs: ONE call of `jobs` image pairs of 1280x960 with `points` points
each, win 21, max_level 3, default iteration limits, on device images (read in place), in steady state after warm-up.
  * lk_pyrdown / lk_track: the two spans of svo_kernel_times (device events around the three k_lk_pyrdown launches and around the
    k_lk_track launch), per call;
  * call_ms: the host clock around the whole call, which ends in a synchronise -- it adds the upload of the points, the download of the
    results and the host-side gather / scatter;
  * the bytes the call must move, computed from the shapes: the pyramids once (level 0 read, levels 1 - 3 written, levels 1 - 2 read
    again for the level below them) and, per point, one (win + 3)^2 template tile per level plus one (win + 1)^2 tile per iteration --
    the tiles come out of L2 / MALL, not HBM.  The iteration count is not known to the host; the figure uses `--iters-per-point`
    (default 9: tests/test_lk_scenes_cpu.py measures 7.7 - 11.0 on this kind of texture, all levels together).
Every job has images of its own (seeded, generated on the device).  Prints one JSON line (profiles/lk_times.json).  No threshold hangs
on these figures.
  --photometric   a second leg of the same shape on the same context and images under svo_lk_set_photometric(ctx, 1), behind the first:
                  its spans, call time and result counts under "photometric", beside the mode-0 figures (profiles/lk_photo_times.json)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stereo_vo_amd import hip

W, H = 1280, 960


def make_pair(gen, dev):
    """a smooth multi-octave texture and its copy moved by about (3.4, -2) px, uint8 on the device"""
    acc = torch.zeros((1, 1, H, W), device=dev)
    for cell in (4, 16, 64):
        g = torch.rand((1, 1, H // cell + 3, W // cell + 3), device=dev, generator=gen)
        acc += torch.nn.functional.interpolate(g, scale_factor=cell, mode="bicubic", align_corners=False)[:, :, :H, :W]
    acc = acc[0, 0]
    acc = (acc - acc.min()) * (255.0 / (acc.max() - acc.min()))
    nxt = 0.6 * torch.roll(acc, (-2, 3), (0, 1)) + 0.4 * torch.roll(acc, (-2, 4), (0, 1))
    return acc.round().clamp(0, 255).to(torch.uint8).contiguous(), nxt.round().clamp(0, 255).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=192)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--iters-per-point", type=float, default=9.0)
    ap.add_argument("--photometric", action="store_true", help="add a leg in mode 1 of svo_lk_set_photometric")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lk_times: no GPU; these figures are measured on the device or not at all")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    lanes = (a.jobs + 3) // 4
    max_kps = 64
    while max_kps < a.points:
        max_kps *= 2
    ctx = hip.Context(n_lanes=lanes, max_w=W, max_h=H, max_kps=max_kps, kernel_times=True)
    p = hip.default_lk_params()
    rng = np.random.default_rng(11)
    keep, jobs = [], []
    for j in range(a.jobs):
        prev, nxt = make_pair(gen, dev)
        keep += [prev, nxt]
        pts = np.stack([rng.uniform(40, W - 40, a.points), rng.uniform(40, H - 40, a.points)], 1).astype(np.float32)
        jobs.append(((prev.data_ptr(), W, H, W), (nxt.data_ptr(), W, H, W), pts))
    torch.cuda.synchronize()

    def leg():
        """(seconds per call, the spans, tracked points, their motion) of warm-up + timed calls in the context's mode"""
        for _ in range(a.warmup):
            res = ctx.lk_track(jobs, p, device=True)
        ctx.kernel_times_reset()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            res = ctx.lk_track(jobs, p, device=True)
        wall = (time.perf_counter() - t0) / a.steps
        kt = ctx.kernel_times(appended=True)
        return wall, kt, int(sum(int(r[1].sum()) for r in res)), np.concatenate([r[0][r[1] == 1] - j[2][r[1] == 1] for r, j in zip(res, jobs)])
    wall, kt, tracked, moved = leg()
    lv = [(W, H)]
    while len(lv) <= p.max_level and (lv[-1][0] + 1) // 2 >= p.win + 4 and (lv[-1][1] + 1) // 2 >= p.win + 4:
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    px = [w * h for w, h in lv]
    pyr_bytes = 2 * a.jobs * (px[0] + sum(px[1:]) + sum(px[1:-1]))
    tile_bytes = a.jobs * a.points * (len(lv) * (p.win + 3) ** 2 + a.iters_per_point * (p.win + 1) ** 2)
    out = {
        "shape": "one call of %d jobs of %dx%d with %d points each on device images, win %d, max_level %d (%d levels), max_iters %d; %d timed calls after %d warm-up calls"
                 % (a.jobs, W, H, a.points, p.win, p.max_level, len(lv), p.max_iters, a.steps, a.warmup),
        "lk_pyrdown_ms_per_call": round(kt["lk_pyrdown"][0] / kt["lk_pyrdown"][1], 3),
        "lk_track_ms_per_call": round(kt["lk_track"][0] / kt["lk_track"][1], 3),
        "spans": {k: list(kt[k]) for k in ("lk_pyrdown", "lk_track")},
        "call_ms": round(1e3 * wall, 3),
        "points_per_call": a.jobs * a.points, "tracked": tracked,
        "median_motion_px": [round(float(np.median(moved[:, 0])), 3), round(float(np.median(moved[:, 1])), 3)],
        "pyramid_bytes": int(pyr_bytes), "tile_bytes_at_%g_iterations_per_point" % a.iters_per_point: int(tile_bytes),
        "pyrdown_GBps": round(pyr_bytes / (1e6 * kt["lk_pyrdown"][0] / kt["lk_pyrdown"][1]), 1),
        "track_tile_GBps": round(tile_bytes / (1e6 * kt["lk_track"][0] / kt["lk_track"][1]), 1),
        "track_Mpoints_per_s": round(a.jobs * a.points / (1e3 * kt["lk_track"][0] / kt["lk_track"][1]), 2),
    }
    if a.photometric:
        ctx.lk_set_photometric(1)
        wall1, kt1, tracked1, moved1 = leg()
        out["photometric"] = {
            "lk_track_ms_per_call": round(kt1["lk_track"][0] / kt1["lk_track"][1], 3),
            "lk_pyrdown_ms_per_call": round(kt1["lk_pyrdown"][0] / kt1["lk_pyrdown"][1], 3),
            "spans": {k: list(kt1[k]) for k in ("lk_pyrdown", "lk_track")},
            "call_ms": round(1e3 * wall1, 3), "tracked": tracked1,
            "median_motion_px": [round(float(np.median(moved1[:, 0])), 3), round(float(np.median(moved1[:, 1])), 3)],
            "lk_track_ratio_to_mode_0": round((kt1["lk_track"][0] / kt1["lk_track"][1]) / (kt["lk_track"][0] / kt["lk_track"][1]), 3),
        }
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
