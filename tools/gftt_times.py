#!/usr/bin/env python3
"""What a svo_gftt_detect call costs at the size a many-stream user runs: ONE call of `jobs` images of 1280x960 with images of their own,
default parameters (block 3, quality 0.01, min_distance 20), on device images (read in place), in steady state after warm-up.
  * gftt_response / gftt_candidates / gftt_select: the three spans of svo_kernel_times, per call;
  * call_ms: the host clock around the whole call, which ends in a synchronise -- it adds the upload of the job records, the download
    of the results and the host-side scatter;
  * the bytes the call must move, computed from the shapes: the image read once (1 B per pixel), the response map written once and
    read once (4 B + 4 B per pixel), and the candidate keys (8 B written and read per candidate);
  * corners and candidates per job.
Prints one JSON line (profiles/gftt_times.json).  No threshold hangs on these figures."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from stereo_vo_amd import hip

W, H = 1280, 960


def make_image(gen, dev):
    """a smooth two-octave texture with hard-edged 32-pixel patches on top (their junctions are the corners), uint8 on the device"""
    acc = torch.zeros((1, 1, H, W), device=dev)
    for cell in (16, 64):
        g = torch.rand((1, 1, H // cell + 3, W // cell + 3), device=dev, generator=gen)
        acc += torch.nn.functional.interpolate(g, scale_factor=cell, mode="bicubic", align_corners=False)[:, :, :H, :W]
    patches = torch.rand((1, 1, H // 32 + 1, W // 32 + 1), device=dev, generator=gen)
    acc += 1.5 * torch.nn.functional.interpolate(patches, scale_factor=32, mode="nearest")[:, :, :H, :W]
    acc = acc[0, 0]
    acc = (acc - acc.min()) * (255.0 / (acc.max() - acc.min()))
    return acc.round().clamp(0, 255).to(torch.uint8).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=192)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gftt_times: no GPU; these figures are measured on the device or not at all")
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev); gen.manual_seed(7)
    ctx = hip.Context(n_lanes=(a.jobs + 3) // 4, max_w=W, max_h=H, max_kps=a.cap, max_cand=1 << 16, kernel_times=True)
    p = hip.default_gftt_params()
    keep, jobs = [], []
    for j in range(a.jobs):
        img = make_image(gen, dev)
        keep.append(img)
        jobs.append(((img.data_ptr(), W, H, W), None, a.cap))
    torch.cuda.synchronize()
    for _ in range(a.warmup):
        res = ctx.gftt_detect(jobs, p, device=True)
    ctx.kernel_times_reset()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        res = ctx.gftt_detect(jobs, p, device=True)
    wall = (time.perf_counter() - t0) / a.steps
    kt = ctx.kernel_times(appended=True)
    names = ("gftt_response", "gftt_candidates", "gftt_select")
    ms = {k: kt[k][0] / kt[k][1] for k in names}
    corners = np.array([len(r[0]) for r in res]); cands = np.array([r[2] for r in res])
    px = a.jobs * W * H
    out = {
        "shape": "one call of %d jobs of %dx%d on device images, block %d, quality %g, min_distance %d, cap %d; %d timed calls after %d warm-up calls"
                 % (a.jobs, W, H, p.block, p.quality, p.min_distance, a.cap, a.steps, a.warmup),
        "gftt_response_ms_per_call": round(ms["gftt_response"], 3),
        "gftt_candidates_ms_per_call": round(ms["gftt_candidates"], 3),
        "gftt_select_ms_per_call": round(ms["gftt_select"], 3),
        "spans": {k: list(kt[k]) for k in names},
        "call_ms": round(1e3 * wall, 3),
        "corners_per_job": [int(corners.min()), float(np.median(corners)), int(corners.max())],
        "candidates_per_job": [int(cands.min()), float(np.median(cands)), int(cands.max())],
        "overflowed_jobs": int(sum(r[3] for r in res)),
        "response_bytes": int(5 * px), "candidates_bytes": int(4 * px + 8 * cands.sum()), "select_bytes": int(8 * cands.sum()),
        "response_GBps": round(5 * px / (1e6 * ms["gftt_response"]), 1),
        "candidates_GBps": round((4 * px + 8 * float(cands.sum())) / (1e6 * ms["gftt_candidates"]), 1),
        "response_Gpixels_per_s": round(px / (1e6 * ms["gftt_response"]), 2),
    }
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
