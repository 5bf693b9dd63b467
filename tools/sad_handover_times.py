#!/usr/bin/env python3
"""What the hand-over records with the SAD windows (k_handover.hip, layout version 3) cost and buy.  Two parts, one JSON line
(profiles/sad_handover_times.json):

  hop       HIP-event times (svo_config.kernel_times) of svo_export_frame on one context and svo_import_frame on another, at max_kps
            1024 and 16384, between contexts that carry no windows (FAST+ORB, row-by-row Hamming pairing: version 2 records, the
            kernels under `export_frame` / `import_frame`) and between contexts that do (the same with smSAD: version 3, the kernels
            under `export_frame_win` / `import_frame_win`).  2048x1536 synthetic street, no NMS, FAST threshold 5: ~14 k keypoints
            per image, cut at 1024 in the small contexts (status bit 2; the copies move full lists, which is what is timed).  The
            launch counts per name show which kernels each kind of context ran.
  stream    ms per frame of ONE 1280x960 stream under dmFASTER + smSAD + ifmSAD on three octaves, enqueued back to back: one
            context fed sequentially, and FrameParallelStream with 2 and 3 contexts.  "Does it help" is read against the one-context
            figure of the same run.

No threshold hangs on these figures."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, DM_FAST_ORB, DM_FASTER
from stereo_vo_amd.synth import SyntheticStereoWorld
from stereo_vo_amd.pipeline import FrameParallelStream

HOP_NAMES = ("export_frame", "import_frame", "export_frame_win", "import_frame_win")


def hop_params(sad):
    p = hip.default_params()
    p.detect_method, p.nOctaves, p.non_maximal_suppression = DM_FAST_ORB, 1, 0
    p.initial_FAST_threshold, p.fast_min_th = 5, 1
    p.match_method, p.enable_robust_1to1_match, p.max_y_diff = (2 if sad else 1), 0, 8.0
    p.orb_max_distance, p.orb_max_th, p.sad_max_distance = 120.0, 256, 800
    p.ifm_method = 0
    return p


def hop(max_kps, sad, frames, cam, W, H, reps):
    ctxs = []
    for k in range(2):
        c = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=max_kps, max_cand=1 << 18, kernel_times=True)
        c.set_params(hop_params(sad)); c.set_camera(cam)
        c.process_host([frames[0]]); c.process_host([frames[1]])
        ctxs.append(c)
    a, b = ctxs
    nb = a.handover_bytes()
    assert nb == b.handover_bytes()
    blob = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for rep in range(reps + 2):                                 # two warm-up hops
        if rep == 2:
            a.kernel_times_reset(); b.kernel_times_reset()
        a.export_frame(blob.data_ptr(), nb); a.wait()
        b.import_frame(blob.data_ptr(), nb); b.wait()
    kta, ktb = a.kernel_times(), b.kernel_times()
    r = a.result(0)
    n_l, n_r, n_m = r.detected_left[0], r.detected_right[0], r.stereo_matches[0]
    moved = (n_l + n_r) * (28 + 32) + n_m * (16 + 4) + (3 * H + 1) * 4 + ((n_l + n_r) * 65 if sad else 0)
    ex, im = ("export_frame_win", "import_frame_win") if sad else ("export_frame", "import_frame")
    out = {"record_bytes": nb, "list_bytes_moved": moved, "keypoints": [n_l, n_r], "pairings": n_m,
           "export_us": round(1e3 * kta[ex][0] / kta[ex][1], 2), "import_us": round(1e3 * ktb[im][0] / ktb[im][1], 2),
           "launches_exporter": {k: kta[k][1] for k in HOP_NAMES}, "launches_importer": {k: ktb[k][1] for k in HOP_NAMES},
           "imported_status": b.status_word(0) & 4}
    out["export_GB_s"] = round(moved / (out["export_us"] * 1e3), 1)
    out["import_GB_s"] = round(moved / (out["import_us"] * 1e3), 1)
    a.close(); b.close()
    return out


def stream(n, warm, nfe, sad):
    W, H, NO = 1280, 960, 3
    dev = torch.device("cuda", 0)
    NF = n + warm
    w = SyntheticStereoWorld(W, H, 800.0, 0.12, seed=0, n_frames=NF, device=dev, scene="street", noise_on_device=True)
    frames = [w.render(t) for t in range(NF)]
    torch.cuda.synchronize()
    cam = w.camera()
    p = north_star_params(hip.default_params(), orb_nfeats=nfe)
    p.detect_method, p.nOctaves, p.max_y_diff, p.match_method, p.ifm_method = DM_FASTER, NO, 2.0, 2, 2
    p.sad_max_distance = p.ifm_sad_max_distance = sad
    out = {"shape": "one %dx%d stream, dmFASTER + smSAD + ifmSAD, %d octaves, orb_nfeats %d, sad_max_distance %d (both groups), max_kps 4096, max_cand 2^18, %d distinct frames enqueued back to back after %d warm-up frames" % (W, H, NO, nfe, sad, n, warm)}
    ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=4096, max_cand=1 << 18, max_octaves=NO)
    ctx.set_params(p); ctx.set_camera(cam)
    for i in range(warm):
        ctx.process_device([(frames[i][0].data_ptr(), frames[i][1].data_ptr())], W, H, W)
    ctx.wait()
    t0 = time.perf_counter()
    for i in range(warm, NF):
        ctx.process_device([(frames[i][0].data_ptr(), frames[i][1].data_ptr())], W, H, W)
    ctx.wait(); dt = time.perf_counter() - t0
    r = ctx.result(0)
    last = (bytes(r), ctx.tracked(0).tobytes())
    out["1ctx_ms"] = round(1e3 * dt / n, 4)
    out["last_frame"] = {"keypoints_left": list(r.detected_left[:NO]), "pairings": list(r.stereo_matches[:NO]), "tracked": r.tracked_feats_from_last_frame, "valid": int(r.valid), "status": r.status}
    ctx.close()
    for G in (2, 3):
        fp = FrameParallelStream(p, cam, W, H, lanes=1, contexts=G, max_kps=4096, max_cand=1 << 18, max_octaves=NO)
        for i in range(warm):
            fp.push([(frames[i][0].data_ptr(), frames[i][1].data_ptr())])
        fp.synchronize()
        t0 = time.perf_counter()
        for i in range(warm, NF):
            c = fp.push([(frames[i][0].data_ptr(), frames[i][1].data_ptr())])
        fp.synchronize(); dt = time.perf_counter() - t0
        out["frame_parallel_%dctx_ms" % G] = round(1e3 * dt / n, 4)
        out["frame_parallel_%dctx_same_last_frame" % G] = bool((bytes(c.result(0)), c.tracked(0).tobytes()) == last)
        out["frame_parallel_%dctx_record_bytes" % G] = c.handover_bytes()
        fp.close()
    out["speedup_2ctx"] = round(out["1ctx_ms"] / out["frame_parallel_2ctx_ms"], 3)
    out["speedup_3ctx"] = round(out["1ctx_ms"] / out["frame_parallel_3ctx_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100, help="timed export + import hops per configuration")
    ap.add_argument("--frames", type=int, default=600, help="timed frames of the single-stream part")
    ap.add_argument("--stream-repeats", type=int, default=3, help="the single-stream part is run this many times over (the spread between them is the noise)")
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--orb-nfeats", type=int, default=1350)
    ap.add_argument("--sad", type=int, default=800)
    ap.add_argument("--skip-hop", action="store_true")
    ap.add_argument("--skip-stream", action="store_true")
    a = ap.parse_args()
    out = {}
    if not a.skip_hop:
        W, H = 2048, 1536
        w = SyntheticStereoWorld(W, H, 1280.0, 0.12, seed=51, n_frames=2)
        frames = [tuple(np.ascontiguousarray(x.numpy()) for x in w.render(t)) for t in range(2)]
        out["hop"] = {"shape": "%dx%d, one lane, one octave, FAST+ORB, no NMS, FAST threshold 5; %d timed hops after 2; us per call from HIP events around the launches of one call" % (W, H, a.reps)}
        for mk in (1024, 16384):
            out["hop"]["max_kps %d" % mk] = {"no windows (version 2)": hop(mk, False, frames, w.camera(), W, H, a.reps),
                                             "windows (version 3)": hop(mk, True, frames, w.camera(), W, H, a.reps)}
    if not a.skip_stream:
        out["stream"] = [stream(a.frames, a.warmup, a.orb_nfeats, a.sad) for _ in range(a.stream_repeats)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
