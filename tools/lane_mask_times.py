#!/usr/bin/env python3
"""What a step costs when some lanes sit it out (svo_process_lanes).  One 96-lane context, 1280x960, north-star parameters,
device-resident frames; a fixed spread of 96, 48, 12 and 1 active lanes.  One JSON line (profiles/lane_mask_times.json):

  step_ms        per active count: ms per step from two device events around `--steps` steps enqueued back to back after the
                 warm-up (every lane has run unmasked frames before, so the active lanes track and solve)
  kernel_ms      per active count, in a separate pass on a context with svo_config.kernel_times: ms per step of every kernel name
                 (HIP events around each launch; the launches then do not overlap, so these do not add up to step_ms)
  one_lane_ctx   the step time of a ONE-lane context on the frames of the lane that is alone in the 1-active case

The grids stay whole: an idle lane's workgroups leave at once.  one_lane_ctx against step_ms["1"] is what launching them costs --
the baseline for a later compaction of the lane list.  No threshold hangs on these figures."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params
from stereo_vo_amd.synth import SyntheticStereoWorld

W, H, LANES = 1280, 960, 96
ACTIVE = {96: list(range(96)), 48: list(range(1, 96, 2)), 12: list(range(5, 96, 8)), 1: [47]}


def ping_pong(step, F):
    period = 2 * (F - 1); k = step % period
    return k if k < F else period - k


def timed(ctx, stream, tables, active, steps, warm):
    """ms per step: `warm` steps with the mask (words of hip.lane_mask_words, or None), then `steps` between two events on the context's stream"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 0
    for i in range(warm + steps):
        if i == warm:
            ctx.wait(); e0.record(stream)
        ctx._process(tables[ping_pong(n, len(tables))], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, active)
        n += 1
    e1.record(stream); e1.synchronize(); ctx.wait()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--frames", type=int, default=4, help="distinct frames per stream, walked back and forth")
    ap.add_argument("--worlds", type=int, default=8, help="distinct streams; lane l shows world l %% worlds")
    ap.add_argument("--orb-nfeats", type=int, default=2000)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    worlds = [SyntheticStereoWorld(W, H, 800.0, 0.12, seed=100 + s, n_frames=a.frames, device=dev, scene_seed=s % 4) for s in range(a.worlds)]
    imgs = [[w.render(t) for t in range(a.frames)] for w in worlds]
    torch.cuda.synchronize()
    cam = worlds[0].camera()
    p = north_star_params(hip.default_params(), orb_nfeats=a.orb_nfeats)

    def tables(n_lanes, first=0):
        out = []
        for t in range(a.frames):
            fr = (hip.Frame * n_lanes)()
            for l in range(n_lanes):
                L, R = imgs[(first + l) % a.worlds][t]
                fr[l].left = hip.Image(L.data_ptr(), W, H, W); fr[l].right = hip.Image(R.data_ptr(), W, H, W)
            out.append(fr)
        return out

    out = {"shape": "one context of %d lanes, %dx%d, north-star ORB + brute force, orb_nfeats %d, max_kps 4096, device frames (%d streams x %d frames, back and forth); "
                    "%d timed steps after %d warm-up steps per mask, all lanes warmed with unmasked frames first" % (LANES, W, H, a.orb_nfeats, a.worlds, a.frames, a.steps, a.warmup),
           "active_lanes": {str(k): (v if len(v) <= 12 else "%d, %d, .. %d" % (v[0], v[1], v[-1])) for k, v in ACTIVE.items()}}
    s = torch.cuda.Stream()
    for pass_name, kt in (("step_ms", False), ("kernel_ms", True)):
        ctx = hip.Context(n_lanes=LANES, max_w=W, max_h=H, max_kps=4096, kernel_times=kt, stream=s.cuda_stream)
        ctx.set_params(p); ctx.set_camera(cam)
        tb = tables(LANES)
        for i in range(3):
            ctx._process(tb[i % a.frames], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, None)
        ctx.wait()
        out[pass_name] = {}
        for n_act, lane_list in ACTIVE.items():
            lanes = hip.lane_mask_words(lane_list, LANES)
            if kt:
                for i in range(a.warmup):
                    ctx._process(tb[ping_pong(i, a.frames)], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, lanes)
                ctx.wait(); ctx.kernel_times_reset()
                for i in range(a.steps):
                    ctx._process(tb[ping_pong(a.warmup + i, a.frames)], hip.RUN_ALL | hip.FLAG_DEVICE_IMAGES, lanes)
                ctx.wait()
                out[pass_name][str(n_act)] = {k: round(v[0] / a.steps, 4) for k, v in ctx.kernel_times().items() if v[1]}
            else:
                out[pass_name][str(n_act)] = round(timed(ctx, s, tb, lanes, a.steps, a.warmup), 4)
        if not kt:
            res = ctx.results()
            out["valid_after_the_1_active_pass"] = {"lane 47": int(res[47].valid), "tracked": res[47].tracked_feats_from_last_frame}
        ctx.close()
    one = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=4096, stream=s.cuda_stream)
    one.set_params(p); one.set_camera(cam)
    out["one_lane_ctx_ms"] = round(timed(one, s, tables(1, first=47), None, a.steps, a.warmup + 3), 4)
    one.close()
    out["idle_grid_price_ms"] = round(out["step_ms"]["1"] - out["one_lane_ctx_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
