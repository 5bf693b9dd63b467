#!/usr/bin/env python3
"""What finding a pairing's row iteration in the row table costs k_track_win (a binary search per previous pairing where it used to take
ceilf of the keypoint's own row): the time of stage 4's tracker kernel ("track_filter" in the context's kernel_times: k_track_filter under
ifmDescBF, k_track_win under ifmDescWin) on the small golden sequence, for two or more builds of the library alternating in one call.

    tools/match_scenes_times.py --libs parent=/path/to/libsvo_hip.so,tree=stereo_vo_amd/libsvo_hip.so [--repeats 3] [--steps 400]

Every (library, repeat) is a fresh child process that loads the library through SVO_HIP_LIB, runs the four frames of
tests/golden/oracle_small_seq.npz back and forth for --steps frames per tracker after 20 of warm-up, and reports us per launch.  One JSON
line, also written to profiles/match_scenes_times.json: per library and tracker the repeats, their mean and spread (max - min), and the
difference of the means against the first library.  The expectation to read it against: equality within the first library's own spread.
No threshold hangs on these figures."""
import argparse, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def child(steps):
    import numpy as np
    from stereo_vo_amd import hip
    from stereo_vo_amd.abi import StereoCamera, north_star_params
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_small_seq.npz"))
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    out = {}
    for name, method in (("ifmDescBF", 0), ("ifmDescWin", 1)):
        p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
        p.ifm_method = method; p.ifm_win_w = 20; p.ifm_win_h = 30
        ctx = hip.Context(n_lanes=1, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=1024, max_cand=1 << 15, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam)
        tracked = 0
        for step in range(20 + steps):
            if step == 20:
                ctx.kernel_times_reset()
            k = step % 6
            t = k if k < 4 else 6 - k
            ctx.process_host([(g["L%d" % t], g["R%d" % t])])
            tracked += len(ctx.tracked(0))
        ms, calls = ctx.kernel_times()["track_filter"]
        ctx.close()
        out[name] = {"us_per_launch": round(1000.0 * ms / calls, 3), "launches": calls, "tracked_pairs_total": tracked}
    print("CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "match_scenes_times.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    libs = [kv.split("=", 1) for kv in a.libs.split(",")]
    runs = {name: {"ifmDescBF": [], "ifmDescWin": []} for name, _ in libs}
    tracked = {}
    for rep in range(a.repeats):
        for name, path in libs:                                                  # alternating: a drift of the box lands on every library alike
            env = dict(os.environ, SVO_HIP_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--libs", a.libs, "--steps", str(a.steps), "--child"], env=env, capture_output=True, text=True, timeout=300)
            line = [l for l in r.stdout.splitlines() if l.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.exit("child failed (%s, repeat %d, rc %d): %s" % (name, rep, r.returncode, r.stderr[-800:]))
            got = json.loads(line[0][6:])
            for k in runs[name]:
                runs[name][k].append(got[k]["us_per_launch"])
                tracked.setdefault(name, {})[k] = got[k]["tracked_pairs_total"]
    first = libs[0][0]
    out = {"shape": "tests/golden/oracle_small_seq.npz (256x192, ~105 pairings per frame), one lane, max_kps 1024, %d timed frames after 20, %d repeats per library, alternating; "
                    "us per launch of the kernel_times entry track_filter (k_track_filter under ifmDescBF, k_track_win with windows 20 / 30 under ifmDescWin)" % (a.steps, a.repeats),
           "expectation": "equal within the spread of the first library's repeats", "libraries": {}}
    for name, _ in libs:
        out["libraries"][name] = {}
        for k, v in runs[name].items():
            mean = sum(v) / len(v)
            base = sum(runs[first][k]) / len(runs[first][k])
            out["libraries"][name][k] = {"us_per_launch": v, "mean": round(mean, 3), "spread": round(max(v) - min(v), 3), "mean_minus_%s" % first: round(mean - base, 3),
                                         "tracked_pairs_total": tracked[name][k]}
    line = json.dumps(out)
    print(line)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
