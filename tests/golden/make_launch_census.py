"""Writes tests/golden/launch_census.json: which kernels a frame launches, name for name and count for count, for every detector,
matcher, tracker and call shape of svo_process -- recorded with the library of the PARENT commit, so that a change of svo_api.hip that
is meant to keep every launch (a refactor) can be held to the table (tests/test_gpu_launch_census.py, which also imports the rows and
the runner from here).

    python tests/golden/make_launch_census.py [--parent REV]     (from the repository root, on the GPU; REV defaults to HEAD~1)

makes a `git worktree` of REV under build/, builds its library there and records with it.  --lib PATH records with a library of the
parent that has already been built elsewhere (a host that builds on one machine and runs on another).

Each row is one configuration run in one call shape on the committed small sequence, two lanes, max_kps 1024, max_cand 1 << 15:
    calls     after the second frame, {kernel name: calls} of svo_kernel_times (kernel_times=True)
    graphs    in a second context with svo_use_graphs, (captured, replayed) after four frames
and each refusal the status and the text of a call that is refused before anything is enqueued.  The runner also returns a hash of
both lanes' outputs (not stored: the test compares the call shapes of one configuration with each other)."""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "launch_census.json")

RUN_DETECT, RUN_MATCH, RUN_TRACK, RUN_OPTIMIZE, RUN_ALL = 1, 2, 4, 8, 15
NO_SHIFT, NO_POST, RUN_DETECT_POST, SPLIT_AT_SELECT, AHEAD = 32, 256, 512, 2048, 4096
REST = RUN_MATCH | RUN_TRACK | RUN_OPTIMIZE
SHAPES = ("all", "split", "split_select", "ahead", "staged")

# (configuration = detector_nms_stage3_stage4, call shape, match IDs, pose covariance, SVO_DEBUG_MODE)
ROWS = [("orb_std_bf_bf", s, 0, 0, 0) for s in SHAPES] + [
    ("orb_std_bf_bf", "all", 1, 0, 0), ("orb_std_bf_bf", "all", 0, 1, 0), ("orb_std_bf_bf", "split", 1, 1, 0), ("orb_std_bf_bf", "ahead", 1, 1, 0),
    ("orb_off_rbr_win", "all", 0, 0, 0), ("orb_off_rbr_win", "split_select", 0, 0, 0),
    ("orb_anms_sad_sad", "all", 0, 0, 0), ("orb_anms_sad_sad", "ahead", 0, 0, 0),
    ("fastorb_std_rbr_win", "all", 1, 0, 0), ("fastorb_std_rbr_win", "split", 1, 0, 0), ("fastorb_std_rbr_win", "ahead", 1, 0, 0),
    ("fastorb_off_bf_bf", "all", 0, 0, 0), ("fastorb_off_bf_bf", "staged", 0, 0, 0),
    ("fastorb_anms_sad_sad", "all", 0, 0, 0), ("fastorb_anms_sad_sad", "split_select", 0, 0, 0),
    ("faster_std_sad_sad", "all", 0, 0, 0), ("faster_std_sad_sad", "split", 0, 0, 0), ("faster_std_sad_sad", "ahead", 0, 0, 0),
    ("faster_std_sad_sad", "staged", 0, 1, 0), ("faster_std_sad_sad", "all", 0, 1, 0),
    ("faster_off_sad_sad", "all", 0, 0, 0), ("faster_off_sad_sad", "split", 0, 0, 0),
    # debug mode 9 (describe everything, then the NMS; results unchanged): read by svo_create from the environment, hence a child process
    ("orb_std_bf_bf", "all", 0, 0, 9), ("orb_std_bf_bf", "split", 0, 0, 9),
]
# what a frame run stage by stage need not share with the one-call frame: every SVO_FLAG_NO_SHIFT call begins with k_begin_frame, which
# starts the result record anew, so the record of the last call (stage 5 alone) speaks of that call only.  The lists are the same.
STAGED_OWN = ("record",)
# (name, configuration, what to change in the parameters, the calls: (flags, active lanes or None), the last one is the refused one)
REFUSALS = [
    ("faster_adaptive_nms", "faster_anms_sad_sad", {}, [(RUN_ALL, None)]),
    ("faster_stage3_bf", "faster_std_bf_sad", {}, [(RUN_ALL, None)]),
    ("faster_stage4_win", "faster_std_sad_win", {}, [(RUN_ALL, None)]),
    ("faster_threshold", "faster_std_sad_sad", {"initial_FAST_threshold": 256}, [(RUN_ALL, None)]),
    ("detector_klt", "orb_std_bf_bf", {"detect_method": 3}, [(RUN_ALL, None)]),
    ("tracker_optical_flow", "orb_std_bf_bf", {"ifm_method": 3}, [(RUN_ALL, None)]),
    ("nms_method", "orb_std_bf_bf", {"nmsMethod": 2}, [(RUN_ALL, None)]),
    ("min_distance", "orb_std_bf_bf", {"min_distance": 1}, [(RUN_ALL, None)]),
    ("ahead_with_post", "orb_std_bf_bf", {}, [(RUN_DETECT | AHEAD, None)]),
    ("ahead_post_no_shift", "orb_std_bf_bf", {}, [(RUN_DETECT_POST | NO_SHIFT | AHEAD, None)]),
    ("another_mask", "orb_std_bf_bf", {}, [(RUN_DETECT | NO_POST, [0]), (RUN_DETECT_POST | REST | NO_SHIFT, [0, 1])]),
    # (not check_frame_call's but the window step's: a stream that switches to ifmSAD on a frame detected without windows)
    ("sad_previous_frame", "orb_std_bf_bf", {}, [(RUN_ALL, None), ("sad", None), (RUN_ALL, None)]),
]


def row_name(row):
    cfg, shape, ids, cov, dbg = row
    return "%s/%s%s%s%s" % (cfg, shape, "+ids" if ids else "", "+cov" if cov else "", "@debug%d" % dbg if dbg else "")


def disagreements(rows):
    """the configurations (with their IDs / covariance setting) whose call shapes do not all leave the same lane outputs, part by part,
    after the second frame ("sha") and after the four frames of the context that runs graphs ("graph_sha")"""
    by_name, seen = {row_name(r): r for r in ROWS}, {}
    for name, r in rows.items():
        cfg, shape, ids, cov, _ = by_name[name]
        for when in ("sha", "graph_sha"):
            for part, h in r[when].items():
                if shape == "staged" and part in STAGED_OWN:
                    continue
                seen.setdefault(("%s ids=%d cov=%d" % (cfg, ids, cov), when, part), {})[name] = h
    return {k: v for k, v in seen.items() if len(set(v.values())) > 1}


def _modules():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from stereo_vo_amd import hip, abi
    return hip, abi


def small():
    hip, abi = _modules()
    g = np.load(os.path.join(HERE, "oracle_small_seq.npz"))
    cam = abi.StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    return g, cam


def params(g, cfg, ids=0, change=None):
    hip, abi = _modules()
    det, nms, sm, ifm = cfg.split("_")
    p = abi.north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]) if det == "orb" else 300)
    p.detect_method = {"orb": abi.DM_ORB, "fastorb": abi.DM_FAST_ORB, "faster": abi.DM_FASTER}[det]
    if det != "orb":
        p.nOctaves = 2
    p.initial_FAST_threshold = 20
    p.non_maximal_suppression, p.nmsMethod = {"off": (0, 0), "std": (1, 0), "anms": (1, 1)}[nms]
    p.match_method = {"bf": abi.SM_DESC_BF, "rbr": abi.SM_DESC_RBR, "sad": abi.SM_SAD}[sm]
    p.ifm_method = {"bf": abi.IFM_DESC_BF, "win": abi.IFM_DESC_WIN, "sad": abi.IFM_SAD}[ifm]
    p.max_y_diff = 2.0
    p.ifm_win_w, p.ifm_win_h = 20, 30
    p.sad_max_distance = p.ifm_sad_max_distance = 800
    p.vo_use_matches_ids = ids
    for k, v in (change or {}).items():
        setattr(p, k, v)
    return p


def context(g, cam, p, cfg, kernel_times, cov=0):
    hip, _ = _modules()
    ctx = hip.Context(n_lanes=2, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=1024, max_cand=1 << 15, kernel_times=kernel_times,
                      max_octaves=1 if cfg.startswith("orb") else 2)
    ctx.set_params(p)
    ctx.set_camera(cam)
    if cov:
        ctx.set_pose_covariance(True)
    return ctx


def frame(ctx, g, t, shape):
    pairs = [(g["L%d" % ((t + l) % 4)], g["R%d" % ((t + l) % 4)]) for l in range(2)]
    if shape == "all":
        ctx.process_host(pairs)
    elif shape in ("split", "split_select"):
        x = SPLIT_AT_SELECT if shape == "split_select" else 0
        ctx.process_host(pairs, RUN_DETECT | NO_POST | x)
        ctx.run_stages(RUN_DETECT_POST | REST | x)
    elif shape == "ahead":
        ctx.process_host(pairs, RUN_DETECT | NO_POST | NO_SHIFT | AHEAD)
        ctx._process(None, RUN_DETECT_POST | REST | AHEAD, None)
    else:
        ctx.process_host(pairs, RUN_DETECT)
        for stage in (RUN_MATCH, RUN_TRACK, RUN_OPTIMIZE):
            ctx.run_stages(stage)


def outputs_hash(ctx, n_oct):
    """{part: hash over both lanes}: the result record and status word, and the lists of every octave"""
    parts = {k: hashlib.sha256() for k in ("record", "keypoints", "pairings", "tracked", "residuals")}
    for lane in range(2):
        parts["record"].update(bytes(ctx.result(lane))); parts["record"].update(b"%d" % ctx.status_word(lane))
        for o in range(n_oct):
            for which in (0, 1):
                for side in (0, 1):
                    k, d = ctx.keypoints(lane, which, side, o)
                    parts["keypoints"].update(k.tobytes()); parts["keypoints"].update(d.tobytes())
                parts["pairings"].update(ctx.matches(lane, which, o).tobytes())
            parts["tracked"].update(ctx.tracked(lane, o).tobytes())
        parts["residuals"].update(ctx.residuals(lane).tobytes()); parts["residuals"].update(ctx.outliers(lane).tobytes())
    return {k: h.hexdigest()[:16] for k, h in parts.items()}


def run_row(g, cam, row):
    cfg, shape, ids, cov, _ = row
    n_oct = 1 if cfg.startswith("orb") else 2
    p = params(g, cfg, ids)
    ctx = context(g, cam, p, cfg, True, cov)
    for t in range(2):
        if t == 1:
            ctx.kernel_times_reset()
        frame(ctx, g, t, shape)
    calls = {k: int(v[1]) for k, v in ctx.kernel_times(appended=True).items() if v[1]}
    sha = outputs_hash(ctx, n_oct)
    ctx.close()
    ctx = context(g, cam, p, cfg, False, cov)
    ctx.use_graphs(True)
    for t in range(4):
        frame(ctx, g, t, shape)
    graphs = list(ctx.graph_count())
    gsha = outputs_hash(ctx, n_oct)
    ctx.close()
    return {"calls": calls, "graphs": graphs, "sha": sha, "graph_sha": gsha}


def run_refusal(g, cam, ref):
    hip, abi = _modules()
    _, cfg, change, calls = ref
    p = params(g, cfg, 0, change)
    ctx = hip.Context(n_lanes=2, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=1024, max_cand=1 << 15, kernel_times=True, max_octaves=2)
    ctx.set_params(p); ctx.set_camera(cam)
    imgs = [np.ascontiguousarray(g[k]) for k in ("L0", "R0")]
    fr = (hip.Frame * 2)()
    for l in range(2):
        fr[l].left = hip.Image(imgs[0].ctypes.data, int(g["W"]), int(g["H"]), int(g["W"]))
        fr[l].right = hip.Image(imgs[1].ctypes.data, int(g["W"]), int(g["H"]), int(g["W"]))
    rc = 0
    for i, (flags, active) in enumerate(calls):
        if flags == "sad":                      # the stream switches to the SAD matchers: the frames it has were detected without windows
            p.match_method, p.ifm_method = abi.SM_SAD, abi.IFM_SAD
            ctx.set_params(p)
            continue
        if i == len(calls) - 1:
            ctx.kernel_times_reset()
        if active is None:
            rc = ctx.L.svo_process(ctx.h, fr, C.c_uint32(flags))
        else:
            w = hip.lane_mask_words(active, 2) + [0]
            rc = ctx.L.svo_process_lanes(ctx.h, fr, C.c_uint32(flags), (C.c_uint64 * 2)(w[0], w[1]))
        assert rc == 0 or i == len(calls) - 1, (ref[0], i, rc, ctx.L.svo_last_error(ctx.h))
    text = ctx.L.svo_last_error(ctx.h).decode()
    ctx.wait()
    enqueued = sum(int(v[1]) for v in ctx.kernel_times(appended=True).values())
    ctx.close()
    return {"rc": int(rc), "text": text, "enqueued": enqueued}


def census(rows=None, refusals=True):
    """every row with debug mode 0 (or the rows named), and the refusals, run in this process"""
    g, cam = small()
    out = {"rows": {}, "refusals": {}}
    for row in ROWS:
        if (rows is None and row[4] == 0) or (rows is not None and row_name(row) in rows):
            out["rows"][row_name(row)] = run_row(g, cam, row)
    if refusals:
        for ref in REFUSALS:
            out["refusals"][ref[0]] = run_refusal(g, cam, ref)
    return out


def census_with_children(env=None):
    """the whole census: the rows of every other debug mode each in a child process that has the mode in its environment"""
    out = census()
    for dbg in sorted({r[4] for r in ROWS if r[4]}):
        names = [row_name(r) for r in ROWS if r[4] == dbg]
        e = dict(env or os.environ, SVO_DEBUG_MODE=str(dbg))
        txt = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--rows", ",".join(names)], env=e, cwd=ROOT)
        out["rows"].update(json.loads(txt.decode().strip().splitlines()[-1])["rows"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD~1")
    ap.add_argument("--lib", default=None, help="a libsvo_hip.so built from the parent commit (skips the worktree)")
    ap.add_argument("--rows", default=None, help="(used by the census itself) run these rows in this process and print them as JSON")
    a = ap.parse_args()
    if a.rows is not None:
        print(json.dumps(census(set(a.rows.split(",")), refusals=False)))
        return
    if os.environ.get("SVO_CENSUS_RECORDING") != "1":         # first pass: find the parent's library, then record in a child that loads it
        lib = a.lib
        if lib is None:
            wt = os.path.join(ROOT, "build", "census_parent")
            if not os.path.isdir(wt):
                subprocess.check_call(["git", "-C", ROOT, "worktree", "add", "--detach", wt, a.parent])
            subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(wt, "stereo_vo_amd", "csrc"), "../libsvo_hip.so"])
            lib = os.path.join(wt, "stereo_vo_amd", "libsvo_hip.so")
        rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", a.parent]).decode().strip() if os.path.isdir(os.path.join(ROOT, ".git")) else a.parent
        env = dict(os.environ, SVO_HIP_LIB=os.path.abspath(lib), SVO_CENSUS_RECORDING="1", SVO_CENSUS_PARENT=rev)
        subprocess.check_call([sys.executable, os.path.abspath(__file__)], env=env, cwd=ROOT)
        return
    out = census_with_children()
    split = disagreements(out["rows"])
    for name, r in sorted(out["rows"].items()):
        print(name, r["sha"], r["graph_sha"])
    enqueued = {k: r.pop("enqueued") for k, r in out["refusals"].items()}
    for r in out["rows"].values():
        del r["sha"], r["graph_sha"]
    out = {"recorded_with": os.environ.get("SVO_CENSUS_PARENT", ""), "rows": out["rows"], "refusals": out["refusals"]}
    with open(os.environ.get("SVO_CENSUS_OUT", TABLE), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d rows and %d refusals" % (len(out["rows"]), len(out["refusals"])))
    # the parent must agree with itself before it is a table
    assert not split and not any(enqueued.values()), (split, enqueued)


if __name__ == "__main__":
    main()
