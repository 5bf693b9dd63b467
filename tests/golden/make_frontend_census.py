"""Writes tests/golden/frontend_census.json: what the entry points outside svo_process launch and list -- svo_lk_track, svo_gftt_detect,
the resident KLT front end with its top-up, RANSAC gate, prediction and stereo re-association -- recorded with the library of the PARENT
commit, so that a change that is meant to keep every launch, listing, status and refusal text of these calls (a refactor) can be held
to the table (tests/test_gpu_frontend_census.py, which imports the rows and the runner from here).

    python tests/golden/make_frontend_census.py [--parent REV]     (from the repository root, on the GPU; REV defaults to HEAD~1)
    python tests/golden/make_frontend_census.py --lib PATH         (a libsvo_hip.so of the parent that has been built elsewhere)

Each row is a fixed call sequence on a fresh context with kernel_times=True (two lanes, max_kps 1024, KLT cap 256) on the committed
small sequence, with points from a fixed grid:
    listing   every name Context.kernel_times(appended=True) returns, in order, zero counts included
    calls     {kernel name: calls}, the names that were launched
    facts     what the sequence returned besides arrays: statuses, modes, a listing taken half way
    sha       {part: hash} of what it produced -- klt_tracks of both lanes, the result records and status words, returned arrays
and each refusal the status and the text of a call that is refused before anything is enqueued.

The recorder runs every row twice with the parent's library.  It refuses to write a table in which the two runs differ in a listing, a
count, a fact or a refusal; a part of `sha` on which they differ is stored as null, and the test skips the comparison of that part."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "frontend_census.json")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_launch_census as M                                                          # noqa: E402

RUN_OPTIMIZE = M.RUN_OPTIMIZE
CAP, DISP = 256, 4.0
MAX_NULL_SHARE = 0.25
# every name svo_kernel_times can list, in its order
ALL_NAMES = ("begin_frame resize fast select describe nms_rowsort hamming_lr match_lr_filter hamming_track track_filter ransac_hyp ransac_count "
             "track_finalize gauss_newton ransac_hyp_1 ransac_count_1 ransac_hyp_2 ransac_count_2 sad_patch match_lr_sad track_sad select_8192 "
             "nms_rowsort_16 hamming_lr_wide hamming_track_wide track_filter_64 export_frame import_frame export_frame_win import_frame_win faster "
             "faster_nms gather_windows pose_covariance landmarks gftt_response gftt_candidates gftt_select lk_pyrdown lk_track klt_select klt_topup "
             "ransac_feed klt_prune klt_predict lk_track_row").split()


class Env:
    """the inputs every row shares: the sequence, its camera, the parameters, the grid"""
    def __init__(self):
        import torch                                        # (the device-image row: torch's HIP runtime has to be the first one loaded)
        assert torch.cuda.is_available()
        self.hip, self.abi = M._modules()
        self.g, self.cam = M.small()
        self.W, self.H = int(self.g["W"]), int(self.g["H"])
        p = self.abi.north_star_params(self.hip.default_params(), orb_nfeats=300)
        p.orb_nlevels = 2                                   # the detector's pyramid also fits the 128 x 96 crop
        self.params = p
        xs, ys = np.meshgrid(np.arange(16, self.W - 8, 16), np.arange(16, self.H - 8, 16))
        self.left = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)           # 15 x 11 points
        self.right = self.left - np.float32([DISP, 0])
        assert len(self.left) <= CAP

    def img(self, side, t):
        return self.g["%s%d" % (side, t % 4)]

    def ctx(self, set_params=True, w=None, h=None):
        c = self.hip.Context(n_lanes=2, max_w=w or self.W, max_h=h or self.H, max_kps=1024, max_cand=1 << 15, kernel_times=True)
        if set_params:
            c.set_params(self.params)
            c.set_camera(self.cam)
        return c

    def pairs(self, t, crop=False):
        """frame t of lane 0, frame t + 1 of lane 1; crop: the top-left 128 x 96 pixels"""
        cut = (lambda a: np.ascontiguousarray(a[:96, :128])) if crop else (lambda a: a)
        return [(cut(self.img("L", t + l)), cut(self.img("R", t + l))) for l in range(2)]

    def klt_params(self, cap=CAP, fb_max=0.0):
        p = self.hip.default_klt_params()
        p.cap, p.lk.fb_max = cap, fb_max
        return p

    def lk_params(self, **kw):
        p = self.hip.default_lk_params()
        for k, v in kw.items():
            setattr(p, k, v)
        return p


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def status_of(c, call):
    """(status, text) of the C call a Context method makes, where the method would raise on a refusal"""
    seen = []
    c._ck = lambda rc, what: (seen.append(int(rc)), rc)[1]
    try:
        call()
    finally:
        del c._ck
    return seen[-1], c.L.svo_last_error(c.h).decode()


def listing(c):
    return list(c.kernel_times(appended=True))


def finish(c, parts, facts=None, klt=True):
    """the row's record; klt: the tables and the records of both lanes are parts of the hash"""
    facts = dict(facts or {})
    if klt:
        tracks = [c.klt_tracks(lane) for lane in range(2)]
        parts = dict(parts, tracks=sha(*flat(tracks)))
        facts["n_tracks"] = [int(len(t[2])) for t in tracks]
    parts = dict(parts, record=sha(*[x for lane in range(2) for x in (bytes(c.result(lane)), b"%d" % c.status_word(lane))]))
    kt = c.kernel_times(appended=True)
    c.close()
    return {"listing": list(kt), "calls": {k: int(v[1]) for k, v in kt.items() if v[1]}, "facts": facts, "sha": parts}


def flat(results):
    return [a for res in results for a in res]


# ---- svo_lk_track, svo_lk_track_rows, svo_gftt_detect ------------------------------------------------------------------------------
def lk_jobs(E, nxt="L"):
    n = 50
    return [(E.img("L", 0), E.img(nxt, 1 if nxt == "L" else 0), E.left),
            (E.img("L", 1), E.img(nxt, 2 if nxt == "L" else 1), E.left[:n], E.left[:n] + np.float32([1.0, -0.5]))]


def row_lk(E, fb_max=0.0, rows=False, device=False):
    c = E.ctx()
    jobs, keep = lk_jobs(E, "R" if rows else "L"), []
    if device:
        import torch
        keep = [[torch.from_numpy(np.ascontiguousarray(im)).cuda() for im in j[:2]] for j in jobs]
        torch.cuda.synchronize()
        jobs = [tuple((t.data_ptr(), E.W, E.H, E.W) for t in ts) + tuple(j[2:]) for ts, j in zip(keep, jobs)]
    got = (c.lk_track_rows if rows else c.lk_track)(jobs, E.lk_params(fb_max=fb_max), device=device)
    lv = c.lk_level(1, 1, 1)
    return finish(c, {"arrays": sha(*flat(got)), "level": sha(lv)}, {"level": list(lv.shape), "no_such_job": c.lk_level(2, 0, 0) is None}, klt=False)


def row_lk_grow(E):
    c = E.ctx()
    first = c.lk_track([(E.img("L", 0), E.img("L", 1), E.left[:20])])
    second = c.lk_track(lk_jobs(E))                          # more jobs, more points, two more images: every buffer grows
    return finish(c, {"first": sha(*flat(first)), "second": sha(*flat(second))}, klt=False)


def row_gftt(E, seeds, cap=100):
    c = E.ctx()
    got = c.gftt_detect([(E.img("L", 0), E.left[:40] if seeds else None), (E.img("R", 1), None, cap)])
    resp = c.gftt_response(1)
    facts = {"n": [int(len(r[0])) for r in got], "n_cand": [r[2] for r in got], "status": [r[3] for r in got]}
    return finish(c, {"arrays": sha(*[a for r in got for a in r[:2]]), "response": sha(resp)}, facts, klt=False)


# ---- the resident KLT front end ------------------------------------------------------------------------------------------------------
def klt_ctx(E, fb_max=0.0, ransac=0, predict=0, stereo=0, add=True):
    c = E.ctx()
    c.klt_enable(E.klt_params(fb_max=fb_max))
    if ransac:
        c.klt_set_ransac(ransac)
    if predict:
        c.klt_set_prediction(predict)
    if stereo:
        c.klt_set_stereo(stereo)
    if add:
        for lane in range(2):
            assert c.klt_add_points(lane, E.left, E.right) == len(E.left)
    return c


def row_klt(E, flags=RUN_OPTIMIZE, active=None, steps=3, crop_third=False, **modes):
    c = klt_ctx(E, **modes)
    for t in range(steps):
        c.klt_step(E.pairs(t, crop_third and t == 2), flags, active)
    return finish(c, {})


def row_topup_sequence(E):
    c = klt_ctx(E)
    c.klt_topup_enable(below=CAP, target=CAP)               # every lane short of a full table counts as thinned
    c.klt_step(E.pairs(0)); c.klt_topup(); c.klt_step(E.pairs(1))
    return finish(c, {"info": sha(*[np.int32(c.klt_topup_info(lane)) for lane in range(2)])})


def row_topup_before_a_step(E):
    c = klt_ctx(E)
    c.klt_topup_enable()
    c.klt_topup([0])
    return finish(c, {}, {"info": [list(c.klt_topup_info(lane)) for lane in range(2)]})


def row_topup_debug_append(E):
    c = klt_ctx(E, add=False)
    c.klt_topup_enable()
    n = 60
    c.klt_debug_topup_append(1, E.left[:n], E.right[:n], (np.arange(n) % 7 != 0).astype(np.uint8))
    return finish(c, {}, {"info": [list(c.klt_topup_info(lane)) for lane in range(2)]})


def row_topup_info(E):
    c = klt_ctx(E)
    p = c.klt_topup_enable(below=200, target=240)
    return finish(c, {}, {"info": [list(c.klt_topup_info(lane)) for lane in range(2)], "params": [p.below, p.target]})


def row_ransac_tracked(E):
    import ransac_tracked_scenes as RS
    c = E.ctx()
    for lane, name in enumerate(("planted_64_10", "planted_40_8")):
        RS.put_case(c, lane, RS.case(name))
    c.ransac_tracked()
    return finish(c, {"tracked": sha(*[c.tracked(lane) for lane in range(2)])}, klt=False)


def row_predicted(E, forced):
    c = klt_ctx(E, predict=1)
    c.klt_step(E.pairs(0)); c.klt_step(E.pairs(1))
    delta = [0.01, -0.02, 0.005, 0.05, -0.02, 0.1]
    got = [c.debug_klt_predict(lane, delta, 1) if forced else c.klt_predicted(lane) for lane in range(2)]
    return finish(c, {"guesses": sha(*flat(got))}, {"n": [int(len(r[0])) for r in got]})


def row_debug_select(E):
    c = klt_ctx(E, add=False)
    c.klt_step(E.pairs(0), 0)                               # a step gives the context its geometry
    assert c.klt_add_points(0, E.left, E.right) == len(E.left)
    n = len(E.left)
    ok = (np.arange(n) % 5 != 0).astype(np.uint8)
    c.klt_debug_select(0, E.left + np.float32([1, 0]), E.right + np.float32([1, 0]), ok, ok[::-1].copy())
    return finish(c, {})


def row_reset_then_step(E):
    c = klt_ctx(E)
    c.klt_step(E.pairs(0))
    c.klt_reset([1])
    c.klt_step(E.pairs(1))
    return finish(c, {})


def row_reenable(E):
    """what a reallocation forgets: the marks behind klt_select, klt_topup and klt_prune until their next launch, the prediction and
    the stereo mode with their buffers -- and what it keeps: the other marks and the RANSAC mode"""
    c = klt_ctx(E, ransac=2, predict=1, stereo=1)
    c.klt_topup_enable(below=CAP, target=CAP)
    c.klt_step(E.pairs(0)); c.klt_topup(); c.klt_step(E.pairs(1))
    facts = {"before_reset": listing(c), "modes_before": [c.klt_ransac(), c.klt_prediction(), c.klt_get_stereo()]}
    c.klt_reset()
    c.klt_enable(E.klt_params(cap=128))
    facts["after_enable"] = listing(c)
    facts["modes_after"] = [c.klt_ransac(), c.klt_prediction(), c.klt_get_stereo()]
    for lane in range(2):
        assert c.klt_add_points(lane, E.left[:128], E.right[:128]) == 128
    c.klt_step(E.pairs(2))
    return finish(c, {}, facts)


def row_select_names(E):
    c = E.ctx()
    facts = {"status": {name: status_of(c, lambda: c.kernel_times_select(name))[0] for name in ALL_NAMES + ["no_such_kernel"]}}
    c.kernel_times_select("lk_track")                       # ... and one selection at work: the tracking launches alone are timed
    c.lk_track(lk_jobs(E))
    c.kernel_times_select(None)
    return finish(c, {}, facts, klt=False)


ROWS = {
    "lk_track/fb0": lambda E: row_lk(E),
    "lk_track/fb": lambda E: row_lk(E, fb_max=0.05),
    "lk_track_rows": lambda E: row_lk(E, rows=True),
    "lk_track_rows/fb": lambda E: row_lk(E, fb_max=0.05, rows=True),
    "lk_track/device": lambda E: row_lk(E, device=True),
    "lk_track/grow": row_lk_grow,
    "gftt_detect/no_seeds": lambda E: row_gftt(E, False),
    "gftt_detect/seeds": lambda E: row_gftt(E, True),
    "gftt_detect/cap_0": lambda E: row_gftt(E, False, cap=0),         # room for no corner is a valid job: the candidates are counted
    "klt/off": lambda E: row_klt(E),
    "klt/fb": lambda E: row_klt(E, fb_max=1.0),
    "klt/ransac1": lambda E: row_klt(E, ransac=1),
    "klt/ransac2": lambda E: row_klt(E, ransac=2),
    "klt/predict1": lambda E: row_klt(E, predict=1),
    "klt/stereo1": lambda E: row_klt(E, stereo=1),
    "klt/stereo1_fb": lambda E: row_klt(E, stereo=1, fb_max=1.0),
    "klt/all_modes": lambda E: row_klt(E, ransac=2, predict=1, stereo=1),
    "klt/flags0": lambda E: row_klt(E, flags=0),
    "klt/ransac1_flags0": lambda E: row_klt(E, flags=0, ransac=1),
    "klt/lane1_out": lambda E: row_klt(E, active=[0]),
    "klt/first_step_only": lambda E: row_klt(E, steps=1),
    "klt/size_change": lambda E: row_klt(E, crop_third=True),
    "klt/size_change_predict": lambda E: row_klt(E, crop_third=True, predict=1),
    "topup/step_topup_step": row_topup_sequence,
    "topup/before_a_step": row_topup_before_a_step,
    "topup/debug_append": row_topup_debug_append,
    "topup/info": row_topup_info,
    "ransac_tracked/put_lists": row_ransac_tracked,
    "klt_predicted": lambda E: row_predicted(E, False),
    "debug_klt_predict": lambda E: row_predicted(E, True),
    "klt_debug_select": row_debug_select,
    "klt_reset/mask_then_step": row_reset_then_step,
    "klt/reenable": row_reenable,
    "kernel_times_select": row_select_names,
}


# ---- refusals: (context, the refused call) -------------------------------------------------------------------------------------------
def _held(E):
    c = klt_ctx(E)
    return c, lambda: c.klt_enable(E.klt_params(cap=128))


def _wrong_count(E):
    c = klt_ctx(E, add=False)
    c.klt_step(E.pairs(0), 0)
    c.klt_add_points(0, E.left[:10], E.right[:10])
    one = np.ones(5, np.uint8)
    return c, lambda: c.klt_debug_select(0, E.left[:5], E.right[:5], one, one)


def _enabled(E, call):
    c = klt_ctx(E)
    return c, lambda: call(c)


def _unenabled_step(E):
    c = E.ctx()
    return c, lambda: c.klt_step(E.pairs(0))


def _no_params_step(E):
    c = E.ctx(set_params=False)
    c.klt_enable(E.klt_params())
    return c, lambda: c.klt_step(E.pairs(0))


def _even_win(E):
    c = E.ctx()
    return c, lambda: c.lk_track(lk_jobs(E), E.lk_params(win=20))


def _gftt_negative_cap(E):
    c = E.ctx()
    return c, lambda: c.gftt_detect([(E.img("L", 0), None, -1)])


REFUSALS = {
    "klt_step_before_enable": _unenabled_step,
    "klt_step_before_set_params": _no_params_step,
    "klt_enable_other_params_with_tracks": _held,
    "klt_set_prediction_unknown_mode": lambda E: _enabled(E, lambda c: c.klt_set_prediction(7)),
    "klt_set_stereo_unknown_mode": lambda E: _enabled(E, lambda c: c.klt_set_stereo(7)),
    "klt_set_ransac_unknown_mode": lambda E: _enabled(E, lambda c: c.klt_set_ransac(7)),
    "klt_topup_before_topup_enable": lambda E: _enabled(E, lambda c: c.klt_topup()),
    "klt_add_points_lane_out_of_range": lambda E: _enabled(E, lambda c: c.klt_add_points(2, E.left, E.right)),
    "lk_track_even_win": _even_win,
    "gftt_detect_negative_cap": _gftt_negative_cap,
    "klt_debug_select_wrong_count": _wrong_count,
}


def run_refusal(E, make):
    c, call = make(E)
    c.kernel_times_reset()
    rc, text = status_of(c, call)
    c.wait()
    enqueued = sum(int(v[1]) for v in c.kernel_times(appended=True).values())
    c.close()
    return {"rc": rc, "text": text, "enqueued": enqueued}


def census():
    """every row and refusal, run once in this process; a call that fails where it should not is recorded as the row's "error" """
    E = Env()
    out = {"rows": {}, "refusals": {}}
    for kind, table, run in (("rows", ROWS, lambda f: f(E)), ("refusals", REFUSALS, lambda f: run_refusal(E, f))):
        for name, f in table.items():
            try:
                out[kind][name] = run(f)
            except (E.hip.SvoError, AssertionError, RuntimeError) as e:
                out[kind][name] = {"error": "%s: %s" % (type(e).__name__, e)}
    return out


def null_share(rows):
    parts = [h for r in rows.values() for h in r["sha"].values()]
    return sum(h is None for h in parts) / float(max(1, len(parts)))


def merge(a, b):
    """the table of two runs of one library: (table, what the runs disagree on besides a hash)"""
    split = []
    for kind in ("rows", "refusals"):
        for name in a[kind]:
            x, y = a[kind][name], b[kind][name]
            if "error" in x or "error" in y:
                split.append((name, x.get("error"), y.get("error")))
            elif kind == "refusals":
                if x != y or x["enqueued"] or x["rc"] >= 0:
                    split.append((name, x, y))
            else:
                split += [(name, key, x[key], y[key]) for key in ("listing", "calls", "facts") if x[key] != y[key]]
                x["sha"] = {part: (h if y["sha"].get(part) == h else None) for part, h in x["sha"].items()}
    return a, split


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="HEAD~1")
    ap.add_argument("--lib", default=None, help="a libsvo_hip.so built from the parent commit (skips the worktree)")
    a = ap.parse_args()
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
    out, split = merge(census(), census())
    for name, r in sorted(out["rows"].items()):
        print(name, r.get("error") or (r["calls"], r["sha"]))
    for name, r in sorted(out["refusals"].items()):
        print(name, r)
    # the parent must agree with itself before it is a table
    assert not split, split
    share = null_share(out["rows"])
    assert share <= MAX_NULL_SHARE, "%.2f of the hashed parts differ between two runs of the parent" % share
    for r in out["refusals"].values():
        del r["enqueued"]
    out = {"recorded_with": os.environ.get("SVO_CENSUS_PARENT", ""), "rows": out["rows"], "refusals": out["refusals"]}
    with open(os.environ.get("SVO_CENSUS_OUT", TABLE), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d rows and %d refusals, %.2f of the hashed parts null" % (len(out["rows"]), len(out["refusals"]), share))


if __name__ == "__main__":
    main()
