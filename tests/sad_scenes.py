"""Images and lists built by hand for the SAD matchers: smSAD = k_match_lr_rbr<true> (stage 3) and ifmSAD = k_track_win<true> (stage 4)
(numpy only: no GPU; the oracle is imported by trk_octaves alone, for its pyramid).  In the style of tests/match_scenes.py, whose _kps,
features_row_index and matches_row_index are reused, with every list closed by a keypoint on a later row ("last row").

Windows are made on purpose.  `pattern(s)`, 0 <= s <= 16320, is the 8 x 8 window whose first s // 255 bytes are 255, the next one s % 255
and the rest 0: of two such windows the one of the larger level is the larger in every byte, so their SAD is exactly the difference of
the two levels.  Every keypoint of interest owns the window [x-3, x+4] x [y-3, y+4] at (int)pt of its image, painted with the pattern of
its level (`paint` asserts that no two windows of an image overlap); a keypoint whose window would leave the image is not painted.  So
every SAD that matters is |level - level|, known before any walk is run.

A stage-3 scene is a dict: kl kr (ascending (y, x)), imgs (left, right), W H, `variants` (parameter settings next to
enable_robust_1to1_match), `label` per left keypoint, `plan` per left keypoint -- the right keypoints the CONSTRUCTION makes its
candidates, [(right index, SAD, condition on the variant or None)] -- and `want(variant, robust)`: the pairings [(left, right, SAD)]
that follow from the plan alone (expected_stereo: no image, no window and no row table is read).  A stage-4 scene holds both frames
(pkl pkr pm pimgs pri / ckl ckr cm cimgs cri), `label` and `plan` per previous pairing ([(current pairing, sad_l, sad_r, condition)])
and `want(variant)`: the candidate pairs [(previous, current)].  Pairing k of a frame joins keypoint k of both its lists; the motion is
sideways (every keypoint moves along its own row), so the RANSAC keeps every candidate; the scenes that move a keypoint to another row
stay under eight candidates, where the masks are not applied.
tests/test_sad_scenes_cpu.py holds tests/sad_ref.py to `want` and shows that every rule, broken on purpose, changes a scene;
tests/test_gpu_sad_scenes.py runs the scenes on the kernels."""
import functools
import math

import numpy as np

from stereo_vo_amd.abi import dmatch_dtype

import match_scenes as MS
from match_scenes import _kps, features_row_index, matches_row_index                  # noqa: F401

W, H = 160, 96                                     # every one-octave scene: the lanes of one context
NEAR = 2.0 ** -10
BANDS = [4 + 8 * k for k in range(11)]             # rows 4 .. 84: one cell of interest per band, no window or row range reaches a neighbour's
NO_TH = 0xFFFFFFFF


def pattern(level):
    assert 0 <= level <= 16320
    q, r = divmod(int(level), 255)
    a = np.zeros(64, np.uint8)
    a[:q] = 255
    if q < 64:
        a[q] = r
    return a.reshape(8, 8)


def is_flagged(x, y, w, h):
    """the border rule of S3:289-295 in binary32, as svo_gather_windows applies it"""
    x, y = np.float32(x), np.float32(y)
    return bool(x < np.float32(3) or y < np.float32(3) or x > np.float32(w - 5) or y > np.float32(h - 5))


def paint(w, h, pts):
    """pts: [(x, y, level)] -> the image; windows at (int)pt, disjoint (the same window twice must carry the same level)"""
    img, own = np.zeros((h, w), np.uint8), {}
    for x, y, level in pts:
        if is_flagged(x, y, w, h):
            continue
        xi, yi = int(np.float32(x)), int(np.float32(y))
        for (ox, oy), lv in own.items():
            assert (ox, oy) == (xi, yi) and lv == level or abs(ox - xi) >= 8 or abs(oy - yi) >= 8, ("windows overlap", (ox, oy), (xi, yi))
        own[(xi, yi)] = level
        img[yi - 3:yi + 5, xi - 3:xi + 5] = pattern(level)
    return img


def threshold(field):
    """sad_max_distance / ifm_sad_max_distance as the reference reads the field: 0 = 200, negative = none"""
    return 200 if field == 0 else NO_TH if field < 0 else field


def c_round(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def _order(pts):
    a = np.array(pts, np.float32).reshape(-1, 2)
    return np.lexsort((a[:, 0], a[:, 1])), a


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------------------------------
STEREO_DEFAULTS = dict(sad_max_distance=0, max_y_diff=1.0, minimum_ORB_response=0.0)


def L(x, y, lvl, label, cands=(), resp=1.0):
    """a left keypoint; cands: [(key of a right keypoint, SAD) or (key, SAD, condition(variant))]"""
    return dict(x=x, y=y, lvl=lvl, label=label, cands=[c if len(c) == 3 else (c[0], c[1], None) for c in cands], resp=resp)


def R(key, x, y, lvl, resp=1.0):
    return dict(key=key, x=x, y=y, lvl=lvl, resp=resp)


def expected_stereo(s, variant, robust):
    """what smSAD leaves of a scene, from the plan alone: every left keypoint takes its candidate of the smallest SAD within the
    threshold, the first in list order among equals (S3:334-345); a right keypoint goes to its first claimant or, with the robust
    rule, to its best one, the first among equals, and a loser gets nothing else (S3:357-387)"""
    v = dict(STEREO_DEFAULTS, **variant)
    th = threshold(v["sad_max_distance"])
    owner = {}
    for i, plan in enumerate(s["plan"]):
        c = [(d, j) for j, d, cond in plan if (cond is None or cond(v)) and d <= th]
        if not c:
            continue
        d, j = min(c)
        if j not in owner or (robust and d < owner[j][1]):
            owner[j] = (i, d)
    return sorted((i, j, d) for j, (i, d) in owner.items())


def _stereo(left, right, variants, w=W, h=H):
    left = left + [L(10.0, h - 3.0, 0, "last row")]                                # the closers: the row tables never visit the last populated row
    right = right + [R("last", 5.0, h - 1.0, 0)]
    ol, pl = _order([(e["x"], e["y"]) for e in left]); orr, pr = _order([(e["x"], e["y"]) for e in right])
    kl, kr = _kps(pl[ol]), _kps(pr[orr])
    kl["response"] = np.array([left[i]["resp"] for i in ol], np.float32); kr["response"] = np.array([right[i]["resp"] for i in orr], np.float32)
    at = {right[j]["key"]: pos for pos, j in enumerate(orr)}
    assert len(at) == len(right)
    plan = []
    for i in ol:
        e = left[i]
        plan.append(sorted((at[k], d, cond) for k, d, cond in e["cands"]))
        for k, d, _ in e["cands"]:                                                 # a planned SAD is the difference of the two levels
            r = right[[q["key"] for q in right].index(k)]
            assert d == abs(e["lvl"] - r["lvl"]) and not is_flagged(e["x"], e["y"], w, h) and not is_flagged(r["x"], r["y"], w, h), (e["label"], k)
    s = dict(kl=kl, kr=kr, W=w, H=h, variants=variants, label=[left[i]["label"] for i in ol], plan=plan, right_at=at,
             imgs=(paint(w, h, [(e["x"], e["y"], e["lvl"]) for e in left]), paint(w, h, [(e["x"], e["y"], e["lvl"]) for e in right])))
    s["want"] = functools.partial(expected_stereo, s)
    return s


THRESHOLD_DS = [0, 1, 2, 199, 200, 201, 255, 256, 16319, 16320]                    # th - 1, th, th + 1 for th = 1, 200 (and 16320), 8 bits, 14 bits
THRESHOLD_FIELDS = [0, 1, 200, 16320, -1]


def sad_threshold():
    """one pair per planted SAD, each on a row band of its own: kept iff d <= threshold, DMatch.distance = d"""
    left = [L(148.0, BANDS[k], 0, "d=%d" % d, [(k, d)]) for k, d in enumerate(THRESHOLD_DS)]
    right = [R(k, 100.0, BANDS[k], d) for k, d in enumerate(THRESHOLD_DS)]
    return _stereo(left, right, [dict(sad_max_distance=f) for f in THRESHOLD_FIELDS])


def sad_ties():
    """candidates of equal SAD (the first in list order wins, also behind a worse one) and pairs of SAD 90 and 100, either way round:
    min_1 / min_2 = 0.9 exceeds sad_max_ratio 0.5 and the best is kept all the same (S3:347-349 skips a print)"""
    b = BANDS
    left = [L(148.0, b[0], 0, "tie of two", [("a0", 64), ("a1", 64)]), L(148.0, b[1], 128, "tie of three", [("b0", 64), ("b1", 64), ("b2", 64)]),
            L(148.0, b[2], 0, "tie behind a worse one", [("c0", 100), ("c1", 64), ("c2", 64)]),
            L(148.0, b[3], 0, "ratio 0.9, best first", [("d0", 90), ("d1", 100)]), L(148.0, b[4], 0, "ratio 0.9, best second", [("e0", 100), ("e1", 90)])]
    right = [R("a0", 60.0, b[0], 64), R("a1", 100.0, b[0], 64), R("b0", 40.0, b[1], 64), R("b1", 80.0, b[1], 192), R("b2", 120.0, b[1], 64),
             R("c0", 40.0, b[2], 100), R("c1", 80.0, b[2], 64), R("c2", 120.0, b[2], 64),
             R("d0", 60.0, b[3], 90), R("d1", 100.0, b[3], 100), R("e0", 60.0, b[4], 100), R("e1", 100.0, b[4], 90)]
    return _stereo(left, right, [{}])


CLAIMS = [(300, 299), (256, 255), (299, 300), (77, 77)]


def sad_one_to_one():
    """two left keypoints of one row claiming one right keypoint (threshold 400).  The SADs of the first two couples differ above bit 8
    only in the order they have: a key that kept 8 bits of the distance would rank them the other way round.  In the last band the
    loser has a second candidate that nobody else wants, and must not get it."""
    left, right = [], []
    for k, (a, b) in enumerate(CLAIMS):
        r = BANDS[k]
        right.append(R(k, 60.0, r, 0))
        left += [L(120.0, r, a, "claim %d/%d first" % (a, b), [(k, a)]), L(148.0, r, b, "claim %d/%d second" % (a, b), [(k, b)])]
    r = BANDS[len(CLAIMS)]
    right += [R("r", 60.0, r, 0), R("alt", 20.0, r, 700)]
    left += [L(120.0, r, 300, "second choice: first", [("r", 300), ("alt", 400)]), L(148.0, r, 299, "second choice: second", [("r", 299), ("alt", 401)])]
    return _stereo(left, right, [dict(sad_max_distance=400)])


def sad_border():
    """keypoints on 3 and W - 5 / H - 5 (they have a window) and on 2.99 and W - 4.99 / H - 4.99 (flagged: a flagged left keypoint never
    pairs, a flagged right one is passed over); fractional coordinates take the window at (int)pt: a left window of 255s against a
    right keypoint at (10.99, 60.99), and a left keypoint at (60.99, 77.99), are at SAD 200 = the threshold only for the windows at
    (10, 60) and (60, 77) -- one pixel off, a row and a column of the 255s meet the black background"""
    b = BANDS
    left = [L(148.0, 3.0, 0, "left y=3", [("t1", 10)]), L(120.0, 2.99, 0, "left y=2.99 flagged"),
            L(W - 5.0, b[1], 0, "left x=W-5", [("x1", 30)]), L(W - 4.99, b[2], 0, "left x=W-4.99 flagged"),
            L(30.0, b[3], 0, "right x=3", [("x3", 40)]), L(30.0, b[4], 0, "flagged right passed over for the second best", [("x5", 50)]),
            L(W - 2.0, b[5], 0, "right x=W-5 and W-4.99 under a flagged left"),
            L(3.0, b[6], 0, "left x=3: its only candidate is flagged"), L(2.99, b[6] + 1.0, 0, "left x=2.99 flagged"),
            L(60.0, 61.0, 16320, "fractional right", [("f", 200)]), L(60.99, 77.99, 16320, "fractional left", [("g", 200)]),
            L(148.0, H - 5.0, 0, "left y=H-5", [("b1", 20)]), L(120.0, H - 4.99, 0, "left y=H-4.99 flagged")]
    right = [R("t1", 100.0, 3.0, 10), R("t2", 60.0, 2.99, 0), R("x1", 100.0, b[1], 30), R("x2", 100.0, b[2], 0), R("x3", 3.0, b[3], 40),
             R("x4", 2.99, b[4], 0), R("x5", 12.0, b[4], 50), R("x6", W - 5.0, b[5], 0), R("x7", W - 4.99, b[5] + 1.0, 0), R("x8", 2.0, b[6], 0),
             R("f", 10.99, 60.99, 16120), R("g", 10.0, 77.0, 16120),
             R("b1", 100.0, H - 5.0, 20), R("b2", 60.0, H - 4.99, 0)]
    return _stereo(left, right, [{}, dict(max_y_diff=2.5)])


MAX_DISPARITY = int(W * 0.7)


def sad_disparity():
    """kl.x - kr.x around the limits 1 and (int)(0.7 W) of S3:283-285: match_scenes.dxs on the SAD instantiation.  Every pair is at SAD 200"""
    left, right = [], []
    for k, dx in enumerate(MS.dxs(MAX_DISPARITY)):
        ok = 1 <= int(dx) <= MAX_DISPARITY
        left.append(L(150.0, BANDS[k], 0, "dx=%r %s" % (dx, "kept" if ok else "dropped"), [(k, 200)] if ok else []))
        right.append(R(k, 150.0 - dx, BANDS[k], 200))
    return _stereo(left, right, [{}])


ROW_OFFSETS = [-3, -2, -1, 0, 1, 2, 3]
Y_DIFFS = [0.49, 0.5, 1.5, 2.5]                                                    # C round(): 0 1 2 3; Python's: 0 0 2 2


def sad_rows():
    """a right keypoint `off` rows from its left one: with d = round(max_y_diff), half away from zero, the left keypoints of row r meet
    the right ones of rows r - d .. r + d - 1 (S3:250-256; d = 0: nobody)"""
    left, right = [], []
    for k, off in enumerate(ROW_OFFSETS):
        r = BANDS[1 + k]
        left.append(L(148.0, r, 0, "off=%d" % off, [(k, 7, lambda v, off=off: -c_round(v["max_y_diff"]) <= off <= c_round(v["max_y_diff"]) - 1)]))
        right.append(R(k, 40.0 + 12 * k, r + off, 7))
    return _stereo(left, right, [dict(max_y_diff=v) for v in Y_DIFFS])


def sad_response():
    """ORB mode: responses on and one ulp under minimum_ORB_response 0.5, on either side (S3:279: `<` rejects)"""
    under = float(np.nextafter(np.float32(0.5), np.float32(0)))
    left, right = [], []
    for k, (rl, rr) in enumerate([(0.5, 0.5), (under, 0.5), (0.5, under), (1.0, 1.0)]):
        left.append(L(148.0, BANDS[k], 0, "response %s %s" % tuple("above" if r > 0.5 else "on" if r == 0.5 else "under" for r in (rl, rr)),
                      [(k, 9, lambda v, m=min(rl, rr): m >= v["minimum_ORB_response"])], resp=rl))
        right.append(R(k, 100.0, BANDS[k], 9, resp=rr))
    return _stereo(left, right, [{}, dict(minimum_ORB_response=0.5)])


def stereo_params(p, variant, robust):
    """the parameter record of a stage-3 variant: smSAD in ORB mode (one octave, minimum_ORB_response in force)"""
    q = p.copy()
    q.detect_method, q.match_method, q.enable_robust_1to1_match = 0, 2, robust
    for k, v in dict(STEREO_DEFAULTS, **variant).items():
        setattr(q, k, v)
    return q


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------------------------------------------------------------------
TRACK_DEFAULTS = dict(ifm_sad_max_distance=0, ifm_win_w=2, ifm_win_h=12)
XS = [32.0, 64.0, 96.0, 128.0]                    # left x of the four cells of a band; right x = left x - 20; both frames' keypoints of a cell stay within +-8 of it (ifm_win_h = 12)


def P(xl, y, xr, ll, lr, label, cands=(), yr=None):
    """a previous pairing: left (xl, y) and right (xr, yr or y) keypoints with their levels; cands: [(key of a current pairing, sad_l,
    sad_r) or (.., condition(variant))]"""
    return dict(xl=xl, y=y, xr=xr, yr=y if yr is None else yr, ll=ll, lr=lr, label=label, cands=[c if len(c) == 4 else (c[0], c[1], c[2], None) for c in cands])


def Cu(key, xl, y, xr, ll, lr, yr=None):
    return dict(key=key, xl=xl, y=y, xr=xr, yr=y if yr is None else yr, ll=ll, lr=lr)


def expected_track(s, variant):
    """what ifmSAD's front end leaves, from the plan alone: a previous pairing takes the candidate of the smallest sad_l + sad_r among
    those with sad_l <= T and sad_r <= T, the first among equals (S4:572-587); a current pairing keeps its claimant of the smallest
    sum, the first among equals (S4:622-636).  -> [(previous, current)], ascending in the current index"""
    v = dict(TRACK_DEFAULTS, **variant)
    th = threshold(v["ifm_sad_max_distance"])
    owner = {}
    for pi, plan in enumerate(s["plan"]):
        c = [(a + b, ci) for ci, a, b, cond in plan if (cond is None or cond(v)) and a <= th and b <= th]
        if not c:
            continue
        sm, ci = min(c)
        if ci not in owner or sm < owner[ci][1]:
            owner[ci] = (pi, sm)
    return sorted(((pi, ci) for ci, (pi, _) in owner.items()), key=lambda t: t[1])


def _identity(n):
    m = np.zeros(n, dmatch_dtype); m["queryIdx"] = np.arange(n); m["trainIdx"] = np.arange(n); m["imgIdx"] = -1; m["distance"] = 10.0
    return m


def _frame(entries, w, h):
    """one frame of a stage-4 scene: pairing k = keypoint k of both lists, in ascending (y, xl) order, one unpaired closer per list"""
    o, _ = _order([(e["xl"], e["y"]) for e in entries])
    es = [entries[i] for i in o]
    kl = _kps(np.array([(e["xl"], e["y"]) for e in es] + [(10.0, h - 2.0)], np.float32))
    kr = _kps(np.array([(e["xr"], e["yr"]) for e in es] + [(5.0, h - 1.0)], np.float32))
    assert (np.diff(kr["y"].astype(np.int64)) >= 0).all(), "right list out of row order"
    m = _identity(len(es))
    imgs = (paint(w, h, [(e["xl"], e["y"], e["ll"]) for e in es]), paint(w, h, [(e["xr"], e["yr"], e["lr"]) for e in es]))
    return es, dict(kl=kl, kr=kr, m=m, imgs=imgs, ri=matches_row_index(m, kl, h))


def _track(prev, cur, variants, w=W, h=H):
    pes, pf = _frame(prev, w, h); ces, cf = _frame(cur, w, h)
    at = {e["key"]: i for i, e in enumerate(ces)}
    assert len(at) == len(ces)
    plan = []
    for e in pes:
        plan.append(sorted((at[k], a, b, cond) for k, a, b, cond in e["cands"]))
        for k, a, b, _ in e["cands"]:
            c = ces[at[k]]
            assert (a, b) == (abs(e["ll"] - c["ll"]), abs(e["lr"] - c["lr"])), (e["label"], k)
            assert not any(is_flagged(x, y, w, h) for x, y in ((e["xl"], e["y"]), (e["xr"], e["yr"]), (c["xl"], c["y"]), (c["xr"], c["yr"]))), (e["label"], k)
    s = dict(pkl=pf["kl"], pkr=pf["kr"], pm=pf["m"], pimgs=pf["imgs"], pri=pf["ri"], ckl=cf["kl"], ckr=cf["kr"], cm=cf["m"], cimgs=cf["imgs"], cri=cf["ri"],
             W=w, H=h, variants=variants, label=[e["label"] for e in pes], plan=plan, cur_at=at)
    s["want"] = functools.partial(expected_track, s)
    return s


def frames(s):
    """(previous, current) as tests/sad_ref.py's track_sad and filter_candidates take them"""
    return (dict(imgs=s["pimgs"], kl=s["pkl"], kr=s["pkr"], m=s["pm"], ri=s["pri"]), dict(imgs=s["cimgs"], kl=s["ckl"], kr=s["ckr"], m=s["cm"], ri=s["cri"]))


def _cell(k):
    return XS[k % 4], BANDS[k // 4]


GATE_FIELDS = [0, 300, 16320, -1]


def trk_gates():
    """per threshold T = 200, 300: a candidate at (sad_l, sad_r) = (T, T) (kept), at (T + 1, 0) and at (0, T + 1) (dropped), and (0, T + 1)
    ahead of (T - 100, T - 100): the second wins although its sum is the larger at T = 300; one candidate at (16320, 16320)"""
    prev, cur = [], []
    k = 0

    def cell(label, cands):
        nonlocal k
        x, y = _cell(k)
        offs = [8.0] if len(cands) == 1 else [-8.0, 8.0]
        prev.append(P(x, y, x - 20, 0, 0, label, [("%d.%d" % (k, i), a, b) for i, (a, b) in enumerate(cands)]))
        cur.extend(Cu("%d.%d" % (k, i), x + o, y, x - 20 + o, a, b) for i, ((a, b), o) in enumerate(zip(cands, offs)))
        k += 1
    for T in (200, 300):
        cell("T=%d (T, T)" % T, [(T, T)]); cell("T=%d (T+1, 0)" % T, [(T + 1, 0)]); cell("T=%d (0, T+1)" % T, [(0, T + 1)])
        cell("T=%d (0, T+1) ahead of (T-100, T-100)" % T, [(0, T + 1), (T - 100, T - 100)])
    cell("(16320, 16320)", [(16320, 16320)])
    return _track(prev, cur, [dict(ifm_sad_max_distance=f) for f in GATE_FIELDS])


def trk_sums():
    """equal sums with different splits (first current index wins), two previous pairings claiming one current pairing at equal sums
    (lowest previous index), at 32640 against 32639 and at 16400 against 16383 (the smaller: the first couple differs in bit 0 of a
    15-bit sum, the second ranks the other way round in any field of fewer than 15 bits), one pairing at 16320 + 16320"""
    prev, cur = [], []
    for k, (a, b) in enumerate([((300, 0), (150, 150)), ((150, 150), (300, 0))]):
        x, y = _cell(k)
        prev.append(P(x, y, x - 20, 0, 0, "equal sums %d+%d ahead of %d+%d" % (a + b), [("s%da" % k,) + a, ("s%db" % k,) + b]))
        cur += [Cu("s%da" % k, x - 8, y, x - 28, *a), Cu("s%db" % k, x + 8, y, x - 12, *b)]
    for k, (a, b) in enumerate([((100, 0), (0, 100)), ((16320, 16320), (16320, 16319)), ((16320, 80), (16320, 63)), ((16320, 63), (16320, 80))], 2):
        x, y = _cell(k)
        prev += [P(x - 8, y, x - 28, a[0], a[1], "claim %d against %d: first" % (sum(a), sum(b)), [("c%d" % k,) + a]),
                 P(x + 8, y, x - 12, b[0], b[1], "claim %d against %d: second" % (sum(a), sum(b)), [("c%d" % k,) + b])]
        cur.append(Cu("c%d" % k, x, y, x - 20, 0, 0))
    x, y = _cell(6)
    prev.append(P(x, y, x - 20, 16320, 16320, "16320 + 16320", [("top", 16320, 16320)])); cur.append(Cu("top", x + 8, y, x - 12, 0, 0))
    return _track(prev, cur, [dict(ifm_sad_max_distance=-1), dict(ifm_sad_max_distance=16320)])


def trk_window():
    """ifm_win_h = 16: current x on wx_min and wx_max of the left or the right window and 2^-10 beside them; inside the left window and
    outside the right one; on 3 and W - 5 and just beyond; a previous x of 3.5, whose (int)(3.5 - 16) = -12 is clamped to 3.  Every
    candidate is at (200, 200): on the default threshold"""
    prev, cur = [], []
    k = 0

    def cell(label, pxl, pxr, cxl, cxr, inside, y=None):
        nonlocal k
        y = BANDS[k // 2] if y is None else y
        prev.append(P(pxl, y, pxr, 0, 0, label, [(k, 200, 200)] if inside else [])); cur.append(Cu(k, cxl, y, cxr, 200, 200))
        k += 1
    for side in ("left", "right"):
        for dx, inside in ((-16.0, True), (-16.0 - NEAR, False), (16.0, True), (16.0 + NEAR, False)):
            pxl = 40.0 if k % 2 == 0 else 110.0
            l, r = (dx, 0.0) if side == "left" else (0.0, dx)
            cell("%s x %+g %s" % (side, dx, "in" if inside else "out"), pxl, pxl - 20, pxl + l, pxl - 20 + r, inside)
    cell("inside the left window, outside the right one", 40.0, 20.0, 44.0, 37.0, False); k += 1
    cell("current left x=3", 10.0, 60.0, 3.0, 60.0, True); k += 1
    cell("current left x=2.99", 10.0, 60.0, 2.99, 60.0, False); k += 1
    cell("current left x=W-5", W - 10.0, 60.0, W - 5.0, 60.0, True); k += 1
    cell("current left x=W-4.99", W - 10.0, 60.0, W - 4.99, 60.0, False); k += 1
    # (the previous left window is all 255: read one pixel off, at (int)(3.5 + 0.5), it would be far over the threshold)
    prev.append(P(3.5, BANDS[k // 2], 60.0, 16320, 0, "previous left x=3.5", [(k, 200, 200)])); cur.append(Cu(k, 3.0, BANDS[k // 2], 60.0, 16120, 200))
    return _track(prev, cur, [dict(ifm_win_h=16)])


def trk_rows():
    """rows: wy_min = max(3, y - ifm_win_w), wy_max = min(H - 5, y + ifm_win_w); a current pairing on row 2 (reached only by a walk
    that starts below 3), a previous pairing on row H - 2 under ifm_win_w = 1 (wy_min = H - 3 above wy_max = H - 5: a wrapped range, no
    candidates).  Four candidates at most: the RANSAC masks are not applied, so the moves to another row are no outliers"""
    def within(dy):
        return lambda v: abs(dy) <= v["ifm_win_w"]
    prev = [P(40.0, 20.0, 20.0, 0, 0, "2 rows up", [("u2", 5, 5, within(2))]), P(110.0, 20.0, 90.0, 0, 0, "3 rows up"),
            P(40.0, 36.0, 20.0, 0, 0, "2 rows down", [("d2", 5, 5, within(2))]), P(110.0, 36.0, 90.0, 0, 0, "3 rows down"),
            P(40.0, 4.0, 20.0, 0, 0, "wy_min=3: row 3", [("r3", 5, 5)]), P(110.0, 4.0, 90.0, 0, 0, "wy_min=3: row 2"),
            P(40.0, H - 6.0, 20.0, 0, 0, "wy_max=H-5: row H-5", [("b1", 5, 5)]), P(110.0, H - 6.0, 90.0, 0, 0, "wy_max=H-5: row H-4.99"),
            P(60.0, H - 2.0, 40.0, 0, 0, "row H-2: wrapped range")]
    cur = [Cu("u2", 44.0, 18.0, 24.0, 5, 5), Cu("u3", 114.0, 17.0, 94.0, 5, 5), Cu("d2", 44.0, 38.0, 24.0, 5, 5), Cu("d3", 114.0, 39.0, 94.0, 5, 5),
           Cu("r3", 44.0, 3.0, 24.0, 5, 5), Cu("r2", 114.0, 2.0, 94.0, 5, 5), Cu("b1", 44.0, H - 5.0, 24.0, 5, 5), Cu("b2", 114.0, H - 4.99, 94.0, 5, 5),
           Cu("w1", 64.0, H - 4.0, 44.0, 0, 0), Cu("w2", 80.0, H - 3.0, 60.0, 0, 0)]
    return _track(prev, cur, [{}, dict(ifm_win_w=1)])


def trk_flags():
    """pairings with a keypoint that has no window, on either side of either frame, each with a partner well inside its windows: the
    library skips them, where the reference would read outside the image; one plain pairing beside them"""
    prev = [P(40.0, 4.0, 20.0, 0, 0, "current left y=2.99"), P(110.0, 4.0, 90.0, 0, 0, "plain", [("plain", 5, 5)]),
            P(2.99, BANDS[2], 60.0, 0, 0, "previous left x=2.99"), P(60.0, BANDS[3], 2.99, 0, 0, "previous right x=2.99"),
            P(100.0, BANDS[4], W - 4.99, 0, 0, "previous right x=W-4.99"),
            P(40.0, H - 6.0, 20.0, 0, 0, "current right y=H-4.99"), P(110.0, H - 4.99, 90.0, 0, 0, "previous left y=H-4.99")]
    cur = [Cu("cl", 44.0, 2.99, 24.0, 0, 0), Cu("plain", 114.0, 4.0, 94.0, 5, 5), Cu("pl", 6.0, BANDS[2], 60.0, 0, 0), Cu("pr", 60.0, BANDS[3], 6.0, 0, 0),
           Cu("px", 100.0, BANDS[4], W - 10.0, 0, 0), Cu("cr", 44.0, H - 5.0, 24.0, 0, 0, yr=H - 4.99), Cu("py", 114.0, H - 5.0, 94.0, 0, 0)]
    return _track(prev, cur, [{}])


def track_params(p, variant, faster=False):
    """the parameter record of a stage-4 variant: ifmSAD (and smSAD, so that a frame needs its windows either way)"""
    q = p.copy()
    q.detect_method, q.match_method, q.ifm_method = (2 if faster else 0), 2, 2
    for k, v in dict(TRACK_DEFAULTS, **variant).items():
        setattr(q, k, v)
    return q


# ---------------------------------------------------------------------------------------------------------------------------------------
# two octaves (dmFASTER geometry)
# ---------------------------------------------------------------------------------------------------------------------------------------
OCT_FIELDS = [191, 192, 193]


def trk_octaves():
    """Octave 1 of a 160 x 96 frame is 80 x 48.  The level-0 images are 24 x 24 blocks of one grey value each on black, one around every
    octave-1 keypoint, so that its window in the half-size image is constant (asserted from faster_ref.pyramid) and a SAD is 64 times
    the difference of two grey values: 192 = 64 * 3 is met by thresholds 191, 192 and 193.  Current left x on (W/2) - 5 and (W/2) - 4.99:
    the borders are those of the octave's own image.  -> (octave-0 scene, octave-1 scene, the four level-0 images)"""
    import faster_ref as F
    w1, h1 = W // 2, H // 2
    ys = [5, 17, 29, 41]                                                          # 12 rows apart: the blocks tile the image
    prev, cur = [], []

    def cell(label, x, y, cx, grey_l, grey_r, inside):
        k = len(prev)
        prev.append(P(x, y, x - 10, 10, 10, label, [(k, 64 * grey_l, 64 * grey_r)] if inside else [])); cur.append(Cu(k, cx, y, cx - 10, 10 + grey_l, 10 + grey_r))
    cell("(192, 192)", 20.0, ys[0], 24.0, 3, 3, True); cell("(192, 0)", 50.0, ys[0], 54.0, 3, 0, True)
    cell("(0, 192)", 20.0, ys[1], 24.0, 0, 3, True); cell("(128, 256)", 50.0, ys[1], 54.0, 2, 4, True)
    cell("current left x=W/2-5", w1 - 12.0, ys[2], w1 - 5.0, 1, 1, True); cell("(64, 64)", 20.0, ys[2], 24.0, 1, 1, True)
    cell("current left x=W/2-4.99", w1 - 12.0, ys[3], w1 - 4.99, 1, 1, False); cell("(0, 0)", 20.0, ys[3], 24.0, 0, 0, True)
    # (levels stand for grey values here: the pattern painter is not used)
    pes, ces = [sorted(v, key=lambda e: (e["y"], e["xl"])) for v in (prev, cur)]

    def level0(es, xk, yk, gk):
        img = np.zeros((H, W), np.uint8)
        for e in es:
            xi, yi = int(np.float32(e[xk])), int(np.float32(e[yk]))
            img[max(0, 2 * yi - 10):2 * yi + 14, max(0, 2 * xi - 10):2 * xi + 14] = e[gk]
        return img
    imgs0 = [level0(pes, "xl", "y", "ll"), level0(pes, "xr", "yr", "lr"), level0(ces, "xl", "y", "ll"), level0(ces, "xr", "yr", "lr")]
    imgs1 = [F.pyramid(i, 2)[1] for i in imgs0]
    assert imgs1[0].shape == (h1, w1)

    def frame(es, imgs):
        kl = _kps(np.array([(e["xl"], e["y"]) for e in es] + [(10.0, h1 - 2.0)], np.float32)); kr = _kps(np.array([(e["xr"], e["yr"]) for e in es] + [(5.0, h1 - 1.0)], np.float32))
        m = _identity(len(es))
        for e in es:                                                              # every window of octave 1 is constant, of its keypoint's grey value
            for (x, y), img, g in (((e["xl"], e["y"]), imgs[0], e["ll"]), ((e["xr"], e["yr"]), imgs[1], e["lr"])):
                if not is_flagged(x, y, w1, h1):
                    win = img[int(y) - 3:int(y) + 5, int(np.float32(x)) - 3:int(np.float32(x)) + 5]
                    assert win.shape == (8, 8) and (win == g).all(), (e.get("label", e.get("key")), win)
        return dict(kl=kl, kr=kr, m=m, imgs=tuple(imgs), ri=matches_row_index(m, kl, h1))
    pf, cf = frame(pes, imgs1[:2]), frame(ces, imgs1[2:])
    at = {e["key"]: i for i, e in enumerate(ces)}
    s1 = dict(pkl=pf["kl"], pkr=pf["kr"], pm=pf["m"], pimgs=pf["imgs"], pri=pf["ri"], ckl=cf["kl"], ckr=cf["kr"], cm=cf["m"], cimgs=cf["imgs"], cri=cf["ri"],
              W=w1, H=h1, variants=[dict(ifm_sad_max_distance=f) for f in OCT_FIELDS], label=[e["label"] for e in pes],
              plan=[sorted((at[k], a, b, c) for k, a, b, c in e["cands"]) for e in pes], cur_at=at)
    s1["want"] = functools.partial(expected_track, s1)
    # octave 0: two pairings in the middle of a block each, 4 px to the right in the current frame (windows constant: SAD 0)
    k0p = _kps(np.array([(2 * e["xl"] + 1.0, 2 * e["y"] + 1.0) for e in pes[:2]] + [(10.0, H - 2.0)], np.float32))
    k0pr = _kps(np.array([(2 * e["xr"] + 1.0, 2 * e["yr"] + 1.0) for e in pes[:2]] + [(5.0, H - 1.0)], np.float32))
    k0c, k0cr = k0p.copy(), k0pr.copy()
    k0c["x"][:2] += 2.0; k0cr["x"][:2] += 2.0
    m0 = _identity(2)
    s0 = dict(pkl=k0p, pkr=k0pr, pm=m0, pimgs=tuple(imgs0[:2]), pri=matches_row_index(m0, k0p, H), ckl=k0c, ckr=k0cr, cm=m0.copy(), cimgs=tuple(imgs0[2:]),
              cri=matches_row_index(m0, k0c, H), W=W, H=H)
    return s0, s1, imgs0


# ---------------------------------------------------------------------------------------------------------------------------------------
# indices from 8192 on (max_kps = 16384)
# ---------------------------------------------------------------------------------------------------------------------------------------
N_FILL = 8200


def big_index():
    """more than 8192 right keypoints / previous pairings ahead of the planted ones: the fillers sit on row 4 at one place, which no row
    range of interest reaches.  Stage 3: the planted right keypoint (index >= 8192) is at SAD 16320 -- index and distance fill the 28
    bits of left_pick.  Stage 4: a planted previous pairing (index >= 8192) claims its current pairing at the sum 32640 -- the
    largest (sum << 16 | index) there is -- and another one wins a current pairing at 16383 against pairing 0 at 16400.  -> (stage-3 scene, stage-4 scene), both run under `no threshold`"""
    right = [R("f%d" % i, 5.0, 4.0, 0) for i in range(N_FILL)] + [R("top", 100.0, 60.0, 16320), R("mid", 60.0, 44.0, 300)]
    s3 = _stereo([L(148.0, 60.0, 0, "right index >= 8192 at SAD 16320", [("top", 16320)]), L(148.0, 44.0, 0, "right index >= 8192", [("mid", 300)])], right,
                 [dict(sad_max_distance=-1)])
    assert min(s3["right_at"]["top"], s3["right_at"]["mid"]) >= 8192
    s4 = _track([P(96.0, 3.0, 76.0, 16320, 80, "index 0 claims at 16400", [("mid", 16320, 80)]),
                 P(108.0, 7.0, 88.0, 16320, 63, "previous index >= 8192 claims at 16383", [("mid", 16320, 63)]),
                 P(94.0, 60.0, 74.0, 16320, 16320, "previous index >= 8192 at the sum 32640", [("top", 16320, 16320)])],
                [Cu("mid", 102.0, 5.0, 82.0, 0, 0), Cu("top", 100.0, 60.0, 80.0, 0, 0)], [dict(ifm_sad_max_distance=-1)])
    # the filler pairings all join one keypoint of either list, on row 4 behind the first pairing; the planted ones move up by one.
    # (Their row iteration reaches the current pairing on row 5, whose x is outside their windows.)
    for side, xy in (("pkl", (20.0, 4.0)), ("pkr", (5.0, 4.0))):
        s4[side] = np.concatenate([s4[side][:1], _kps(np.array([xy], np.float32)), s4[side][1:]])
    fill = _identity(N_FILL); fill["queryIdx"] = 1; fill["trainIdx"] = 1
    pm = s4["pm"].copy(); pm["queryIdx"][1:] += 1; pm["trainIdx"][1:] += 1
    s4["pm"] = np.concatenate([pm[:1], fill, pm[1:]])
    s4["pri"] = matches_row_index(s4["pm"], s4["pkl"], H)
    s4["plan"] = s4["plan"][:1] + [[] for _ in range(N_FILL)] + s4["plan"][1:]
    s4["label"] = s4["label"][:1] + ["fill"] * N_FILL + s4["label"][1:]
    s4["want"] = functools.partial(expected_track, s4)
    return s3, s4


STEREO = [("sad_threshold", sad_threshold), ("sad_ties", sad_ties), ("sad_one_to_one", sad_one_to_one), ("sad_border", sad_border),
          ("sad_disparity", sad_disparity), ("sad_rows", sad_rows), ("sad_response", sad_response)]
TRACK = [("trk_gates", trk_gates), ("trk_sums", trk_sums), ("trk_window", trk_window), ("trk_rows", trk_rows), ("trk_flags", trk_flags)]
OTHER = [("trk_octaves", trk_octaves), ("big_index", big_index)]


@functools.lru_cache(maxsize=None)
def scene(name):
    return dict(STEREO + TRACK + OTHER)[name]()


def stereo_names():
    return [nm for nm, _ in STEREO]


def track_names():
    return [nm for nm, _ in TRACK]


def all_variants(names):
    """every distinct variant of the named scenes, in the order met"""
    out = []
    for nm in names:
        for v in scene(nm)["variants"]:
            if v not in out:
                out.append(v)
    return out
