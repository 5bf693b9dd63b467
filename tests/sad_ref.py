"""The reference for smSAD and ifmSAD (TEST INFRASTRUCTURE): literal walks of the reference's own loops.

The CPU oracle refuses match_method = smSAD, so the SAD matchers bring their reference with them: plain Python walks of
stage3_match_left_right.cpp:185-419 ("S3", SAD branch) and stage4_match_consecutive.cpp:435-679 ("S4", use_SAD branch), written
against the reference text line by line, on numpy images and keypoint arrays.  Everything downstream of the two candidate lists
is composed from oracle entry points that exist: the F-matrix RANSAC (oracle.ransac_fundamental), the both-masks rule as the
oracle's windowed tracker applies it, and stage 5 (Oracle.change_in_pose).

rso::compute_SAD8 (compute_SAD8.cpp:71-98) is `sad8` below; tests/test_sad_cpu.py holds it equal to oracle.sad8, which
tests/golden/sad8_kat.npz pins."""
import math

import numpy as np

from stereo_vo_amd.abi import dmatch_dtype, index_pair_dtype

INVALID_IDX = -1
UINT32_MAX = 0xFFFFFFFF
SAD_DEFAULT = 200                                    # S3:48; H:297 "~200" for the tracker, whose group has no constructor default


def sad8(img_l, img_r, lx, ly, rx, ry):
    """sum of |l - r| over the 8 x 8 windows [x-3, x+4] x [y-3, y+4] (compute_SAD8.cpp:71-98)"""
    a = img_l[ly - 3:ly + 5, lx - 3:lx + 5].astype(np.int32)
    b = img_r[ry - 3:ry + 5, rx - 3:rx + 5].astype(np.int32)
    assert a.shape == (8, 8) and b.shape == (8, 8), "window outside the image"
    return int(np.abs(a - b).sum())


def effective_threshold(field):
    """svo_params.sad_max_distance / ifm_sad_max_distance -> the reference's unsigned threshold: 0 = 200, negative wraps"""
    return SAD_DEFAULT if field == 0 else (field & UINT32_MAX if field < 0 else field)


def c_round(v):
    """C's round(): half away from zero"""
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


MUTANTS_S3 = ("ge_threshold", "and_ff", "le_min", "le_claim", "round_pt", "py_round", "no_flag", "round_disparity", "le_response")
MUTANTS_S4 = ("ge_left", "ge_right", "and_ff", "le_min", "le_claim", "sum_gate", "lo0", "awx", "round_pt", "no_flag", "oct0_size")


def _pt(v, mutant):
    """(int)pt: towards zero.  (mutant round_pt: to nearest)"""
    return int(math.floor(v + 0.5)) if mutant == "round_pt" else int(v)


def flagged(k, W, H):
    """the border rule of S3:289-295 on one keypoint: no 8 x 8 window inside a W x H image"""
    return bool(k["x"] < 3 or k["y"] < 3 or k["x"] > W - 4 - 1 or k["y"] > H - 4 - 1)


def match_lr_sad(img_l, img_r, kl, kr, idx_l, idx_r, sad_max_distance, max_y_diff, one_to_one, minimum_response=0.0, sad_max_ratio=0.5, mutant=None):
    """S3:185-419 with match_method == smSAD on one octave.  kl / kr: keypoint_dtype arrays (row-sorted), idx_l / idx_r: their
    pyr_feats_index tables (one entry per image row).  Returns the DMatch list (dmatch_dtype, imgIdx = -1).
    mutant (None: the walk as the reference has it): one of MUTANTS_S3, a walk that is wrong in exactly one rule; the hand-built
    scenes of tests/sad_scenes.py must tell every one of them from the walk (tests/test_sad_scenes_cpu.py)."""
    assert mutant is None or mutant in MUTANTS_S3, mutant
    H, W = img_l.shape
    max_ratio = sad_max_ratio                                                     # S3:200
    max_distance = effective_threshold(sad_max_distance)                          # S3:201 size_t(sad_max_distance)
    n_rows_max = len(idx_l)                                                       # S3:224
    assert len(idx_l) == len(idx_r)
    left_matches_idxs = [INVALID_IDX] * len(kl)                                   # S3:228
    right_feat_assign = [[INVALID_IDX, UINT32_MAX] for _ in range(len(kr))]       # S3:229
    max_pt = (W - 4 - 1, H - 4 - 1)                                               # S3:235
    max_disparity = int(W * 0.7)                                                  # S3:247
    d = c_round(max_y_diff) if mutant != "py_round" else round(max_y_diff)
    for y in range(n_rows_max - 1):                                               # S3:250
        l0, l1 = int(idx_l[y]), int(idx_l[y + 1])                                 # S3:253
        min_row_right = max(0, y - d)                                             # S3:254
        max_row_right = min(H - 1, y + d)                                         # S3:255
        r0, r1 = int(idx_r[min_row_right]), int(idx_r[max_row_right])             # S3:256
        if l1 - l0 == 0 or r1 - r0 == 0:                                          # S3:259-263 (unsigned: a wrapped range is not zero)
            continue
        for il in range(l0, l1):                                                  # S3:265
            fl = kl[il]
            min_1 = min_2 = UINT32_MAX                                            # S3:270-271
            min_idx = INVALID_IDX
            for ir in range(r0, r1):                                              # S3:274
                fr = kr[ir]
                if fl["response"] < minimum_response or fr["response"] < minimum_response:   # S3:279
                    continue
                if mutant == "le_response" and (fl["response"] <= minimum_response or fr["response"] <= minimum_response):
                    continue
                disparity = int(fl["x"] - fr["x"])                                # S3:283 (float subtraction, truncated)
                if mutant == "round_disparity":
                    disparity = c_round(float(fl["x"] - fr["x"]))
                if disparity < 1 or disparity > max_disparity:
                    continue
                if mutant != "no_flag" and (fl["x"] < 3 or fr["x"] < 3 or fl["y"] < 3 or fr["y"] < 3 or                    # S3:289-295
                        fl["x"] > max_pt[0] or fr["x"] > max_pt[0] or fl["y"] > max_pt[1] or fr["y"] > max_pt[1]):
                    continue
                dist = sad8(img_l, img_r, _pt(fl["x"], mutant), _pt(fl["y"], mutant), _pt(fr["x"], mutant), _pt(fr["y"], mutant))   # S3:309-313
                if mutant == "and_ff":
                    dist &= 0xFF
                if dist > max_distance or (mutant == "ge_threshold" and dist == max_distance):   # S3:334
                    continue
                if dist < min_1 or (mutant == "le_min" and dist == min_1):        # S3:338-345
                    min_2, min_1, min_idx = min_1, dist, ir
                elif dist < min_2:
                    min_2 = dist
                if 1.0 * min_1 / min_2 > max_ratio:                               # S3:347-349: skips a debug print only
                    continue
            if min_idx != INVALID_IDX:                                            # S3:357
                a = right_feat_assign[min_idx]
                if one_to_one:                                                    # S3:359-377
                    if a[0] == INVALID_IDX:
                        left_matches_idxs[il] = min_idx
                        a[0], a[1] = il, min_1
                    elif min_1 < a[1] or (mutant == "le_claim" and min_1 == a[1]):
                        left_matches_idxs[a[0]] = INVALID_IDX
                        left_matches_idxs[il] = min_idx
                        a[0], a[1] = il, min_1
                elif a[0] == INVALID_IDX:                                         # S3:378-387
                    left_matches_idxs[il] = min_idx
                    a[0], a[1] = il, min_1
    out = []
    for i, fr in enumerate(left_matches_idxs):                                    # S3:396-409
        if fr != INVALID_IDX:
            out.append((i, fr, -1, float(right_feat_assign[fr][1])))              # DMatch(i, fr, d): imgIdx = -1
    return np.array(out, dmatch_dtype)


def matches_row_index(matches, kl, img_h):
    """S3:425-445, with the documented deviation ri[H] = M (the reference stores the number of left FEATURES there)"""
    ri = np.zeros(img_h + 1, np.int64)
    idx, n = 0, len(matches)
    for y in range(img_h):
        ri[y] = idx
        while idx < n and kl[matches[idx]["queryIdx"]]["y"] <= int(y):
            idx += 1
    ri[img_h] = n
    return ri


def track_sad(prev, cur, win_w, win_h, ifm_sad_max_distance, skip_flagged=False, mutant=None):
    """S4:435-679 with use_SAD on one octave.  prev / cur: dicts with imgs (left, right), kl, kr, m (DMatch list), ri (its row
    index).  Returns potential_match_idxs as an index_pair_dtype array (previous pairing, current pairing), ascending in the
    current index.
    skip_flagged: the library's documented deviation: a pairing of either frame with a keypoint that has no window
    (`flagged`) is skipped, where the reference reads whatever lies there (`sad8` refuses that here).  Lists that stage 3 made hold
    no such pairing, so the two forms differ on put lists only.
    mutant: one of MUTANTS_S4 (see match_lr_sad); "no_flag" is the walk without the deviation."""
    assert mutant is None or mutant in MUTANTS_S4, mutant
    H, W = prev["imgs"][0].shape
    Wb, Hb = (2 * W, 2 * H) if mutant == "oct0_size" else (W, H)                  # (mutant: the borders of the octave-0 image)
    skip_flagged = skip_flagged and mutant != "no_flag"
    PATCHSIZE_L, PATCHSIZE_R = 0 if mutant == "lo0" else 3, 4                     # S4:445-446
    MAX_SAD = effective_threshold(ifm_sad_max_distance)                           # S4:448 (uint32_t)
    pm, cm = prev["m"], cur["m"]
    absolute_wx_max = Wb - 1 - (0 if mutant == "awx" else PATCHSIZE_R)            # S4:489
    absolute_wy_max = Hb - 1 - PATCHSIZE_R                                        # S4:490
    current_matches = [[INVALID_IDX, UINT32_MAX] for _ in range(len(cm))]         # S4:509
    for y in range(H - 1):                                                        # S4:514
        prev_idx0, prev_idx1 = int(prev["ri"][y]), int(prev["ri"][y + 1])         # S4:517-518
        if prev_idx1 - prev_idx0 == 0:                                            # S4:519-522
            continue
        wy_min = max(PATCHSIZE_L, y - win_w)                                      # S4:525
        wy_max = min(absolute_wy_max, y + win_w)                                  # S4:526
        cur_idx0, cur_idx1 = int(cur["ri"][wy_min]), int(cur["ri"][wy_max + 1])   # S4:529-530
        if cur_idx1 - cur_idx0 == 0:                                              # S4:531-534 (unsigned: a wrapped range runs no loop)
            continue
        for pi in range(prev_idx0, prev_idx1):                                    # S4:537
            p_ft_l, p_ft_r = prev["kl"][pm[pi]["queryIdx"]], prev["kr"][pm[pi]["trainIdx"]]
            if skip_flagged and (flagged(p_ft_l, Wb, Hb) or flagged(p_ft_r, Wb, Hb)):
                continue
            best_pairing_in_curimg, best_pairing_sad = None, UINT32_MAX           # S4:543-544
            wx_min_l = max(PATCHSIZE_L, int(p_ft_l["x"] - np.float32(win_h)))     # S4:552-555
            wx_max_l = min(absolute_wx_max, int(p_ft_l["x"] + np.float32(win_h)))
            wx_min_r = max(PATCHSIZE_L, int(p_ft_r["x"] - np.float32(win_h)))
            wx_max_r = min(absolute_wx_max, int(p_ft_r["x"] + np.float32(win_h)))
            for ci in range(cur_idx0, cur_idx1):                                  # S4:557
                ft_l, ft_r = cur["kl"][cm[ci]["queryIdx"]], cur["kr"][cm[ci]["trainIdx"]]
                if ft_l["x"] < wx_min_l or ft_l["x"] > wx_max_l or ft_r["x"] < wx_min_r or ft_r["x"] > wx_max_r:   # S4:567
                    continue
                if skip_flagged and (flagged(ft_l, Wb, Hb) or flagged(ft_r, Wb, Hb)):
                    continue
                sad_l = sad8(prev["imgs"][0], cur["imgs"][0], _pt(p_ft_l["x"], mutant), _pt(p_ft_l["y"], mutant), _pt(ft_l["x"], mutant), _pt(ft_l["y"], mutant))   # S4:572
                if mutant != "sum_gate" and (sad_l > MAX_SAD or (mutant == "ge_left" and sad_l == MAX_SAD)):
                    continue
                sad_r = sad8(prev["imgs"][1], cur["imgs"][1], _pt(p_ft_r["x"], mutant), _pt(p_ft_r["y"], mutant), _pt(ft_r["x"], mutant), _pt(ft_r["y"], mutant))   # S4:576
                if mutant != "sum_gate" and (sad_r > MAX_SAD or (mutant == "ge_right" and sad_r == MAX_SAD)):
                    continue
                sad = sad_l + sad_r                                               # S4:580
                if mutant == "sum_gate" and sad > MAX_SAD:
                    continue
                if mutant == "and_ff":
                    sad &= 0xFF
                if sad < best_pairing_sad or (mutant == "le_min" and sad == best_pairing_sad):   # S4:583-587
                    best_pairing_sad, best_pairing_in_curimg = sad, ci
            if best_pairing_in_curimg is not None:                                # S4:622-636
                e = current_matches[best_pairing_in_curimg]
                if e[0] == INVALID_IDX:
                    e[0], e[1] = pi, best_pairing_sad
                if e[0] != INVALID_IDX and (best_pairing_sad < e[1] or (mutant == "le_claim" and best_pairing_sad == e[1])):
                    e[0], e[1] = pi, best_pairing_sad
    pot = [(e[0], ci) for ci, e in enumerate(current_matches) if e[0] != INVALID_IDX]   # S4:640-679
    return np.array(pot, index_pair_dtype)


def filter_candidates(O, prev, cur, pot):
    """S4:681-722 as the oracle's windowed tracker composes it (svo_oracle.c, track_win): both RANSACs, the masks applied only
    when both models have >= 8 inliers.  Returns (tracked pairs, the eight SVO_TS_* counters of svo_result.track_stats)."""
    def pts(frame, side, idx):
        k = frame["kl" if side == 0 else "kr"][frame["m"][idx]["queryIdx" if side == 0 else "trainIdx"]]
        return np.stack([k["x"], k["y"]], 1).astype(np.float32).reshape(-1, 2)
    n = len(pot)
    l1, l2 = pts(prev, 0, pot["first"]), pts(cur, 0, pot["second"])               # S4:651-666
    r1, r2 = pts(prev, 1, pot["first"]), pts(cur, 1, pot["second"])
    cnt_l, in_l, _, _, hyp_l = O.ransac_fundamental(l1, l2)                       # S4:684-687
    cnt_r, in_r, _, _, hyp_r = O.ransac_fundamental(r1, r2)                       # S4:696-699
    use_f = cnt_l >= 8 and cnt_r >= 8
    keep = [i for i in range(n) if not (use_f and (not in_l[i] or not in_r[i]))]  # S4:708-714
    tracked = pot[keep] if n else pot
    stats = [n, n, cnt_l, cnt_r, hyp_l, hyp_r, len(tracked), len(tracked)]
    return tracked, stats


def oracle_features(O, params, left, right, cam):
    """keypoints, descriptors and row tables of one frame from the oracle's detector, which does not depend on the matcher and
    tracker selectors: those are swapped for ones the oracle accepts.  (kl, dl, kr, dr, idx_l, idx_r)"""
    q = params.copy()
    q.match_method, q.ifm_method = 1, 1
    o = O.Oracle(q)
    o.process(left, right, cam)
    out = o.keypoints(0, 0) + o.keypoints(0, 1) + (o.row_index(0, 0), o.row_index(0, 1))
    o.close()
    return out


def photo_params(base, orb_nfeats=1200, sad_max_distance=400, one_to_one=1, ifm_sad_max_distance=0, match_method=2, ifm_method=2):
    """the parameter sets of the SAD tests on the photograph: north-star base, max_y_diff 2, windows 16 / 16"""
    from stereo_vo_amd.abi import north_star_params
    p = north_star_params(base, orb_nfeats=orb_nfeats)
    p.match_method, p.ifm_method, p.max_y_diff, p.enable_robust_1to1_match = match_method, ifm_method, 2.0, one_to_one
    p.sad_max_distance, p.ifm_sad_max_distance, p.ifm_win_w, p.ifm_win_h = sad_max_distance, ifm_sad_max_distance, 16, 16
    return p


CROPS = ((20, 20), (17, 22), (13, 23), (10, 25))       # 760 x 560 crops of the 800 x 600 photograph, as a moving sequence
CROP_W, CROP_H = 760, 560


class SadStream:
    """One estimator's worth of state for the composed reference: frames go in with their keypoints (from the oracle's detector:
    detection does not depend on the selectors), pairings come from match_lr_sad (or are handed in), the tracker is track_sad
    (or, with ifm_method 0 / 1, the oracle's own), and stage 5 is Oracle.change_in_pose on ONE oracle instance, which keeps
    m_last_computed_pose from frame to frame as the pipeline does."""

    def __init__(self, O, params, cam):
        self.O, self.p, self.cam = O, params, cam
        self.orc5 = O.Oracle(params)
        self.prev = None
        self.last_id = 0

    def step(self, imgs, kl, kr, idx_l, idx_r, dl=None, dr=None, orb_th=None):
        O, p = self.O, self.p
        H, W = imgs[0].shape
        f = {"imgs": imgs, "kl": kl, "kr": kr, "dl": dl, "dr": dr}
        if p.match_method == 2:
            minresp = p.minimum_ORB_response if p.detect_method == 0 else 0.0    # S3:189-193
            f["m"] = match_lr_sad(imgs[0], imgs[1], kl, kr, idx_l, idx_r, p.sad_max_distance, p.max_y_diff, p.enable_robust_1to1_match, minresp)
            f["ri"] = matches_row_index(f["m"], kl, H)
        else:
            f["m"], f["ri"] = O.match_lr(p, orb_th, kl, dl, np.asarray(idx_l, np.int64), kr, dr, np.asarray(idx_r, np.int64), W, H)
        out = {"matches": f["m"], "mri": f["ri"], "candidates": None, "tracked": np.zeros(0, index_pair_dtype), "stats": [0] * 8,
               "valid": False, "result": None, "residuals": None, "inliers": None}
        prev = self.prev
        if prev is None:
            if p.vo_use_matches_ids:                                              # S3:406-407
                f["ids"] = np.arange(self.last_id, self.last_id + len(f["m"]), dtype=np.int64); self.last_id += len(f["m"])
        else:
            if p.ifm_method == 2:
                out["candidates"] = track_sad(prev, f, p.ifm_win_w, p.ifm_win_h, p.ifm_sad_max_distance)
                out["tracked"], out["stats"] = filter_candidates(O, prev, f, out["candidates"])
            else:
                out["tracked"], ts = O.track(p, orb_th, prev["kl"], prev["dl"], prev["kr"], prev["dr"], prev["m"], np.asarray(prev["ri"], np.int64),
                                             kl, dl, kr, dr, f["m"], np.asarray(f["ri"], np.int64), W, H, stats=True)
                out["stats"] = list(ts)
            if p.vo_use_matches_ids:                                              # S4:716-733
                ids = np.full(len(f["m"]), -1, np.int64)
                ids[out["tracked"]["second"]] = prev["ids"][out["tracked"]["first"]]
                for k in range(len(ids)):
                    if ids[k] < 0:
                        ids[k] = self.last_id; self.last_id += 1
                f["ids"] = ids
            if len(out["tracked"]) >= p.bad_tracking_th:                          # P:326-341
                valid, res, resid, inl = self.orc5.change_in_pose(out["tracked"], prev["m"], f["m"], prev["kl"], prev["kr"], kl, kr, self.cam)
                out.update(valid=valid, result=res, residuals=resid, inliers=inl)
        out["ids"] = f.get("ids")
        self.prev = f
        return out
