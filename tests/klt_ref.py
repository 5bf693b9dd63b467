"""The specification of the resident KLT front end (include/svo_hip.h: svo_klt_step).

Two things live here.  `select` is a literal numpy walk of the selection step: the gate, the stable order, the lists the survivors
become, the tracked pairs, both row tables and the new table, with the rule that moves a track's previous index under a shift or a
hold.  `KltHostFrontEnd` is the host recipe of INTEGRATION.md 3d written against the public Python calls only (a shift-only
svo_process call, Context.lk_track, the svo_put_* calls, svo_process with SVO_RUN_OPTIMIZE | SVO_FLAG_NO_SHIFT): the device front end
must leave, byte for byte, what this recipe leaves.  The GPU tests run it on a second context.

The keypoint fields beyond x, y are defined here once: size = lk.win, angle = -1, response = 0, octave = 0, class_id = the track ID.
A pairing is (i, i, imgIdx 0, distance 0)."""
import numpy as np

F = np.float32
keypoint_dtype = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
dmatch_dtype = np.dtype([("queryIdx", "<i4"), ("trainIdx", "<i4"), ("imgIdx", "<i4"), ("distance", "<f4")])
index_pair_dtype = np.dtype([("first", "<i4"), ("second", "<i4")])
VOEC_BAD_COND_NUMBER, VOEC_BAD_TRACKING = 1, 5
RUN_OPTIMIZE, FLAG_NO_SHIFT = 8, 32


class Gate:
    """the gates of svo_klt_params with the keypoint size (lk.win), all float32"""
    def __init__(self, max_dy=1.5, min_disp=0.5, max_disp=np.inf, win=21):
        self.max_dy, self.min_disp, self.max_disp, self.win = F(max_dy), F(min_disp), F(max_disp), int(win)


class Table:
    """a lane's track table: the live tracks only (the device keeps cap slots and NaN behind the live count)"""
    def __init__(self):
        self.left = np.zeros((0, 2), F); self.right = np.zeros((0, 2), F)
        self.ids = np.zeros(0, np.int32); self.age = np.zeros(0, np.int32)
        self.idx = np.zeros(0, np.int32)       # index in the list of the last step, -1: none
        self.pidx = np.zeros(0, np.int32)      # index in the list of the lane's previous slot, -1: none
        self.next_id = 0

    def __len__(self):
        return len(self.ids)

    def copy(self):
        t = Table()
        for k in ("left", "right", "ids", "age", "idx", "pidx"):
            setattr(t, k, getattr(self, k).copy())
        t.next_id = self.next_id
        return t

    def cleared(self):
        """svo_klt_reset: no tracks, the IDs start over"""
        return Table()


def add_points(table, left, right, cap):
    """svo_klt_add_points: (new table, number appended)"""
    left = np.ascontiguousarray(left, F).reshape(-1, 2); right = np.ascontiguousarray(right, F).reshape(-1, 2)
    m = max(0, min(len(left), cap - len(table)))
    t = table.copy()
    t.left = np.concatenate([t.left, left[:m]]); t.right = np.concatenate([t.right, right[:m]])
    t.ids = np.concatenate([t.ids, np.arange(t.next_id, t.next_id + m, dtype=np.int32)])
    t.age = np.concatenate([t.age, np.zeros(m, np.int32)])
    t.idx = np.concatenate([t.idx, np.full(m, -1, np.int32)]); t.pidx = np.concatenate([t.pidx, np.full(m, -1, np.int32)])
    t.next_id += m
    return t, m


def row_of(y):
    """(long long)y of svo_put_features_oct, saturated at +-1e9 (float32 y, truncation towards zero)"""
    y = F(y)
    if y >= F(0):
        return int(y) if y < F(1.0e9) else 1000000000
    return int(y) if y > F(-1.0e9) else -1000000000


def feats_row_index(ys, H):
    """pyr_feats_index of a keypoint list in ITS order: a row histogram (rows clamped to 0 .. H) and its running sum, kept between the
    first and the last entry's rows and 0 elsewhere"""
    ri = np.zeros(H, np.int32)
    if len(ys) == 0 or H <= 0:
        return ri
    rows = np.array([row_of(y) for y in ys], np.int64)
    cnt = np.bincount(np.clip(rows, 0, H), minlength=H + 1)
    acc = np.cumsum(cnt[:H])
    r = np.arange(H)
    keep = (r >= rows[0]) & (r < rows[-1])
    ri[keep] = acc[keep]
    return ri


def matches_row_index(ys, H):
    """matches_lr_row_index of identity pairings over left keypoints with these y, in list order: ri[y + 1] = #{i : max(y_0 .. y_i) <= y}
    for y + 1 < H, ri[0] = 0, ri[H] = n -- a prefix maximum and a count, no sequential walk"""
    n = len(ys)
    ri = np.zeros(H + 1, np.int32)
    if n and H > 0:
        pm = np.maximum.accumulate(np.asarray(ys, F))
        for y in range(H - 1):
            ri[y + 1] = int(np.count_nonzero(pm <= F(y)))
    ri[H] = n
    return ri


class Lists:
    """what a step leaves in the lane's current-frame lists at octave 0"""
    pass


REASONS = ("status", "nonfinite", "max_dy", "min_disp", "max_disp")


def select(table, left_xy, right_xy, status_l, status_r, gate, shifted, H):
    """One lane's selection.  table: the lane's Table before the step; left_xy / right_xy / status_*: the tracker's results for its
    slots (or hand-built arrays); shifted: the lane's prev/cur shift moved its slots in this step; H: the rows of the row tables.
    Returns (Lists, new Table, reasons) -- reasons[slot] is None for a survivor, else the FIRST rule that dropped it."""
    n = len(table)
    L = np.ascontiguousarray(left_xy, F).reshape(-1, 2); R = np.ascontiguousarray(right_xy, F).reshape(-1, 2)
    sl = np.ascontiguousarray(status_l, np.uint8); sr = np.ascontiguousarray(status_r, np.uint8)
    assert len(L) == len(R) == len(sl) == len(sr) == n
    reasons, keep = [], []
    for s in range(n):
        xl, yl, xr, yr = L[s, 0], L[s, 1], R[s, 0], R[s, 1]
        why = None
        if not (sl[s] == 1 and sr[s] == 1):
            why = "status"
        elif not (np.isfinite(xl) and np.isfinite(yl) and np.isfinite(xr) and np.isfinite(yr)):
            why = "nonfinite"
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                dy, disp = F(abs(F(yl - yr))), F(xl - xr)
            if not dy <= gate.max_dy:
                why = "max_dy"
            elif not disp >= gate.min_disp:
                why = "min_disp"
            elif not disp <= gate.max_disp:
                why = "max_disp"
        reasons.append(why)
        if why is None:
            keep.append(s)
    keep = np.array(keep, np.int64)
    m = len(keep)
    p_old = table.idx if shifted else table.pidx
    out = Lists()
    out.kps = []
    for pts in (L, R):
        k = np.zeros(m, keypoint_dtype)
        k["x"], k["y"] = pts[keep, 0], pts[keep, 1]
        k["size"], k["angle"], k["response"], k["octave"], k["class_id"] = F(gate.win), F(-1), F(0), 0, table.ids[keep]
        out.kps.append(k)
    out.matches = np.zeros(m, dmatch_dtype)
    out.matches["queryIdx"] = out.matches["trainIdx"] = np.arange(m)
    out.ids = table.ids[keep].astype(np.int32)
    p = p_old[keep].astype(np.int32)
    has = np.flatnonzero(p >= 0)
    out.tracked = np.zeros(len(has), index_pair_dtype)
    out.tracked["first"], out.tracked["second"] = p[has], has
    out.row_index = [feats_row_index(out.kps[0]["y"], H), feats_row_index(out.kps[1]["y"], H)]
    out.mrow_index = matches_row_index(out.kps[0]["y"], H)
    out.last_match_id = int(max([0] + list(out.ids)))
    t = Table()
    t.left, t.right = L[keep].copy(), R[keep].copy()
    t.ids, t.age = table.ids[keep].copy(), (table.age[keep] + 1).astype(np.int32)
    t.idx, t.pidx = np.arange(m, dtype=np.int32), p.copy()
    t.next_id = table.next_id
    return out, t, reasons


def lane_shifts(stepped, error_code):
    """the prev/cur shift of svo_process for a lane: its slots move unless it has no current frame yet or its last call ended in
    voecBadTracking / voecBadCondNumber (the lane then keeps its previous frame)"""
    return bool(stepped) and error_code not in (VOEC_BAD_TRACKING, VOEC_BAD_COND_NUMBER)


class KltHostFrontEnd:
    """The recipe of INTEGRATION.md 3d on a context, lane by lane, through public calls only.  params: an abi.KltParams.  The images of
    a step are host arrays.  After step() the context holds what svo_klt_step must leave."""

    def __init__(self, ctx, params, img_h):
        self.ctx, self.p, self.H = ctx, params, int(img_h)
        self.gate = Gate(params.max_dy, params.min_disp, params.max_disp, params.lk.win)
        self.tables = [Table() for _ in range(ctx.n_lanes)]
        self.prev = [None] * ctx.n_lanes           # the lane's last (left, right) images
        self.stepped = [False] * ctx.n_lanes       # the lane has a current frame

    def add_points(self, lane, left, right):
        self.tables[lane], m = add_points(self.tables[lane], left, right, self.p.cap)
        return m

    def reset(self, lanes=None):
        for l in (range(self.ctx.n_lanes) if lanes is None else lanes):
            self.tables[l] = self.tables[l].cleared(); self.prev[l] = None

    def put(self, lane, lists, img_w, img_h):
        c = self.ctx
        c.put_features(lane, 0, 0, lists.kps[0], None, img_w, img_h)
        c.put_features(lane, 0, 1, lists.kps[1], None, img_w, img_h)
        c.put_matches(lane, 0, lists.matches)
        c.put_match_ids(lane, 0, lists.ids)
        c.put_tracked(lane, lists.tracked, octave=0)

    def shift(self, lanes):
        """the shift-only call; returns {lane: shifted}"""
        c = self.ctx
        moved = {l: lane_shifts(self.stepped[l], c.result(l).error_code) for l in lanes}
        c._process(None, 0, c._mask(lanes)[0])
        for l in lanes:
            self.stepped[l] = True
        return moved

    def step(self, frames, flags=RUN_OPTIMIZE, active=None):
        c = self.ctx
        lanes = list(range(c.n_lanes)) if active is None else sorted(active)
        moved = self.shift(lanes)
        jobs, who = [], []
        for l in lanes:
            if self.prev[l] is not None:
                t = self.tables[l]
                jobs += [(self.prev[l][0], frames[l][0], t.left), (self.prev[l][1], frames[l][1], t.right)]
                who.append(l)
        res = c.lk_track(jobs, self.p.lk) if jobs else []
        for l in lanes:
            t = self.tables[l]
            if l in who:
                j = 2 * who.index(l)
                (ol, sl, _), (or_, sr, _) = res[j], res[j + 1]
            else:                                  # no last pair: the points stand as they are
                ol, or_, sl, sr = t.left, t.right, np.ones(len(t), np.uint8), np.ones(len(t), np.uint8)
            h, w = frames[l][0].shape
            lists, self.tables[l], _ = select(t, ol, or_, sl, sr, self.gate, moved[l], self.H)
            self.put(l, lists, w, h)
            self.prev[l] = (frames[l][0].copy(), frames[l][1].copy())
        if flags & RUN_OPTIMIZE:
            c.run_stages(RUN_OPTIMIZE, lanes if active is not None else None)

    def debug_select(self, lane, left_xy, right_xy, status_l, status_r, img_w, img_h):
        """svo_debug_klt_select's counterpart: the shift and the selection on one lane with the caller's arrays"""
        moved = self.shift([lane])
        lists, self.tables[lane], reasons = select(self.tables[lane], left_xy, right_xy, status_l, status_r, self.gate, moved[lane], self.H)
        self.put(lane, lists, img_w, img_h)
        return lists, reasons
