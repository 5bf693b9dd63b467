"""Descriptor lists built by hand for the edges of the product brute-force matcher itself, k_hamming_f4 (csrc/k_match.hip: FP4 matrix-core
products instead of popcount, the nearest neighbour packed into one f32 accumulator as 2 ham - 256 + index / 8192), and of its int8 A/B form
(numpy only: no GPU, and the oracle is imported by the functions that need it).  tests/match_scenes.py keeps away from these edges on
purpose -- unique planted matches, identity pairing lists --; here the lists are made so that EVERY output word of the matcher is visible
and the ties, the tile / block / split boundaries, the distances 0 .. 256 and the gather through the pairing lists decide it.

The reference is popcount in integers plus numpy's argmin (the first minimum), nothing else: a stage-3 scene carries the svo_dmatch array
(i, argmin_i, 0, float(min_i)) it predicts, a stage-4 scene its tracked pairs.

A stage-3 scene is a dict: kl dl kr dr W H (match_scenes' keys), `D` (all distances, nq x nt), `want` (the predicted pairings), `want_ri` (their
row table), `family` and `plan` (what was planted where).  It is run under orb_max_distance 256, enable_robust_1to1_match 0, brute force:
every keypoint sits on ONE row, every left x is 2 .. 266 pixels right of every right x, so no filter of stage 3 drops anything and the
pairings ARE the matcher's words.  A stage-4 scene is a dict of ransac_scenes' keys with `pri` / `cri`, `want` (predicted tracked pairs) and
`tL tR dL dR` (per previous pairing its nearest current pairing and distance, left and right, through the pairing lists).  Its pairing
lists are no identity: unpaired keypoints lie between the paired ones, the right lists are in another order than the left ones (shuffled
inside every row, so both stay in row order), queryIdx ascends and trainIdx is a permutation.  Motion is sideways, as in match_scenes.
tests/test_ham_scenes_cpu.py asserts all of that on the oracle alone; tests/test_gpu_ham_scenes.py runs the scenes on the kernels."""
import functools

import numpy as np

from stereo_vo_amd.abi import dmatch_dtype, index_pair_dtype

import match_scenes as MS
from match_scenes import hamming_matrix, flipped, features_row_index, matches_row_index, drawn, Retry      # noqa: F401
from ransac_scenes import _kps, put_scene, oracle_track, check_case                                       # noqa: F401

W, H, ROW = 640, 480, 7
ORB_TH = 256                          # orb_max_distance of every scene here: no distance is over the threshold


def rand_desc(rng, n):
    return rng.randint(0, 256, (n, 32)).astype(np.uint8)


def distances(Q, T):
    """hamming_matrix in slices of 64 queries (a 16384-row train list stays a few MB per slice)"""
    Q, T = np.ascontiguousarray(Q, np.uint8).reshape(-1, 32), np.ascontiguousarray(T, np.uint8).reshape(-1, 32)
    if len(Q) == 0 or len(T) == 0:
        return np.zeros((len(Q), len(T)), np.int32)
    return np.concatenate([hamming_matrix(Q[s:s + 64], T) for s in range(0, len(Q), 64)])


def even_weight(T):
    """bit 0 of every row of odd weight flipped: any two rows are an even number of bits apart"""
    T[:, 0] ^= (MS._POP8[T].sum(1) & 1).astype(np.uint8)
    return T


def between(rng, a, b):
    """a descriptor exactly half way between a and b (an even number h of bits apart): h / 2 of the differing bits of a flipped"""
    diff = np.flatnonzero(np.unpackbits(a ^ b, bitorder="little"))
    assert len(diff) % 2 == 0
    out = a.copy()
    for bit in rng.choice(diff, len(diff) // 2, replace=False):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def at_distances(rng, q, d):
    """len(d) rows, row j exactly d[j] bits away from q (d[j] = 256: the complement): d[j] cyclically adjacent slots of one shuffled bit order"""
    d = np.asarray(d, np.int64)
    start = rng.randint(0, 256, len(d))
    mask = ((np.arange(256)[None, :] - start[:, None]) % 256) < d[:, None]
    bits = np.zeros((len(d), 256), np.uint8)
    bits[:, rng.permutation(256)] = mask
    return np.packbits(bits, axis=1, bitorder="little") ^ q[None, :]


def minima(D):
    """per query the train rows that attain its minimum"""
    return [np.flatnonzero(r == r.min()) for r in D]


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------------------------------------------------------------------
def _stereo(family, Q, T, plan=()):
    """right keypoint j at x = j / 64, left keypoint i at x = 258 + i / 64, all on row ROW (exact in binary32; 16384 right keypoints end
    under x = 256): (int)(xl - xr) is 2 .. 266 for every pair and the row difference 0"""
    Q, T = np.ascontiguousarray(Q, np.uint8).reshape(-1, 32), np.ascontiguousarray(T, np.uint8).reshape(-1, 32)
    nq, nt = len(Q), len(T)
    kr = _kps(np.stack([np.arange(nt) / 64.0, np.full(nt, float(ROW))], 1).astype(np.float32))
    kl = _kps(np.stack([258.0 + np.arange(nq) / 64.0, np.full(nq, float(ROW))], 1).astype(np.float32))
    D = distances(Q, T)
    want = np.zeros(nq if nt else 0, dmatch_dtype)
    if len(want):
        want["queryIdx"], want["trainIdx"], want["distance"] = np.arange(nq), D.argmin(1), D.min(1)
    return dict(family=family, kl=kl, dl=Q, kr=kr, dr=T, W=W, H=H, D=D, want=want, want_ri=matches_row_index(want, kl, H), plan=list(plan))


def _exactly(s, q, rows, d=None):
    """query q's minimum is attained by exactly `rows` (and is d)"""
    r = s["D"][q]
    if list(np.flatnonzero(r == r.min())) != list(rows) or (d is not None and r.min() != d):
        raise Retry("planted")


LENGTHS = [(1, 1), (1, 33), (1, 289), (31, 31), (31, 96), (32, 32), (32, 257), (33, 33), (33, 63), (33, 97), (64, 63), (64, 128), (64, 289), (65, 64), (65, 129),
           (255, 65), (255, 255), (256, 31), (256, 97), (256, 256), (257, 1), (257, 257), (513, 32), (513, 129), (513, 289)]


@drawn
def lengths(rng, nq, nt, turn=0, family="lengths"):
    """random lists (their own minima tie now and then), and planted from the last query down, as many as fit: copies of the last row, of
    row 32; rows 0 and 31 one bit away; ties (31, 32), (middle, last), (0, last).  `turn` rotates which plant comes first."""
    T, Q = even_weight(rand_desc(rng, nt)), rand_desc(rng, nq)
    cand = []
    if nt:
        cand = [("copy", nt - 1, 0), ("near", 0, 1)]
        if nt > 32:
            cand += [("tie", 31, 32), ("copy", 32, 0), ("near", 31, 1)]
        if nt > 2:
            cand += [("tie", (nt - 1) // 2, nt - 1), ("tie", 0, nt - 1)]
        cand = cand[turn % len(cand):] + cand[:turn % len(cand)]
    plan = []
    step = max(1, nq // max(1, len(cand)))
    for i, (kind, a, b) in enumerate(cand[:nq]):
        q = nq - 1 - i * step
        Q[q] = between(rng, T[a], T[b]) if kind == "tie" else flipped(rng, T[a], b)
        plan.append((q, kind, a, b))
    s = _stereo(family, Q, T, plan)
    for q, kind, a, b in plan:
        _exactly(s, q, [a, b] if kind == "tie" else [a], None if kind == "tie" else b)
    return s


TIE_NT, TIE_TILE = 128, 1             # the tie scene's train list: four tiles; `a` walks the rows of tile 1


def tie_classes(r):
    """the partners b > a of a = 32 + r: the next row of a's register group (rows 8 g + 4 kb + 0 .. 3 sit in four consecutive accumulator
    registers of one lane half; from a group's last row on: the next register of the same lane half, five rows on; from the half's last register: the next row),
    the row of the other lane half at the same place (a + 4), the same row one tile later, the list's last row"""
    a = 32 * TIE_TILE + r
    nxt = a + 1 if r % 4 < 3 else (a + 5 if r + 5 < 32 else a + 1)
    return [("next", nxt), ("half", a + 4), ("tile", a + 32), ("last", TIE_NT - 1)]


@drawn
def tie_positions(rng):
    """128 queries, each exactly half way between two train rows a < b and farther from every other row"""
    T = even_weight(rand_desc(rng, TIE_NT))
    Q, plan = [], []
    for r in range(32):
        for cls, b in tie_classes(r):
            plan.append((len(Q), cls, 32 * TIE_TILE + r, b)); Q.append(between(rng, T[32 * TIE_TILE + r], T[b]))
    s = _stereo("ties", Q, T, plan)
    for q, _, a, b in plan:
        _exactly(s, q, [a, b])
    return s


@drawn
def tie_boundaries(rng, first, nt=289):
    """a 289-row list (nine whole tiles and a tenth of one row: whatever the split count, every split boundary is one of its tile
    boundaries).  first = 0: one query half way between rows 32 k - 1 and 32 k for every k -- the winner is the LAST row of its tile;
    first = 1: row 32 k has an exact copy 37 rows on (k = 8: the last row), the query is three bits from both -- the winner is the FIRST
    row of its tile, the loser in the next tile.  Random queries bring the list to 33."""
    T = even_weight(rand_desc(rng, nt))
    Q, plan = [], []
    for k in range(1, (nt - 1) // 32 + 1 - first):
        a, b = (32 * k, min(32 * k + 37, nt - 1)) if first else (32 * k - 1, 32 * k)
        if first:
            T[b] = T[a]
        plan.append((len(plan), "first" if first else "last", a, b))
    for _, _, a, b in plan:
        Q.append(flipped(rng, T[a], 3) if first else between(rng, T[a], T[b]))
    s = _stereo("ties", Q + list(rand_desc(rng, 33 - len(Q))), T, plan)
    for q, _, a, b in plan:
        _exactly(s, q, [a, b])
    return s


DIST = (0, 1, 127, 128, 129, 255, 256)
DIST_NT = 65
DIST_WINNERS = (0, 31, 32, DIST_NT - 1)


@drawn
def distance_near(rng):
    """d = 0 and 1 from a random list, the winner at 0, 31, 32 and the last row"""
    T = rand_desc(rng, DIST_NT)
    plan = [(i, "d", w, d) for i, (d, w) in enumerate((d, w) for d in (0, 1) for w in DIST_WINNERS)]
    s = _stereo("distances", [flipped(rng, T[w], d) for _, _, w, d in plan], T, plan)
    for q, _, w, d in plan:
        _exactly(s, q, [w], d)
    return s


@drawn
def distance_far(rng, d, w, nt=DIST_NT, nq=3, family="distances"):
    """the nearest row at a LARGE distance d: the train list is made of near-complements of the query -- row w exactly d bits away, every
    other row d + 1 .. d + 12 (256 at the most: d = 255 leaves the complement itself, d = 256 makes every row the complement and the
    first one must win).  The nq queries are one descriptor."""
    q = rand_desc(rng, 1)[0]
    far = np.minimum(256, d + 1 + rng.randint(0, 12, nt))
    far[w] = d
    s = _stereo(family, np.stack([q] * nq), at_distances(rng, q, far), [(i, "d", w, d) for i in range(nq)])
    for i in range(nq):
        _exactly(s, i, [w] if d < 256 else range(nt), d)
    return s


WIDE_NT = (8191, 8192, 8193, 8225, 16383, 16384)


@drawn
def wide_lengths(rng, nt, nq=40):
    """train lists around 8192 and 16384 rows: copies of rows 0, 8191, 8192, 8193 and the last one, the same one bit away, ties
    (8191, 8192) and (8192, last); the other queries are random"""
    T, Q = even_weight(rand_desc(rng, nt)), rand_desc(rng, nq)
    plan = []
    winners = sorted(set(w for w in (0, 8191, 8192, 8193, nt - 1) if w < nt))
    for d in (0, 1):
        for w in winners:
            plan.append((len(plan), "d", w, d)); Q[len(plan) - 1] = flipped(rng, T[w], d)
    for a, b in ((8191, 8192), (8192, nt - 1)):
        if a < b < nt:
            plan.append((len(plan), "tie", a, b)); Q[len(plan) - 1] = between(rng, T[a], T[b])
    s = _stereo("wide", Q, T, plan)
    for q, kind, a, b in plan:
        _exactly(s, q, [a, b] if kind == "tie" else [a], None if kind == "tie" else b)
    return s


STEREO = (
    [("len-%d-%d" % (nq, nt), lengths, (1, nq, nt, i)) for i, (nq, nt) in enumerate(LENGTHS)]
    + [("ties-positions", tie_positions, (2,)), ("ties-289-last", tie_boundaries, (3, 0)), ("ties-289-first", tie_boundaries, (3, 1))]
    + [("dist-near", distance_near, (4,))] + [("dist-%d-%d" % (d, w), distance_far, (5, d, w)) for d in (127, 128, 129, 255) for w in DIST_WINNERS]
    + [("dist-256", distance_far, (5, 256, 0))]
    # lists for the lanes test: an empty train list, an empty query list
    + [("lane-40-0", lengths, (6, 40, 0, 0, "lanes")), ("lane-0-40", lengths, (6, 0, 40, 0, "lanes"))]
)
# (a minimum of 256 is the first row's, always: only the smaller distances can be planted past row 8192)
WIDE = (
    [("wide-%d" % nt, wide_lengths, (7, nt)) for nt in WIDE_NT]
    + [("wide-dist-%d-%d" % (d, w), distance_far, (8, d, w, 8225, 3, "wide")) for d in (127, 128) for w in (8191, 8192)]
    + [("wide-dist-256", distance_far, (8, 256, 0, 8225, 3, "wide"))]
)
FAMILY_COUNTS = dict(lengths=25, ties=3, distances=18, lanes=2, wide=11)
LANES = ["len-257-257", "len-33-97", "lane-40-0", "len-513-289", "lane-0-40"]          # five lanes of one call
LANE_SWAP = "len-64-128"                                                              # what the idle lane is given
OCTAVES = ["len-65-129", "len-256-97"]                                                # octave 0, octave 1 of one lane


def stereo_names(family=None):
    return [nm for nm, _, _ in STEREO if family is None or scene(nm)["family"] == family]


def wide_names():
    return [nm for nm, _, _ in WIDE]


def stereo_params(p):
    """the parameter record every stage-3 scene is run under: brute force, no 1-to-1 filter, no distance over the threshold"""
    q = p.copy()
    q.match_method, q.enable_robust_1to1_match, q.orb_max_distance, q.max_y_diff = 0, 0, float(ORB_TH), 1.0
    return q


def oracle_match(p, s, img=None):
    """the oracle's stage 3 on a scene under the row tables the library builds for put lists: (pairings, their row table)"""
    from oracle import oracle
    w, h = img or (s["W"], s["H"])
    return oracle.match_lr(p, ORB_TH, s["kl"], s["dl"], features_row_index(s["kl"], h), s["kr"], s["dr"], features_row_index(s["kr"], h), w, h)


# ---------------------------------------------------------------------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------------------------------------------------------------------
def _within_rows(rng, pos):
    """a permutation of a row-sorted list that shuffles inside every row: the permuted list is in row order too"""
    perm = np.arange(len(pos))
    for y in np.unique(pos[:, 1]):
        idx = np.flatnonzero(pos[:, 1] == y)
        perm[idx] = rng.permutation(idx)
    return perm


def _frame(rng, pos, paired):
    """One frame's lists from its left keypoint positions (row-sorted) and the indices of the paired ones (ascending): the right list is
    the left one 20 pixels to the left, shuffled inside its rows.  -> (left kps, right kps, pairings)"""
    perm = _within_rows(rng, pos)
    inv = np.empty(len(pos), np.int64); inv[perm] = np.arange(len(pos))
    m = np.zeros(len(paired), dmatch_dtype)
    m["queryIdx"], m["trainIdx"], m["distance"] = paired, inv[paired], 10.0
    return _kps(pos.astype(np.float32)), _kps((pos[perm] - np.array([20.0, 0.0])).astype(np.float32)), m


def expect_track(s):
    """Stage 4's brute-force tracker from popcount and argmin alone: the descriptors of the paired features gathered through the pairing
    lists (S4:105-131), per previous pairing the first minimum on either side, the sequential joint filter (S4:145-160; no distance
    is over 256), the consistency test (S4:282).  The RANSAC keeps every survivor of a sideways motion."""
    pm, cm = s["pm"], s["cm"]
    DL = distances(s["pdl"][pm["queryIdx"]], s["cdl"][cm["queryIdx"]]); DR = distances(s["pdr"][pm["trainIdx"]], s["cdr"][cm["trainIdx"]])
    tL, tR = DL.argmin(1), DR.argmin(1)
    takenL, takenR, out = set(), set(), []
    for k in range(len(pm)):
        if tL[k] in takenL or tR[k] in takenR:
            continue
        takenL.add(tL[k]); takenR.add(tR[k])
        if tL[k] == tR[k]:
            out.append((k, tL[k]))
    want = np.zeros(len(out), index_pair_dtype)
    if out:
        want["first"], want["second"] = np.array(out).T
    return dict(want=want, tL=tL, tR=tR, dL=DL.min(1), dR=DR.min(1), DL=DL, DR=DR)


@drawn
def track(rng, nprev, ncur, extra=(), step=8):
    """ncur current pairings among ncur + ncur // 3 + 3 keypoints, nprev previous ones among nprev + nprev // 3 + 3.  Planted in the
    current PAIRING order (a the wanted pairing, b its copy further on, wanted by nobody):
      both    pairing ncur - 3 repeats pairing 3 on both sides            tile    pairing 32 m repeats pairing 32 m - 1 on both sides, every m
      left    pairing ncur - 5 repeats pairing 7 on the left side only     (`extra`: further (a, b) of that kind)
    Every a is wanted by one previous pairing, 1 .. 7 bits away on the left and 1 .. 5 on the right; the other previous pairings want
    current pairings of their own while there are any, then one that is taken (a collision).  Three previous pairings have DECOYS: an
    unpaired current keypoint, with an index below ncur, that holds their own descriptor -- on the left and on the right."""
    n_ckp, n_pkp = ncur + ncur // 3 + 3, nprev + nprev // 3 + 3
    cpos = MS._grid(rng, n_ckp, step=step)
    cpaired = np.sort(rng.choice(n_ckp, ncur, replace=False))
    ckl, ckr, cm = _frame(rng, cpos, cpaired)
    TL, TR = rand_desc(rng, ncur), rand_desc(rng, ncur)
    plants = [("both", 3, ncur - 3), ("left", 7, ncur - 5)] + [("tile", 32 * m - 1, 32 * m) for m in range(1, (ncur - 1) // 32 + 1) if not extra or m == 1] + [("tile", a, b) for a, b in extra]
    for kind, a, b in plants:
        TL[b] = TL[a]
        if kind != "left":
            TR[b] = TR[a]
    cdl, cdr = rand_desc(rng, n_ckp), rand_desc(rng, n_ckp)
    cdl[cm["queryIdx"]], cdr[cm["trainIdx"]] = TL, TR
    # which current pairing every previous pairing wants
    forced = [a for _, a, _ in plants] + [t for t in (0, ncur - 1) if extra]
    losers = set(b for _, _, b in plants)
    free = [t for t in rng.permutation(ncur) if t not in losers and t not in forced]
    t = (forced + free)[:nprev]
    t = np.array(t + list(rng.choice(forced + free, nprev - len(t))), np.int64)
    dL, dR = 1 + np.arange(nprev) % 7, 1 + np.arange(nprev) % 5
    qL = np.stack([flipped(rng, TL[a], d) for a, d in zip(t, dL)]); qR = np.stack([flipped(rng, TR[a], d) for a, d in zip(t, dR)])
    ppos = cpos[cpaired[t]] - np.stack([rng.randint(2, 41, nprev), np.zeros(nprev, np.int64)], 1)
    allp = np.concatenate([ppos, MS._grid(rng, n_pkp - nprev, step=step)])
    order = np.lexsort((np.arange(n_pkp), allp[:, 0], allp[:, 1]))
    at = np.empty(n_pkp, np.int64); at[order] = np.arange(n_pkp)
    ko = np.argsort(at[:nprev])                                                # the previous pairings in the order of their left keypoints
    pkl, pkr, pm = _frame(rng, allp[order], at[:nprev][ko])
    t, qL, qR = t[ko], qL[ko], qR[ko]
    pdl, pdr = rand_desc(rng, n_pkp), rand_desc(rng, n_pkp)
    pdl[pm["queryIdx"]], pdr[pm["trainIdx"]] = qL, qR
    # decoys: copies of three queries in unpaired current keypoints
    loose_l, loose_r = np.setdiff1d(np.arange(ncur), cm["queryIdx"]), np.setdiff1d(np.arange(ncur), cm["trainIdx"])
    decoys = []
    for i, k in enumerate((0, nprev // 2, nprev - 1)):
        ul, ur = loose_l[(i * len(loose_l)) // 3], loose_r[(i * len(loose_r)) // 3]
        cdl[ul], cdr[ur] = qL[k], qR[k]
        decoys.append((k, ul, ur))
    s = dict(pkl=pkl, pkr=pkr, pdl=pdl, pdr=pdr, pm=pm, ckl=ckl, ckr=ckr, cdl=cdl, cdr=cdr, cm=cm, W=W, H=H, plan_t=t, plants=plants, decoys=decoys)
    s["pri"], s["cri"] = matches_row_index(pm, pkl, H), matches_row_index(cm, ckl, H)
    s.update(expect_track(s))
    # every previous pairing finds what it was meant to find, at the planted distance, and ties only with the planted copies
    copies = {a: b for _, a, b in plants}
    if not ((s["tL"] == t).all() and (s["tR"] == t).all() and (s["dL"] == dL[ko]).all() and (s["dR"] == dR[ko]).all()):
        raise Retry("planted")
    for k in range(nprev):
        kind = [kd for kd, a, _ in plants if a == t[k]]
        tiesL, tiesR = np.flatnonzero(s["DL"][k] == s["dL"][k]), np.flatnonzero(s["DR"][k] == s["dR"][k])
        if list(tiesL) != ([t[k], copies[t[k]]] if kind else [t[k]]) or list(tiesR) != ([t[k], copies[t[k]]] if kind and kind[0] != "left" else [t[k]]):
            raise Retry("ties")
    return s


TRACK_SIZES = [(32, 33), (33, 64), (32, 65), (33, 97), (255, 257), (256, 257), (257, 257), (256, 65), (257, 97)]
TRACK = [("track-%d-%d" % sz, track, (9,) + sz) for sz in TRACK_SIZES]
# a current pairing list past 8192: ties across 8191 / 8192 and 4095 / 4096, wanted pairings 0 and the last one
TRACK_WIDE = [("track-wide-300-8200", track, (10, 300, 8200, ((8191, 8192), (4095, 4096), (8193, 8198)), 4))]


def track_names():
    return [nm for nm, _, _ in TRACK]


def track_params(p):
    q = p.copy()
    q.ifm_method, q.orb_max_distance = 0, float(ORB_TH)
    return q


@functools.lru_cache(maxsize=None)
def scene(name):
    for nm, gen, args in STEREO + WIDE + TRACK + TRACK_WIDE:
        if nm == name:
            return gen(*args)
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------------------------------------------
# the accumulator key of k_hamming_f4 in numpy binary32, operation for operation
# ---------------------------------------------------------------------------------------------------------------------------------------
def f4_key(ham, row, j0):
    """what the kernel holds for train row j0 + row (row < 32, j0 a multiple of 32) at distance ham: the C operand row / 8192 plus the
    exact product sum 2 ham - 256, then the tile origin j0 / 8192 added to the tile's minimum"""
    f = np.float32
    c = np.asarray(row).astype(f) * f(1.0 / 8192.0)
    return (c + (2 * np.asarray(ham) - 256).astype(f)) + np.asarray(j0).astype(f) * f(1.0 / 8192.0)


def f4_unpack(m, wide):
    """the kernel's unpacking of a key: (ham, index)"""
    fl = np.floor(m)
    ham = (fl.astype(np.int64) + 256) >> 1
    base = (2 * ham - 256).astype(np.float32) if wide else fl
    return ham, ((m - base) * np.float32(8192.0)).astype(np.int64)
