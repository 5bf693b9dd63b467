"""Inputs and parameter sets of the 16384-entry tests (test_big_lists_cpu.py, test_gpu_big_lists.py): one 2048 x 1536 synthetic
street, rendered once per process, on which the detector keeps between 8192 and 16384 keypoints per image.

  A   ORB, 8 levels, orb_nfeats 10900: 16350 keypoints asked of the detector before the NMS, 2 x 3551 corners ranked at level 0
  B   FAST+ORB, one octave, no NMS, FAST threshold 5: every corner kept (14.4 k), row-by-row pairing without the 1-to-1 rule
      (9.3 k pairings), brute-force or 40 x 40 window tracker
  B'  the frames of B with the brute-force matcher, with and without the 1-to-1 rule
  C   the parameters of A with smSAD / ifmSAD (tests/sad_ref.py is the reference: the oracle refuses these selectors)
  D   stage 4 alone on lists of exactly 16384 entries built from B's
"""
import numpy as np

from stereo_vo_amd import hip
from stereo_vo_amd.abi import north_star_params, DM_FAST_ORB
from stereo_vo_amd.synth import SyntheticStereoWorld

W, H, MAX_KPS, MAX_CAND = 2048, 1536, 16384, 1 << 18
LO, HI = 8192, 16384                      # every list the cases are about is longer than LO and no longer than HI

_cache = {}


def world():
    if "world" not in _cache:
        _cache["world"] = SyntheticStereoWorld(W, H, 1280.0, 0.12, seed=51, n_frames=3)
    return _cache["world"]


def camera():
    return world().camera()


def frames():
    """the three (left, right) frames as numpy arrays"""
    if "frames" not in _cache:
        _cache["frames"] = [tuple(np.ascontiguousarray(x.numpy()) for x in world().render(t)) for t in range(3)]
    return _cache["frames"]


def params_a(orb_nfeats=10900):
    return north_star_params(hip.default_params(), orb_nfeats=orb_nfeats)


def params_b(ifm_method=0, match_method=1, one_to_one=0, fast_th=5):
    p = hip.default_params()
    p.detect_method, p.nOctaves, p.non_maximal_suppression = DM_FAST_ORB, 1, 0
    p.initial_FAST_threshold, p.fast_min_th = fast_th, 1
    p.match_method, p.enable_robust_1to1_match, p.max_y_diff = match_method, one_to_one, 8.0
    p.orb_max_distance, p.orb_max_th = 120.0, 256
    p.ifm_method, p.ifm_win_w, p.ifm_win_h = ifm_method, 40, 40
    return p


def params_c():
    p = params_a()
    p.match_method, p.ifm_method, p.max_y_diff = 2, 2, 2.0
    p.sad_max_distance, p.ifm_sad_max_distance, p.ifm_win_w, p.ifm_win_h = 400, 400, 40, 40
    return p


def record(orc, ro):
    """what one oracle frame leaves behind, copied out (the oracle object moves on)"""
    return {"kl": orc.keypoints(0, 0), "kr": orc.keypoints(0, 1), "m": orc.matches(0), "mri": orc.matches_row_index(0), "tracked": orc.tracked(),
            "outliers": orc.outliers(), "residuals": orc.residuals(), "result": type(ro).from_buffer_copy(ro),
            "valid": bool(ro.valid), "error_code": ro.error_code, "stats": [int(v) for v in ro.track_stats]}


class Replay:
    """a record behind the getters of oracle.Oracle that test_gpu_parity.assert_same_frame reads"""

    def __init__(self, rec):
        self.rec = rec

    def keypoints(self, which=0, side=0):
        assert which == 0
        return self.rec["kr" if side else "kl"]

    def matches(self, which=0):
        assert which == 0
        return self.rec["m"]

    def tracked(self):
        return self.rec["tracked"]

    def outliers(self):
        return self.rec["outliers"]

    def residuals(self):
        return self.rec["residuals"]


def oracle_run(O, key, p, first=0, n=3):
    """the oracle's records of frames first .. n - 1 under parameters p, computed once per process and key (never modified afterwards)"""
    if key not in _cache:
        orc, cam, out = O.Oracle(p), camera(), []
        for L, R in frames()[first:n]:
            out.append(record(orc, orc.process(L, R, cam)))
        _cache[key] = out
    return _cache[key]


def pairings_row_index(m, kl, h=H):
    """matches_lr_row_index (S3:425-445) of a pairing list in ascending left row: ri[y] = pairings with left y <= y - 1, ri[h] = all"""
    ys = kl["y"][m["queryIdx"]]
    ri = np.zeros(h + 1, np.int64)
    idx = 0
    for y in range(h):
        ri[y] = idx
        while idx < len(m) and ys[idx] <= np.float32(y):
            idx += 1
    ri[h] = len(m)
    return ri


def full_lists(rec):
    """One frame of case B blown up to EXACTLY 16384 keypoints per side and 16384 pairings.  Extra keypoint e of a side is a copy of
    the keypoint pairing e joins on that side (same position, same descriptor); extra pairing e joins the two copies of pairing
    e % len(m) -- or, once a side has run out of extra keypoints, the original keypoint again -- at the original distance.  Every
    copied descriptor ties with its original in the tracker's brute force, and repeated pairings claim the same train indices.  The
    pairings are then put in ascending left row (stable), as stage 3 delivers them.  Returns (kl, dl, kr, dr, m, row index of m)."""
    (kl, dl), (kr, dr), m = rec["kl"], rec["kr"], rec["m"]
    nl, nr, nm = len(kl), len(kr), len(m)
    el, er, em = HI - nl, HI - nr, HI - nm
    assert 0 < el <= em and 0 < er <= em and el <= nm and er <= nm, (nl, nr, nm)
    src = np.arange(em) % nm
    kl2 = np.concatenate([kl, kl[m["queryIdx"][src[:el]]]]); dl2 = np.concatenate([dl, dl[m["queryIdx"][src[:el]]]])
    kr2 = np.concatenate([kr, kr[m["trainIdx"][src[:er]]]]); dr2 = np.concatenate([dr, dr[m["trainIdx"][src[:er]]]])
    extra = m[src].copy()
    e = np.arange(em)
    extra["queryIdx"] = np.where(e < el, nl + e, m["queryIdx"][src])
    extra["trainIdx"] = np.where(e < er, nr + e, m["trainIdx"][src])
    m2 = np.concatenate([m, extra])
    m2 = np.ascontiguousarray(m2[np.argsort(kl2["y"][m2["queryIdx"]], kind="stable")])
    assert len(kl2) == len(kr2) == len(m2) == HI
    return np.ascontiguousarray(kl2), np.ascontiguousarray(dl2), np.ascontiguousarray(kr2), np.ascontiguousarray(dr2), m2, pairings_row_index(m2, kl2)
