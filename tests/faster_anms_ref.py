"""The reference for dmFASTER under the adaptive NMS (TEST INFRASTRUCTURE): tests/faster_ref.py with ONE change -- the raw corner list
of an octave image goes through the oracle's m_adaptive_non_max_sup (oracle.anms_copy, S2:141-215: rank = response desc, index asc;
output = radius desc, index asc; num_out_points = kps_to_detect[octave], min_radius_th = 0) in place of the grid NMS.  The row sort,
the pyramid and the assembly per octave are those of faster_ref."""
import numpy as np

import faster_ref as F


def detect(img, t, win, keep):
    """one octave image through stage 2: (final keypoints in m_update_indexes order, the row table, the raw corner count)"""
    from oracle import oracle as O
    h, w = img.shape
    raw = F.corners(img, t, win)
    kept = raw[O.anms_copy(raw, keep)]                                       # S2:599-606
    order, idx = O.row_sort_index(np.ascontiguousarray(kept), h)             # S2:618
    return np.ascontiguousarray(kept[order]), idx, len(raw)


def features(left, right, params, klt_win=4, t_left=None, t_right=None):
    """per octave: (kl, kr, idx_l, idx_r, img_l, img_r, raw_l, raw_r) under dmFASTER + nmsmAdaptive with the fields of `params`;
    t_left / t_right: per-octave thresholds in place of initial_FAST_threshold (the dynamic threshold's walk)"""
    n_oct = max(1, params.nOctaves)
    keep = F.kps_to_detect(params.orb_nfeats, n_oct)
    out = []
    for o, (l, r) in enumerate(zip(F.pyramid(left, n_oct), F.pyramid(right, n_oct))):
        tl = params.initial_FAST_threshold if t_left is None else t_left[o]
        tr = params.initial_FAST_threshold if t_right is None else t_right[o]
        kl, il, nl = detect(l, tl, klt_win, keep[o])
        kr, ir, nr = detect(r, tr, klt_win, keep[o])
        out.append((kl, kr, il, ir, l, r, nl, nr))
    return out


def params(base, t=20, orb_nfeats=500, n_oct=3, **kw):
    """faster_ref.faster_params with non_maximal_suppression = 1 and nmsMethod = nmsmAdaptive"""
    p = F.faster_params(base, t=t, orb_nfeats=orb_nfeats, n_oct=n_oct, nms=1, **kw)
    p.nmsMethod = 1
    return p
