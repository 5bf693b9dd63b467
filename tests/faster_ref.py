"""The reference for dmFASTER (TEST INFRASTRUCTURE): stage2_detect.cpp:519-576 ("S2") in plain numpy.

The CPU oracle has no dmFASTER, and MRPT (whose detectFeatures_SSE2_FASTER12 and CImage::KLT_response the reference calls) is not
vendored with it, so the two definitions are written down here as published:

  * FAST-12: (x, y) with 3 <= x < w-3, 3 <= y < h-3 is a corner iff at least 12 CONTIGUOUS pixels of the 16-pixel Bresenham circle
    of radius 3 are all > I(x, y) + t or all < I(x, y) - t (strict, cyclic); no score, no 3 x 3 suppression, raster order;
  * KLT response: exactly 0.0f unless win+1 <= x < w-win-1 and win+1 <= y < h-win-1 (S2:565); otherwise the smaller eigenvalue
    of the gradient matrix over the (2 win + 1)^2 window, central differences, int32 sums, float32 arithmetic with one IEEE
    operation per operator (klt_from_sums; the clamp of a negative radicand is this project's).

Everything downstream is composed from oracle entry points that exist: the grid NMS in the oracle's total order (oracle.nms_copy:
response desc, detector index asc -- the detector index is the raster position), m_update_indexes (oracle.row_sort_index) and
the x1/2 pyramid (oracle.half_smooth).  Downstream of the lists the SAD walks of tests/sad_ref.py apply unchanged."""
import numpy as np

from stereo_vo_amd.abi import keypoint_dtype

CIRCLE = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3),
          (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3))     # clockwise from the top


def fast12(img, t):
    """(xs, ys) of the FAST-12 corners of a uint8 image at threshold t, in raster order (y, then x)"""
    h, w = img.shape
    if w < 7 or h < 7:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    I = img.astype(np.int32)
    c = I[3:h - 3, 3:w - 3]
    ring = [I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE]
    corner = np.zeros(c.shape, bool)
    for masks in ([r > c + t for r in ring], [r < c - t for r in ring]):
        for start in range(16):
            run = masks[start].copy()
            for k in range(1, 12):
                run &= masks[(start + k) % 16]
            corner |= run
    ys, xs = np.nonzero(corner)                                  # np.nonzero walks in row-major order: raster
    return xs + 3, ys + 3


def klt_from_sums(gxx, gxy, gyy, win):
    """float32 response from the int32 sums (scalars or arrays), one IEEE operation per operator"""
    f = np.float32
    side = 2 * int(win) + 1
    K = f(0.5) / f(side * side)
    Gxx, Gxy, Gyy = np.asarray(gxx, np.int32).astype(f) * K, np.asarray(gxy, np.int32).astype(f) * K, np.asarray(gyy, np.int32).astype(f) * K
    t = Gxx + Gyy
    de = Gxx * Gyy - Gxy * Gxy
    rad = t * t - f(4.0) * de
    rad = np.where(rad < 0, f(0.0), rad).astype(f)
    return (f(0.5) * (t - np.sqrt(rad))).astype(f)


def klt_sums(img, x, y, win):
    """(gxx, gxy, gyy) over [x-win, x+win] x [y-win, y+win]; every pixel read lies inside the image when the border rule holds"""
    I = img.astype(np.int64)
    ys, xs = slice(y - win, y + win + 1), slice(x - win, x + win + 1)
    dx = I[ys, x - win + 1:x + win + 2] - I[ys, x - win - 1:x + win]
    dy = I[y - win + 1:y + win + 2, xs] - I[y - win - 1:y + win, xs]
    s = int((dx * dx).sum()), int((dx * dy).sum()), int((dy * dy).sum())
    assert all(abs(v) < 2 ** 31 for v in s)
    return s


def in_klt_border(x, y, w, h, win):
    return x >= win + 1 and y >= win + 1 and x < w - win - 1 and y < h - win - 1


def klt_response(img, x, y, win):
    h, w = img.shape
    if not in_klt_border(x, y, w, h, win):
        return np.float32(0.0)
    return np.float32(klt_from_sums(*klt_sums(img, x, y, win), win))


def responses(img, xs, ys, win):
    """klt_response of many positions at once (box sums over the whole image through integral images; int64, the sums fit int32)"""
    h, w = img.shape
    out = np.zeros(len(xs), np.float32)
    if not len(xs) or w < 2 * win + 3 or h < 2 * win + 3:
        return out
    I = img.astype(np.int64)
    dx = np.zeros((h, w), np.int64); dy = np.zeros((h, w), np.int64)
    dx[:, 1:w - 1] = I[:, 2:] - I[:, :w - 2]
    dy[1:h - 1, :] = I[2:, :] - I[:h - 2, :]
    ok = (xs >= win + 1) & (ys >= win + 1) & (xs < w - win - 1) & (ys < h - win - 1)
    x, y = xs[ok], ys[ok]
    sums = []
    for prod in (dx * dx, dx * dy, dy * dy):
        S = np.zeros((h + 1, w + 1), np.int64)
        S[1:, 1:] = prod.cumsum(0).cumsum(1)
        sums.append(S[y + win + 1, x + win + 1] - S[y - win, x + win + 1] - S[y + win + 1, x - win] + S[y - win, x - win])
    assert all(np.abs(s).max(initial=0) < 2 ** 31 for s in sums)
    out[ok] = klt_from_sums(sums[0], sums[1], sums[2], win)
    return out


def corners(img, t, win):
    """the detector's output before the NMS: keypoint records in raster order (S2:31-42: pt and response into default cv::KeyPoints)"""
    xs, ys = fast12(img, t)
    k = np.zeros(len(xs), keypoint_dtype)
    k["x"], k["y"], k["size"], k["angle"], k["octave"], k["class_id"] = xs, ys, 0.0, -1.0, 0, -1
    k["response"] = responses(img, xs, ys, win)
    return k


def detect(img, t, win, keep, min_distance, nms):
    """one octave image through stage 2: (final keypoints in m_update_indexes order, the row table, the raw corner count)"""
    from oracle import oracle as O
    h, w = img.shape
    raw = corners(img, t, win)
    kept = raw[O.nms_copy(raw, min_distance, w, h, keep)] if nms else raw      # S2:583-598 / 613-614
    order, idx = O.row_sort_index(np.ascontiguousarray(kept), h)             # S2:618
    return np.ascontiguousarray(kept[order]), idx, len(raw)


def kps_to_detect(orb_nfeats, n_oct):
    """S2:404-407"""
    k0 = int(float(orb_nfeats) * float(2 * n_oct) / (2.0 ** n_oct - 1.0))
    return [k0 if o == 0 else int(np.floor(k0 / 2.0 ** o + 0.5)) for o in range(n_oct)]


def pyramid(img, n_oct):
    from oracle import oracle as O
    out = [np.ascontiguousarray(img)]
    for _ in range(1, n_oct):
        out.append(O.half_smooth(out[-1]))
    return out


def faster_features(left, right, params, klt_win=4):
    """per octave: (kl, kr, idx_l, idx_r, img_l, img_r, raw_l, raw_r) under dmFASTER with the fields of `params`"""
    n_oct = max(1, params.nOctaves)
    keep = kps_to_detect(params.orb_nfeats, n_oct)
    out = []
    for o, (l, r) in enumerate(zip(pyramid(left, n_oct), pyramid(right, n_oct))):
        kl, il, nl = detect(l, params.initial_FAST_threshold, klt_win, keep[o], params.min_distance, bool(params.non_maximal_suppression))
        kr, ir, nr = detect(r, params.initial_FAST_threshold, klt_win, keep[o], params.min_distance, bool(params.non_maximal_suppression))
        out.append((kl, kr, il, ir, l, r, nl, nr))
    return out


def faster_params(base, t=20, orb_nfeats=500, n_oct=3, nms=1, sad=400, ifm_sad=400):
    """the reference's out-of-the-box configuration on this library's record: dmFASTER + smSAD + ifmSAD, grid NMS, min_distance 3,
    max_y_diff 2, windows 16 / 16"""
    import sad_ref as S
    p = S.photo_params(base, orb_nfeats=orb_nfeats, sad_max_distance=sad, ifm_sad_max_distance=ifm_sad)
    p.detect_method, p.nOctaves, p.initial_FAST_threshold, p.non_maximal_suppression, p.nmsMethod, p.min_distance = 2, n_oct, t, nms, 0, 3
    return p
