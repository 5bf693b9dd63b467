"""The definition of svo_gftt_detect: a literal numpy walk of this project's Shi-Tomasi corner detector.

The device (stereo_vo_amd/csrc/k_gftt.hip) must equal this walk bit for bit: the response map as float32 patterns, pts, response and
the three info words.  It follows the algorithm of cv::goodFeaturesToTrack (minimum eigenvalue of the structure tensor, a quality
threshold relative to the image's maximum, 3 x 3 local maxima, a greedy minimum distance walked by descending response), but its
arithmetic is this project's own (integer derivatives and sums, one stated order for the double eigenvalue): no equality with OpenCV
is claimed.  Frozen: the tests are written against it.

Choices that the prose description of the detector (include/svo_hip.h) leaves open -- the walk decides:
  * Sobel: dx = (p[y-1][x+1] + 2 p[y][x+1] + p[y+1][x+1]) - (the same at x-1), dy likewise with the axes swapped; no scale factor.
    Image pixels outside the image are read at reflect-101 indices.
  * "Derivatives outside the image are taken at reflect-101 positions" means: the derivative MAPS dx, dy are formed for the w x h pixels
    of the image, and the box sum reads those maps at reflect-101 indices.  (This is not the derivative of the reflected image: that
    one would have the opposite sign of dx behind a vertical border, and of dy behind a horizontal one.)
  * lambda = 0.5 * (double(a + c) - sqrt(double((a - c)^2 + 4 b^2))), the sqrt correctly rounded, each operator one IEEE double
    operation; resp = float32(max(lambda, 0.0)), round to nearest even.
  * quality is a float32 parameter; thr = float32(quality * m) is ONE float32 product of two float32 values.
  * The 3 x 3 maximum test compares float32 values with >=; it is applied only to pixels 1 <= x <= w - 2, 1 <= y <= h - 2, whose eight
    neighbours all exist.  The maximum m is taken over all w x h pixels.
  * Seeds are float32 pairs (x, y).  A seed counts when both coordinates are finite and 0 <= x < w and 0 <= y < h as float32 compares.
    A seed closer than min_distance to a candidate rejects it: fx = float32(x) - sx, fy = float32(y) - sy, float32(float32(fx * fx) +
    float32(fy * fy)) < float32(min_distance * min_distance); min_distance^2 <= 65025 is exact in float32.
  * min_distance = 0 accepts every candidate, seeds or not.
  * limit = min(cap, max_corners) when max_corners > 0, else cap; the output is the first `limit` accepted candidates of the walk.
  * n_cand counts candidates before the distance rule.  With more than `cand_cap` (the device's max(1024, max_cand)) candidates the
    job returns no corners, status 1 and that count.
  * info = (corners written, n_cand, status).
"""
import numpy as np

F = np.float32


class GfttParams:
    def __init__(self, max_corners=0, block=3, min_distance=20, quality=0.01):
        self.max_corners, self.block, self.min_distance = int(max_corners), int(block), int(min_distance)
        self.quality = F(quality)

    def check(self):
        assert self.max_corners >= 0 and self.block in (3, 5, 7) and 0 <= self.min_distance <= 255
        assert np.isfinite(self.quality) and F(0) < self.quality <= F(1)


def _reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def sobel(img):
    """integer 3 x 3 Sobel derivatives at every pixel; image pixels outside the image at reflect-101 indices"""
    h, w = img.shape
    a = img.astype(np.int64)
    ym, y0, yp = _reflect101(np.arange(h) - 1, h), np.arange(h), _reflect101(np.arange(h) + 1, h)
    xm, x0, xp = _reflect101(np.arange(w) - 1, w), np.arange(w), _reflect101(np.arange(w) + 1, w)

    def px(ys, xs):
        return a[np.ix_(ys, xs)]
    dx = (px(ym, xp) + 2 * px(y0, xp) + px(yp, xp)) - (px(ym, xm) + 2 * px(y0, xm) + px(yp, xm))
    dy = (px(yp, xm) + 2 * px(yp, x0) + px(yp, xp)) - (px(ym, xm) + 2 * px(ym, x0) + px(ym, xp))
    return dx, dy


def tensor(img, block):
    """(a, b, c): the sums of dx^2, dx dy, dy^2 over the block x block window of every pixel; the maps read at reflect-101 indices"""
    h, w = img.shape
    dx, dy = sobel(img)
    r = block // 2
    a = np.zeros((h, w), np.int64); b = np.zeros((h, w), np.int64); c = np.zeros((h, w), np.int64)
    for oy in range(-r, r + 1):
        ys = _reflect101(np.arange(h) + oy, h)
        for ox in range(-r, r + 1):
            xs = _reflect101(np.arange(w) + ox, w)
            gx, gy = dx[np.ix_(ys, xs)], dy[np.ix_(ys, xs)]
            a += gx * gx; b += gx * gy; c += gy * gy
    assert (a + c).max() < 2 ** 31
    return a, b, c


def response_of(a, b, c):
    """float32 min-eigenvalue response of integer tensors (arrays of int64)"""
    s = a + c
    d = (a - c) * (a - c) + 4 * b * b
    assert d.max(initial=0) < 2 ** 53
    lam = 0.5 * (s.astype(np.float64) - np.sqrt(d.astype(np.float64)))
    return np.maximum(lam, 0.0).astype(np.float32)


def response_map(img, block):
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 2 and img.shape[0] >= 8 and img.shape[1] >= 8
    return response_of(*tensor(img, block))


def candidates(resp, quality):
    """(m, thr, ys, xs) with the candidates in walk order: resp descending, then raster index ascending"""
    h, w = resp.shape
    m = resp.max()
    thr = F(F(quality) * m)
    inner = resp[1:-1, 1:-1]
    ok = inner > thr
    for oy in range(3):
        for ox in range(3):
            if (oy, ox) != (1, 1):
                ok &= inner >= resp[oy:oy + h - 2, ox:ox + w - 2]
    ys, xs = np.nonzero(ok)
    ys, xs = ys + 1, xs + 1
    order = np.lexsort((ys * w + xs, -resp[ys, xs].astype(np.float64)))
    return m, thr, ys[order], xs[order]


def valid_seeds(seeds, w, h):
    s = np.zeros((0, 2), F) if seeds is None else np.asarray(seeds, F).reshape(-1, 2)
    keep = [i for i in range(len(s))
            if np.isfinite(s[i, 0]) and np.isfinite(s[i, 1]) and F(0) <= s[i, 0] < F(w) and F(0) <= s[i, 1] < F(h)]
    return s[keep]


def detect(img, seeds=None, cap=1 << 30, params=None, cand_cap=1 << 30):
    """-> (pts [n, 2] float32, response [n] float32, info (n, n_cand, status), resp map): the whole walk on one image"""
    p = params or GfttParams()
    p.check()
    resp = response_map(img, p.block)
    h, w = resp.shape
    none = (np.zeros((0, 2), F), np.zeros(0, F))
    m, thr, ys, xs = candidates(resp, p.quality)
    n_cand = len(ys)
    if n_cand > cand_cap:
        return none[0], none[1], (0, n_cand, 1), resp
    limit = min(cap, p.max_corners) if p.max_corners > 0 else cap
    sd = valid_seeds(seeds, w, h)
    md = p.min_distance
    md2f = F(md * md)
    out = []
    for y, x in zip(ys.tolist(), xs.tolist()):
        if len(out) >= limit:
            break
        ok = True
        if md > 0:
            for (ax, ay) in out:
                if (x - ax) * (x - ax) + (y - ay) * (y - ay) < md * md:
                    ok = False
                    break
            if ok and len(sd):
                fx = F(x) - sd[:, 0]
                fy = F(y) - sd[:, 1]
                assert fx.dtype == F
                ok = not bool(((fx * fx + fy * fy) < md2f).any())
        if ok:
            out.append((x, y))
    if not out:
        return none[0], none[1], (0, n_cand, 0), resp
    pts = np.array(out, F).reshape(-1, 2)
    rs = np.array([resp[y, x] for x, y in out], F)
    return pts, rs, (len(out), n_cand, 0), resp
