"""The reference for dmFASTER's dynamic threshold (TEST INFRASTRUCTURE): a literal walk of stage2_detect.cpp:522-546 ("S2") over a
sequence, as if processNewImagePair passed update_dyn_thresholds = true to both of its stage-2 calls (P:166-167).

One estimator keeps m_threshold[octave].  A call detects ONE image: for every octave, (re)size m_threshold when its length is not
nOctaves (S2:522-523), detect at m_threshold[octave] (S2:527-533), count ALL corners found (S2:535), move the threshold by the rule
(S2:540-545).  A frame is the left call, then the right call: the right image is detected at thresholds the left image has moved.

Composed from tests/faster_ref.py (fast12 / corners / detect, the pyramid) with the threshold given per side and octave; Python
floats are IEEE doubles, so `step` is the reference's expression operation for operation."""
import faster_ref as F

DEFAULT_TARGET = 10. / 1000.                                   # S2:46


def step(T, n, wh, target):
    """S2:540-545"""
    feats_density = n / float(wh)
    if feats_density < 0.8 * target:
        return max(1, T - 1)
    if feats_density > 1.2 * target:
        return T + 1
    return T


class Estimator:
    """the members of one rso::CStereoOdometryEstimator that stage 2 touches under dmFASTER"""

    def __init__(self, target=DEFAULT_TARGET, klt_win=4):
        self.target, self.klt_win = target, klt_win
        self.m_threshold = []

    def detect_image(self, img, params):
        """one stage-2 call under dmFASTER with update_dyn_thresholds = true.  Per octave: (keypoints, row table, octave image, raw
        corner count, threshold used)"""
        n_oct = max(1, params.nOctaves)
        keep = F.kps_to_detect(params.orb_nfeats, n_oct)
        out = []
        for o, im in enumerate(F.pyramid(img, n_oct)):
            if len(self.m_threshold) != n_oct:                                                  # S2:522-523
                self.m_threshold = [params.initial_FAST_threshold] * n_oct
            used = self.m_threshold[o]
            k, idx, n = F.detect(im, used, self.klt_win, keep[o], params.min_distance, bool(params.non_maximal_suppression))
            self.m_threshold[o] = step(used, n, im.shape[1] * im.shape[0], self.target)        # S2:537-546
            out.append((k, idx, im, n, used))
        return out

    def frame(self, left, right, params):
        """(feats, stats): feats = the per-octave tuples of faster_ref.faster_features (kl, kr, idx_l, idx_r, img_l, img_r, raw_l, raw_r);
        stats = dict of per-octave lists used_left, used_right, corners_left, corners_right, next"""
        a = self.detect_image(left, params)
        b = self.detect_image(right, params)
        feats = [(l[0], r[0], l[1], r[1], l[2], r[2], l[3], r[3]) for l, r in zip(a, b)]
        stats = {"used_left": [l[4] for l in a], "used_right": [r[4] for r in b], "corners_left": [l[3] for l in a],
                 "corners_right": [r[3] for r in b], "next": list(self.m_threshold)}
        return feats, stats


def walk(frames, params, target=DEFAULT_TARGET, klt_win=4):
    """a fresh estimator over a list of (left, right) pairs: [(feats, stats)] per frame"""
    e = Estimator(target, klt_win)
    return [e.frame(l, r, params) for l, r in frames]
