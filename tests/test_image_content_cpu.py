"""CPU guard of tests/image_content.py: the structured images keep the properties the GPU tests rely on.

Computed from the oracle and tests/independent_ref.py alone (no GPU, no HIP library):
  * the four tie contents give at least TIE_FLOOR tied Harris responses among the detector's raw keypoints of a 640x480 frame
    (750 requested, 8 levels, FAST 20), `periodic` and `checker` repeated descriptors too -- the floor is a condition the GPU
    tests depend on, not a measurement;
  * for every content and pyramid level, the list cv::KeyPointsFilter::retainBest keeps -- every candidate at or above the
    score of the 2 x quota-th best, after the strict 3x3 NMS, border 31 -- fits the selection kernels' SEL_MAX = 2048
    entries, so a device that reports SVO_ST_CAND_OVERFLOW on these frames has no excuse."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_content as IC                     # noqa: E402
import independent_ref as IR                   # noqa: E402

SEL_MAX = 2048
EDGE = 31


def O():
    from oracle import oracle
    return oracle


def kept_lists(img, requested, nlevels=8, fast_th=20):
    """per level: (candidates, K = 2 x quota, entries retainBest keeps: all with score >= the K-th best score)"""
    o = O()
    h, w = img.shape
    n_detect = int(1.5 * requested)                                  # what the estimator asks the detector for when the NMS follows
    quota = o.level_quota(n_detect, nlevels)
    lw, lh, _ = o.pyramid_sizes(w, h, nlevels)
    out, lvl = [], img
    for l in range(nlevels):
        if l:
            lvl = o.resize(lvl, lw[l], lh[l])
        if lw[l] <= 2 * EDGE or lh[l] <= 2 * EDGE:
            out.append((0, 2 * quota[l], 0)); continue
        score = o.fast_score_map(lvl, fast_th).astype(np.int32)
        cand = np.sort(score[IR.nms3x3(score, EDGE)])[::-1]
        K = 2 * quota[l]
        kept = len(cand) if len(cand) <= K else int((cand >= cand[K - 1]).sum())
        out.append((len(cand), K, kept))
    return out


@pytest.mark.parametrize("name", sorted(IC.CONTENTS))
def test_content_keeps_ties_and_fits_the_selection(name):
    img = IC.CONTENTS[name](640, 480, seed=1)
    assert img.shape == (480, 640) and img.dtype == np.uint8
    k, d = O().orb_detect(img, int(1.5 * 750), 8, 20)
    tied, dup = IC.tied_responses(k), IC.duplicate_descriptors(d)
    lists = kept_lists(img, 750)
    print("%s: %d raw keypoints, %d tied responses, %d repeated descriptors, kept lists %s" % (name, len(k), tied, dup, [x[2] for x in lists]))
    assert len(k) > 200
    if name in IC.TIE_CONTENTS:
        assert tied >= IC.TIE_FLOOR, (name, tied)
    if name in ("periodic", "checker"):
        assert dup > 0, name
    for l, (ncand, K, kept) in enumerate(lists):
        assert kept <= SEL_MAX, (name, l, ncand, K, kept)
    if name in ("binary_blocks", "checker", "threshold_edge"):
        assert img.min() == 0 and img.max() == 255                  # saturated at both ends


def test_periodic_full_size_fits_the_selection():
    """1280x960, 2000 requested (what tests/test_gpu_image_content.py runs at full size)"""
    img = IC.periodic(1280, 960, seed=1)
    lists = kept_lists(img, 2000)
    print("periodic 1280x960: candidates / K / kept per level %s" % lists)
    for l, (ncand, K, kept) in enumerate(lists):
        assert kept <= SEL_MAX, (l, ncand, K, kept)
    k, _ = O().orb_detect(img, 3000, 8, 20)
    assert IC.tied_responses(k) >= IC.TIE_FLOOR


def test_threshold_edge_scores_sit_on_the_threshold():
    """level-0 FAST scores of the {100, 120, 141} half are th and 2 th, nothing lower exists anywhere, and at least a hundred
    isolated corners of score exactly th survive the strict NMS inside the border (one grey level less contrast, as in the dots
    placed at th, and the corner is gone): the selection of level 0 is decided among equal scores"""
    img = IC.threshold_edge(640, 480, seed=1)
    s = O().fast_score_map(img, 20).astype(np.int32)
    vals = set(np.unique(s[:230][s[:230] > 0]).tolist())
    assert {20, 40} <= vals and min(vals) == 20 and s[s > 0].min() == 20, sorted(vals)
    cand = s[IR.nms3x3(s, EDGE)]
    print("threshold_edge level 0: scores of the upper half %s, %d candidates after the NMS, %d of them at score 20" % (sorted(vals), len(cand), (cand == 20).sum()))
    assert (cand == 20).sum() >= 100
    assert (O().fast_score_map(img, 21) == 20).sum() == 0


def test_generators_are_deterministic_and_moves_are_rolls():
    for name, f in IC.CONTENTS.items():
        a, b = f(417, 311, seed=3) if name != "mirror" else f(418, 311, seed=3), f(417, 311, seed=3) if name != "mirror" else f(418, 311, seed=3)
        assert (a == b).all() and a.flags["C_CONTIGUOUS"], name
    img = IC.binary_blocks(64, 48, seed=0)
    assert (IC.right_of(img, 6)[:, :58] == img[:, 6:]).all()
    assert (IC.moved(img, 3, 2)[2:, 3:] == img[:-2, :-3]).all()
    m = IC.mirror(640, 480, seed=2)
    assert (m == m[:, ::-1]).all()
