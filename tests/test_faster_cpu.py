"""dmFASTER without a GPU: hand-built known answers for the two definitions of tests/faster_ref.py (FAST-12 segment test, KLT
response), the reference held equal to its committed lists (tests/golden/faster_kat.npz), the host-only half of the feature
(KLT_win on the context, its INI key, the frozen svo_params), and guards on every input of tests/test_gpu_faster.py so that no
GPU case compares an empty list against an empty list."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import Params, StereoCamera

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
import image_content as IC                                      # noqa: E402
import sad_ref as S                                             # noqa: E402
from oracle import oracle as O                                  # noqa: E402

SVO_ERR_ARG = -2
CHECKER_SEED = 3
BIG_T = 100                   # threshold of the 16384-entry case of test_gpu_faster.py on `periodic` tiled to 640 x 480


def photograph(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_pair_800x600.npz"))
    return g["left"], g["right"]


def big_list_frame():
    """`periodic` tiled to 640 x 480 and its right image (shared with test_gpu_faster.py)"""
    L = np.ascontiguousarray(np.tile(IC.periodic(320, 240, seed=1), (2, 2)))
    return L, IC.right_of(L, 6)


# ---- 1. known answers that do not come from faster_ref ------------------------------------------------------------------------
def ring_image(centre, values):
    img = np.full((9, 9), centre, np.uint8)
    for (dx, dy), v in zip(F.CIRCLE, values):
        img[4 + dy, 4 + dx] = v
    return img


def arc(start, length, on, off):
    return [on if (i - start) % 16 < length else off for i in range(16)]


def is_corner(img, t):
    xs, ys = F.fast12(img, t)
    return (4, 4) in set(zip(xs.tolist(), ys.tolist()))


@pytest.mark.parametrize("centre,on,edge", [(100, 121, 120), (100, 79, 80)])       # brighter arc, and its darker mirror image
def test_segment_test_known_answers(centre, on, edge):
    for start in range(16):                                     # every arc start, the arcs that wrap among them
        assert is_corner(ring_image(centre, arc(start, 12, on, centre)), 20), start
        assert is_corner(ring_image(centre, arc(start, 13, on, centre)), 20), start
        assert not is_corner(ring_image(centre, arc(start, 11, on, centre)), 20), start
        assert not is_corner(ring_image(centre, arc(start, 12, edge, centre)), 20), start       # strict comparisons
    assert is_corner(ring_image(centre, [on] * 16), 20)
    assert not is_corner(ring_image(centre, [centre] * 16), 20)


def test_segment_test_needs_a_contiguous_arc():
    split = [121 if (i % 8) < 6 else 100 for i in range(16)]    # 6 + 6 brighter pixels
    assert sum(v == 121 for v in split) == 12 and not is_corner(ring_image(100, split), 20)
    mixed = arc(0, 6, 121, 100)
    for i in range(8, 14):
        mixed[i] = 79                                           # 6 brighter + 6 darker: no arc of one kind
    assert not is_corner(ring_image(100, mixed), 20)


def test_segment_test_border_and_order():
    img = np.full((12, 14), 100, np.uint8)
    img[3, 3] = 200; img[8, 10] = 200; img[3, 10] = 0; img[2, 5] = 200          # isolated dots: whole circle darker / brighter
    xs, ys = F.fast12(img, 20)
    got = list(zip(xs.tolist(), ys.tolist()))
    assert (5, 2) not in got                                    # y = 2 < 3: outside the tested interior
    assert [g for g in got if g in ((3, 3), (10, 3), (10, 8))] == [(3, 3), (10, 3), (10, 8)]      # raster order, (w-4, h-4) included
    assert got == sorted(got, key=lambda q: (q[1], q[0]))


def test_klt_response_known_answers():
    f = np.float32
    ramp = np.tile((2 * np.arange(40)).astype(np.uint8), (40, 1))                # I = 2 u: dx = 4, dy = 0
    assert F.klt_sums(ramp, 20, 20, 4) == (81 * 16, 0, 0)
    assert F.klt_response(ramp, 20, 20, 4) == 0.0
    K = f(0.5) / f(81)
    assert F.klt_from_sums(1000, 0, 1000, 4) == f(1000) * K                     # gxx = gyy, gxy = 0: exactly Gxx
    diag = np.add.outer(np.arange(40), np.arange(40)).astype(np.uint8)           # I = u + v: dx = dy = 2, rank one
    assert F.klt_sums(diag, 20, 20, 4) == (324, 324, 324) and F.klt_response(diag, 20, 20, 4) == 0.0
    # the near-isotropic triple: the radicand is negative in float32 before the clamp, the response finite and 0.5 t
    Gxx, Gxy, Gyy = f(535439) * K, f(14) * K, f(535472) * K
    t = Gxx + Gyy
    rad = t * t - f(4.0) * (Gxx * Gyy - Gxy * Gxy)
    assert rad == -4.0
    r = F.klt_from_sums(535439, 14, 535472, 4)
    assert np.isfinite(r) and r == f(0.5) * t
    # vectorised form == scalar form
    a = F.klt_from_sums(np.array([1296, 1000, 535439]), np.array([0, 0, 14]), np.array([0, 1000, 535472]), 4)
    assert a.dtype == np.float32 and a.tolist() == [0.0, float(f(1000) * K), float(r)]


def test_klt_border_rule():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (30, 40)).astype(np.uint8)
    h, w = img.shape
    for win in (1, 4, 7):
        for x, inside in ((win, False), (win + 1, True), (w - win - 2, True), (w - win - 1, False)):
            r = F.klt_response(img, x, 15, win)
            assert (r != 0.0) == inside, (win, x, r)
            assert F.responses(img, np.array([x]), np.array([15]), win)[0] == r
        for y, inside in ((win, False), (win + 1, True), (h - win - 2, True), (h - win - 1, False)):
            assert (F.klt_response(img, 20, y, win) != 0.0) == inside, (win, y)
    xs, ys = np.meshgrid(np.arange(3, w - 3), np.arange(3, h - 3))
    xs, ys = xs.ravel(), ys.ravel()
    fast = F.responses(img, xs, ys, 4)                          # the integral-image form == the literal sums, everywhere
    assert fast.tolist() == [float(F.klt_response(img, int(x), int(y), 4)) for x, y in zip(xs, ys)]


# ---- 2. the reference against its committed lists ------------------------------------------------------------------------------
def test_reference_equals_committed_lists(golden_dir):
    sys.path.insert(0, golden_dir)
    import make_faster_kat as M
    kat = np.load(os.path.join(golden_dir, "faster_kat.npz"))
    now = M.lists(golden_dir)
    assert sorted(kat.files) == sorted(now)
    for k in kat.files:
        assert kat[k].dtype == now[k].dtype and kat[k].tobytes() == now[k].tobytes(), k
    assert len(kat["photo_t20_o0_s0_xy"]) == 413 and kat["photo_t20_o0_s0_raw"][0] == 675


# ---- 3. ABI ---------------------------------------------------------------------------------------------------------------------
def test_klt_win_abi(tmp_path):
    L = hip.lib()
    for name in ("svo_set_klt_win", "svo_get_klt_win", "svo_klt_win_load_ini", "svo_batch_set_klt_win", "svo_fpstream_set_klt_win"):
        assert getattr(L, name) is not None
    sizes = (C.c_int32 * 6)()
    L.svo_abi_sizes(sizes)
    assert sizes[3] == C.sizeof(Params) == 160                  # KLT_win lives on the context: the record did not grow
    assert hip.default_params().detect_method == 0              # ... and no default moved
    ini = tmp_path / "ref.ini"
    ini.write_text("[DETECT]\ndetect_method = 2    // dmFASTER\nKLT_win = 7\ninitial_FAST_threshold = 25\n[OTHER]\nx = 1\n")
    assert hip.load_klt_win_ini(ini, "DETECT") == 7
    assert hip.load_klt_win_ini(ini, "detect", 5) == 7          # section names are case-insensitive, as in the parameter loader
    assert hip.load_klt_win_ini(ini, "OTHER", 5) == 5           # key absent: the value stays
    assert hip.load_klt_win_ini(ini, "NONE", 6) == 6            # section absent
    assert hip.load_klt_win_ini(ini, "", 6) == 6
    with pytest.raises(hip.SvoError):
        hip.load_klt_win_ini(tmp_path / "missing.ini", "DETECT")
    p = hip.load_params_ini(ini, ["", "DETECT", "", "", "", "", ""])
    assert (p.detect_method, p.initial_FAST_threshold) == (2, 25)
    assert L.svo_set_klt_win(None, 4) == SVO_ERR_ARG and L.svo_get_klt_win(None) == SVO_ERR_ARG


# ---- 4. guards on the inputs of the GPU tests ----------------------------------------------------------------------------------
def test_guard_photograph_defaults(golden_dir):
    L, R = photograph(golden_dir)
    p = F.faster_params(O.default_params(), t=20, orb_nfeats=500, n_oct=3)
    fe = F.faster_features(L, R, p, 4)
    floors = ((500, 350, 330, 230), (320, 290, 170, 170), (160, 180, 85, 85))       # ~80 % of 675/489/413/287, 401/371/214/214, 209/227/107/107
    pair_floor = (70, 70, 20)                                                           # of 92 / 92 / 26
    for o, (kl, kr, il, ir, l, r, nl, nr) in enumerate(fe):
        assert nl >= floors[o][0] and nr >= floors[o][1] and len(kl) >= floors[o][2] and len(kr) >= floors[o][3], (o, nl, nr, len(kl), len(kr))
        m = S.match_lr_sad(l, r, kl, kr, il, ir, 400, 2.0, 1, 0.0)
        assert len(m) >= pair_floor[o], (o, len(m))
        assert (kl["size"] == 0).all() and (kl["angle"] == -1).all() and (kl["octave"] == 0).all() and (kl["class_id"] == -1).all()
        assert (np.diff(kl["y"]) >= 0).all()
    assert F.kps_to_detect(500, 3) == [428, 214, 107]


def test_guard_photograph_t10_and_crops(golden_dir):
    L, R = photograph(golden_dir)
    p = F.faster_params(O.default_params(), t=10, orb_nfeats=1200, n_oct=1)
    (kl, kr, il, ir, _, _, nl, nr), = F.faster_features(L, R, p, 4)
    assert nl >= 1800 and nr >= 1550 and len(kl) >= 1080 and len(kr) >= 930, (nl, nr, len(kl), len(kr))      # of 2294 / 1973, 1358 / 1168
    assert len(S.match_lr_sad(L, R, kl, kr, il, ir, 400, 2.0, 1, 0.0)) >= 400                                  # of 507
    q = p.copy(); q.non_maximal_suppression = 0
    (kl0, _, _, _, _, _, nl0, _), = F.faster_features(L, R, q, 4)
    assert len(kl0) == nl0 == nl and nl0 <= 4096                # without NMS every corner stays; they fit max_kps 4096
    assert list(zip(kl0["y"].tolist(), kl0["x"].tolist())) == sorted(zip(kl0["y"].tolist(), kl0["x"].tolist()))   # raster order
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    p.vo_use_matches_ids = 1
    st = S.SadStream(O, p, cam)
    for t, (x, y) in enumerate(S.CROPS):
        l, r = np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])
        (kl, kr, il, ir, _, _, _, _), = F.faster_features(l, r, p, 4)
        o = st.step((l, r), kl, kr, il, ir)
        assert len(o["matches"]) >= 400, (t, len(o["matches"]))                                               # of >= 495
        if t:
            assert len(o["tracked"]) >= 400 and o["valid"], (t, len(o["tracked"]), o["valid"])                # of 495-496


def test_guard_structured_content():
    im = IC.periodic(320, 240, seed=1)
    k = F.corners(im, 20, 4)
    _, inv, cnt = np.unique(k["response"].view(np.uint32), return_inverse=True, return_counts=True)
    assert len(k) >= 14700 and (cnt[inv.reshape(-1)] > 1).all() and (k["response"] == 0).sum() >= 480         # of 18470, all tied, 607 zeros
    assert (1 << 13) < len(k) <= (1 << 15)                      # overflows max_cand = 1 << 13, fits 1 << 15
    assert len(F.corners(IC.right_of(im, 6), 20, 4)) <= (1 << 15)
    te = IC.threshold_edge(320, 240, seed=1, th=20)
    assert [len(F.corners(te, t, 4)) for t in (19, 20, 21)] == [396, 188, 0]
    for name in ("mirror", "binary_blocks", "checker"):
        assert len(F.corners(IC.CONTENTS[name](320, 240, seed=1), 20, 4)) == 0, name
    # (a checker whose phase is odd turns into grey edges under the 2 x 2 average and has thousands of corners at octave 1: the
    # all-octaves-empty case of the GPU file uses CHECKER_SEED, whose phase (2, 0) is even)
    for o, img in enumerate(F.pyramid(IC.checker(320, 240, seed=CHECKER_SEED), 3)):
        assert len(F.fast12(img, 20)[0]) == 0, o
    L, R = big_list_frame()
    for img in (L, R):
        n = len(F.fast12(img, BIG_T)[0])
        assert 8192 < n <= 16384, n                             # needs the 16384-entry lists, and fits them (10531 / 10533)


def geometry_crops(golden_dir):
    """the 251 x 187 and 100 x 76 crops of the small sequence's first frame, left and right (shared with test_gpu_faster.py)"""
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    odd = tuple(np.ascontiguousarray(g[k][1:188, 3:254]) for k in ("L0", "R0"))
    small = tuple(np.ascontiguousarray(g[k][50:126, 60:160]) for k in ("L0", "R0"))
    return odd, small


def test_guard_geometry_inputs(golden_dir):
    (c, _), (s, _) = geometry_crops(golden_dir)
    assert c.shape == (187, 251)
    for win in (1, 4, 7, 15):
        k = [F.corners(img, 20, win) for img in F.pyramid(c, 3)]
        assert [len(x) for x in k] == [3271, 1428, 359]
        # the first and last column and row of the tested interior [3, w-3) x [3, h-3) all hold corners
        assert all((k[0]["x"] == v).any() for v in (3, 251 - 4)) and all((k[0]["y"] == v).any() for v in (3, 187 - 4))
        assert (k[2]["response"] > 0).any() and ((k[0]["response"] == 0).any() or win == 1), win
    k = [F.corners(img, 10, 4) for img in F.pyramid(s, 4)]
    assert [x.shape for x in F.pyramid(s, 4)] == [(76, 100), (38, 50), (19, 25), (9, 12)]
    assert [len(x) for x in k] == [677, 309, 62, 3]
    assert (k[3]["response"] == 0).all()                        # 12 x 9: no position passes the border rule of KLT_win 4
