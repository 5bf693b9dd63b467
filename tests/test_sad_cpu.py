"""smSAD / ifmSAD without a GPU: the reference walks of tests/sad_ref.py held to the oracle's sad8 and to their own counts on the
photograph (so that the GPU tests cannot pass on an empty list), and the host-only half of the feature -- the two new fields of
svo_params, their INI keys and their defaults."""
import ctypes as C
import os
import sys

import numpy as np

from stereo_vo_amd import hip
from stereo_vo_amd.abi import Params, StereoCamera

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sad_ref as S                                             # noqa: E402
from oracle import oracle as O                                  # noqa: E402

SECTIONS = ["RECTIFY", "DETECT", "MATCH", "IF-MATCH", "LEAST_SQUARES", "GUI", "GENERAL"]


def photograph(golden_dir):
    g = np.load(os.path.join(golden_dir, "ref_pair_800x600.npz"))
    return g["left"], g["right"]


def test_numpy_sad8_equals_the_oracle(golden_dir):
    g = np.load(os.path.join(golden_dir, "sad8_kat.npz"))
    L, R, tab, h = g["left"], g["right"], g["table"], int(g["half"])
    for iy in (-1, 0, 1):
        for ix in (-1, 0, 1):
            assert S.sad8(L, R, h, h, h + ix, h + iy) == O.sad8(L, R, h, h, h + ix, h + iy) == tab[iy + 1, ix + 1]
    L, R = photograph(golden_dir)
    H, W = L.shape
    rng = np.random.RandomState(7)
    for _ in range(2000):                                      # every legal window position, the four corners among them
        lx, rx = rng.randint(3, W - 4, 2); ly, ry = rng.randint(3, H - 4, 2)
        assert S.sad8(L, R, lx, ly, rx, ry) == O.sad8(L, R, int(lx), int(ly), int(rx), int(ry))
    for lx, ly in ((3, 3), (W - 5, 3), (3, H - 5), (W - 5, H - 5)):
        assert S.sad8(L, R, lx, ly, W - 5, H - 5) == O.sad8(L, R, lx, ly, W - 5, H - 5)
    assert S.sad8(np.zeros((8, 8), np.uint8), np.full((8, 8), 255, np.uint8), 3, 3, 3, 3) == 64 * 255 == 16320    # 14 bits


def test_walks_on_the_photograph_give_the_recorded_counts(golden_dir):
    """the reference itself: pairings of the full frame at both thresholds and both assignment rules, then the four crops as a
    sequence through the tracker walk and the composed filter at both tracker thresholds"""
    L, R = photograph(golden_dir)
    cam = StereoCamera.simple(500.0, 400.0, 300.0, 0.12, 800, 600)
    p = S.photo_params(O.default_params())
    kl, dl, kr, dr, il, ir = S.oracle_features(O, p, L, R, cam)
    assert (len(kl), len(kr)) == (1050, 1079)
    m1 = S.match_lr_sad(L, R, kl, kr, il, ir, 400, 2.0, 1)
    m0 = S.match_lr_sad(L, R, kl, kr, il, ir, 400, 2.0, 0)
    assert len(m1) == 339 and len(m0) == 339 and m1.tobytes() != m0.tobytes()          # the two rules pick different winners
    assert (m1["imgIdx"] == -1).all() and m1["distance"].max() <= 400 and (np.diff(m1["queryIdx"]) > 0).all()
    assert len(np.unique(m1["trainIdx"])) == len(m1) and len(np.unique(m0["trainIdx"])) == len(m0)
    for one in (0, 1):
        m200 = S.match_lr_sad(L, R, kl, kr, il, ir, 200, 2.0, one)
        assert len(m200) == 61
        assert S.match_lr_sad(L, R, kl, kr, il, ir, 0, 2.0, one).tobytes() == m200.tobytes()       # field 0 = the default 200
    assert len(S.match_lr_sad(L, R, kl, kr, il, ir, -1, 2.0, 1)) > 339                              # negative: no threshold
    ri = S.matches_row_index(m1, kl, 600)
    assert ri[0] == 0 and ri[600] == 339 and (np.diff(ri) >= 0).all()
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    expect = {200: ((340, None, None), (358, 83, 82), (339, 94, 93), (338, 82, 81)),
              400: ((340, None, None), (358, 143, 132), (339, 141, 131), (338, 138, 127))}
    for th in (200, 400):
        p = S.photo_params(O.default_params(), ifm_sad_max_distance=th)
        st = S.SadStream(O, p, cam)
        for t, (x, y) in enumerate(S.CROPS):
            l, r = np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])
            kl, dl, kr, dr, il, ir = S.oracle_features(O, p, l, r, cam)
            o = st.step((l, r), kl, kr, il, ir, dl, dr, 60)
            n_pair, n_cand, n_inl = expect[th][t]
            assert len(o["matches"]) == n_pair, (th, t, len(o["matches"]))
            if t:
                assert len(o["candidates"]) == n_cand and o["stats"][2] == n_inl, (th, t, len(o["candidates"]), o["stats"])
                assert (np.diff(o["candidates"]["second"]) > 0).all() and o["valid"], (th, t)
                assert 50 <= len(o["tracked"]) <= n_cand


INI = """\
[MATCH]
match_method = 2             // smSAD, the reference's default
sad_max_distance = 400
sad_max_ratio = 0.5
[IF-MATCH]
if_match_method = 2
sad_max_distance = 250
sad_max_ratio = 0.5
"""


def test_ini_loader_fills_the_sad_thresholds(tmp_path):
    f = tmp_path / "sad.ini"
    f.write_text(INI)
    p = hip.load_params_ini(f, SECTIONS)
    assert (p.match_method, p.sad_max_distance, p.ifm_method, p.ifm_sad_max_distance) == (2, 400, 2, 250)
    g = tmp_path / "none.ini"
    g.write_text("[MATCH]\nmatch_method = 1\n[IF-MATCH]\nif_match_method = 1\n")
    q = hip.default_params()
    q.sad_max_distance, q.ifm_sad_max_distance = 123, -1
    q = hip.load_params_ini(g, SECTIONS, q)
    assert (q.sad_max_distance, q.ifm_sad_max_distance) == (123, -1)       # absent keys keep the current values
    # only the MATCH group: the tracker's field is not touched by the MATCH section's key
    r = hip.load_params_ini(f, ["", "", "MATCH", "", "", "", ""])
    assert (r.sad_max_distance, r.ifm_sad_max_distance) == (400, 0)


def test_defaults_and_record_layout():
    p = hip.default_params()
    assert (p.sad_max_distance, p.ifm_sad_max_distance) == (0, 0)          # 0 = the reference's 200 in both groups
    sizes = (C.c_int32 * 6)()
    hip.lib().svo_abi_sizes(sizes)
    assert sizes[3] == C.sizeof(Params) == 160                             # as before the fields had names: they were padding
    assert (Params.sad_max_distance.offset, Params.ifm_sad_max_distance.offset) == (124, 156)
    assert (Params.kernel_param.offset, Params.vo_use_matches_ids.offset) == (128, 152)
    assert S.effective_threshold(0) == 200 and S.effective_threshold(-1) == 0xFFFFFFFF and S.effective_threshold(37) == 37
