"""Preconditions of tests/test_gpu_match_scenes.py, on the oracle alone (no GPU): the hand-built lists of tests/match_scenes.py do reach the
edges the stage-3 filters and the stage-4 trackers are built around -- otherwise the GPU tests would pass without having met them -- and
on every scene the oracle agrees with the Python walks of tests/test_independent_own_logic.py (ref_match_lr_bf, ref_match_lr_rbr,
ref_track_bf, ref_track_win, ref_pairings_row_index: imported, not copied), so that the GPU tests have a reference two independent
readings of the reference agree on."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd.abi import north_star_params

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_scenes as MS                                                            # noqa: E402
import ransac_scenes as RS                                                           # noqa: E402
import test_independent_own_logic as IND                                             # noqa: E402


def O():
    from oracle import oracle
    return oracle


def params():
    return north_star_params(O().default_params(), orb_nfeats=600)


def triples(m):
    return [(int(a), int(b), float(c)) for a, b, c in zip(m["queryIdx"], m["trainIdx"], m["distance"])]


def pairs(t):
    return [(int(a), int(b)) for a, b in zip(t["first"], t["second"])]


def stereo_runs():
    """(scene name, scene, variant number, match_method, robust, parameters): everything the GPU test runs in stage 3"""
    for nm in MS.stereo_names():
        s = MS.scene(nm)
        for v, variant in enumerate(s["variants"]):
            for method in (0, 1):
                for robust in (0, 1):
                    yield nm, s, v, method, robust, MS.stereo_params(params(), variant, method, robust)


def test_generators_are_deterministic_and_exact():
    """the same lists from the same seed; every coordinate exact in binary32 (an integer or a multiple of 2^-10); lists in ascending row
    order; 40 to 600 keypoints per side in the stage-3 scenes that are not the tiny ones; the 9200 candidates of the longest chain"""
    for nm, gen, args in MS.STEREO + [t for t in MS.TRACK if t[0] not in ("track-chain-2100", "track-chain-4600")]:
        a, b = MS.scene(nm), gen(*args)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert a[k].tobytes() == b[k].tobytes(), (nm, k)
    for nm in MS.stereo_names():
        s = MS.scene(nm)
        for k in ("kl", "kr"):
            xy = np.stack([s[k]["x"], s[k]["y"]], 1).astype(np.float64)
            frac = xy[(xy != np.round(xy)) & (s[k]["response"][:, None] == 1.0)]
            assert (frac * 1024 == np.round(frac * 1024)).all(), (nm, k)
            assert (np.diff(s[k]["y"]) >= 0).all(), (nm, k)
        if not nm.startswith("stereo-"):
            assert 40 <= len(s["kl"]) <= 600 and 40 <= len(s["kr"]) <= 600 and s["W"] <= 320 and s["H"] <= 240, nm
    for nm in MS.track_names():
        s = MS.scene(nm)
        for a, b in (("pkl", "pkr"), ("ckl", "ckr")):
            assert (s[a]["x"] - s[b]["x"] == 20).all() and (s[a]["y"] == s[b]["y"]).all(), nm
            assert (np.diff(s[a]["y"][s["pm" if a == "pkl" else "cm"]["queryIdx"]]) >= 0).all(), nm
    assert len(MS.scene("track-chain-4600")["pm"]) == 9200 and len(MS.scene("track-chain-4600")["cm"]) == 4601


def test_planted_matches_are_unique_first_minima():
    """on the lists as they are handed over: O.hamming_bf finds the planted match at the planted distance for every query planted within
    62 bits, and no other candidate is closer than 90 bits (checked again here, from the finished lists, with the oracle's own matcher)"""
    for nm in MS.stereo_names():
        s = MS.scene(nm)
        if len(s["kl"]) == 0 or len(s["kr"]) == 0:
            continue
        idx, dist = O().hamming_bf(s["dl"], s["dr"])
        near = (s["want_r"] >= 0) & (s["want_d"] <= 62)
        assert (idx[near] == s["want_r"][near]).all() and (dist[near] == s["want_d"][near]).all(), nm
        assert (dist[~near] >= 90).all(), nm
        D = MS.hamming_matrix(s["dl"], s["dr"])
        D[np.flatnonzero(near), s["want_r"][near]] = 999
        assert D.min() >= 90, (nm, D.min())
    for nm in ("track-chain-300", "track-chain-2100", "track-threshold", "track-inconsistent"):
        s = MS.scene(nm)
        for q, t, want, d in ((s["pdl"], s["cdl"], s["tl"], s["dL"]), (s["pdr"], s["cdr"], s["tr"], s["dR"])):
            idx, dist = O().hamming_bf(q, t)
            assert (idx == want).all() and (dist == d).all(), nm
            _, lo, _ = MS.extremes(q, t, want)
            assert lo.min() >= 90, (nm, lo.min())


def test_row_tables_follow_the_documented_rules():
    """features_row_index against the oracle's own table on lists that lie inside the image (there the two rules coincide: O.row_sort_index
    of a list already in row order), its documented behaviour outside (rows below 0 counted in row 0, rows from H on never);
    matches_row_index is the walk of S3:425-445 (ref_pairings_row_index)"""
    for nm in ("bf-threshold", "bf-one-to-one", "rbr-wrap"):
        s = MS.scene(nm)
        for k in ("kl", "kr"):
            _, idx = O().row_sort_index(s[k], s["H"])
            assert list(MS.features_row_index(s[k], s["H"])) == list(idx), (nm, k)
    k = RS._kps(np.array([[5, -3.5], [6, -0.5], [7, 0.0], [8, 2.0], [9, 2.5], [3, 7.0], [4, 9.0]], np.float32))
    assert list(MS.features_row_index(k, 8)) == [3, 3, 5, 5, 5, 5, 5, 6]
    assert list(MS.features_row_index(k[2:6], 8)) == [1, 1, 3, 3, 3, 3, 3, 0]
    for nm in ("win-edges", "win-negative-rows-0", "track-chain-40"):
        s = MS.scene(nm)
        for m, kl, ri in ((s["pm"], s["pkl"], s["pri"]), (s["cm"], s["ckl"], s["cri"])):
            assert list(ri) == IND.ref_pairings_row_index(kl, [(int(q),) for q in m["queryIdx"]], s["H"]), nm
            assert ri[0] == 0 and ri[s["H"]] == len(m), nm


def test_oracle_equals_the_independent_walks_on_every_stage3_scene():
    for nm, s, v, method, robust, p in stereo_runs():
        m, ri = MS.oracle_match(p, s)
        got = triples(m)
        if method == 0:
            want = IND.ref_match_lr_bf(s["kl"], s["dl"], s["kr"], s["dr"], robust, p.max_y_diff, MS.ORB_TH, s["W"])
            want = [(q, t, float(d)) for q, t, d in want]
        else:
            want = IND.ref_match_lr_rbr(s["kl"], s["dl"], MS.features_row_index(s["kl"], s["H"]), s["kr"], s["dr"], MS.features_row_index(s["kr"], s["H"]),
                                        robust, p.max_y_diff, p.orb_max_distance, p.minimum_ORB_response, s["W"], s["H"])
        assert got == want, (nm, v, method, robust)
        assert list(ri) == IND.ref_pairings_row_index(s["kl"], got, s["H"]), (nm, v, method, robust, "row table")
        assert ri[0] == 0 and ri[s["H"]] == len(got)


def test_brute_force_scenes_keep_and_drop_what_their_edges_say():
    """smDescBF on every stage-3 scene equals the prediction made from the planted structure alone (MS.expected_bf), and edge by edge:"""
    for nm, s, v, method, robust, p in stereo_runs():
        if method == 0:
            assert triples(MS.oracle_match(p, s)[0]) == MS.expected_bf(s, p), (nm, v, robust)

    def kept_labels(nm, v, robust):
        s = MS.scene(nm)
        m, _ = MS.oracle_match(MS.stereo_params(params(), s["variants"][v], 0, robust), s)
        return [s["label"][q] for q in m["queryIdx"]], s
    # distances up to orb_th stay, orb_th + 1 and the complement go: nine of each
    kept, s = kept_labels("bf-threshold", 0, 1)
    assert sorted(set(kept)) == ["d=0", "d=59", "d=60"] and len(kept) == 27 and s["label"].count("d=61") == 9 and s["label"].count("d=256") == 9
    # (int)(yl - yr): under max_y_diff 1 everything short of two rows stays, under 0 everything short of one
    for v, lim in ((0, 2.0), (1, 1.0)):
        kept, s = kept_labels("bf-epipolar", v, 1)
        for dy in MS.DY:
            assert (("dy=%r dx=10.0" % dy) in kept) == (abs(dy) < lim), (v, dy)
        for dx in MS.dxs(s["W"]):
            assert (("dy=0.0 dx=%r" % dx) in kept) == (1.0 <= dx < s["W"] + 1), (v, dx)
    # 1-to-1: one survivor per group (none where the winner fails the epipolar filter); without it every claimant that passes
    kept, s = kept_labels("bf-one-to-one", 0, 1)
    for size in (2, 3, 40):
        assert "equal-%d #0" % size in kept and "unequal-%d #0" % size in kept and "loser-passes-%d #%d" % (size, size - 1) in kept
        assert sum(k.startswith(("equal-%d " % size, "unequal-%d " % size, "loser-passes-%d " % size, "winner-fails-%d " % size)) for k in kept) == 3
    kept0, _ = kept_labels("bf-one-to-one", 0, 0)
    assert len(kept0) == len(s["label"]) - 3 and not any(k in kept0 for k in ("winner-fails-2 #1", "winner-fails-3 #2", "winner-fails-40 #39"))
    # rows: everything stays; row 0, a row of 70, empty rows between, rows H - 2 and H - 1
    s = MS.scene("bf-rows")
    m, ri = MS.oracle_match(MS.stereo_params(params(), {}, 0, 1), s)
    H = s["H"]
    assert len(m) == 86 and list(ri[:3]) == [0, 5, 5] and ri[50] == 5 and ri[51] == 75 and ri[H - 2] == 78 and ri[H - 1] == 82 and ri[H] == 86
    # the one pair whose descriptors are complements: the brute-force matcher reports 256, and drops it
    s = MS.scene("stereo-1-1-complement")
    assert list(O().hamming_bf(s["dl"], s["dr"])[1]) == [256] and len(MS.oracle_match(MS.stereo_params(params(), {}, 0, 1), s)[0]) == 0


def test_row_by_row_scenes_reach_their_edges():
    def run(nm, v, robust):
        s = MS.scene(nm)
        m, _ = MS.oracle_match(MS.stereo_params(params(), s["variants"][v], 1, robust), s)
        return m, s
    for robust in (0, 1):
        m, s = run("rbr-wrap", 0, robust)
        got = {int(q): (int(t), float(d)) for q, t, d in triples(m)}
        lab = s["label"]
        # the complement wins at distance 0, whichever side of the 3-bit candidate it is on
        wraps = [i for i, k in enumerate(lab) if k == "wrap"]
        assert len(wraps) == 6 and sorted(got[i][0] for i in wraps) == sorted(s["right_at"]["wrap%d" % g] for g in range(6)) and all(got[i][1] == 0.0 for i in wraps)
        # max_distance 60: 59 and 60 stay, 61 goes
        assert all((i in got) == (k != "d=61") for i, k in enumerate(lab) if k.startswith("d="))
        # first claimant (robust off) / best claimant (robust on); at equal distance the first either way
        first, second = [i for i, k in enumerate(lab) if k == "claim-first"], [i for i, k in enumerate(lab) if k == "claim-second"]
        better = [s["want_d"][b] < s["want_d"][a] for a, b in zip(first, second)]
        assert better == [True, False, True, False]
        for a, b, bt in zip(first, second, better):
            assert ((b in got) and (a not in got)) if (robust and bt) else ((a in got) and (b not in got)), (robust, a, b)
        assert "last row" == lab[-1] and len(lab) - 1 not in got
        # a response ON minimum_ORB_response stays, one ulp under it (either side) goes; with the default 0 all stay
        resp = [i for i, k in enumerate(lab) if k.startswith("resp")]
        assert all(i in got for i in resp)
        m2, _ = run("rbr-wrap", 1, robust)
        got2 = set(int(q) for q in m2["queryIdx"])
        assert [i in got2 for i in resp] == [lab[i] == "resp True True" for i in resp] and sum(i in got2 for i in resp) == 2
    # rows: the right keypoint may be d rows above .. d - 1 rows below, d = round(max_y_diff): 0 0 1 1 2 3
    counts = []
    for v, d in enumerate([0, 0, 1, 1, 2, 3]):
        m, s = run("rbr-rows", v, 1)
        got, lab = set(int(q) for q in m["queryIdx"]), s["label"]
        for off in range(-4, 5):
            assert (lab.index("offset %d" % off) in got) == (-d <= off <= d - 1), (v, off)
        counts.append(len(got))
        if d >= 1:                                                                # disparities 1 and (int)(0.7 W) stay; just under 1, 0.5 and one pixel more go
            big = float(int(s["W"] * 0.7))
            assert [lab.index("disparity %r" % dx) in got for dx in (1.0, MS.NEAR1, big, big + MS.NEAR1, big + 1.0, 0.5)] == [True, False, True, True, False, False]
            assert lab.index("first row") not in got and lab.index("last row") not in got
            H = s["H"]
            for r in (1, 2, H - 2, H - 1):                                        # right rows in reach of left row r: (max(0, r - 1 - d), min(H - 1, r - 1 + d)], the clamps of S3:254-255
                for off in (-1, 1):
                    hit = [i in got for i, l in enumerate(lab) if l == "border row %d offset %d" % (r, off)]
                    assert hit == [max(0, r - 1 - d) < r + off <= min(H - 1, r - 1 + d)] * 2, (v, r, off, hit)
    assert counts[0] == counts[1] == 0 and counts[2] == counts[3] and counts[3] < counts[4] < counts[5], counts


def track_want(nm):
    s = MS.scene(nm)
    return s, MS.track_params(params(), s), RS.oracle_track(MS.track_params(params(), s), s, key=("match-scenes", nm))


def test_oracle_equals_the_independent_walks_on_every_stage4_scene():
    for nm in MS.track_names(small_only=True):
        s, p, (trk, ts) = track_want(nm)
        if p.ifm_method == 0:
            want = IND.ref_track_bf(s["pkl"], s["pdl"], s["pkr"], s["pdr"], s["pm"], s["ckl"], s["cdl"], s["ckr"], s["cdr"], s["cm"], MS.ORB_TH)
        else:
            want = IND.ref_track_win(s["pkl"], s["pdl"], s["pkr"], s["pm"], s["pri"], s["ckl"], s["cdl"], s["ckr"], s["cm"], s["cri"], p.ifm_win_w, p.ifm_win_h, s["W"], s["H"])
        assert pairs(trk) == [(int(a), int(b)) for a, b in want], nm


def test_stage4_scenes_reach_their_edges():
    """every scene: the RANSAC keeps every survivor (SVO_TS_BOTH_MASKS == SVO_TS_COLLISION); the scenes that name their survivors: the
    tracked list is the predicted one and SVO_TS_TRACKED == SVO_TS_COLLISION; track-inconsistent: short by exactly the six"""
    for nm in MS.track_names():
        s, p, (trk, ts) = track_want(nm)
        ts = [int(v) for v in ts]
        assert ts[6] == ts[1], (nm, ts)
        if s["th_col"] is not None:
            assert tuple(ts[:2]) == tuple(s["th_col"]), (nm, ts)
        if s["want"] is not None:
            assert pairs(trk) == [(int(a), int(b)) for a, b in s["want"]], nm
        if nm == "track-inconsistent":
            assert s["n_inconsistent"] == 6 and ts[7] == ts[1] - 6, ts
        elif not nm.startswith("track-tiny"):
            assert ts[7] == ts[1] > 0, (nm, ts)
    for J in (300, 2100, 4600):
        _, _, (trk, ts) = track_want("track-chain-%d" % J)
        assert [int(v) for v in ts] == [2 * J, J, J, J, 1, 1, J, J] and (trk["first"] == 2 * np.arange(J)).all() and (trk["second"] == np.arange(J)).all(), J
    s, _, (_, ts) = track_want("track-threshold")
    assert ts[0] - ts[1] == 8 and len(s["pm"]) - ts[0] == 12 + 10, ts        # eight collisions; 22 pairings over the threshold, ten of them ahead of a good one for the same pair
    s, _, (trk, ts) = track_want("win-edges")
    assert len(trk) == 30 and len(s["pm"]) - len(trk) == 7                       # not tracked: row H - 1, two x windows, the 255, three second-best claimants
    for nm in ("win-negative-rows-0", "win-negative-rows-1"):
        s, _, (trk, ts) = track_want(nm)                                         # (scene 1: the x windows start at 0, so pairings left of the image find nothing)
        neg = s["pkl"]["y"][s["pm"]["queryIdx"][trk["first"]]] < 0
        assert (len(trk) == len(s["pm"]) if nm.endswith("0") else len(trk) > 100) and neg.sum() >= 10 and (s["ckl"]["y"][s["cm"]["queryIdx"][trk["second"]]] < 0).sum() >= 10, (nm, int(neg.sum()))


@pytest.mark.parametrize("J", [40, 300, 2100, 4600])
def test_chain_needs_the_rounds(J):
    """k_track_filter's round rule, replayed in numpy, keeps the pairings the sequential walk keeps and needs at least J - 1 rounds for it"""
    s = MS.scene("track-chain-%d" % J)
    ok = (s["dL"] <= MS.ORB_TH) & (s["dR"] <= MS.ORB_TH)
    kept, rounds = MS.filter_rounds(s["tl"], s["tr"], ok, len(s["cm"]))
    assert rounds >= J - 1 and (np.flatnonzero(kept) == 2 * np.arange(J)).all(), (J, rounds)
    s = MS.scene("track-threshold")
    kept, rounds = MS.filter_rounds(s["tl"], s["tr"], (s["dL"] <= MS.ORB_TH) & (s["dR"] <= MS.ORB_TH), len(s["cm"]))
    assert int(kept.sum()) == s["th_col"][1] and rounds == 1


def test_shuffled_pairings_are_walked_by_position():
    """the scene of the GPU test on lists outside ascending row order: the oracle equals the independent walk there too, tracks ten
    pairings or more, and most previous pairings are visited in an iteration other than the one their own row names"""
    t = MS.unsorted_track()
    q = MS.track_params(params(), t)
    trk, ts = RS.oracle_track(q, t)
    want = IND.ref_track_win(t["pkl"], t["pdl"], t["pkr"], t["pm"], t["pri"], t["ckl"], t["cdl"], t["ckr"], t["cm"], t["cri"], q.ifm_win_w, q.ifm_win_h, t["W"], t["H"])
    assert pairs(trk) == [(int(a), int(b)) for a, b in want] and len(trk) >= 10, len(trk)
    own = np.ceil(t["pkl"]["y"][t["pm"]["queryIdx"][trk["first"]]]).astype(np.int64)
    walked = np.searchsorted(t["pri"][:t["H"]], trk["first"], side="right") - 1
    assert (own != walked).sum() >= 5, (own, walked)
