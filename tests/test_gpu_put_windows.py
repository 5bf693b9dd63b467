"""svo_gather_windows / svo_get_windows_oct: SAD windows for frames the library did not detect (the precomputed-data bypass under
smSAD / ifmSAD).

The windows are compared byte for byte with a numpy gather of [x-3, x+4] x [y-3, y+4] at (int)pt from the octave image, the flags with
the float border rule of S3:290-293; downstream of them a context that never detects must track exactly like one that does."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, keypoint_dtype

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
import image_content as IC                                      # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_faster_cpu import geometry_crops, photograph          # noqa: E402
from test_gpu_parity import O, POSE_TOL_M, POSE_TOL_RAD, _distortion_maps      # noqa: E402
from test_gpu_frame_layouts import lay_out                      # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6
SAD_KERNELS = ("sad_patch", "match_lr_sad", "track_sad")


def params(t=20, orb_nfeats=500, n_oct=3):
    return F.faster_params(hip.default_params(), t=t, orb_nfeats=orb_nfeats, n_oct=n_oct, nms=1)


def np_windows(img, k):
    """(windows [n, 8, 8], flags [n]) of the keypoints k on one octave image: the float rule, then (int)pt"""
    h, w = img.shape
    x, y = k["x"].astype(np.float32), k["y"].astype(np.float32)
    flag = (x < np.float32(3)) | (y < np.float32(3)) | (x > np.float32(w - 5)) | (y > np.float32(h - 5))
    win = np.zeros((len(k), 8, 8), np.uint8)
    for i in np.flatnonzero(~flag):
        xi, yi = int(x[i]), int(y[i])
        win[i] = img[yi - 3:yi + 5, xi - 3:xi + 5]
    return win, flag.astype(np.uint8)


def hand_made(w, h, corners):
    """border cases on both axes, fractional coordinates and the detector's corners of that octave image, in one list"""
    edge_x, edge_y = (2.99, 3.0, w - 5, w - 4.99), (2.99, 3.0, h - 5, h - 4.99)
    pts = [(x, h / 2 + 0.5) for x in edge_x] + [(w / 2 + 0.25, y) for y in edge_y] + [(a, b) for a in edge_x[1:3] for b in edge_y[1:3]]
    pts += [(10.5, 17.25), (w - 9.75, 11.999), (w / 3 + 0.999, h - 8.5), (3.0001, 3.9999)]
    k = np.zeros(len(pts) + len(corners), keypoint_dtype)
    k["x"][:len(pts)], k["y"][:len(pts)] = [p[0] for p in pts], [p[1] for p in pts]
    k["size"], k["angle"], k["class_id"] = 0.0, -1.0, -1
    k[len(pts):] = corners
    return k


def assert_windows(ctx, lane, which, side, octave, img, k, tag):
    win, flag = ctx.windows(lane, which, side, octave)
    w0, f0 = np_windows(img, k)
    assert len(flag) == len(k) and (flag == f0).all(), (tag, "flags", np.flatnonzero(flag != f0)[:8])
    keep = f0 == 0
    assert (win[keep] == w0[keep]).all(), (tag, "windows", np.flatnonzero((win != w0).any((1, 2)) & keep)[:8])
    return int(keep.sum()), int((~keep).sum())


def put_lists(ctx, lane, which, lists, w, h):
    for o, per_side in enumerate(lists):
        for side in (0, 1):
            ctx.put_features(lane, which, side, per_side[side], None, w, h, octave=o)


@pytest.mark.parametrize("which", [0, 1])
def test_windows_against_numpy(golden_dir, which):
    """251 x 187 read in place at stride 259 from odd byte offsets inside poison bytes, three octaves"""
    (l, r), _ = geometry_crops(golden_dir)
    p = params(20, 500, 3)
    feats = F.faster_features(l, r, p, 4)
    pyr = [F.pyramid(l, 3), F.pyramid(r, 3)]
    lists = [[hand_made(pyr[side][o].shape[1], pyr[side][o].shape[0], feats[o][side]) for side in (0, 1)] for o in range(3)]
    [(pl, pr)], buf, host = lay_out([(l, r)], "rows", 259, [(3, 7)], seed=11)
    ctx = hip.Context(n_lanes=1, max_w=251, max_h=187, max_kps=1024, max_cand=1 << 15, max_octaves=3)
    ctx.set_params(p)
    put_lists(ctx, 0, which, lists, 251, 187)
    with pytest.raises(hip.SvoError, match="never gathered"):
        ctx.windows(0, which, 0, 0)
    before = [ctx.keypoints(0, which, side, o)[0].tobytes() for o in range(3) for side in (0, 1)]
    ctx.gather_windows_device([(pl, pr)], 251, 187, 259, which=which)
    for o in range(3):
        for side in (0, 1):
            assert (ctx.level(0, side, o) == pyr[side][o]).all(), ("octave image", o, side)
            n_win, n_flag = assert_windows(ctx, 0, which, side, o, pyr[side][o], lists[o][side], (which, o, side))
            assert n_win >= 8 and n_flag >= 4, (o, side, n_win, n_flag)           # both kinds in every list
            assert len(feats[o][side]) >= 20, (o, side)                           # ... and real corners among them
    # the other slot has no frame, the lists and the record are what they were
    assert len(ctx.windows(0, 1 - which, 0, 0)[1]) == 0
    assert [ctx.keypoints(0, which, side, o)[0].tobytes() for o in range(3) for side in (0, 1)] == before
    r0 = ctx.result(0)
    assert (r0.valid, r0.error_code, r0.tracked_feats_from_last_frame) == (0, 0, 0) and ctx.status_word(0) == 0
    ctx.close()
    IC.assert_untouched(buf, host)


def lists_of(ctx, lane, which, n_oct):
    return [dict(kl=ctx.keypoints(lane, which, 0, o), kr=ctx.keypoints(lane, which, 1, o), m=ctx.matches(lane, which, o), ids=ctx.match_ids(lane, which, o))
            for o in range(n_oct)]


def put_frame(ctx, lane, which, fr, w, h):
    for o, d in enumerate(fr):
        ctx.put_features(lane, which, 0, d["kl"][0], d["kl"][1], w, h, octave=o)
        ctx.put_features(lane, which, 1, d["kr"][0], d["kr"][1], w, h, octave=o)
        ctx.put_matches(lane, which, d["m"], octave=o)
        ctx.put_match_ids(lane, which, d["ids"], octave=o)


def test_bypass_equals_detection(golden_dir):
    """context B never detects: A's lists of frames t-1 and t, the windows gathered from the two image pairs, then stages 4-5 -- the
    tracked pairs, stage counters and verdict of the context that detected; stage 3 alone on B's current frame gives A's pairings"""
    L, R = photograph(golden_dir)
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = params(10, 1200, 3)
    p.vo_use_matches_ids = 1
    crops = [(np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])) for x, y in S.CROPS]
    a = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 17, max_octaves=3)
    b = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 17, max_octaves=3)
    for c in (a, b):
        c.set_params(p); c.set_camera(cam)
    prev = None
    for t, pair in enumerate(crops):
        a.process_host([pair])
        ra = a.result(0)
        cur = lists_of(a, 0, 0, 3)
        trk = [a.tracked(0, o) for o in range(3)]
        if t:
            print("t=%d tracked per octave %s valid %d" % (t, [len(x) for x in trk], ra.valid))
            assert len(trk[0]) >= 100 and len(trk[1]) >= 10 and len(trk[2]) >= 10, (t, [len(x) for x in trk])   # the condition, on the detecting context
            # (B is not reset between the frames: like a caller that tracks a stream through the bypass it warm-starts stage 5 from its
            # own last pose, as A does from its own; only the first tracked frame starts from the identity in both)
            put_frame(b, 0, 1, prev, w, h); put_frame(b, 0, 0, cur, w, h)
            b.gather_windows([crops[t - 1]], which=1)
            b.gather_windows([pair], which=0)
            for which in (0, 1):
                for o in range(3):
                    for side in (0, 1):
                        wa, fa = a.windows(0, which, side, o); wb, fb = b.windows(0, which, side, o)
                        assert (fa == fb).all() and (wa[fa == 0] == wb[fb == 0]).all(), (t, which, o, side)
            b.run_stages(hip.RUN_TRACK | hip.RUN_OPTIMIZE)
            rb = b.result(0)
            for o in range(3):
                assert b.tracked(0, o).tobytes() == trk[o].tobytes(), (t, "tracked", o, len(b.tracked(0, o)), len(trk[o]))
            assert list(rb.track_stats) == list(ra.track_stats), (t, list(rb.track_stats), list(ra.track_stats))
            assert (rb.valid, rb.error_code) == (ra.valid, ra.error_code), (t, rb.valid, rb.error_code, ra.valid, ra.error_code)
            assert ra.valid
            dp = np.abs(np.array(rb.outPose) - np.array(ra.outPose))         # (the warm start differs: B's own last pose, not A's)
            print("t=%d pose difference %s" % (t, dp))
            assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (t, dp)
            b.run_stages(hip.RUN_MATCH)                                       # stage 3 alone: the row tables of the put lists and the gathered windows
            for o in range(3):
                assert b.matches(0, 0, o).tobytes() == cur[o]["m"].tobytes(), (t, "pairings", o, len(b.matches(0, 0, o)), len(cur[o]["m"]))
                assert (b.matches_row_index(0, 0, o) == a.matches_row_index(0, 0, o)).all(), (t, o)
                for side in (0, 1):
                    assert (b.row_index(0, 0, side, o) == a.row_index(0, 0, side, o)).all(), (t, "row table", o, side)
        prev = cur
    a.close(); b.close()


def small_lanes(golden_dir, n):
    """n different 100 x 76 pairs (the small crop, rolled) with a two-octave list each"""
    _, (l, r) = geometry_crops(golden_dir)
    p = params(20, 300, 2)
    pairs = [(np.ascontiguousarray(np.roll(l, 5 * i, 1)), np.ascontiguousarray(np.roll(r, 5 * i, 1))) for i in range(n)]
    lists = []
    for pl, pr in pairs:
        feats = F.faster_features(pl, pr, p, 4)
        pyr = [F.pyramid(pl, 2), F.pyramid(pr, 2)]
        lists.append([[hand_made(pyr[side][o].shape[1], pyr[side][o].shape[0], feats[o][side]) for side in (0, 1)] for o in range(2)])
    return p, pairs, lists


def test_masks(golden_dir):
    """three lanes, lane 1 sits the gather out: its windows stay, its frames[] entry is not read, a SAD stage on it is still refused"""
    p, pairs, lists = small_lanes(golden_dir, 6)
    x, y = pairs[:3], pairs[3:]
    ctx = hip.Context(n_lanes=3, max_w=100, max_h=76, max_kps=512, max_cand=1 << 14, max_octaves=2)
    one = hip.Context(n_lanes=1, max_w=100, max_h=76, max_kps=512, max_cand=1 << 14, max_octaves=2)
    ctx.set_params(p); one.set_params(p)
    for lane in range(3):
        put_lists(ctx, lane, 0, lists[lane], 100, 76)
    ctx.gather_windows(x, which=0)
    w1 = [[ctx.windows(1, 0, side, o) for side in (0, 1)] for o in range(2)]
    for o in range(2):
        for side in (0, 1):
            assert_windows(ctx, 1, 0, side, o, F.pyramid(x[1][side], 2)[o], lists[1][o][side], ("x", o, side))
    ctx.gather_windows([y[0], None, y[2]], which=0, active=[0, 2])
    for o in range(2):
        for side in (0, 1):
            a, b = ctx.windows(1, 0, side, o), w1[o][side]
            assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes(), ("the idle lane's windows", o, side)
    for lane in (0, 2):
        put_lists(one, 0, 0, lists[lane], 100, 76)
        one.gather_windows([y[lane]], which=0)
        for o in range(2):
            for side in (0, 1):
                a, b = ctx.windows(lane, 0, side, o), one.windows(0, 0, side, o)
                assert (a[1] == b[1]).all() and (a[0][a[1] == 0] == b[0][b[1] == 0]).all(), (lane, o, side)
                assert_windows(ctx, lane, 0, side, o, F.pyramid(y[lane][side], 2)[o], lists[lane][o][side], ("y", lane, o, side))
    # lists put again come without windows again; a gather that leaves the lane out does not change that
    put_lists(ctx, 1, 0, lists[1], 100, 76)
    ctx.gather_windows([y[0], None, y[2]], which=0, active=[0, 2])
    with pytest.raises(hip.SvoError, match="never gathered"):
        ctx.windows(1, 0, 0, 0)
    rc = ctx.L.svo_process(ctx.h, None, hip.RUN_MATCH | hip.FLAG_NO_SHIFT)
    text = ctx.L.svo_last_error(ctx.h)
    assert rc == SVO_ERR_STATE and b"lane 1" in text and b"never gathered" in text, (rc, text)
    # no bit set: nothing happens
    assert ctx.L.svo_gather_windows(ctx.h, None, 0, 0, (C.c_uint64 * 2)(0, 0)) == SVO_ERR_ARG          # (frames == NULL comes first)
    fr = (hip.Frame * 3)()
    assert ctx.L.svo_gather_windows(ctx.h, fr, 0, 0, (C.c_uint64 * 2)(0, 0)) == 0
    ctx.close(); one.close()


def test_bgr_frame_with_a_rectify_map(golden_dir):
    """ORB mode, one octave: the windows come from the grey, rectified level 0 that stage 1 made of the caller's BGR frame"""
    (l, r), _ = geometry_crops(golden_dir)
    w, h = 251, 187
    bgr = [np.ascontiguousarray(np.stack([g, np.roll(g, 3, 1), 255 - g // 2], -1)) for g in (l, r)]
    maps = [_distortion_maps(w, h), _distortion_maps(w, h, k1=-0.05, shift=(-3.25, 0.5), rot=-0.004)]
    p = S.photo_params(hip.default_params(), orb_nfeats=300)
    ctx = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=512, max_cand=1 << 15)
    ctx.set_params(p)
    ctx.set_rectify_map(0, 0, *maps[0]); ctx.set_rectify_map(0, 1, *maps[1])
    rng = np.random.default_rng(5)
    lists = [[hand_made(w, h, np.zeros(0, keypoint_dtype)) for side in (0, 1)]]
    for side in (0, 1):
        extra = np.zeros(40, keypoint_dtype)
        extra["x"], extra["y"] = rng.uniform(0, w, 40).astype(np.float32), np.sort(rng.uniform(0, h, 40).astype(np.float32))
        lists[0][side] = np.concatenate([lists[0][side], extra])
    put_lists(ctx, 0, 0, lists, w, h)
    ctx.gather_windows([tuple(bgr)], which=0)
    for side in (0, 1):
        grey = ctx.level(0, side, 0)
        assert (grey == O().prepare(bgr[side], *maps[side])).all() and grey.std() > 10, side
        n_win, n_flag = assert_windows(ctx, 0, 0, side, 0, grey, lists[0][side], ("bgr", side))
        assert n_win >= 20 and n_flag >= 4
    ctx.close()


def test_refusals(golden_dir):
    """every refusal comes before anything is enqueued, with a text, and leaves lists, record and windows as they were"""
    p, pairs, lists = small_lanes(golden_dir, 2)
    ctx = hip.Context(n_lanes=2, max_w=128, max_h=96, max_kps=512, max_cand=1 << 14, max_octaves=2)
    ctx.set_params(p)
    L = ctx.L

    def frames(w=100, h=76, stride=100, data=True):
        fr = (hip.Frame * 2)()
        keep = []
        for i in range(2):
            l, r = pairs[i]
            keep += [l, r]
            fr[i].left = hip.Image(l.ctypes.data if data else None, w, h, stride); fr[i].right = hip.Image(r.ctypes.data if data else None, w, h, stride)
        return fr, keep

    fr, keep = frames()
    # no geometry yet
    rc = L.svo_gather_windows(ctx.h, fr, 0, 0, None)
    assert rc == SVO_ERR_STATE and b"no geometry" in L.svo_last_error(ctx.h), (rc, L.svo_last_error(ctx.h))
    for lane in range(2):
        put_lists(ctx, lane, 0, lists[lane], 100, 76)
    ctx.gather_windows([pairs[0], None], which=0, active=[0])              # lane 0 has windows, lane 1 has none

    def state():
        out = [ctx.keypoints(lane, 0, side, o)[0].tobytes() for lane in range(2) for o in range(2) for side in (0, 1)]
        out += [bytes(ctx.result(lane)) for lane in range(2)]
        out += [ctx.windows(0, 0, side, o)[i].tobytes() for o in range(2) for side in (0, 1) for i in (0, 1)]
        rc = L.svo_process(ctx.h, None, hip.RUN_MATCH | hip.FLAG_NO_SHIFT)
        assert rc == SVO_ERR_STATE and b"lane 1" in L.svo_last_error(ctx.h) and b"never gathered" in L.svo_last_error(ctx.h)
        return out

    before = state()
    big = (1 << 31) // 76 + 1
    cases = [
        (fr, 0, 2, None, SVO_ERR_ARG, b"which"), (fr, 0, -1, None, SVO_ERR_ARG, b"which"),
        (None, 0, 0, None, SVO_ERR_ARG, b"frames"),
        (fr, hip.RUN_DETECT, 0, None, SVO_ERR_ARG, b"flags"), (fr, hip.FLAG_NO_SHIFT, 0, None, SVO_ERR_ARG, b"flags"), (fr, 1 << 20, 1, None, SVO_ERR_ARG, b"flags"),
        (fr, 0, 0, (C.c_uint64 * 2)(4, 0), SVO_ERR_ARG, b"n_lanes"), (fr, 0, 0, (C.c_uint64 * 2)(1, 1), SVO_ERR_ARG, b"n_lanes"),
        (frames(stride=99)[0], 0, 0, None, SVO_ERR_ARG, b"smaller than a row"),
        (frames(stride=299)[0], hip.FLAG_BGR_IMAGES, 0, None, SVO_ERR_ARG, b"smaller than a row"),
        (frames(stride=big)[0], hip.FLAG_DEVICE_IMAGES, 0, None, SVO_ERR_ARG, b"exceeds"),
        (frames(data=False)[0], 0, 0, None, SVO_ERR_ARG, b""),
        (frames(w=128, h=96, stride=128)[0], 0, 0, None, SVO_ERR_STATE, b"100 x 76"),
        (frames(w=100, h=75)[0], 0, 1, None, SVO_ERR_STATE, b"100 x 76"),
    ]
    for i, (f, flags, which, mask, want, text) in enumerate(cases):
        rc = L.svo_gather_windows(ctx.h, f, flags, which, mask)
        assert rc == want and text in L.svo_last_error(ctx.h), (i, rc, L.svo_last_error(ctx.h))
        assert state() == before, i
    # ... and the call the refusals were about still works
    ctx.gather_windows(pairs, which=0)
    assert L.svo_process(ctx.h, None, hip.RUN_MATCH | hip.FLAG_NO_SHIFT) == 0
    ctx.wait()
    assert all(ctx.status_word(lane) == 0 for lane in range(2))
    del keep
    ctx.close()


def test_no_cost(golden_dir):
    """a context that never calls the new entry points counts no launch under the new name and the launches it always made; one
    that gathers counts exactly its gathers"""
    g = np.load(os.path.join(golden_dir, "oracle_small_seq.npz"))
    W, H = int(g["W"]), int(g["H"])
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), W, H)
    for sad in (False, True):
        p = hip.default_params()
        if sad:
            p.match_method, p.ifm_method, p.max_y_diff = 2, 2, 2.0
        ctx = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, kernel_times=True)
        ctx.set_params(p); ctx.set_camera(cam)
        for t in range(3):
            ctx.process_host([(g["L%d" % t], g["R%d" % t])])
        kt = ctx.kernel_times(appended=True)
        assert kt["gather_windows"][1] == 0 and list(kt)[-1] == "gather_windows"          # appended: the earlier names keep their places
        assert list(ctx.kernel_times()) == list(kt)[:-1]
        assert [kt[k][1] for k in SAD_KERNELS] == ([3, 3, 3] if sad else [0, 0, 0]), {k: kt[k] for k in SAD_KERNELS}
        assert kt["fast"][1] == 3 and kt["begin_frame"][1] == 3 and kt["resize"][1] == 3
        if sad:
            k, d = ctx.keypoints(0, 0, 0)
            ctx.put_features(0, 0, 0, k, d, W, H)
            ctx.gather_windows([(g["L2"], g["R2"])], which=0)
            kt = ctx.kernel_times(appended=True)
            assert kt["gather_windows"][1] == 1 and kt["sad_patch"][1] == 3 and kt["begin_frame"][1] == 3 and kt["fast"][1] == 3
        ctx.close()
