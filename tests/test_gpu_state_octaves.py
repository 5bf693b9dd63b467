"""State files for every octave, with the SAD matchers' windows: svo_save_state / svo_load_state under the default configuration
(dmFASTER + smSAD + ifmSAD on three octaves), FAST+ORB on two, ORB with the SAD matchers -- and the unchanged single-octave file.

The file is read back through stereo_vo_amd/state_file.py (an independent reading of the layout) and compared with the getters; a
context of another shape that loads it must continue the stream like the one that kept running."""
import os
import struct
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera, DM_FAST_ORB
from stereo_vo_amd import state_file as SF

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_ref as F                                          # noqa: E402
import sad_ref as S                                             # noqa: E402
from test_faster_cpu import photograph                          # noqa: E402
from test_gpu_parity import load_small, POSE_TOL_M, POSE_TOL_RAD      # noqa: E402

pytestmark = pytest.mark.gpu

SVO_ERR_ARG, SVO_ERR_STATE = -2, -6


def lane_lists(ctx, lane, n_oct):
    """everything a state file carries of one lane, as bytes: [which][octave] -> (left, left desc, right, right desc, pairings, ids)"""
    out = []
    for which in (1, 0):
        for o in range(n_oct):
            kl, dl = ctx.keypoints(lane, which, 0, o); kr, dr = ctx.keypoints(lane, which, 1, o)
            out.append((kl.tobytes(), dl.tobytes(), kr.tobytes(), dr.tobytes(), ctx.matches(lane, which, o).tobytes(), ctx.match_ids(lane, which, o).tobytes()))
    return out


def assert_file_equals_getters(s, ctx, lane, n_oct, windows):
    """read_state's record against the getters; windows: per frame name, whether the file must carry them"""
    for which, name in ((1, "pre"), (0, "cur")):
        for o in range(n_oct):
            g = s[name] if o == 0 else s["octaves"][o - 1][name]
            for side, sn in ((0, "left"), (1, "right")):
                k, d = ctx.keypoints(lane, which, side, o)
                assert g[sn][0].tobytes() == k.tobytes() and g[sn][1].tobytes() == d.tobytes(), (name, o, sn, len(g[sn][0]), len(k))
            assert g["matches"].tobytes() == ctx.matches(lane, which, o).tobytes(), (name, o)
            assert list(g["ids"]) == list(ctx.match_ids(lane, which, o)), (name, o)
            if windows[name]:
                for side, sn in ((0, "left"), (1, "right")):
                    win, flag = ctx.windows(lane, which, side, o)
                    fw, ff = s["windows"][name][o][sn]
                    assert (ff == flag).all() and (fw[flag == 0] == win[flag == 0]).all() and not fw[flag != 0].any(), (name, o, sn)
        if not windows[name]:
            assert s["windows"] is None or s["windows"][name] is None, name


def assert_resumed_like(a, la, b, lb, n_oct, tag, first_iteration_ok=False):
    """lane lb of b (which loaded) against lane la of a (which kept running), after both processed the same next frame"""
    ra, rb = a.result(la), b.result(lb)
    for o in range(n_oct):
        for which in (0, 1):
            for side in (0, 1):
                assert b.keypoints(lb, which, side, o)[0].tobytes() == a.keypoints(la, which, side, o)[0].tobytes(), (tag, "keypoints", which, o, side)
            assert b.matches(lb, which, o).tobytes() == a.matches(la, which, o).tobytes(), (tag, "pairings", which, o)
            assert b.match_ids(lb, which, o).tobytes() == a.match_ids(la, which, o).tobytes(), (tag, "ids", which, o)
        assert b.tracked(lb, o).tobytes() == a.tracked(la, o).tobytes(), (tag, "tracked", o, len(b.tracked(lb, o)), len(a.tracked(la, o)))
    assert (rb.valid, rb.error_code, rb.tracked_feats_from_last_frame, list(rb.track_stats)) == (ra.valid, ra.error_code, ra.tracked_feats_from_last_frame, list(ra.track_stats)), tag
    assert first_iteration_ok or (ra.valid and ra.error_code != 4), (tag, ra.valid, ra.error_code)        # tracked, not voecFirstIteration
    if ra.valid:      # the file does not carry the warm start: same optimum within the suite's tolerance
        dp = np.abs(np.array(rb.outPose) - np.array(ra.outPose))
        print("%s: pose difference %s" % (tag, dp))
        assert dp[:3].max() < POSE_TOL_M and dp[3:].max() < POSE_TOL_RAD, (tag, dp)


@pytest.fixture(scope="module")
def default_stream(golden_dir, tmp_path_factory):
    """the default configuration on three crops of the photograph, saved: (context A, parameters, camera, crops, path)"""
    L, R = photograph(golden_dir)
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    p = F.faster_params(hip.default_params(), t=10, orb_nfeats=1200, n_oct=3, nms=1)
    p.vo_use_matches_ids = 1
    crops = [(np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])) for x, y in S.CROPS]
    a = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 17, max_octaves=3)
    a.set_params(p); a.set_camera(cam)
    for t in range(3):
        a.process_host([crops[t]])
    path = str(tmp_path_factory.mktemp("state") / "default.bin")
    a.save_state(0, path)
    yield a, p, cam, crops, path
    a.close()


def test_default_configuration(default_stream):
    a, p, cam, crops, path = default_stream
    w, h = S.CROP_W, S.CROP_H
    s = SF.read_state(path)
    assert s["npyr"] == 3 and s["size"] == (w, h) and len(s["octaves"]) == 2
    assert s["num_tracked_last_frame"] == a.result(0).tracked_feats_from_last_frame
    assert_file_equals_getters(s, a, 0, 3, {"pre": True, "cur": True})
    assert min(len(s["pre"]["left"][0]), len(s["octaves"][1]["cur"]["right"][0])) >= 50
    b = hip.Context(n_lanes=2, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 17, max_octaves=3)       # another lane count on purpose
    b.set_params(p); b.set_camera(cam)
    b.process_host([crops[0]] * 2); b.wait()                                                           # unrelated history in the target lane
    b.load_state(1, path)
    assert lane_lists(b, 1, 3) == lane_lists(a, 0, 3)
    for which in (0, 1):
        for o in range(3):
            for side in (0, 1):
                wa, fa = a.windows(0, which, side, o); wb, fb = b.windows(1, which, side, o)
                assert (fa == fb).all() and (wa[fa == 0] == wb[fb == 0]).all(), (which, o, side)
                assert (b.row_index(1, which, side, o) == a.row_index(0, which, side, o)).all(), ("row table", which, o, side)
            assert (b.matches_row_index(1, which, o) == a.matches_row_index(0, which, o)).all(), ("row table of the pairings", which, o)
    a.process_host([crops[3]]); b.process_host([crops[3]] * 2)
    print("tracked per octave after the resume:", [len(a.tracked(0, o)) for o in range(3)])
    assert all(len(a.tracked(0, o)) >= 10 for o in range(3))
    assert_resumed_like(a, 0, b, 1, 3, "default configuration")
    b.close()


def section_ends(buf):
    """the byte offset behind every section of a state file with a block (npyr, each list, the tail, the block's header, ...)"""
    ends = [8]
    off = 8
    groups = {"pre": [], "cur": []}
    for name in ("pre", "cur"):
        for _ in range(2):
            k, _d, off = SF._load_keypoints(buf, off); ends.append(off)
            groups[name].append([len(k)])
        _m, _i, off = SF._load_matches(buf, off); ends.append(off)
    off += 41; ends.append(off)
    ends.append(off + 8); ends.append(off + 20)                  # inside the block's header: behind magic + version, behind n_oct, w, h
    n_oct, = struct.unpack_from("<I", buf, off + 8)
    hw = buf[off + 20], buf[off + 21]
    off += 22; ends.append(off)
    for _ in range(1, n_oct):
        for name in ("pre", "cur"):
            for i in range(2):
                k, _d, off = SF._load_keypoints(buf, off); ends.append(off)
                groups[name][i].append(len(k))
            _m, _i, off = SF._load_matches(buf, off); ends.append(off)
    first_windows = off
    for f, name in enumerate(("pre", "cur")):
        if not hw[f]:
            continue
        for o in range(n_oct):
            for i in range(2):
                n, = struct.unpack_from("<Q", buf, off)
                assert n == groups[name][i][o]
                ends.append(off + 8); ends.append(off + 8 + n)
                off += 8 + 65 * n; ends.append(off)
    assert off == len(buf)
    return sorted(set(e for e in ends if e < len(buf))), first_windows


def test_malformed_files(default_stream, tmp_path):
    """truncation at every section boundary, an n_oct mismatch, a windows count that is not its list's, a bad magic, a size above the
    context's maximum: SVO_ERR_ARG each, and the target lane's lists are what they were"""
    a, p, cam, crops, path = default_stream
    w, h = S.CROP_W, S.CROP_H
    buf = open(path, "rb").read()
    ends, first_windows = section_ends(buf)
    assert len(ends) >= 40
    b = hip.Context(n_lanes=2, max_w=w, max_h=h, max_kps=2048, max_cand=1 << 17, max_octaves=3)
    b.set_params(p); b.set_camera(cam)
    b.process_host([crops[1]] * 2); b.process_host([crops[2]] * 2); b.wait()
    before = lane_lists(b, 1, 3), bytes(b.result(1))
    bad = str(tmp_path / "bad.bin")
    legacy = ends[7]                                              # behind the tail: a file without a block, which a three-octave context refuses too
    assert struct.unpack_from("<I", buf, legacy) == (SF.EXT_MAGIC,)

    def refused(data, text, ctx=b, lane=1):
        open(bad, "wb").write(data)
        rc = ctx.L.svo_load_state(ctx.h, lane, os.fsencode(bad))
        msg = ctx.L.svo_last_error(ctx.h)
        assert rc == SVO_ERR_ARG and text in msg, (rc, msg, len(data))

    for e in ends + [ends[-1] + 1, len(buf) - 1]:
        refused(buf[:e], b"n_oct = 1" if e == legacy else b"malformed or truncated")
    assert (lane_lists(b, 1, 3), bytes(b.result(1))) == before
    refused(buf + b"\0", b"behind the end")
    refused(buf[:legacy] + b"SVEY" + buf[legacy + 4:], b"magic")
    refused(buf[:legacy + 4] + struct.pack("<I", 2) + buf[legacy + 8:], b"version")
    n0, = struct.unpack_from("<Q", buf, first_windows)
    refused(buf[:first_windows] + struct.pack("<Q", n0 - 1) + buf[first_windows + 8:], b"windows count differs")
    refused(buf[:8] + struct.pack("<Q", 2049) + buf[16:], b"max_kps")
    assert (lane_lists(b, 1, 3), bytes(b.result(1))) == before
    # another octave count than the file's, and a context too small for the file's frames
    q = p.copy(); q.nOctaves = 2
    b.set_params(q)
    refused(buf, b"n_oct = 3")
    assert b"n_oct = 2" in b.L.svo_last_error(b.h)
    b.set_params(p)
    assert (lane_lists(b, 1, 3), bytes(b.result(1))) == before
    small = hip.Context(n_lanes=1, max_w=640, max_h=480, max_kps=2048, max_cand=1 << 16, max_octaves=3)
    small.set_params(p)
    refused(buf, b"760 x 560", ctx=small, lane=0)
    small.close()
    # the lane still continues its own stream, and the good file still loads
    b.process_host([crops[3]] * 2); a_like = lane_lists(b, 0, 3)
    assert lane_lists(b, 1, 3) == a_like
    b.load_state(1, path)
    assert_file_equals_getters(SF.read_state(path), b, 1, 3, {"pre": True, "cur": True})
    b.close()


def small_stream(golden_dir, p, n_oct, frames=3, max_octaves=None):
    g, cam, _ = load_small(golden_dir)
    W, H = int(g["W"]), int(g["H"])
    a = hip.Context(n_lanes=1, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, max_octaves=max_octaves or n_oct)
    a.set_params(p); a.set_camera(cam)
    for t in range(frames):
        a.process_host([(g["L%d" % t], g["R%d" % t])])
    b = hip.Context(n_lanes=2, max_w=W, max_h=H, max_kps=1024, max_cand=1 << 15, max_octaves=max_octaves or n_oct)
    b.set_params(p); b.set_camera(cam)
    b.process_host([(g["L0"], g["R0"])] * 2); b.wait()
    return g, cam, a, b, W, H


def test_fast_orb_two_octaves_hamming(golden_dir, tmp_path):
    """lists of two octaves, no windows: a block with has_windows = (0, 0)"""
    _, _, p = load_small(golden_dir)
    p.detect_method, p.nOctaves, p.vo_use_matches_ids = DM_FAST_ORB, 2, 1
    g, cam, a, b, W, H = small_stream(golden_dir, p, 2)
    path = str(tmp_path / "fast_orb.bin")
    a.save_state(0, path)
    s = SF.read_state(path)
    assert s["npyr"] == 2 and s["size"] == (W, H) and len(s["octaves"]) == 1 and s["windows"] == {"pre": None, "cur": None}
    assert_file_equals_getters(s, a, 0, 2, {"pre": False, "cur": False})
    assert len(s["octaves"][0]["cur"]["matches"]) >= 10
    b.load_state(1, path)
    assert lane_lists(b, 1, 2) == lane_lists(a, 0, 2)
    a.process_host([(g["L3"], g["R3"])]); b.process_host([(g["L3"], g["R3"])] * 2)
    assert len(a.tracked(0, 0)) >= 10
    assert_resumed_like(a, 0, b, 1, 2, "FAST+ORB", first_iteration_ok=True)
    a.close(); b.close()


def test_orb_single_octave_sad(golden_dir, tmp_path):
    """one octave, smSAD + ifmSAD on the photograph crops: the block carries the windows, and the loaded lane tracks the next frame
    with ifmSAD"""
    L, R = photograph(golden_dir)
    w, h = S.CROP_W, S.CROP_H
    cam = StereoCamera.simple(500.0, w / 2.0, h / 2.0, 0.12, w, h)
    crops = [(np.ascontiguousarray(L[y:y + h, x:x + w]), np.ascontiguousarray(R[y:y + h, x:x + w])) for x, y in S.CROPS]
    p = S.photo_params(hip.default_params(), orb_nfeats=600)
    a = hip.Context(n_lanes=1, max_w=w, max_h=h, max_kps=1024, max_cand=1 << 17)
    b = hip.Context(n_lanes=2, max_w=w, max_h=h, max_kps=1024, max_cand=1 << 17)
    for c in (a, b):
        c.set_params(p); c.set_camera(cam)
    for t in range(3):
        a.process_host([crops[t]])
    b.process_host([crops[0]] * 2); b.wait()
    path = str(tmp_path / "orb_sad.bin")
    a.save_state(0, path)
    s = SF.read_state(path)
    assert s["npyr"] == 1 and s["size"] == (w, h) and s["octaves"] == []
    assert_file_equals_getters(s, a, 0, 1, {"pre": True, "cur": True})
    b.load_state(1, path)
    a.process_host([crops[3]]); b.process_host([crops[3]] * 2)
    print("ORB + SAD: tracked", len(a.tracked(0, 0)))
    assert len(a.tracked(0, 0)) >= 20
    assert_resumed_like(a, 0, b, 1, 1, "ORB + SAD")
    a.close(); b.close()


def legacy_size(s):
    """the length of a file of the reference's layout that holds these octave-0 lists"""
    n = 8 + 41
    for name in ("pre", "cur"):
        for side in ("left", "right"):
            n += 8 + 28 * len(s[name][side][0]) + 12 + 32 * len(s[name][side][0])
        m, ids = s[name]["matches"], s[name]["ids"]
        n += 16 + len(m) * (16 + (8 if len(ids) == len(m) else 0))
    return n


def test_single_octave_without_sad_writes_no_block(golden_dir, tmp_path):
    _, _, p = load_small(golden_dir)
    p.vo_use_matches_ids = 1
    g, cam, a, b, W, H = small_stream(golden_dir, p, 1, max_octaves=2)       # (room for more octaves does not make a block)
    path = str(tmp_path / "legacy.bin")
    a.save_state(0, path)
    s = SF.read_state(path)
    assert (s["size"], s["octaves"], s["windows"]) == (None, [], None) and s["npyr"] == 1
    assert os.path.getsize(path) == legacy_size(s)
    assert_file_equals_getters(s, a, 0, 1, {"pre": False, "cur": False})
    b.load_state(1, path)
    a.process_host([(g["L3"], g["R3"])]); b.process_host([(g["L3"], g["R3"])] * 2)
    assert_resumed_like(a, 0, b, 1, 1, "no block")
    a.close(); b.close()


def test_sad_selected_for_the_last_frame_only(golden_dir, tmp_path):
    """frames 0-1 without a SAD method, frame 2 under smSAD: has_windows = (0, 1); after the load the refusal rule of a stream that
    switches to ifmSAD applies to the loaded lane exactly as to the one that kept running"""
    g0, _, _ = load_small(golden_dir)
    base = S.photo_params(hip.default_params(), orb_nfeats=int(g0["orb_nfeats"]), match_method=1, ifm_method=1)
    g, cam, a, b, W, H = small_stream(golden_dir, base, 1, frames=2)
    sad = base.copy(); sad.match_method = 2
    a.set_params(sad)
    a.process_host([(g["L2"], g["R2"])])
    path = str(tmp_path / "last.bin")
    a.save_state(0, path)
    buf = open(path, "rb").read()
    s = SF.read_state(path)
    assert s["windows"]["pre"] is None and s["windows"]["cur"] is not None
    assert buf[legacy_size(s) + 20:legacy_size(s) + 22] == bytes([0, 1])
    assert_file_equals_getters(s, a, 0, 1, {"pre": False, "cur": True})
    b.set_params(sad)
    b.load_state(1, path)
    with pytest.raises(hip.SvoError, match="never gathered"):
        b.windows(1, 1, 0, 0)
    assert (b.windows(1, 0, 0, 0)[1] == a.windows(0, 0, 0, 0)[1]).all()
    trk = sad.copy(); trk.ifm_method = 2; trk.ifm_sad_max_distance = -1
    a.set_params(trk); b.set_params(trk)
    fr = (hip.Frame * 2)()
    for i in range(2):
        fr[i].left = hip.Image(g["L3"].ctypes.data, W, H, W); fr[i].right = hip.Image(g["R3"].ctypes.data, W, H, W)
    mask = (hip.C.c_uint64 * 2)(2, 0)                                      # lane 1 alone: lane 0 of b has other history
    rcs = a.L.svo_process(a.h, fr, hip.RUN_ALL), b.L.svo_process_lanes(b.h, fr, hip.RUN_ALL, mask)
    assert rcs == (SVO_ERR_STATE, SVO_ERR_STATE), rcs
    assert b"previous frame" in a.L.svo_last_error(a.h) and b"lane 1" in b.L.svo_last_error(b.h) and b"previous frame" in b.L.svo_last_error(b.h)
    # the next frame starts both lanes afresh
    a.process_host([(g["L3"], g["R3"])]); b.process_host([None, (g["L3"], g["R3"])], active=[1])
    assert_resumed_like(a, 0, b, 1, 1, "after the refusal", first_iteration_ok=True)
    assert a.result(0).error_code == 4 and b.result(1).error_code == 4      # voecFirstIteration
    a.close(); b.close()
