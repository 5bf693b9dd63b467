"""dmFASTER's detect chain of csrc/k_detect.hip -- k_half, k_faster / k_faster_dyn, k_faster_nms (chunked_grid_nms<FasterKeys>) and
k_nms_rowsort behind them -- on the hand-built images of tests/faster_scenes.py: every arc of the segment test on both sides of 12 and
of the threshold, on every tile seam and on the first and last row a thread owns; responses that are computed zeros, clamped radicands,
sums beyond 2^24, windows over four tiles and on the columns of the border rule; octaves with one-pixel-wide last tiles and with a single
pixel that can carry a response; NMS grids whose cells hold several corners, decision chains 59 deep, caps inside a tie group and lists
that cross the 2048-corner chunk.  tests/test_faster_scenes_cpu.py asserts on the reference alone that the scenes do hold these.

Bit for bit against tests/faster_ref.py through test_gpu_faster.assert_same_lists (all seven fields, the row tables, the zero descriptor
rows), status word 0, the octave images byte for byte -- every scene twice: with the NMS off (every corner with its response: the raw view
of k_faster) and with the scene's NMS setting.  Families 1 and 2 once more as one lane of five, read in place from unaligned device
memory, through k_faster_dyn and under graph replay.  A failure names the family, the scene, the octave and the first keypoint that
differs.  Every test needs a real MI355X: `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import faster_dyn_ref as D                                                           # noqa: E402
import faster_scenes as FS                                                           # noqa: E402
import image_content as IC                                                           # noqa: E402
from test_gpu_faster import assert_same_lists                                        # noqa: E402

pytestmark = pytest.mark.gpu

FORM_FAMILIES = ("rings", "response")
DYN_TARGET = D.DEFAULT_TARGET


def shapes(families):
    """{(w, h, octaves): the scenes of that shape}"""
    out = {}
    for f in families:
        for s in FS.scenes(f):
            out.setdefault((s["w"], s["h"], s["n_oct"]), []).append(s)
    return out


def context(w, h, n_oct, n_lanes=1):
    """a context for w x h frames (svo_create asks for a capacity of 64 x 64 at least)"""
    return hip.Context(n_lanes=n_lanes, max_w=max(w, 64), max_h=max(h, 64), max_kps=4096, max_cand=1 << 15, max_octaves=n_oct)


def use(ctx, s, nms):
    ctx.set_params(FS.scene_params(hip.default_params(), s, nms))
    ctx.set_klt_win(s["win"])


def describe_kp(k, i):
    return "(%d, %d) response %08x" % (int(k["x"][i]), int(k["y"][i]), int(k["response"][i:i + 1].view(np.uint32)[0]))


def first_difference(ctx, lane, s, feats):
    """the octave, side and first keypoint at which the lane's lists leave the reference's"""
    for o, f in enumerate(feats):
        for side in (0, 1):
            k, want = ctx.keypoints(lane, 0, side, o)[0], f[side]
            n = min(len(k), len(want))
            bad = next((i for i in range(n) if k[i].tobytes() != want[i].tobytes()), None)
            if bad is not None:
                return "octave %d side %d: %d keypoints against %d; first, keypoint %d: got %s, reference %s" % (o, side, len(k), len(want), bad, describe_kp(k, bad), describe_kp(want, bad))
            if len(k) != len(want):
                longer = k if len(k) > n else want
                return "octave %d side %d: %d keypoints against %d; keypoint %d only in %s: %s" % (o, side, len(k), len(want), n, "the kernels' list" if len(k) > n else "the reference's list", describe_kp(longer, n))
            if (ctx.row_index(lane, 0, side, o) != f[2 + side]).any():
                return "octave %d side %d: the row tables differ" % (o, side)
    return "no keypoint differs"


def check(ctx, lane, s, nms, thresholds=None, form=""):
    """the lane's lists against the reference's for the scene: the first failure's text or None"""
    head = "%s / %s / %s%s" % (s["family"], s["name"], "NMS %d" % s["md"] if nms else "no NMS", form and " / " + form)
    if ctx.status_word(lane):
        return "%s: status word %x" % (head, ctx.status_word(lane))
    feats = FS.feats(s["name"], bool(nms), thresholds)
    for o in range(1, s["n_oct"]):
        for side in (0, 1):
            got, want = ctx.level(lane, side, o), feats[o][4]
            if got.shape != want.shape or (got != want).any():
                ys, xs = np.nonzero(got != want) if got.shape == want.shape else ([-1], [-1])
                return "%s / octave %d side %d (%dx%d): %d pixels of the image differ, first at (%d, %d)" % (head, o, side, want.shape[1], want.shape[0], len(ys), xs[0], ys[0])
    try:
        assert_same_lists(ctx, lane, feats, head, ctx.result(lane))
    except AssertionError as e:
        return "%s: %s [%s]" % (head, first_difference(ctx, lane, s, feats), str(e).split("\n")[0][:160])
    return None


def feed_in_place(ctx, img, held, flags=hip.RUN_DETECT):
    """the image as a device frame read in place: rows w + 3 bytes apart, the first at an odd byte offset, random bytes around (held: kept alive)"""
    h, w = img.shape
    ptrs, buf, host = IC.place([img], w + 3, [1 + 2 * (len(held) % 7)], seed=len(held))
    held.append((buf, host))
    ctx.process_device([(ptrs[0], ptrs[0])], w, h, w + 3, flags)


def run_scenes(ctx, scenes, held=None, settings=(False, True)):
    """every scene through lane 0 with the NMS off and on (held: read in place instead of from host arrays): the failures' texts"""
    failed = []
    for s in scenes:
        for nms in settings:
            use(ctx, s, nms)
            if held is None:
                ctx.process_host([(s["img"], s["img"])], hip.RUN_DETECT)
            else:
                feed_in_place(ctx, s["img"], held)
            msg = check(ctx, 0, s, nms, form="in place" if held is not None else "")
            if msg:
                failed.append(msg)
    return failed


def report(failed):
    return "%d failures; the first three: %s" % (len(failed), failed[:3])


def assert_untouched(ctx, held):
    ctx.wait()
    for buf, host in held:
        IC.assert_untouched(buf, host)


@pytest.mark.parametrize("family", list(FS.FAMILIES))
def test_family_raw_and_under_its_nms(family):
    """every scene of the family with the NMS off -- every corner with its response, k_faster's raw view -- and with its NMS setting; the
    octave images; the sizes family once more in place at stride w + 3 from an odd address"""
    failed, n = [], 0
    for (w, h, n_oct), scenes in shapes([family]).items():
        ctx = context(w, h, n_oct)
        failed += run_scenes(ctx, scenes)
        if family == "sizes":
            held = []
            failed += run_scenes(ctx, scenes, held)
            assert_untouched(ctx, held)
        n += len(scenes)
        ctx.close()
    assert n == len(FS.scenes(family))
    assert not failed, report(failed)


def test_frames_below_64x64_are_refused():
    """the 13 x 9 image of the sizes family is an octave, not a frame: a frame that small is refused before anything is enqueued"""
    ctx = context(64, 64, 1)
    use(ctx, FS.scene("rings-t20-c100-0"), True)
    img = FS.noise(13, 9, 0)
    with pytest.raises(hip.SvoError, match="capacity"):
        ctx.process_host([(img, img)], hip.RUN_DETECT)
    ctx.close()


def test_as_lane_three_of_five():
    """lane 3 of a five-lane context whose lane 1 sits out and whose other lanes hold noise: the lists stay as they were"""
    failed = []
    for (w, h, n_oct), scenes in shapes(FORM_FAMILIES).items():
        noise = [FS.noise(w, h, 100 + i) for i in range(3)]
        ctx = context(w, h, n_oct, n_lanes=5)
        for n, s in enumerate(scenes):
            a, b, c = noise[n % 3], noise[(n + 1) % 3], noise[(n + 2) % 3]
            for nms in (False, True):
                use(ctx, s, nms)
                ctx.process_host([(a, b), None, (b, c), (s["img"], s["img"]), (c, a)], hip.RUN_DETECT, active=[0, 2, 3, 4])
                msg = check(ctx, 3, s, nms, form="lane 3 of 5")
                if msg:
                    failed.append(msg)
            assert len(ctx.keypoints(1, 0, 0)[0]) == 0, s["name"]
            assert len(ctx.keypoints(0, 0, 0)[0]) > 0 or s["t"] == 254, s["name"]
        ctx.close()
    assert not failed, report(failed)


def test_read_in_place_from_unaligned_memory():
    """device frames read in place at stride w + 3 from an odd byte offset, poison around: k_faster's byte loads at level 0 clamp to the
    image, not to the row pitch; nothing writes the caller's memory"""
    failed = []
    for (w, h, n_oct), scenes in shapes(FORM_FAMILIES).items():
        ctx = context(w, h, n_oct)
        held = []
        failed += run_scenes(ctx, scenes, held)
        assert_untouched(ctx, held)
        ctx.close()
    assert not failed, report(failed)


def test_through_k_faster_dyn():
    """svo_set_dyn_fast_threshold on: a fresh estimator per scene, so the left image is detected at the scene's threshold and the right
    one at the threshold the left count leads to (tests/faster_dyn_ref.py).  The thresholds are read back, held to the walk, and the
    expected lists are built at them"""
    failed, moved = [], 0
    for (w, h, n_oct), scenes in shapes(FORM_FAMILIES).items():
        ctx = context(w, h, n_oct)
        ctx.set_dyn_fast_threshold(True, DYN_TARGET)
        for s in scenes:
            for nms in (False, True):
                p = FS.scene_params(hip.default_params(), s, nms)
                use(ctx, s, nms)
                ctx.reset()
                ctx.process_host([(s["img"], s["img"])], hip.RUN_DETECT)
                st = ctx.faster_stats(0).as_dict(n_oct)
                used = (tuple(st["used_left"]), tuple(st["used_right"]))
                want = D.Estimator(DYN_TARGET, s["win"]).frame(s["img"], s["img"], p)[1]
                if (list(used[0]), list(used[1])) != (want["used_left"], want["used_right"]) or st["corners_left"] != want["corners_left"] or st["next"] != want["next"]:
                    failed.append("%s / %s: thresholds and counts %s against the walk's %s" % (s["family"], s["name"], st, want))
                    continue
                moved += used[1] != used[0]
                msg = check(ctx, 0, s, nms, thresholds=used, form="k_faster_dyn at %s" % (used,))
                if msg:
                    failed.append(msg)
        ctx.close()
    assert moved > 20, moved                                                  # the right image did run at another threshold than the left one
    assert not failed, report(failed)


def test_under_graph_replay():
    """svo_use_graphs: every scene with the NMS off and on, four times in a row each -- one capture per upload slot, then the third and fourth call replay them"""
    failed = []
    for (w, h, n_oct), scenes in shapes(FORM_FAMILIES).items():
        ctx = context(w, h, n_oct)
        ctx.use_graphs(True)
        for s in scenes:
            for nms in (False, True):
                use(ctx, s, nms)
                for rep in range(4):
                    ctx.process_host([(s["img"], s["img"])], hip.RUN_DETECT)
                    msg = check(ctx, 0, s, nms, form="graphs, call %d" % rep)
                    if msg:
                        failed.append(msg)
        captured, replayed = ctx.graph_count()
        assert captured >= 1 and replayed >= 2 * len(scenes), (captured, replayed)
        ctx.close()
    assert not failed, report(failed)
