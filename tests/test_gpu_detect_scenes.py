"""The detect chain of csrc/k_detect.hip -- k_resize, k_fast / k_fast_redo, k_select, k_harris, k_select_sort, k_describe and k_nms_rowsort
behind them -- on the hand-built images of tests/detect_scenes.py: dots on every tile seam, group lane and row block of k_fast and on both
sides of its threshold, selection cuts inside and outside a tie group, one weight pixel per octant of the orientation, blur windows that
saturate, pyramid levels whose last k_resize tile is 127, 128, 1 and 3 columns wide and whose interior is one row.
tests/test_detect_scenes_cpu.py asserts on the oracle alone that the scenes do reach those edges and that the oracle gives what their
construction predicts.

Byte for byte against the oracle: the pyramid levels (oracle.resize chained from the image), the detector's raw list under SVO_DEBUG_MODE=9
(positions, response bits, angle bits, descriptors; and the scene's own prediction where it has one), and the final lists in the default
order -- the same image on both sides, detection only.  The one-level families once more under the linear tile order, without the
speculative threshold, under other k_describe shapes, as one lane of five, and read in place from unaligned caller memory.  A failure names
the family, the scene, the level and the first keypoint that differs in level coordinates.  Every test needs a real MI355X: `pytest -m gpu`."""
import os
import sys

import numpy as np
import pytest

from stereo_vo_amd import hip
from stereo_vo_amd.abi import StereoCamera

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_scenes as DS                                                           # noqa: E402
import image_content as IC                                                           # noqa: E402

pytestmark = pytest.mark.gpu

KNOBS = ("SVO_DEBUG_MODE", "SVO_DESC_KPW", "SVO_DESC_TL")
SCALES = [np.float32(1.2 ** l) for l in range(8)]
ONE_LEVEL = ("dots", "orient", "blur")


def context(monkeypatch, w, h, env=None, n_lanes=1):
    """a context for w x h frames; the knobs of `env` are read when it is created and gone from the environment afterwards"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    ctx = hip.Context(n_lanes=n_lanes, max_w=w, max_h=h, max_kps=1024, max_cand=1 << 15, kernel_times=True)
    for k in env or {}:
        monkeypatch.delenv(k)
    ctx.set_camera(StereoCamera.simple(200.0, w / 2.0, h / 2.0, 0.1, w, h))
    return ctx


def calls(ctx, name):
    return int(ctx.kernel_times()[name][1])


def shapes(families):
    """{(w, h): the scenes of that shape}, scenes with equal parameters next to each other"""
    out = {}
    for f in families:
        for s in DS.scenes(f):
            out.setdefault((s["w"], s["h"]), []).append(s)
    return out


class Params:
    """set_params only when the scene's parameters differ from the ones in force"""

    def __init__(self, ctx):
        self.ctx, self.key = ctx, None

    def use(self, s):
        key = (s["orb_nlevels"], s["orb_nfeats"], s["nms"], s["min_distance"])
        if key != self.key:
            self.ctx.set_params(DS.scene_params(hip.default_params(), s))
            self.key = key


def describe_kp(k, d, i):
    x, y = DS.level_xy(k[i:i + 1], SCALES)
    return "level %d at (%d, %d) response %08x angle %08x descriptor %s.." % (int(k["octave"][i]), x[0], y[0], int(k["response"][i:i + 1].view(np.uint32)[0]),
                                                                          int(k["angle"][i:i + 1].view(np.uint32)[0]), d[i, :6].tobytes().hex())


def same_list(what, s, got, want):
    """None, or the family, scene, list and first differing keypoint (level coordinates) of two (keypoints, descriptors) lists"""
    (k, d), (ko, do) = got, want
    if len(k) == len(ko) and k.tobytes() == ko.tobytes() and (d == do).all():
        return None
    n = min(len(k), len(ko))
    bad = [i for i in range(n) if k[i].tobytes() != ko[i].tobytes() or (d[i] != do[i]).any()]
    head = "%s / %s / %s: %d keypoints against the oracle's %d, %d of the first %d differ" % (s["family"], s["name"], what, len(k), len(ko), len(bad), n)
    if bad:
        return head + "; first, keypoint %d: got %s, oracle %s" % (bad[0], describe_kp(k, d, bad[0]), describe_kp(ko, do, bad[0]))
    longer, dl = (k, d) if len(k) > n else (ko, do)
    return head + "; keypoint %d only in %s: %s" % (n, "the kernels' list" if len(k) > n else "the oracle's list", describe_kp(longer, dl, n))


def check_levels(ctx, lane, s, which=-1):
    want = DS.oracle_levels(s["name"], which)
    for side in (0, 1):
        for l in range(1, 8):
            got = ctx.level(lane, side, l)
            if got.shape != want[l].shape or (got != want[l]).any():
                ys, xs = np.nonzero(got != want[l]) if got.shape == want[l].shape else ([-1], [-1])
                return "%s / %s / level %d side %d (%dx%d): %d pixels differ, first at (%d, %d)" % (s["family"], s["name"], l, side, want[l].shape[1], want[l].shape[0], len(ys), xs[0], ys[0])
    return None


def check_expect(s, k):
    """the raw list against what the scene's construction predicts"""
    e = s["expect"]
    pos = [(int(x), int(y)) for x, y in zip(k["x"], k["y"])]
    if "fast" in e and sorted(pos, key=lambda p: (p[1], p[0])) != [(x, y) for x, y, _ in e["fast"]]:
        want = {(x, y) for x, y, _ in e["fast"]}
        return "%s / %s / level 0: corners against the prediction: not predicted %s, missing %s" % (s["family"], s["name"], sorted(set(pos) - want)[:4], sorted(want - set(pos))[:4])
    if "kept" in e and pos != e["kept"]:
        first = next((i for i, (a, b) in enumerate(zip(pos, e["kept"])) if a != b), min(len(pos), len(e["kept"])))
        return "%s / %s / level 0: kept %d against %d predicted, first difference at keypoint %d: %s against %s" % (s["family"], s["name"], len(pos), len(e["kept"]), first, pos[first:first + 1], e["kept"][first:first + 1])
    if "angle" in e:
        for p, a in zip(pos, k["angle"]):
            want = e["angle"].get(p)
            if want is None or (abs((float(a) - want + 180.0) % 360.0 - 180.0) > 0.3 if s["weighted"] and want % 90.0 else float(a) != want):
                return "%s / %s / level 0 at %s: angle %r against %r predicted" % (s["family"], s["name"], p, float(a), want)
    return None


def check(ctx, lane, s, which, raw, levels=False):
    """the lane's lists of image `which` of the scene: the first failure's text or None"""
    if ctx.status_word(lane):
        return "%s / %s: status word %x" % (s["family"], s["name"], ctx.status_word(lane))
    msg = check_levels(ctx, lane, s, which) if levels and s["orb_nlevels"] == 8 else None
    for side in (0, 1):
        if raw and not msg:
            got = ctx.raw_keypoints(lane, side)
            msg = same_list("raw list, side %d" % side, s, got, DS.oracle_raw(s["name"], which)) or (check_expect(s, got[0]) if which in (-1, len(s["imgs"]) - 1) else None)
        msg = msg or same_list("final list, side %d" % side, s, ctx.keypoints(lane, 0, side), DS.oracle_final(s["name"], which))
    return msg


def run_scenes(ctx, scenes, raw, levels=False, feed=None):
    """every image of every scene through lane 0 (feed(ctx, img) hands it over; default: host arrays): the failures' texts"""
    failed, par = [], Params(ctx)
    for s in scenes:
        par.use(s)
        for which, img in enumerate(s["imgs"]):
            if feed:
                feed(ctx, img)
            else:
                ctx.process_host([(img, img)], hip.RUN_DETECT)
            msg = check(ctx, 0, s, which, raw, levels)
            if msg:
                failed.append(msg)
    return failed


def feed_in_place(ctx, img, held):
    """the image as a device frame read in place: rows w + 3 bytes apart, the first at an odd byte offset, random bytes around (held: kept alive)"""
    h, w = img.shape
    ptrs, buf, host = IC.place([img], w + 3, [1 + 2 * (len(held) % 7)], seed=len(held))
    held.append((buf, host))
    ctx.process_device([(ptrs[0], ptrs[0])], w, h, w + 3, hip.RUN_DETECT)


def report(failed):
    return "%d failures; the first three: %s" % (len(failed), failed[:3])


# ---------------------------------------------------------------------------------------------------------------------------------------
# the detector's own order (SVO_DEBUG_MODE=9): levels, raw lists, predictions, final lists
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", DS.LEVEL_SIZES, ids=["%dx%d" % wh for wh in DS.LEVEL_SIZES])
def test_levels_family(monkeypatch, w, h):
    """eight levels of every content at one size: the levels themselves, the raw list, the final list -- in the detector's order and in the default one"""
    scenes = shapes(["levels"])[w, h]
    assert len(scenes) == 7
    ctx = context(monkeypatch, w, h, {"SVO_DEBUG_MODE": "9"})
    failed = run_scenes(ctx, scenes, raw=True, levels=True)
    assert calls(ctx, "resize") >= len(scenes) and calls(ctx, "describe") == len(scenes), ctx.kernel_times()
    # ... and read in place from caller memory at stride w + 3 from an odd byte offset, poison around: the byte-staging branch of k_resize
    held = []
    failed += run_scenes(ctx, scenes, raw=True, levels=True, feed=lambda c, img: feed_in_place(c, img, held))
    ctx.wait()
    for buf, host in held:
        IC.assert_untouched(buf, host)
    ctx.close()
    ctx = context(monkeypatch, w, h)
    failed += run_scenes(ctx, scenes, raw=False, levels=True)
    ctx.close()
    assert not failed, report(failed)


@pytest.mark.parametrize("family", ["dots", "cuts", "orient", "blur", "spacing"])
def test_raw_and_final_lists_in_the_detectors_order(monkeypatch, family):
    """SVO_DEBUG_MODE=9: k_describe on every raw keypoint (its mode without the survivors' list), then the NMS"""
    failed, n = [], 0
    for (w, h), scenes in shapes([family]).items():
        ctx = context(monkeypatch, w, h, {"SVO_DEBUG_MODE": "9"})
        failed += run_scenes(ctx, scenes, raw=True)
        assert calls(ctx, "describe") == sum(len(s["imgs"]) for s in scenes) and calls(ctx, "fast") == calls(ctx, "describe"), (family, ctx.kernel_times())
        n += len(scenes)
        ctx.close()
    assert n == len(DS.scenes(family))
    assert not failed, report(failed)


def test_redo_scene_runs_k_fast_redo(monkeypatch):
    """the redo scene of `cuts`: the first image speculates the level's threshold up to its dots' score, the second has fewer than
    2 x quota corners there, so k_select queues the level and k_fast_redo finds its corners at the caller's threshold"""
    s = DS.scene("cuts-redo-10")
    for env in ({"SVO_DEBUG_MODE": "9"}, None):
        ctx = context(monkeypatch, s["w"], s["h"], env)
        ctx.set_params(DS.scene_params(hip.default_params(), s))
        ctx.process_host([(s["imgs"][0],) * 2], hip.RUN_DETECT)
        assert check(ctx, 0, s, 0, raw=env is not None) is None and ctx.redo_count() == 0
        ctx.process_host([(s["imgs"][1],) * 2], hip.RUN_DETECT)
        msg = check(ctx, 0, s, 1, raw=env is not None)
        assert msg is None, msg
        assert ctx.redo_count() == 2, ctx.redo_count()                  # level 0 of both images
        kt = ctx.kernel_times()
        assert kt["select"][1] == 2 and kt["select"][0] > 0.0 and kt["fast"][1] == 2, kt          # the span of k_select, k_fast_redo, k_harris and k_select_sort
        ctx.close()


def test_k_describe_runs_in_both_of_its_modes(monkeypatch):
    """k_describe over the level-segmented detector slots, dead ones among them (SVO_DEBUG_MODE=9), and over the work items k_nms_rowsort
    leaves (the default order): one launch per frame in either, the same final list"""
    s = DS.scene("blur-blocks-100")
    lists = []
    for env in ({"SVO_DEBUG_MODE": "9"}, None):
        ctx = context(monkeypatch, s["w"], s["h"], env)
        failed = run_scenes(ctx, [s], raw=env is not None)
        assert not failed, report(failed)
        assert calls(ctx, "describe") == 1 and calls(ctx, "nms_rowsort") == 1, ctx.kernel_times()
        lists.append(ctx.keypoints(0, 0, 0))
        ctx.close()
    assert lists[0][0].tobytes() == lists[1][0].tobytes() and (lists[0][1] == lists[1][1]).all() and len(lists[0][0]) == len(DS.blur_positions())


# ---------------------------------------------------------------------------------------------------------------------------------------
# the default order and the other forms: final lists
# ---------------------------------------------------------------------------------------------------------------------------------------
FORMS = [None, {"SVO_DEBUG_MODE": "8"}, {"SVO_DEBUG_MODE": "12"}, {"SVO_DESC_KPW": "1"}, {"SVO_DESC_KPW": "3"}, {"SVO_DESC_KPW": "64"}, {"SVO_DESC_TL": "0"}]


@pytest.mark.parametrize("env", FORMS, ids=["default" if e is None else "-".join("%s=%s" % kv for kv in e.items()) for e in FORMS])
def test_final_lists_under_every_form(monkeypatch, env):
    """the default order (k_describe on the NMS survivors), the linear tile order, no speculative threshold, one, three and 64 keypoints per
    wave of k_describe, its operands in registers: a fresh context each, as the knobs are read once per context"""
    families = ("dots", "cuts", "orient", "blur", "spacing") if env is None else ONE_LEVEL
    failed = []
    for (w, h), scenes in shapes(families).items():
        ctx = context(monkeypatch, w, h, env)
        failed += run_scenes(ctx, scenes, raw=False)
        assert calls(ctx, "describe") == sum(len(s["imgs"]) for s in scenes), ctx.kernel_times()
        if env == {"SVO_DEBUG_MODE": "12"}:
            assert ctx.redo_count() == 0
        ctx.close()
    assert not failed, (env, report(failed))


def test_as_lane_three_of_five(monkeypatch):
    """lane 3 of a five-lane context whose lane 1 sits out and whose other lanes hold noise"""
    failed = []
    for (w, h), scenes in shapes(ONE_LEVEL).items():
        rng = np.random.RandomState(w)
        noise = [rng.randint(0, 256, (h, w)).astype(np.uint8) for _ in range(3)]
        ctx = context(monkeypatch, w, h, n_lanes=5)
        par = Params(ctx)
        for n, s in enumerate(scenes):
            par.use(s)
            img = s["imgs"][0]
            a, b, c = noise[n % 3], noise[(n + 1) % 3], noise[(n + 2) % 3]
            ctx.process_host([(a, b), None, (b, c), (img, img), (c, a)], hip.RUN_DETECT, active=[0, 2, 3, 4])
            msg = check(ctx, 3, s, 0, raw=False)
            if msg:
                failed.append(msg)
            assert len(ctx.keypoints(1, 0, 0)[0]) == 0 and len(ctx.keypoints(0, 0, 0)[0]) > 20, s["name"]
        ctx.close()
    assert not failed, report(failed)


def test_read_in_place_from_unaligned_memory(monkeypatch):
    """device frames read in place at stride w + 3 from an odd byte offset, poison around: the byte form of k_harris, k_fast's and
    k_describe's window DMA from any byte at level 0 (test_levels_family does the same for k_resize); nothing writes the caller's memory"""
    failed = []
    for (w, h), scenes in shapes(ONE_LEVEL).items():
        ctx = context(monkeypatch, w, h, {"SVO_DEBUG_MODE": "9"})
        held = []
        failed += run_scenes(ctx, scenes, raw=True, feed=lambda c, img: feed_in_place(c, img, held))
        ctx.wait()
        for buf, host in held:
            IC.assert_untouched(buf, host)
        ctx.close()
    assert not failed, report(failed)
