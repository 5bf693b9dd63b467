"""The covariance of every pose increment (svo_set_pose_covariance, k_pose_covariance in csrc/k_gn.hip) held to the
extended-precision reference of tests/pose_cov_ref.py.

With initial_max_iters = max_iters = 0 and a custom start stage 5 iterates nowhere: the returned delta is the start bit for bit, the
mask is the NMS survivors, and the record is one evaluation at a known point -- the point tests/test_pose_cov_ref_cpu.py qualifies
without a GPU (no pixel within 1e-10 px of a rounding midpoint, so n_used is exact and what is left is float64 rounding).  The
tolerances are 16 times what a plain float64 walk of the same formulas reaches (constants and their measurement: that file).
Then full runs at the returned delta over the returned inliers, several lanes bit for bit against the one-lane entry, idle lanes,
off / on / graphs, the batch scheduler, and the other block sizes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import stage5_ref as S
import pose_cov_ref as Pc
from stereo_vo_amd import hip
from stereo_vo_amd.abi import PoseCov, StereoCamera, north_star_params
from test_pose_cov_ref_cpu import K_INFO, K_SIG, K_COV, K_INFO_ORDINARY, K_COV_ORDINARY, SWITCH_CASE, FACTOR, cov_skipped, state_is_asserted_ok

pytestmark = pytest.mark.gpu

EPS = Pc.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SINGLE = Pc.single_cases()
_ids = lambda cases: [c[0] for c in cases]


def O():
    from oracle import oracle
    return oracle


def base_params():
    return north_star_params(hip.default_params(), orb_nfeats=40)


def new_context(max_kps, n_lanes=1, **kw):
    return hip.Context(n_lanes=n_lanes, max_w=S.W, max_h=S.H, max_kps=max_kps, max_cand=1 << 15, **kw)


@pytest.fixture(scope="module")
def contexts():
    """one one-lane context per max_kps with the feature on, shared by the tests of this file"""
    made = {}
    def get(max_kps):
        if max_kps not in made:
            made[max_kps] = new_context(max_kps)
            made[max_kps].set_pose_covariance(True)
        return made[max_kps]
    yield get
    for c in made.values(): c.close()


def mats(cov):
    return {f: np.array(cov.matrix(f)) for f in ("info", "cov_delta", "cov_pose")}


def check_record(tag, cov, ref, expect_state):
    """the record against the reference: integers exact, info / sigma2 / covariances within FACTOR x the CPU test's constants, every
    matrix symmetric to the bit.  expect_state None: SVO_COV_OK or SVO_COV_RANK_DEFICIENT (too close to the pivot test to predict)."""
    m = mats(cov)
    fro = np.linalg.norm
    k_info_max, k_cov_max = (K_INFO, K_COV) if tag.startswith(SWITCH_CASE) else (K_INFO_ORDINARY, K_COV_ORDINARY)
    assert (cov.n_used, cov.dof) == (ref["n_used"], ref["dof"]), (tag, cov.n_used, cov.dof, ref["n_used"], ref["dof"])
    if expect_state is None: assert cov.state in (Pc.COV_OK, Pc.COV_RANK_DEFICIENT), (tag, cov.state)
    else: assert cov.state == expect_state, (tag, cov.state, expect_state)
    for f in m: assert m[f].tobytes() == m[f].T.copy().tobytes(), (tag, f, "not symmetric to the bit")
    k_info = fro(m["info"] - ref["info"]) / (fro(ref["info"]) * EPS)
    if cov.state == Pc.COV_NO_DOF:
        assert cov.sigma2 == 0 and not m["cov_delta"].any() and not m["cov_pose"].any() and m["info"].any(), tag
        k_sig = 0.0
    else: k_sig = abs(cov.sigma2 - ref["sigma2"]) / (ref["sigma2"] * EPS)
    line = "\n%s: n_used %d, state %d, kappa %.3g, info %.4g of 2^-52 (bound %.4g), sigma2 %.4g (bound %.4g)" % (tag, cov.n_used, cov.state, ref["kappa"], k_info, FACTOR * k_info_max, k_sig, FACTOR * K_SIG)
    k_cov = {}
    if cov.state in (Pc.COV_OK, Pc.COV_DELTA_ONLY) and not cov_skipped(ref["kappa"]):
        for f in (("cov_delta", "cov_pose") if cov.state == Pc.COV_OK else ("cov_delta",)):
            k_cov[f] = fro(m[f] - ref[f]) / (fro(ref[f]) * ref["kappa"] * EPS)
            line += ", %s %.4g of kappa 2^-52 (bound %.4g)" % (f, k_cov[f], FACTOR * k_cov_max)
    print(line)
    assert k_info <= FACTOR * k_info_max, (tag, "info", k_info)
    assert k_sig <= FACTOR * K_SIG, (tag, "sigma2", k_sig)
    for f, k in k_cov.items(): assert k <= FACTOR * k_cov_max, (tag, f, k)
    if cov.state == Pc.COV_RANK_DEFICIENT: assert not m["cov_delta"].any() and not m["cov_pose"].any(), tag
    if cov.state == Pc.COV_DELTA_ONLY: assert not m["cov_pose"].any() and m["cov_delta"].any(), tag
    if cov.state == Pc.COV_OK: assert (np.diag(m["cov_delta"]) > 0).all() and (np.diag(m["cov_pose"]) > 0).all(), tag


def expected_state(name):
    if name == "collinear-eps0": return Pc.COV_RANK_DEFICIENT
    return Pc.COV_OK if state_is_asserted_ok(name) else None


def run_zero_iterations(ctx, case, robust):
    """stage 5 with both iteration limits at zero from the case's start: (result, record)"""
    name, mk, build, start, md = case
    lists = Pc.case_scene(case)
    ctx.set_params(Pc.zero_iteration_params(base_params(), robust, md))
    v, r, resid, outl = ctx.change_in_pose(*lists, S.camera(), init6=start)
    assert v and (r.num_it, r.num_it_final, r.error_code, r.status) == (0, 0, 0, 0), (name, v, r.num_it, r.num_it_final)
    assert bytes(r.delta) == np.asarray(start, np.float64).tobytes(), (name, "the returned delta is the custom start, bit for bit")
    return r, ctx.pose_covariance(0)


@pytest.mark.parametrize("robust", [1, 0])
@pytest.mark.parametrize("case", SINGLE, ids=_ids(SINGLE))
def test_single_evaluation_at_a_known_pose(contexts, case, robust):
    """T 8 (dof 26), 64 / 65 (one wave and one more), 1024 / 1025 on 2048 entries (the last LDS size of k_gauss_newton's mask and the first
    `big` one), the smallest context, starts on either side of the small-angle switch, a mask that removes a real share (perm-md12:
    the survivors are the oracle's, and the kernel's own single evaluation returns the same ones), non-finite Jacobians
    (n_used < |M|), and the collinear scene down to a rank-deficient A."""
    name, mk, build, start, md = case
    ctx = contexts(mk)
    survivors = None
    if name.startswith("perm"):
        p1 = S.single_step_params(base_params(), robust, md)
        o = O().Oracle(p1); resid_o = o.change_in_pose(*S.scene(case), S.camera(), init6=start)[2]; o.close()
        ctx.set_params(p1)
        resid = ctx.change_in_pose(*S.scene(case), S.camera(), init6=start)[2]
        survivors = resid_o < 1e300
        assert np.array_equal(resid < 1e300, survivors), (name, "survivors of the stage-5 NMS mask")
        assert survivors.sum() < len(survivors) - 3, "the mask removes a real share"
    lists, ref, surv = Pc.case_reference(case, robust, survivors=survivors)
    r, cov = run_zero_iterations(ctx, case, robust)
    if name.startswith("nonfinite"): assert cov.n_used < int(surv.sum())
    check_record("%s %s" % (name, "robust" if robust else "plain"), cov, ref, expected_state(name))


@pytest.mark.parametrize("robust", [1, 0])
def test_pitch_of_ninety_degrees_gives_delta_only(contexts, robust):
    """a start of (0, pi / 2, 0, 0, 0, 0): cos(pitch) = 0, yaw and roll are not separable, G is singular"""
    case = Pc.pitch_case()
    lists, ref, surv = Pc.case_reference(case, robust)
    r, cov = run_zero_iterations(contexts(case[1]), case, robust)
    check_record("%s %s" % (case[0], "robust" if robust else "plain"), cov, ref, Pc.COV_DELTA_ONLY)


def test_one_point_left_gives_no_dof(contexts):
    """nine points in the mask, eight of them with a non-finite Jacobian: stage 5 ends valid at zero iterations, n_used = 1, dof = -2:
    SVO_COV_NO_DOF with info, n_used and dof set and everything else zero"""
    case = Pc.no_dof_case()
    lists, ref, surv = Pc.case_reference(case, 1)
    r, cov = run_zero_iterations(contexts(case[1]), case, 1)
    assert (cov.n_used, cov.dof) == (1, -2)
    check_record(case[0], cov, ref, Pc.COV_NO_DOF)


FULL = Pc.full_cases()


@pytest.mark.parametrize("case", FULL, ids=_ids(FULL))
def test_full_runs(case):
    """default iteration limits: the reference is evaluated at the RETURNED delta over the points of the returned inlier list; runs
    that do not end valid leave SVO_COV_NONE and an all-zero record"""
    name, mk, build, ov, expect = case
    lists = build(S.camera())
    p = S.with_overrides(base_params(), ov)
    ctx = new_context(mk)
    ctx.set_params(p); ctx.set_pose_covariance(True)
    v, r, resid, outl = ctx.change_in_pose(*lists, S.camera())
    cov = ctx.pose_covariance(0)
    ctx.close()
    assert bool(v) == (name in Pc.FULL_VALID), (name, v)
    if not v:
        assert cov.state == Pc.COV_NONE and bytes(cov) == bytes(PoseCov()), (name, cov.state)
        return
    ref = Pc.reference(lists, S.camera(), np.array(r.delta), p.use_robust_kernel, p.kernel_param, Pc.inlier_mask(lists, outl))
    assert ref["dmid"] >= 1e-10, (name, ref["dmid"])
    assert ref["rel_pd"] >= 1e3
    check_record(name, cov, ref, Pc.COV_OK)


def lane_content(cam):
    return {0: S.permuted(cam, S.BASE_TRUE, 1100, seed=51, noise=0.3, n_out=100),           # scratch path of k_gauss_newton
            1: S.permuted(cam, S.BASE_TRUE, 40, seed=52, noise=0.3, n_out=4),
            2: S.permuted(cam, S.BASE_TRUE, 300, seed=53, noise=0.3, n_out=30)}


def put_lists(ctx, lane, lists):
    t, pre_m, cur_m, pre_l, pre_r, cur_l, cur_r = lists
    ctx.put_features(lane, 1, 0, pre_l, None, S.W, S.H); ctx.put_features(lane, 1, 1, pre_r, None, S.W, S.H)
    ctx.put_features(lane, 0, 0, cur_l, None, S.W, S.H); ctx.put_features(lane, 0, 1, cur_r, None, S.W, S.H)
    ctx.put_matches(lane, 1, pre_m); ctx.put_matches(lane, 0, cur_m)
    ctx.put_tracked(lane, t)


def test_lanes_and_idle_lanes():
    """three lanes fed through svo_put_*, SVO_RUN_OPTIMIZE alone: every lane's record is, bit for bit, the one-lane getChangeInPose
    record of the same lists.  Then lanes 0 and 2 swap their lists and a step leaves lane 1 out: its record keeps every byte, the
    other two are rewritten.  (No warm start here: a lane's second call would otherwise begin where its first one ended.)"""
    cam = S.camera()
    p = base_params(); p.use_previous_pose_as_initial = 0
    content = lane_content(cam)
    one = {}
    for lane, lists in content.items():
        c1 = new_context(2048); c1.set_params(p); c1.set_pose_covariance(True)
        v = c1.change_in_pose(*lists, cam)[0]
        one[lane] = bytes(c1.pose_covariance(0))
        assert v and c1.pose_covariance(0).state == Pc.COV_OK
        c1.close()
    assert len(set(one.values())) == 3
    ctx = new_context(2048, n_lanes=3)
    ctx.set_params(p); ctx.set_camera(cam); ctx.set_pose_covariance(True)
    for lane, lists in content.items(): put_lists(ctx, lane, lists)
    ctx.run_stages(hip.RUN_OPTIMIZE)
    recs = ctx.pose_covariances()
    for lane in content:
        assert bytes(recs[lane]) == one[lane] == bytes(ctx.pose_covariance(lane)), (lane, recs[lane].state, recs[lane].n_used)
    put_lists(ctx, 0, content[2]); put_lists(ctx, 2, content[0])
    ctx.run_stages(hip.RUN_OPTIMIZE, active=[0, 2])
    recs = ctx.pose_covariances()
    assert bytes(recs[1]) == one[1], "an idle lane keeps its record"
    assert bytes(recs[0]) == one[2] and bytes(recs[2]) == one[0], "the active lanes are rewritten"
    ctx.reset(1)
    assert bytes(ctx.pose_covariance(1)) == bytes(PoseCov()) and bytes(ctx.pose_covariance(0)) == one[2], "svo_reset zeroes the lane's record, as its svo_result"
    ctx.close()


def small_sequence():
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_small_seq.npz"))
    cam = StereoCamera.simple(float(g["F"]), float(g["cx"]), float(g["cy"]), float(g["baseline"]), int(g["W"]), int(g["H"]))
    p = north_star_params(hip.default_params(), orb_nfeats=int(g["orb_nfeats"]))
    return g, cam, p, [(g["L%d" % t], g["R%d" % t]) for t in range(4)]


def run_sequence(ctx, frames):
    """every frame's (result bytes, record bytes or None)"""
    out = []
    for pair in frames:
        ctx.process_host([pair])
        out.append(bytes(ctx.result(0)))
    return out


def test_off_on_and_graphs():
    g, cam, p, frames = small_sequence()
    mk = lambda **kw: hip.Context(n_lanes=1, max_w=int(g["W"]), max_h=int(g["H"]), max_kps=1024, max_cand=1 << 15, **kw)
    # off: the getters refuse, no launch of the new kernel, results byte for byte those of a context that never heard of the feature
    never = mk(kernel_times=True); never.set_params(p); never.set_camera(cam)
    want = run_sequence(never, frames)
    assert sum(1 for r in want if hip.Result.from_buffer_copy(r).valid) >= 2
    off = mk(kernel_times=True); off.set_params(p); off.set_camera(cam)
    off.set_pose_covariance(True); off.set_pose_covariance(False)
    assert run_sequence(off, frames) == want
    kt_never, kt_off = never.kernel_times(appended=True), off.kernel_times(appended=True)
    assert list(kt_off) == list(kt_never) and "pose_covariance" not in kt_off, "off: the list of names is the one it always was"
    assert [c for _, c in kt_off.values()] == [c for _, c in kt_never.values()]
    rec = PoseCov()
    for rc in (off.L.svo_get_pose_covariance(off.h, 0, C.byref(rec)), off.L.svo_get_pose_covariances(off.h, C.byref(rec)), never.L.svo_get_pose_covariance(never.h, 0, C.byref(rec))):
        assert rc == -6
    assert b"svo_set_pose_covariance" in off.L.svo_last_error(off.h)
    never.close()
    # on, plain launches: the poses do not move, the kernel runs once per frame, a record per valid frame
    off.kernel_times_reset(); off.reset(); off.set_pose_covariance(True)
    plain = []
    for i, pair in enumerate(frames):
        off.process_host([pair])
        assert bytes(off.result(0)) == want[i]
        plain.append(bytes(off.pose_covariance(0)))
        cov, r = off.pose_covariance(0), off.result(0)
        assert cov.state == (Pc.COV_OK if r.valid else Pc.COV_NONE), (i, cov.state, r.valid)
        if not r.valid: assert plain[-1] == bytes(PoseCov())
    kt = off.kernel_times(appended=True)
    assert list(kt)[:-1] == list(kt_never) and list(kt)[-1] == "pose_covariance" and "pose_covariance" not in off.kernel_times()
    assert kt["pose_covariance"][1] == kt["gauss_newton"][1] == len(frames)
    off.close()
    # on, under svo_use_graphs: the replayed frames give the same records; toggling drops the graphs
    gr = mk(); gr.set_params(p); gr.set_camera(cam); gr.set_pose_covariance(True); gr.use_graphs(True)
    for i, pair in enumerate(frames):
        gr.process_host([pair])
        assert bytes(gr.result(0)) == want[i] and bytes(gr.pose_covariance(0)) == plain[i], i
    captured, replayed = gr.graph_count()
    assert captured >= 1 and replayed >= 1, (captured, replayed)
    gr.set_pose_covariance(True)
    assert gr.graph_count()[0] == captured, "the same value again changes nothing"
    gr.set_pose_covariance(False)
    assert gr.graph_count()[0] == 0, "a change of value drops the captured graphs"
    gr.close()


def test_batch_and_device_copy():
    """2 contexts x 2 lanes on the small sequence: svo_batch_pose_covariances is the per-context getters in global lane order, and
    svo_copy_pose_covariances_async delivers the same bytes"""
    import torch
    from stereo_vo_amd.pipeline import StreamBatch
    g, cam, p, frames = small_sequence()
    batch = StreamBatch(p, cam, int(g["W"]), int(g["H"]), 4, 2, max_kps=1024, max_cand=1 << 15)
    arr = (PoseCov * 4)()
    assert batch.L.svo_batch_pose_covariances(batch.h, arr) == -6, "off: SVO_ERR_STATE"
    batch.set_pose_covariance(True)
    # streams 0 and 2 run the sequence forwards, 1 and 3 start one frame later: four different records per step
    order = [[0, 1, 2, 3], [1, 2, 3, 0], [0, 1, 2, 3], [1, 2, 3, 0]]
    dev = [(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()) for l, r in frames]
    torch.cuda.synchronize()
    for step in range(3):
        batch.step([(dev[order[s][step]][0].data_ptr(), dev[order[s][step]][1].data_ptr()) for s in range(4)])
    recs = batch.pose_covariances()
    res = batch.results()
    own = [bytes(r) for c in batch.ctxs for r in c.pose_covariances()]
    assert [bytes(r) for r in recs] == own
    assert all(r.valid for r in res) and all(r.state == Pc.COV_OK for r in recs)
    assert bytes(recs[0]) == bytes(recs[2]) and bytes(recs[1]) == bytes(recs[3]) and bytes(recs[0]) != bytes(recs[1])
    for k, c in enumerate(batch.ctxs):
        dst = torch.zeros(2 * C.sizeof(PoseCov), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.copy_pose_covariances_async(dst.data_ptr(), dst.numel())
        c.wait()
        assert dst.cpu().numpy().tobytes() == b"".join(own[2 * k:2 * k + 2])
    batch.close()


def gn_nt_child():
    """the body of the child process of test_other_block_sizes: SVO_GN_NT is read when a context is created, from the environment of its process"""
    case = [c for c in SINGLE if c[0] == "shape-T1025-mk2048"][0]
    ctx = new_context(case[1]); ctx.set_pose_covariance(True)
    for robust in (1, 0):
        lists, ref, surv = Pc.case_reference(case, robust)
        r, cov = run_zero_iterations(ctx, case, robust)
        check_record("%s %s" % (case[0], "robust" if robust else "plain"), cov, ref, Pc.COV_OK)
    ctx.close()
    print("bounds hold")


@pytest.mark.parametrize("nt", [256, 512])
def test_other_block_sizes(nt):
    """SVO_GN_NT = 256 and 512 (other instances of both kernel templates, another number of partial sums) on the T = 1025 case"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_pose_cov as G; G.gn_nt_child()" % (ROOT, here)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, SVO_GN_NT=str(nt)), capture_output=True, text=True, timeout=300)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "bounds hold" in out.stdout, (nt, out.stdout[-600:], out.stderr[-1500:])
