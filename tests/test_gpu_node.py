"""The device-resident node graph (include/viekf_node.h, vi_ekf_amd.NodeGraph) against its restatement tests/node_ref.py by
the tolerance of tests/test_gpu_parity.py (max|d| <= 1e-9 max|ref| per array and 1e-6 element-wise, integers exact) -- and
against itself where the claim is bit for bit: device pointers against host pointers, the packed against the canonical form
of P, a resumed run against the run it resumes.  The restatement is fed the device's own edges, x and P: what is held to it
here is the node algebra, the intake has tests/test_gpu_frame.py."""
import ctypes as C

import numpy as np
import pytest

from tests import node_ref as NR
from tests import sim_ref as R
from tests.test_frame_ref_cpu import SCRIPT
from tests.test_gpu_frame import RESIDENT, STREAMING, _batch, _params, frame, hover, noise, same_bits, script_frames, state
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu


def cuda(a):
    import torch
    return None if a is None else torch.as_tensor(a).cuda().contiguous()


def host(t):
    return t.cpu().numpy() if hasattr(t, "is_cuda") else np.asarray(t)


def random_edges(rng, B):
    """edges as a reset reports them: {t, q_yaw, cov_pos (column-major, symmetric positive definite), cov_yaw}"""
    e = np.zeros((B, 17))
    for b in range(B):
        A = rng.normal(0.0, 0.1, (3, 3))
        e[b] = np.concatenate([rng.normal(0.0, 1.0, 3), NR.from_euler(0.0, 0.0, rng.uniform(-3.0, 3.0)),
                               (A @ A.T + 0.01 * np.eye(3)).ravel(order="F"), [rng.uniform(0.001, 0.01)]])
    return e


def node_bits(st):
    return [host(st[k]) for k in ("node", "node_cov", "true_node", "count")]


def against_ref(ng, ref, g, what):
    """node, node_cov, count, global pose and covariance against the restatement on the device's own x and P.  The query
    comes FIRST: it reads P in whatever form the last launch left it in."""
    pose, cov = ng.global_pose()
    st = ng.get()
    rst = ref.get()
    assert np.array_equal(st["count"], rst["count"]), what
    assert_close(st["node"], rst["node"], what + " node")
    assert_close(st["node_cov"], rst["node_cov"], what + " node_cov")
    rpose, rcov = ref.global_pose(g.get_state(), g.get_covariance())
    assert_close(pose, rpose, what + " pose")
    assert_close(cov, rcov, what + " cov")
    return pose, cov, st


# ---- scripted frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [STREAMING, RESIDENT])
def test_scripted_frames_against_the_restatement(family):
    """B = 5, N = 8, M = 10, the twelve frames of test_frame_ref_cpu.SCRIPT (resets at frames 2, 3, 6, 8, 11; filter 3 sits two
    frames out, so that the filters' counts differ) with three propagates before each: after every frame node, node_cov, count,
    global pose and covariance against the restatement; a node graph fed device pointers agrees bit for bit with one fed host
    pointers; filters that did not reset keep their node bit for bit"""
    import vi_ekf_amd as v
    B, N, M, K = 5, 8, 10, 3
    p = _params(use_keyframe_reset=True)
    g = _batch(B, N, p, family)
    fi = v.FrameIntake(g)
    ngh, ngd, ref = v.NodeGraph(g, 4), v.NodeGraph(g, 4), NR.BatchNodeRef(B, 4)
    rng = np.random.default_rng(7)
    Rm = noise(B, M, 2)
    resets = np.zeros(B, int)
    for k, rows in enumerate(SCRIPT):
        u, dt = hover(K, B, 100 + k)
        g.step_n(u, dt, None, None, None)
        z, ids, depth = frame(rng, B, M, rows)
        active = np.ones(B, np.uint8)
        active[3] = k not in (2, 3)
        out = fi.intake(z, ids, Rm, depth=depth, active=active)
        xt = rng.normal(0.0, 1.0, (B, 12))
        xt[:, 6:10] /= np.linalg.norm(xt[:, 6:10], axis=1, keepdims=True)
        before = ngh.get()
        ngh.update(out, x_true=xt)
        ngd.update(cuda(out["did_reset"]), cuda(out["edges"]), x_true=cuda(xt))
        ref.update(out["did_reset"], out["edges"], xt)
        pose, cov, st = against_ref(ngh, ref, g, "frame %d" % k)
        assert_close(st["true_node"], ref.get()["true_node"], "true node")
        pd, cd = ngd.global_pose(device=True)
        std = ngd.get(device=True)
        assert pd.is_cuda and cd.is_cuda and all(std[key].is_cuda for key in std)
        assert np.array_equal(host(pd), pose) and np.array_equal(host(cd), cov)
        assert same_bits(node_bits(std), node_bits(st))
        keep = ~out["did_reset"].astype(bool)
        for key in ("node", "node_cov", "true_node", "count"):
            assert np.array_equal(st[key][keep], before[key][keep]), (k, key)
        assert (st["count"][~keep] == before["count"][~keep] + 1).all()
        resets += out["did_reset"]
    assert np.array_equal(ngh.get()["count"], resets) and resets.min() >= 3 and resets[0] == 5 and resets[3] != 5
    th, td = ngh.trail(), ngd.trail(device=True)
    rt = ref.trail()
    assert np.array_equal(th[0], host(td[0])) and np.array_equal(th[1], host(td[1]))
    assert_close(th[0], rt[0], "trail nodes")
    assert np.array_equal(th[1], rt[1])
    assert g.get_status().max() < 8


# ---- any form of P --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,family,inst", [(12, RESIDENT, 0), (50, RESIDENT, -1), (90, STREAMING, -1)])
def test_any_form_of_P(N, family, inst):
    """B = 3.  After a fused step_n the resident family leaves P PACKED (N = 12 on instance <2,1> and N = 50 on <3,7>: two
    different images), the streaming family leaves the part above the diagonal stale: the query before and after
    get_covariance() forces the canonical form agrees bit for bit, it agrees with the restatement, and x, P, len_features and
    the status flags are what a twin batch that was never queried holds"""
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, M = 3, 6
    p = _params(use_keyframe_reset=True)
    rng = np.random.default_rng(31)
    z0, _, _ = frame(rng, B, N, list(range(N)), spread=0)
    u, dt = hover(4, B, 5)
    zs = np.stack([z0[:, j] + rng.normal(0.0, 0.5, (B, 2)) for j in range(M)], axis=1)
    slot = np.tile(np.arange(M, dtype=np.int32), (B, 1))
    ga, gb = _batch(B, N, p, family), _batch(B, N, p, family)
    for g in (ga, gb):
        if inst >= 0:
            g.set_tuning(capi.TUNE_RES_INSTANCE, inst)
        for j in range(N):
            g.init_feature(z0[:, j].copy(), np.full(B, np.nan))
        g.step_n(u, dt, zs, slot, noise(B, M, 0))
    if family == RESIDENT:
        assert "P packed" in ga.describe(), ga.describe()
    ng, ref = v.NodeGraph(ga), NR.BatchNodeRef(B)
    for _ in range(2):                                       # the node away from the identity
        e = random_edges(rng, B)
        ng.update(np.ones(B, np.uint8), e)
        ref.update(np.ones(B), e)
    pose1, cov1 = ng.global_pose()                           # P as the launch left it
    pd, cd = ng.global_pose(device=True)
    xt = ga.get_state() + rng.normal(0.0, 0.01, (B, ga.nx))
    ge1 = ng.global_error(xt)
    sa = state(ga) + (ga.get_status(),)                      # (get_covariance: canonical from here on)
    pose2, cov2 = ng.global_pose()
    ge2 = ng.global_error(xt)
    assert np.array_equal(pose1, pose2) and np.array_equal(cov1, cov2)
    assert np.array_equal(host(pd), pose1) and np.array_equal(host(cd), cov1)
    assert all(np.array_equal(ge1[k], ge2[k]) for k in ge1)
    assert same_bits(sa, state(gb) + (gb.get_status(),))
    rpose, rcov = ref.global_pose(sa[0], sa[1])
    assert_close(pose1, rpose, "pose")
    assert_close(cov1, rcov, "cov")
    rge = ref.global_error(sa[0], sa[1], xt)
    assert (ge1["info"] == 0).all() and np.array_equal(ge1["info"], rge["info"])
    assert_close(ge1["err"], rge["err"], "err")
    assert_close(ge1["nees"], rge["nees"], "nees")
    # a covariance that is not positive definite: info names the pivot, nees is NaN
    st = ng.get()
    bad = st["node_cov"].copy()
    bad[1, 2 + 6 * 2] = -1.0e3
    ng.set(node_cov=bad)
    ge3 = ng.global_error(xt)
    assert ge3["info"].tolist() == [0, 3, 0] and np.isnan(ge3["nees"][1]) and np.array_equal(ge3["nees"][[0, 2]], ge1["nees"][[0, 2]])


# ---- ring slots -----------------------------------------------------------------------------------------------------------
def test_per_filter_live_slots_are_followed():
    """B = 3 with a history ring and select_filters, a different slot per filter: the frames are taken in and the query reads
    the filters where they live (the batch's own buffers hold the state from before the frames)"""
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, N, M = 3, 8, 10
    p = _params(use_keyframe_reset=True)
    g = _batch(B, N, p)
    g.history_resize(4)
    live = np.array([2, 0, 3], np.int32)
    capi.check(capi.lib().viekf_batch_snapshot_filters(g._h, C.c_void_p(live.ctypes.data), capi.HOST))
    g.select_filters(live)
    fi, ng, ref = v.FrameIntake(g), v.NodeGraph(g), NR.BatchNodeRef(B)
    resets = 0
    for k, (z, ids, depth, active, Rm) in enumerate(script_frames(B, N, M, 19, count=6)):
        out = fi.intake(z, ids, Rm, depth=depth, active=active)
        ng.update(out)
        ref.update(out["did_reset"], out["edges"])
        against_ref(ng, ref, g, "frame %d" % k)
        resets += int(out["did_reset"].sum())
    assert resets > 0 and np.abs(ng.get()["node"][:, :3]).max() > 0


# ---- trail ----------------------------------------------------------------------------------------------------------------
def test_trail_is_a_ring():
    """capacity 2 and five resets: count == 5 and the ring holds resets 3 and 4 at positions k % 2 (filter 2 resets three
    times only: resets 1 and 2).  Capacity 0 is legal and stores nothing."""
    import vi_ekf_amd as v
    B, N = 3, 4
    g = _batch(B, N, _params())
    ng, ng0, ref = v.NodeGraph(g, 2), v.NodeGraph(g, 0), NR.BatchNodeRef(B, 2)
    rng = np.random.default_rng(37)
    edges, nodes = [], []
    for k in range(5):
        e = random_edges(rng, B)
        dr = np.array([1, 1, k % 2 == 0], np.uint8)
        nodes.append(ng.get()["node"])
        edges.append(e)
        ng.update(dr, e)
        ng0.update(dr, e)
        ref.update(dr, e)
    assert ng.get()["count"].tolist() == [5, 5, 3] and ng0.get()["count"].tolist() == [5, 5, 3]
    tn, te = ng.trail()
    assert tn.shape == (B, 2, 7) and te.shape == (B, 2, 17)
    for b in (0, 1):
        for k in (3, 4):
            assert np.array_equal(te[b, k % 2], edges[k][b]) and np.array_equal(tn[b, k % 2], nodes[k][b])
    for r, k in ((1, 2), (2, 4)):                            # filter 2: its resets 1 and 2 came with calls 2 and 4
        assert np.array_equal(te[2, r % 2], edges[k][2]) and np.array_equal(tn[2, r % 2], nodes[k][2])
    rn, re_ = ref.trail()
    assert_close(tn, rn, "trail nodes")
    assert np.array_equal(te, re_)
    t0 = ng0.trail()
    assert t0[0].shape == (B, 0, 7) and t0[1].shape == (B, 0, 17)
    assert same_bits(node_bits(ng0.get()), node_bits(ng.get()))
    ng.reset()
    st = ng.get()
    assert not st["count"].any() and not st["node_cov"].any() and not ng.trail()[0].any() and not ng.trail()[1].any()
    assert np.array_equal(st["node"], np.tile(NR.IDENTITY, (B, 1))) and np.array_equal(st["true_node"], st["node"])


# ---- resume ---------------------------------------------------------------------------------------------------------------
def test_get_reset_set_resumes_bit_for_bit():
    import vi_ekf_amd as v
    B, N = 3, 4
    g = _batch(B, N, _params())
    u, dt = hover(3, B, 41)
    g.step_n(u, dt, None, None, None)
    rng = np.random.default_rng(43)
    es = [random_edges(rng, B) for _ in range(4)]
    xs = [rng.normal(0.0, 1.0, (B, 10)) for _ in range(4)]
    dr = [np.array(m, np.uint8) for m in ([1, 1, 0], [1, 0, 1], [0, 1, 1], [1, 1, 1])]
    na, nb = v.NodeGraph(g, 3), v.NodeGraph(g, 3)
    for k in range(2):
        na.update(dr[k], es[k], x_true=xs[k])
    saved = na.get()
    nb.update(dr[3], es[3], x_true=xs[3])                    # (something to forget)
    nb.reset()
    nb.set(**saved)
    assert same_bits(node_bits(nb.get()), node_bits(saved))
    for k in range(2, 4):
        na.update(dr[k], es[k], x_true=xs[k])
        nb.update(dr[k], es[k], x_true=xs[k])
    assert same_bits(node_bits(na.get()), node_bits(nb.get()))
    assert same_bits(na.global_pose(), nb.global_pose())
    xt = rng.normal(0.0, 1.0, (B, g.nx))
    assert np.array_equal(na.relative_truth(xt), nb.relative_truth(xt), equal_nan=True)
    nb.set(count=np.array([7, 8, 9], np.int32))              # one array alone: the others keep every bit
    st = nb.get()
    assert st["count"].tolist() == [7, 8, 9] and same_bits(node_bits(st)[:3], node_bits(na.get())[:3])


# ---- closed loop ----------------------------------------------------------------------------------------------------------
def test_closed_loop_with_resets_on():
    """node_ref.LOOP_KFR, B = 4, N = 8, 3 s at 250 / 25 Hz with use_keyframe_reset ON: BatchSimulator.step -> step_n ->
    camera -> FrameIntake.intake -> NodeGraph.update(out, x_true = truth), every array between the calls a CUDA tensor.  The
    frames on which each vehicle resets are the restated flight's (they depend on the simulator alone); on the tick before
    each frame consistency(batch, relative_truth(truth)) and global_error factor their matrices (info == 0, finite NEES), and
    after t = 1 s the errors there are inside node_ref.LOOP_KFR_BOUNDS (twice what the restated flight measures on the CPU:
    0.552 m, 2.01 deg global, 0.216 m, 2.03 deg relative to the true node, NEES 5.82)."""
    import torch
    import vi_ekf_amd as v
    B, N = 4, NR.LOOP_KFR_N
    p = NR.loop_kfr_params()
    per = {k: NR.LOOP_KFR[k] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    bs = v.BatchSimulator(B, p, max_features=N, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5, **per)
    bs.set_landmarks(R.jittered_landmarks(77))
    g = v.BatchVIEKF(B, N, dict(p, name="node"))
    fi, ng = v.FrameIntake(g), v.NodeGraph(g, 8)
    R_pix = torch.diag(torch.tensor([10.0, 10.0], dtype=torch.float64)).cuda()
    dt9 = torch.full((9, B), bs.dt, dtype=torch.float64, device="cuda")
    dt1 = torch.full((1, B), bs.dt, dtype=torch.float64, device="cuda")
    frames = int(round(NR.LOOP_KFR_TMAX * 25))
    reset_frames = [[] for _ in range(B)]
    worst = np.zeros((B, 5))
    for f in range(frames):
        u = bs.step(9, device=True)
        g.step_n(u, dt9, None, None, None)
        # the tick before the frame
        tracked, _ = fi.tracked(device=True)
        xt = bs.truth_state(tracked)
        ge = ng.global_error(xt)                             # (first: P is still as the fused launch left it)
        xr = ng.relative_truth(xt)
        diag = v.consistency(g, xr)
        g.sync()
        assert xt.is_cuda and xr.is_cuda and all(ge[k].is_cuda for k in ge)
        info, nees = host(ge["info"]), host(ge["nees"])      # (the test's own look at the results, not part of the loop)
        assert (info == 0).all() and np.isfinite(nees).all(), (f, info, nees)
        assert (host(diag["info"]) == 0).all() and np.isfinite(host(diag["nees"])).all(), f
        if bs.t > 1.0:
            err, x, xrh = host(ge["err"]), g.get_state(), host(xr)
            for b in range(B):
                rel = NR.pose_errors(x[b, 0:3], x[b, 6:10], xrh[b, 0:3], xrh[b, 6:10])
                worst[b] = np.maximum(worst[b], [np.abs(err[b, :3]).max(), np.degrees(np.abs(err[b, 3:]).max()), rel[0], rel[1], nees[b]])
        else:
            worst[:, 4] = np.maximum(worst[:, 4], nees)
        u = bs.step(1, device=True)
        g.step_n(u, dt1, None, None, None)
        z, ids, cnt, dep, _ = bs.camera(N, device=True)
        out = fi.intake(z, ids, R_pix)
        tracked, _ = fi.tracked(device=True)
        ng.update(out, x_true=bs.truth_state(tracked))
        assert u.is_cuda and z.is_cuda and all(out[k].is_cuda for k in out)
        for b in np.nonzero(host(out["did_reset"]))[0]:
            reset_frames[b].append(f)
    w = worst.max(axis=0)
    print("closed loop with resets on, worst on the tick before each frame after t = 1 s: global %.4f m %.4f deg, relative to the "
          "true node %.4f m %.4f deg; global NEES %.4f; resets %s" % (w[0], w[1], w[2], w[3], w[4], [len(r) for r in reset_frames]))
    assert reset_frames == NR.loop_kfr_recorded()["reset_frames"], reset_frames
    st = ng.get()
    assert st["count"].tolist() == [len(r) for r in reset_frames] and min(st["count"]) >= 5
    bound = NR.LOOP_KFR_BOUNDS
    for i, k in enumerate(("global_m", "global_deg", "relative_m", "relative_deg", "nees")):
        assert (worst[:, i] < bound[k]).all() and (worst[:, i] > 0).all(), (k, worst[:, i], bound[k])
    assert not np.isnan(st["node"]).any() and not np.isnan(st["node_cov"]).any() and g.get_status().max() < 8
    # the trail's latest entry composes to the node: node before the move * edge
    tn, te = ng.trail()
    for b in range(B):
        at = (st["count"][b] - 1) % 8
        from oracle.seq_oracle import xform_mul
        assert_close(st["node"][b], xform_mul(tn[b, at], te[b, at, :7]), "trail -> node")


# ---- argument rules -------------------------------------------------------------------------------------------------------
def test_argument_rules():
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, N = 2, 4
    g = _batch(B, N, _params())
    for bad in (-1, 4097):
        with pytest.raises(v.ViekfError) as e:
            v.NodeGraph(g, bad)
        assert e.value.code == capi.ERR_INVALID and "4096" in str(e.value)
    ng = v.NodeGraph(g, 4096)
    ng.close()
    ng = v.NodeGraph(g, 1)
    rng = np.random.default_rng(47)
    dr, e = np.ones(B, np.uint8), random_edges(rng, B)
    for call in (lambda x: ng.update(dr, e, x_true=x), ng.relative_truth, ng.global_error):
        with pytest.raises(v.ViekfError) as ex:
            call(np.zeros((B, 9)))
        assert ex.value.code == capi.ERR_INVALID and "ldx" in str(ex.value)
    assert not ng.get()["count"].any()                       # (the refused update did nothing)
    ng.update(dr, e, x_true=np.tile(NR.IDENTITY[[0, 1, 2, 0, 0, 0, 3, 4, 5, 6]], (B, 1)))      # ldx == 10 is enough
    assert ng.relative_truth(np.zeros((B, 10))).shape == (B, 10)
    with pytest.raises(ValueError, match="mix"):
        ng.update(cuda(dr), e)
    with pytest.raises(ValueError, match="mix"):
        ng.update(dr, e, x_true=torch.zeros((B, 10), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="mix"):
        ng.set(node=np.zeros((B, 7)), count=torch.zeros(B, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        ng.update(dr, e[:, :16])
    with pytest.raises(ValueError, match="shape"):
        ng.update(dr[:1], e)
    with pytest.raises(ValueError, match="both"):
        ng.update(dr)
    with pytest.raises(ValueError, match="x_true"):
        ng.relative_truth(np.zeros(10))
    L, h = capi.lib(), ng._h
    ptr = C.c_void_p(e.ctypes.data)
    assert L.viekf_node_update(h, None, ptr, None, 0, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_node_update(h, ptr, ptr, None, 0, 7) == capi.ERR_INVALID
    assert L.viekf_node_global(h, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_node_global(h, ptr, None, 7) == capi.ERR_INVALID
    assert L.viekf_node_global_error(h, ptr, 17, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_node_relative_truth(h, ptr, None, 17, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_node_get(h, None, None, None, None, 7) == capi.ERR_INVALID
    assert L.viekf_node_get(h, None, None, None, None, capi.HOST) == capi.OK          # NULL skips an array: all four
    pose, cov = ng.global_pose(cov=False)
    assert pose.shape == (B, 7) and cov is None
    # values are taken as given: a NaN edge gives a NaN node, and no flag is raised
    e2 = e.copy()
    e2[1, 0] = np.nan
    ng.update(dr, e2)
    st = ng.get()
    assert np.isnan(st["node"][1, 0]) and not np.isnan(st["node"][0]).any() and not g.get_status().any()
    # a destroyed batch: the node graph refuses to go on, and its own tables can still be released
    g.close()
    with pytest.raises(ValueError, match="closed"):
        ng.global_pose()
    with pytest.raises(ValueError, match="closed"):
        v.NodeGraph(g)
    ng.close()
    with pytest.raises(ValueError, match="closed"):
        ng.get()
