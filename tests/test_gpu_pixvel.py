"""BatchVIEKF.update_pixel_vels / eval_pixel_vel / pixel_flow (include/viekf_pixvel.h, csrc/viekf_kernels_pixvel.hpp) against the
numpy restatement of tests/pixvel_ref.py over the oracle's numpy twin.  Result codes and status bits are compared exactly, x and
P with assert_close of tests/test_gpu_parity.py, and P == P^T is checked.  The cases, the reasons for their inputs and the start
states are in tests/pixvel_cases.py; tests/test_pixvel_ref_cpu.py checks the model itself (finite differences, the oracle's
dynamics, the simulator's kinematics) and that the cases reach what they are for.

Sizes: N = 1, 3, 12 (n = 19, 25, 52), 16, 17, 44 (n = 64, 67, 148: past a 64-row block), 2 with M = 70, B = 5 with the ragged fill [N, N - 3, 1, 0, N - 1] clipped at 0."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from tests import meas_cases as mc
from tests import pixvel_cases as pc
from tests import pixvel_ref as pr
from tests.test_gpu_parity import assert_close
from vi_ekf_amd import capi, scene

pytestmark = pytest.mark.gpu

B = pc.B


def make_gpu(c, batch=B):
    idx = np.arange(batch) % B
    g = v.BatchVIEKF(batch, c["N"], c["params"])
    g.set_state(x=c["x0"][idx], P=c["P0"][idx], len_features=c["len"][idx])
    return g


def call(g, c, z=None, active="case"):
    return g.update_pixel_vels(c["z"] if z is None else z, c["slot"], c["gyro"], c["R"], c["gyro_var"],
                               c["active"] if isinstance(active, str) else active, c["order"])


def check(g, c, res, route, what, want_route=None):
    assert route in (0, 1) and (want_route is None or route == want_route), (what, route)
    assert np.array_equal(res, c["codes"]), (what, res, c["codes"])
    x, P = g.get_state(), g.get_covariance()
    keep = [b for b in range(B) if b != c["poisoned"]]
    assert_close(x[keep], c["x_ref"][keep], "x after " + what)
    assert_close(P[keep], c["P_ref"][keep], "P after " + what)
    assert np.array_equal(P, P.transpose(0, 2, 1), equal_nan=True), "P != P^T after " + what
    for b in c["untouched"]:
        assert np.array_equal(x[b], c["x0"][b]) and np.array_equal(P[b], c["P0"][b], equal_nan=True), "filter %d touched by %s" % (b, what)
    return x, P


def lower(P):
    return np.tril(P)


def run_case(c, want_route=1):
    """the call on two batches at the case's start state, one left to choose (the fused launch) and one held to the M launches:
    both against the reference, and against each other bit for bit -- codes, x, the lower triangle of P, len, status bits"""
    g1, g0 = make_gpu(c), make_gpu(c)
    g0.pixel_vels_route(0)
    r1, route1 = call(g1, c)
    r0, route0 = call(g0, c)
    x1, P1 = check(g1, c, r1, route1, c["name"] + ", fused", want_route)
    x0, P0 = check(g0, c, r0, route0, c["name"] + ", M launches", 0)
    assert np.array_equal(r1, r0) and np.array_equal(x1, x0, equal_nan=True) and np.array_equal(lower(P1), lower(P0), equal_nan=True), c["name"]
    assert np.array_equal(g1.get_len_features(), g0.get_len_features()) and np.array_equal(g1.get_status(), g0.get_status())
    return g1, r1, x1, P1


@pytest.mark.parametrize("N", pc.SIZES)
@pytest.mark.parametrize("drag", [1, 0])
def test_eval_pixel_vel(N, drag):
    """zhat and H of three filters of the ragged batch (one slot each; a filter without that slot answers NaN) against the
    restatement; the batch is bit for bit untouched"""
    sc, ts = pc.start(N, 1, drag, 60 + N)
    pick = [0, 2, 4]
    ts = [ts[b] for b in pick]
    g = v.BatchVIEKF(3, N, sc["params"])
    g.set_state(x=np.stack([t.x for t in ts]), P=np.stack([t.P for t in ts]), len_features=np.array([t.len for t in ts], np.int32))
    before = g.get_state(), g.get_covariance(), g.get_len_features()
    slot = np.array([N - 1, 0, N - 2 if N > 1 else 0], np.int32)
    gyro = np.random.default_rng(N).normal(0.0, 0.3, (3, 3))
    zhat, H = g.eval_pixel_vel(slot, gyro)
    z2, none = g.eval_pixel_vel(slot, gyro, jacobian=False)
    assert none is None and np.array_equal(zhat, z2, equal_nan=True)
    seen = 0
    for b, t in enumerate(ts):
        if slot[b] >= t.len:
            assert np.isnan(zhat[b]).all() and np.isnan(H[b]).all()
            continue
        zr, Hr = pr.h_pixel_vel(t, t.x, int(slot[b]), gyro[b])
        assert_close(zhat[b], zr, "zhat of filter %d" % b)
        assert_close(H[b], Hr, "H of filter %d" % b)
        assert (H[b][Hr == 0.0] == 0.0).all()
        seen += 1
    assert seen >= 1
    after = g.get_state(), g.get_covariance(), g.get_len_features()
    assert all(np.array_equal(a, b) for a, b in zip(before, after)) and not g.get_status().any()


@pytest.mark.parametrize("N,variant", [(N, vv) for N in pc.SIZES for vv in range(len(pc.ONCE_VARIANTS))])
def test_every_slot_once(N, variant):
    """M = N entries, per-filter shuffled slots (slots >= len: INVALID; a -1: SKIPPED); partial update on and off, the three R
    modes with a different R per entry, both orders, gyro_var 0 and > 0, drag on and off"""
    c = pc.case("once", N, variant)
    g, res, x, P = run_case(c)
    assert not g.get_status().any()


@pytest.mark.parametrize("N,variant", [(N, vv) for N in (16, 17, 44) for vv in (0, 3)])
def test_every_slot_once_past_a_row_block(N, variant):
    """nact = 64, 67, 148 in the full filter: one 64-row block of the trailing pass (and of route 0's column walk) exactly, one
    row into the second, a partly filled third -- the partly valid last block and the j <= i mask across blocks; partial update
    on with order 0, off with order 1"""
    c = pc.case("once", N, variant)
    g, res, x, P = run_case(c)
    assert not g.get_status().any()


@pytest.mark.parametrize("order", [0, 1])
def test_m_past_a_wave_and_past_n(order):
    """N = 2, M = 70: the two slots over and over"""
    c = pc.case("repeat", pc.REPEAT_N, order)
    g, res, x, P = run_case(c)
    assert not g.get_status().any()


@pytest.mark.parametrize("order", [0, 1])
def test_mixed_script(order):
    """M = 8 in one call: active 0, 1 and 2 within one filter's row, a flow 5000 px/s off (gated) in the middle with accepted
    entries after it, a NaN z, a filter with a NaN gyro sample (every entry MEAS_NAN) and a filter whose whole row is 2 -- bit
    for bit untouched.  Then a call all of whose entries are gated: every filter bit for bit as before"""
    c = pc.case("mixed", pc.MIXED_N, order)
    g, res, x, P = run_case(c)
    assert not g.get_status().any()
    res, route = call(g, c, z=c["z"] + 5000.0, active=None)
    want = np.where(c["slot"] >= c["len"][:, None], orc.MEAS_INVALID, orc.MEAS_GATED)
    want[pc.MIXED_GYRO_NAN_FILTER][want[pc.MIXED_GYRO_NAN_FILTER] == orc.MEAS_GATED] = orc.MEAS_NAN
    want[pc.MIXED_NAN_FILTER, pc.MIXED_NAN] = orc.MEAS_NAN
    assert route == 1 and np.array_equal(res, want) and (res == orc.MEAS_GATED).sum() >= 16
    assert np.array_equal(g.get_state(), x) and np.array_equal(g.get_covariance(), P) and not g.get_status().any()


@pytest.mark.parametrize("N,variant", [(3, 0), (3, 1), (12, 0), (12, 1)])
def test_fix_depth_inside_the_chain(N, variant):
    """rho < 0 and rho > 1e2 prepared in x, met by an inactive entry (variant 0) or behind an applied one (1); entries on the
    repaired slots behind them; the negative-depth bit only where it belongs"""
    c = pc.case("fix", N, variant)
    g, res, x, P = run_case(c)
    st = g.get_status()
    assert list((st & pc.NEG_DEPTH_BIT) != 0) == [b == pc.FIX_NEG_FILTER for b in range(B)] and not (st & ~np.uint32(pc.NEG_DEPTH_BIT)).any(), st


def test_nan_in_p_that_one_entrys_columns_meet():
    """P(7, first bearing column of slot 1) = NaN in one filter: the entry on slot 1 reads that column, its gain has a NaN and
    its correction is skipped (vi_ekf_meas.cpp:247); the filter's other entries are applied; the codes are 0; both routes agree
    bit for bit (run_case); the other filters against the reference"""
    c = pc.case("poison", 12)
    g, res, x, P = run_case(c)
    b = pc.POISONED
    assert (res[b][c["slot"][b] < c["len"][b]] == 0).all() and pc.POISON_SLOT in list(c["slot"][b])
    assert not np.isnan(x).any() and not np.array_equal(x[b], c["x0"][b]) and np.isnan(P[b]).sum() == 2
    st = g.get_status()                                                 # (set_state raises the NaN bit for the P handed in;
    assert list(st) == [pc.NAN_BIT if k == b else 0 for k in range(B)], st      # no NaN reached x, nothing else is raised)
    # the entry that met the NaN left the filter alone: bit for bit what a run without that entry gives
    act = np.ones(c["slot"].shape, dtype=np.uint8)
    act[b, list(c["slot"][b]).index(pc.POISON_SLOT)] = 2
    h = make_gpu(c)
    call(h, c, active=act)
    assert np.array_equal(h.get_state()[b], x[b]) and np.array_equal(h.get_covariance()[b], P[b], equal_nan=True)


def test_fallback_where_the_lds_layout_does_not_fit():
    """M = 256 at N = 12 needs more LDS than the device gives a workgroup, at N = 3 it fits (viekf_pixvels_lds_bytes against
    viekf_body_lds_limit): routes 0 and 1, the same results -- the entries past the case's own sit out"""
    L = capi.lib()
    limit = C.c_int64(0)
    capi.check(L.viekf_body_lds_limit(0, C.byref(limit)))
    Mx = capi.PIXVELS_MAX_M
    assert L.viekf_pixvels_lds_bytes(12, Mx) > limit.value >= L.viekf_pixvels_lds_bytes(3, Mx)
    assert L.viekf_pixvels_lds_bytes(50, 50) <= limit.value                 # the headline size fuses
    for N, want in ((12, 0), (3, 1)):
        c = pc.case("once", N, 0)
        g = make_gpu(c)
        reps = -(-Mx // N)
        sl = np.ascontiguousarray(np.tile(c["slot"], (1, reps))[:, :Mx])
        zz = np.ascontiguousarray(np.tile(c["z"], (1, reps, 1))[:, :Mx])
        a2 = np.full(sl.shape, 2, dtype=np.uint8)
        a2[:, :N] = 1
        res, route = g.update_pixel_vels(zz, sl, c["gyro"], c["R"], c["gyro_var"], a2, 0)
        assert route == want and np.array_equal(res[:, :N], c["codes"]) and (res[:, N:] == -1).all()
        x, P = g.get_state(), g.get_covariance()
        assert_close(x, c["x_ref"], "x, N = %d" % N)
        assert_close(P, c["P_ref"], "P, N = %d" % N)


# ---- context ----------------------------------------------------------------------------------------------------------------
CTX_N, CTX_M = 12, 10


def _stepped(batch=B, ring=None, per_filter=None):
    """a batch behind two fused steps (P in the kernel's own form), optionally with the live state in a ring slot or in
    per-filter ring slots"""
    sc = scene.make_scene(B, CTX_N, 2, seed=77)
    idx = np.arange(batch) % B
    g = v.BatchVIEKF(batch, CTX_N, sc["params"])
    for i in range(CTX_M):
        assert (g.init_feature(sc["pix"][idx, i, :].copy(), np.full(batch, np.nan)) == 1).all()
    if ring is not None:
        g.history_resize(3)
        g.snapshot(ring)
        capi.check(capi.lib().viekf_batch_select(g._h, ring))
    if per_filter is not None:
        g.history_resize(2)
        g.snapshot(0)
        g.snapshot(1)
        g.select_filters(per_filter)
    z = np.ascontiguousarray(sc["z"][:, idx][:, :, CTX_N - CTX_M:])    # (slot[b, m] = N - 1 - m: the slots that are tracked)
    slot = np.ascontiguousarray(sc["slot"][idx][:, CTX_N - CTX_M:])
    for s in range(2):
        res = g.step(sc["u"][s][idx], sc["dt"][idx], z[s], slot, sc["R"])
        assert (res == 0).all()
    return sc, g


def _ctx_inputs(sc, x, P, ln):
    """twins at the state (x, P, len), honest measurements 3 px/s off the prediction for every tracked slot, last first, and the
    restated result"""
    prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
    from oracle import np_twin
    ts = []
    for b in range(B):
        t = np_twin.TwinFilter(CTX_N, **prm)
        t.x, t.P, t.len = x[b].copy(), P[b].copy(), int(ln[b])
        ts.append(t)
    r = np.random.default_rng(5)
    gyro = r.normal(0.0, 0.2, (B, 3))
    slot = np.tile(np.arange(CTX_M, dtype=np.int32), (B, 1))
    R = np.array([[150.0, 20.0], [20.0, 220.0]])
    z = np.zeros((B, CTX_M, 2))
    codes = np.zeros((B, CTX_M), np.int32)
    for b, t in enumerate(ts):
        for m in reversed(range(CTX_M)):
            z[b, m] = pr.h_pixel_vel(t, t.x, m, gyro[b])[0] + 3.0
            codes[b, m] = pr.update_pixel_vel(t, m, z[b, m], gyro[b], R, 1e-4)
    return dict(slot=slot, z=z, gyro=gyro, R=R, codes=codes, x_ref=np.stack([t.x for t in ts]), P_ref=np.stack([t.P for t in ts]))


_CTX = {}


def _ctx():
    """the start state behind the two steps (read from a batch of its own: reading changes the form of P) and the reference"""
    if not _CTX:
        sc, g0 = _stepped()
        x, P, ln = g0.get_state(), g0.get_covariance(), g0.get_len_features()
        _CTX.update(sc=sc, x0=x, P0=P, **_ctx_inputs(sc, x, P, ln))
    return _CTX


def _ctx_call(g, c, idx=None):
    idx = np.arange(B) if idx is None else idx
    return g.update_pixel_vels(c["z"][idx], c["slot"][idx], c["gyro"][idx], c["R"], 1e-4, None, 1)


def _ctx_check(g, c, res, route):
    assert route == 1 and np.array_equal(res, c["codes"]) and (res == 0).all()
    x, P = g.get_state(), g.get_covariance()
    assert_close(x, c["x_ref"], "x")
    assert_close(P, c["P_ref"], "P")
    assert np.array_equal(P, P.transpose(0, 2, 1)) and not g.get_status().any()
    assert np.abs(x[:, 3:6] - c["x0"][:, 3:6]).max() > 1e-6
    return x, P


def test_behind_a_fused_step():
    c = _ctx()
    sc, g = _stepped()
    print(g.describe())
    assert "P packed" in g.describe() or "P canonical" in g.describe()
    res, route = _ctx_call(g, c)
    x, P = _ctx_check(g, c, res, route)
    sc, g0 = _stepped()                                                 # the M launches behind the same steps: the same bits
    g0.pixel_vels_route(0)
    r0, route0 = _ctx_call(g0, c)
    assert route0 == 0 and np.array_equal(r0, res) and np.array_equal(g0.get_state(), x) and np.array_equal(lower(g0.get_covariance()), lower(P))


def test_in_a_ring_slot():
    c = _ctx()
    sc, g = _stepped(ring=2)
    res, route = _ctx_call(g, c)
    _ctx_check(g, c, res, route)
    capi.check(capi.lib().viekf_batch_select(g._h, -1))                 # the batch's own buffers were not written
    assert not np.array_equal(g.get_state(), c["x_ref"])


def test_with_per_filter_live_slots():
    c = _ctx()
    sc, g = _stepped(per_filter=np.array([0, 1, 1, 0, 1], np.int32))
    res, route = _ctx_call(g, c)
    _ctx_check(g, c, res, route)


def test_more_filters_than_resident_workgroups():
    """B = 600 (the five case filters repeated), N = 3: every copy is bit-equal to its first"""
    c = pc.case("once", 3, 1)
    nb = 600
    idx = np.arange(nb) % B
    g = make_gpu(c, nb)
    res, route = g.update_pixel_vels(c["z"][idx], c["slot"][idx], c["gyro"][idx], c["R"][idx], c["gyro_var"], None, c["order"])
    assert route == 1 and np.array_equal(res, c["codes"][idx])
    x, P = g.get_state(), g.get_covariance()
    assert np.array_equal(x, x[idx]) and np.array_equal(P, P[idx])
    assert_close(x[:B], c["x_ref"], "x of the first five")
    assert_close(P[:B], c["P_ref"], "P of the first five")
    assert not g.get_status().any()


def test_determinism_and_device_pointers():
    """the same call on two fresh batches gives bit-equal x, P and codes; so does the call with device pointers"""
    import torch
    c = pc.case("repeat", pc.REPEAT_N, 1)
    ga, gb, gd = make_gpu(c), make_gpu(c), make_gpu(c)
    ra, _ = call(ga, c)
    rb, _ = call(gb, c)
    dev = torch.device("cuda:0")
    gd.use_torch_stream()
    t = lambda a: torch.tensor(a, device=dev)
    rd, route = gd.update_pixel_vels(t(c["z"]), t(c["slot"]), t(c["gyro"]), t(c["R"]), c["gyro_var"], None, c["order"])
    torch.cuda.synchronize()
    assert route == 1 and np.array_equal(ra, rb) and np.array_equal(rd.cpu().numpy(), ra)
    xa, Pa = ga.get_state(), ga.get_covariance()
    for g in (gb, gd):
        assert np.array_equal(xa, g.get_state()) and np.array_equal(Pa, g.get_covariance())
        assert np.array_equal(ga.get_status(), g.get_status())
    zh, H = ga.eval_pixel_vel(c["slot"][:, 0].copy(), c["gyro"])
    zd, Hd = ga.eval_pixel_vel(t(c["slot"][:, 0].copy()), t(c["gyro"]))
    torch.cuda.synchronize()
    assert np.array_equal(zh, zd.cpu().numpy(), equal_nan=True) and np.array_equal(H, Hd.cpu().numpy(), equal_nan=True)


def test_pixel_flow():
    """ids that vanish, appear and repeat, NaN and infinite coordinates, M_prev != M, a dt that is not positive; host and
    device pointers"""
    import torch
    g = v.BatchVIEKF(3, 2, dict(scene.EKF_YAML))
    r = np.random.default_rng(2)
    Mp, M = 5, 70                                                       # (M past a wave)
    ids_prev = np.array([[4, 7, 7, -1, 9], [1, 2, 3, 4, 5], [0, 1, 2, 3, 4]], np.int32)
    z_prev = r.uniform(0, 600, (3, Mp, 2))
    z_prev[1, 2, 0] = np.nan
    ids = r.integers(-1, 12, (3, M)).astype(np.int32)
    ids[0, :4] = [7, 5, 9, -1]
    z = r.uniform(0, 600, (3, M, 2))
    z[1, 6, 1] = np.inf
    z[0, 9] = np.nan
    dt = np.array([0.04, 0.05, 0.0])
    want = pr.pixel_flow(z_prev, ids_prev, z, ids, np.where(dt > 0, dt, np.nan))
    got = v.pixel_flow(g, z_prev, ids_prev, z, ids, dt)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[2]).all() and np.isfinite(got[0]).any() and np.isnan(got[0, 3]).all()
    assert np.array_equal(got[0, 0], (z[0, 0] - z_prev[0, 1]) / 0.04)   # the first match of a repeated id
    t = lambda a: torch.tensor(a, device="cuda:0")
    gd = v.pixel_flow(g, t(z_prev), t(ids_prev), t(z), t(ids), t(dt))
    g.sync()
    assert np.array_equal(gd.cpu().numpy(), want, equal_nan=True)
    L, p = capi.lib(), (lambda a: C.c_void_p(a.ctypes.data))
    out = np.zeros((3, M, 2))
    args = [p(z_prev), p(ids_prev), p(z), p(ids), p(dt), p(out)]
    for k in range(6):
        a = list(args)
        a[k] = None
        assert L.viekf_pixel_flow(g._h, Mp, a[0], a[1], M, a[2], a[3], a[4], a[5], capi.HOST) == capi.ERR_INVALID
    assert L.viekf_pixel_flow(g._h, 0, *args[:2], M, *args[2:], capi.HOST) == capi.ERR_INVALID
    assert L.viekf_pixel_flow(g._h, Mp, *args[:2], 4097, *args[2:], capi.HOST) == capi.ERR_INVALID
    assert not out.any()


def test_refusals():
    """VIEKF_ERR_INVALID, and nothing changed: M = 0 and above the bound, NULL slot / z / gyro / R, r_mode 3, order 2, a gyro_var
    that is negative or NaN; viekf_batch_update, viekf_batch_eval_h and viekf_batch_eval_h_jacobian keep refusing the type"""
    c = pc.case("once", 3, 0)
    g = make_gpu(c)
    L = capi.lib()
    x0, P0 = g.get_state(), g.get_covariance()
    big = capi.PIXVELS_MAX_M + 1
    z, slot, R, gyro = np.full((B, big, 2), 3.0), np.zeros((B, big), dtype=np.int32), np.tile(np.eye(2) * 100.0, (B, big, 1, 1)), np.zeros((B, 3))
    res, route = np.zeros((B, big), dtype=np.int32), C.c_int32(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def go(M, ps=p(slot), pz=p(z), pg=p(gyro), pR=p(R), r_mode=2, order=0, gv=0.0, where=capi.HOST):
        return L.viekf_batch_update_pixel_vels(g._h, M, ps, pz, pg, pR, r_mode, gv, None, order, p(res), C.byref(route), where)

    for M in (0, -1, big):
        assert go(M) == capi.ERR_INVALID, M
    assert go(3, ps=None) == capi.ERR_INVALID and go(3, pz=None) == capi.ERR_INVALID and go(3, pg=None) == capi.ERR_INVALID
    assert go(3, pR=None) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
    assert go(3, r_mode=3) == capi.ERR_INVALID and go(3, r_mode=-1) == capi.ERR_INVALID and go(3, order=2) == capi.ERR_INVALID
    assert go(3, gv=-1e-9) == capi.ERR_INVALID and go(3, gv=float("nan")) == capi.ERR_INVALID and go(3, gv=float("inf")) == capi.ERR_INVALID
    assert go(3, where=7) == capi.ERR_INVALID
    assert L.viekf_batch_pixel_vels_route(g._h, 2) == capi.ERR_INVALID and L.viekf_batch_pixel_vels_route(None, 0) == capi.ERR_INVALID
    assert L.viekf_batch_update_pixel_vels(None, 3, p(slot), p(z), p(gyro), p(R), 2, 0.0, None, 0, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_batch_eval_pixel_vel(g._h, None, p(gyro), p(z), None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_batch_eval_pixel_vel(g._h, p(slot), None, p(z), None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_batch_eval_pixel_vel(g._h, p(slot), p(gyro), None, None, capi.HOST) == capi.ERR_INVALID
    assert route.value == -7 and not res.any()
    # the table's own entry points keep refusing the type
    zz, RR, rr = np.zeros((B, 2)), np.eye(2), np.zeros(B, np.int32)
    sl = np.zeros(B, np.int32)
    assert L.viekf_batch_update(g._h, 7, p(zz), 2, p(RR), 2, 0, p(sl), None, p(rr), capi.HOST) != capi.OK
    out4, outH, xx = np.zeros((B, 4)), np.zeros((B, 3, g.n)), g.get_state()
    assert L.viekf_batch_eval_h(g._h, 7, p(sl), p(out4), capi.HOST) == capi.ERR_INVALID
    assert L.viekf_batch_eval_h_jacobian(g._h, p(xx), 7, p(sl), p(out4), p(outH), capi.HOST) == capi.ERR_INVALID
    assert np.array_equal(g.get_state(), x0) and np.array_equal(g.get_covariance(), P0) and not g.get_status().any()
    res2, r2 = call(g, c)                                               # and the handle still works
    check(g, c, res2, r2, c["name"] + " after the refusals")
    # the largest M is taken: entries past the case's own sit out (active 2)
    h = make_gpu(c)
    reps = -(-capi.PIXVELS_MAX_M // 3)
    sl = np.ascontiguousarray(np.tile(c["slot"], (1, reps))[:, :capi.PIXVELS_MAX_M])
    zz = np.ascontiguousarray(np.tile(c["z"], (1, reps, 1))[:, :capi.PIXVELS_MAX_M])
    a2 = np.full(sl.shape, 2, dtype=np.uint8)
    a2[:, :3] = 1
    res3, r3 = h.update_pixel_vels(zz, sl, c["gyro"], c["R"], c["gyro_var"], a2, 0)
    assert r3 == 1 and np.array_equal(res3[:, :3], c["codes"]) and (res3[:, 3:] == -1).all()
    assert np.array_equal(h.get_state(), g.get_state()) and np.array_equal(h.get_covariance(), g.get_covariance())
