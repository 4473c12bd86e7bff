"""BatchVIEKF.update_depths (viekf_batch_update_depths, k_update_depths: a frame's DEPTH updates in one pass over P) against
the CPU oracle applying the entries one by one, and against a second batch driven by M viekf_batch_update calls.  Result
codes and status bits are compared exactly, x and P with assert_close of tests/test_gpu_parity.py, and P == P^T is checked.
The cases, the reasons for their inputs and the start states are in tests/depth_cases.py; tests/test_depth_cases_cpu.py
checks on the CPU that no entry is near the gate, that the cases reach what they are for, and the identity the kernel rests
on.

Sizes: N = 1, 5 (n = 31: odd, one pad row), 16 / 17 (nact = 64 / 67: a wave boundary), 50 (n = ld = 166), B = 5 with the
ragged fill [N, N - 3, 1, 0, N - 1] clipped at 0.

A filter with a NaN in P is held to the M-call route alone (tests/test_depth_cases_cpu.py says why the oracle is no reference
there)."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from tests import depth_cases as dc
from tests import meas_cases as mc
from tests.test_gpu_parity import assert_close
from vi_ekf_amd import capi

pytestmark = pytest.mark.gpu

B = dc.B


def make_gpu(c, batch=B):
    """a batch at the case's start state (the oracle's own x, P and len, written with set_state); batch > 5: the case's five
    filters over and over"""
    idx = np.arange(batch) % B
    g = v.BatchVIEKF(batch, c["N"], c["params"])
    g.set_state(x=c["x0"][idx], P=dc.start_P(c)[idx], len_features=c["len"][idx])
    return g


def call(g, c, z=None):
    return g.update_depths(c["mtype"], c["z"] if z is None else z, c["slot"], c["R"], c["active"], c["order"])


def run_generic(g, c, z=None):
    """the parent's route: one viekf_batch_update per entry, in the call's order"""
    z = c["z"] if z is None else z
    M = c["slot"].shape[1]
    res = np.zeros((B, M), dtype=np.int32)
    for e in range(M):
        m = M - 1 - e if c["order"] else e
        R = np.array([[[dc.r_at(c["R"], b, m)]] for b in range(B)])
        res[:, m] = g.update(c["mtype"], z[:, m:m + 1], R, c["slot"][:, m], None if c["active"] is None else c["active"][:, m])
    return res


def check_against_oracle(g, c, res, what, skip=()):
    assert np.array_equal(res, c["codes"]), (what, res, c["codes"])
    x, P = g.get_state(), g.get_covariance()
    keep = [b for b in range(B) if b not in skip]
    assert_close(*mc.nan_split(x[keep], c["x_ref"][keep]), "x after " + what)
    assert_close(*mc.nan_split(P[keep], c["P_ref"][keep]), "P after " + what)
    assert np.array_equal(P, P.transpose(0, 2, 1), equal_nan=True), "P != P^T after " + what
    for b in c["untouched"]:
        assert np.array_equal(x[b], c["x0"][b]) and np.array_equal(P[b], dc.start_P(c)[b], equal_nan=True), "filter %d touched by %s" % (b, what)
    return x, P


def check_against_generic(g, c, res, x, P, what):
    """a second batch through M viekf_batch_update calls: same codes and status bits, x and P to assert_close"""
    h = make_gpu(c)
    assert np.array_equal(run_generic(h, c), res), what
    assert np.array_equal(h.get_status(), g.get_status()), (what, h.get_status(), g.get_status())
    xh, Ph = h.get_state(), h.get_covariance()
    print("%s: fused == M calls bit for bit: x %s, P %s" % (what, np.array_equal(x, xh, equal_nan=True), np.array_equal(P, Ph, equal_nan=True)))
    assert_close(*mc.nan_split(x, xh), "x against the M-call route, " + what)
    assert_close(*mc.nan_split(P, Ph), "P against the M-call route, " + what)


@pytest.mark.parametrize("N,variant", [(N, vv) for N in dc.SIZES for vv in range(len(dc.ONCE_VARIANTS))])
def test_every_slot_once(N, variant):
    """M = N DEPTH entries, per-filter shuffled slots (slots >= len: INVALID; a -1: SKIPPED); partial update on and off, the
    three R modes, both orders"""
    c = dc.case("once", N, variant)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()
    check_against_generic(g, c, res, x, P, c["name"])


@pytest.mark.parametrize("N,order", [(5, 0), (5, 1), (17, 0), (17, 1)])
def test_every_slot_once_inv_depth(N, order):
    c = dc.case("once_inv", N, order)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()
    check_against_generic(g, c, res, x, P, c["name"])


@pytest.mark.parametrize("order", [0, 1])
def test_m_past_a_wave_and_past_n(order):
    """N = 17, M = 70: slots repeat, slot 2 three times with others between"""
    c = dc.case("repeat", dc.REPEAT_N, order)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()
    check_against_generic(g, c, res, x, P, c["name"])


@pytest.mark.parametrize("N", dc.MIXED_SIZES)
def test_mixed_script(N):
    """M = 8 in one call: active 0, 1 and 2 within one filter's row, a depth 40 m off (gated) in the middle with accepted
    entries after it, a NaN z, and a filter whose whole row is 2 -- bit for bit untouched.  Then a call all of whose entries
    are gated: every filter bit for bit as before"""
    c = dc.case("mixed", N, N % 2)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()
    check_against_generic(g, c, res, x, P, c["name"])
    z, codes, mah = dc.all_gated(c)
    assert (mah[codes == orc.MEAS_GATED] > 25.0).all()
    res, route = g.update_depths(c["mtype"], z, c["slot"], c["R"], None, c["order"])
    assert route == 1 and np.array_equal(res, codes) and (res == orc.MEAS_GATED).any()
    assert np.array_equal(g.get_state(), x) and np.array_equal(g.get_covariance(), P) and not g.get_status().any()


@pytest.mark.parametrize("N", [5, 17])
def test_fix_depth_inside_the_chain(N):
    """rho < 0 and rho > 1e2 prepared in x, met by an inactive entry and after an accepted one, entries on the edited
    diagonals behind them; an INV_DEPTH that drives rho negative, followed by another entry on the same slot; the
    negative-depth bit only where it belongs"""
    c = dc.case("fix", N)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    st = g.get_status()
    assert list((st & dc.NEG_DEPTH_BIT) != 0) == [b in dc.FIX_NEG_FILTERS for b in range(B)] and not (st & ~np.uint32(dc.NEG_DEPTH_BIT)).any(), st
    check_against_generic(g, c, res, x, P, c["name"])
    c = dc.case("neg", N)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    st = g.get_status()
    assert list((st & dc.NEG_DEPTH_BIT) != 0) == [b in dc.NEG_FILTERS for b in range(B)] and not (st & ~np.uint32(dc.NEG_DEPTH_BIT)).any(), st
    check_against_generic(g, c, res, x, P, c["name"])


@pytest.mark.parametrize("N", [5, 50])
def test_nan_in_p_that_one_column_meets(N):
    """P[7, rho column of slot 1] = NaN in one filter: that entry's gain has a NaN and its correction is skipped
    (vi_ekf_meas.cpp:247), the entries on other columns are applied, the codes are 0, the NaN bit is on that filter only"""
    c = dc.case("poison", N)
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == 1 and (res[dc.POISONED] == 0).all()
    x, P = check_against_oracle(g, c, res, c["name"], skip=(dc.POISONED,))
    b = dc.POISONED
    assert np.isnan(P[b]).sum() == 2 and not np.isnan(x).any() and not np.array_equal(x[b], c["x0"][b])     # others applied
    st = g.get_status()
    assert list((st & dc.NAN_BIT) != 0) == [k == b for k in range(B)] and not (st & ~np.uint32(dc.NAN_BIT)).any(), st
    check_against_generic(g, c, res, x, P, c["name"])
    # the entry that met the NaN left its own feature alone: bit for bit what a run without that entry gives
    act = np.ones(c["slot"].shape, dtype=np.uint8)
    act[b, list(c["slot"][b]).index(dc.POISON_SLOT)] = 2
    h = make_gpu(c)
    h.update_depths(c["mtype"], c["z"], c["slot"], c["R"], act, c["order"])
    assert np.array_equal(h.get_state()[b], x[b]) and np.array_equal(h.get_covariance()[b], P[b], equal_nan=True)


def _steps_batch(c):
    sc, N, nfeat = c["sc"], c["N"], c["nfeat"]
    g = v.BatchVIEKF(B, N, sc["params"])
    for i in range(nfeat):
        assert (g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan)) == 1).all()
    return g


def _two_steps(g, c):
    sc = c["sc"]
    for s in range(2):
        assert np.array_equal(g.step(sc["u"][s], sc["dt"], c["step_z"][s], c["step_slot"], sc["R"]), c["step_codes"][s])


def _check_steps(g, c, res, route):
    assert route == 1 and np.array_equal(res, c["codes"])
    x, P = g.get_state(), g.get_covariance()
    assert_close(x, c["x_ref"], "x after step, step, update_depths")
    assert_close(P, c["P_ref"], "P after step, step, update_depths")
    assert np.array_equal(P, P.transpose(0, 2, 1))
    na = 16 + 3 * c["nfeat"]
    assert (P[:, na:, :] == c["P_ref"][:, na:, :]).all() and (P[:, :, na:] == c["P_ref"][:, :, na:]).all()
    assert not g.get_status().any()


def test_behind_a_fused_step():
    """N = 50, 48 features tracked: step, step, then update_depths (M = 48, reverse order, R per entry) on the PACKED P the
    steps leave; rows and columns past the active block are bit for bit what the filter was created with"""
    c = dc.steps_case()
    g = _steps_batch(c)
    _two_steps(g, c)
    assert "P packed" in g.describe(), g.describe()
    res, route = g.update_depths(orc.DEPTH, c["z"], c["slot"], c["R"], None, 1)
    _check_steps(g, c, res, route)


def test_in_a_ring_slot():
    """the same run with the live state in slot 2 of a ring of 3 (viekf_batch_select)"""
    c = dc.steps_case()
    g = _steps_batch(c)
    g.history_resize(3)
    g.snapshot(2)
    capi.check(capi.lib().viekf_batch_select(g._h, 2))
    _two_steps(g, c)
    res, route = g.update_depths(orc.DEPTH, c["z"], c["slot"], c["R"], None, 1)
    _check_steps(g, c, res, route)
    capi.check(capi.lib().viekf_batch_select(g._h, -1))                 # the batch's own buffers were not written
    assert not np.array_equal(g.get_state(), c["x_ref"])


@pytest.mark.parametrize("which,want", [("largest that fits", 1), ("the next one", 0)])
def test_fallback_where_the_lds_layout_does_not_fit(which, want):
    """the largest N = M that viekf_depths_lds_bytes puts under what the device gives one workgroup, and the next one: routes 1
    and 0 (M launches of the generic kernel issued by the entry point), the same parity"""
    L = capi.lib()
    limit = C.c_int64(0)
    capi.check(L.viekf_body_lds_limit(0, C.byref(limit)))
    nfb = next(N for N in range(1, capi.DEPTHS_MAX_M + 1) if L.viekf_depths_lds_bytes(N, N) > limit.value)
    print("LDS per workgroup %d bytes: N = M falls back from %d (%d bytes)" % (limit.value, nfb, L.viekf_depths_lds_bytes(nfb, nfb)))
    assert 50 < nfb <= 128, "the headline size must fuse and the fallback must be reachable"
    N = nfb - 1 if want else nfb
    c = dc.case("once", N, 2)
    mah = c["mahal"][~np.isnan(c["mahal"])]
    assert (mah < 0.25).all()
    g = make_gpu(c)
    res, route = call(g, c)
    assert route == want, (N, route)
    check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()


def test_more_filters_than_resident_workgroups():
    """B = 600 (the five case filters repeated), N = M = 50: every copy is bit-equal to its first"""
    c = dc.case("once", 50, 1)
    nb = 600
    idx = np.arange(nb) % B
    g = make_gpu(c, nb)
    res, route = g.update_depths(c["mtype"], c["z"][idx], c["slot"][idx], c["R"][idx], None, c["order"])
    assert route == 1 and np.array_equal(res, c["codes"][idx])
    x, P = g.get_state(), g.get_covariance()
    assert np.array_equal(x, x[idx]) and np.array_equal(P, P[idx])
    assert_close(x[:B], c["x_ref"], "x of the first five")
    assert_close(P[:B], c["P_ref"], "P of the first five")
    assert not g.get_status().any()


def test_determinism_and_device_pointers():
    """the same call on two fresh batches gives bit-equal x, P and codes; so does the call with device pointers"""
    torch = pytest.importorskip("torch")
    c = dc.case("repeat", dc.REPEAT_N, 1)
    ga, gb, gd = make_gpu(c), make_gpu(c), make_gpu(c)
    ra, _ = call(ga, c)
    rb, _ = call(gb, c)
    dev = torch.device("cuda:0")
    gd.use_torch_stream()
    rd, route = gd.update_depths(c["mtype"], torch.tensor(c["z"], device=dev), torch.tensor(c["slot"], device=dev),
                                 torch.tensor(c["R"], device=dev), None, c["order"])
    torch.cuda.synchronize()
    assert route == 1 and np.array_equal(ra, rb) and np.array_equal(rd.cpu().numpy(), ra)
    xa, Pa = ga.get_state(), ga.get_covariance()
    for g in (gb, gd):
        assert np.array_equal(xa, g.get_state()) and np.array_equal(Pa, g.get_covariance())
        assert np.array_equal(ga.get_status(), g.get_status())


def test_refusals():
    """VIEKF_ERR_INVALID, and nothing changed: another model, M = 0 and above the bound, NULL z / slot / R, r_mode 3, order 2"""
    c = dc.case("once", 5, 0)
    g = make_gpu(c)
    L = capi.lib()
    x0, P0 = g.get_state(), g.get_covariance()
    big = capi.DEPTHS_MAX_M + 1
    z, slot, R = np.full((B, big), 3.0), np.zeros((B, big), dtype=np.int32), np.full((B, big), 0.01)
    res, route = np.zeros((B, big), dtype=np.int32), C.c_int32(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)

    def go(mtype, M, ps=p(slot), pz=p(z), pR=p(R), r_mode=2, order=0):
        return L.viekf_batch_update_depths(g._h, mtype, M, ps, pz, pR, r_mode, None, order, p(res), C.byref(route), capi.HOST)

    for mtype in (orc.ACC, orc.ALT, orc.ATT, orc.POS, orc.VEL, orc.QZETA, orc.FEAT, 7, -1, 10):
        assert go(mtype, 5) == capi.ERR_INVALID, mtype
    for M in (0, -1, big):
        assert go(orc.DEPTH, M) == capi.ERR_INVALID, M
    assert go(orc.DEPTH, 5, ps=None) == capi.ERR_INVALID and go(orc.DEPTH, 5, pz=None) == capi.ERR_INVALID
    assert go(orc.INV_DEPTH, 5, pR=None) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
    assert go(orc.DEPTH, 5, r_mode=3) == capi.ERR_INVALID and go(orc.DEPTH, 5, r_mode=-1) == capi.ERR_INVALID
    assert go(orc.DEPTH, 5, order=2) == capi.ERR_INVALID
    assert L.viekf_batch_update_depths(None, orc.DEPTH, 5, p(slot), p(z), p(R), 2, None, 0, None, None, capi.HOST) == capi.ERR_INVALID
    assert route.value == -7
    assert np.array_equal(g.get_state(), x0) and np.array_equal(g.get_covariance(), P0) and not g.get_status().any()
    res2, r2 = call(g, c)                                              # and the handle still works
    assert r2 == 1
    check_against_oracle(g, c, res2, c["name"] + " after the refusals")
    # the largest M is taken (N = 5: 256 entries fuse)
    c = dc.case("once", 5, 0)
    h = make_gpu(c)
    reps = -(-capi.DEPTHS_MAX_M // 5)
    sl = np.ascontiguousarray(np.tile(c["slot"], (1, reps))[:, :capi.DEPTHS_MAX_M])
    a2 = np.full(sl.shape, 2, dtype=np.uint8)
    a2[:, :5] = 1
    res3, r3 = h.update_depths(c["mtype"], np.ascontiguousarray(np.tile(c["z"], (1, reps))[:, :capi.DEPTHS_MAX_M]), sl, c["R"], a2, 0)
    assert r3 == 1 and np.array_equal(res3[:, :5], c["codes"]) and (res3[:, 5:] == -1).all()
    assert np.array_equal(h.get_state(), g.get_state()) and np.array_equal(h.get_covariance(), g.get_covariance())
