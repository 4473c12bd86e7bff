"""BatchVIEKF.update_body (viekf_batch_update_body, k_update_body_n: the body-sensor updates of one tick in one pass over P)
against the CPU oracle applying the entries one by one, and where noted against a second batch driven by M
viekf_batch_update calls.  Result codes and status bits are compared exactly, x and P with assert_close of
tests/test_gpu_parity.py.  The cases, the reasons for their inputs and the start states are in tests/body_cases.py;
tests/test_body_cases_cpu.py checks on the CPU that no entry is near the gate, that the cases reach what they are for, and
the identity the kernel rests on.

Sizes: N = 1, 5 (n = 31: odd, one pad row), 16 / 17 (nact = 64 / 67: the wave boundary of the column walk), 50 (n = ld = 166),
B = 5 with the ragged fill [N, N - 3, 1, 0, N - 1] clipped at 0 (the empty filter's panel is all of its P)."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from tests import body_cases as bc
from tests import meas_cases as mc
from tests.test_gpu_parity import assert_close
from vi_ekf_amd import capi

pytestmark = pytest.mark.gpu

B = bc.B


def start_P(c):
    """The case's start covariance as the device gets it: the oracle's lower triangle, mirrored.  (The oracle's own P is
    symmetric to rounding only; the library keeps P exactly symmetric, and a launch that leaves the lower triangle has the
    upper one mirrored from it on the next read.)"""
    low = np.tril(c["P0"])
    return low + np.tril(low, -1).transpose(0, 2, 1)


def make_gpu(c, batch=B):
    """a batch at the case's start state (the oracle's own x, P and len, written with set_state); batch > 5: the case's five
    filters over and over"""
    idx = np.arange(batch) % B
    g = v.BatchVIEKF(batch, c["N"], c["params"])
    g.set_state(x=c["x0"][idx], P=start_P(c)[idx], len_features=c["len"][idx])
    return g


def run_generic(g, c):
    """the parent's route: one viekf_batch_update per entry"""
    return np.stack([g.update(mtype, z, R, None, None if c["active"] is None else c["active"][m])
                     for m, (mtype, z, R) in enumerate(c["entries"])])


def check_against_oracle(g, c, res, what):
    assert np.array_equal(res, c["codes"]), (what, res, c["codes"])
    x, P = g.get_state(), g.get_covariance()
    assert_close(*mc.nan_split(x, c["x_ref"]), "x after " + what)
    assert_close(*mc.nan_split(P, c["P_ref"]), "P after " + what)
    assert np.array_equal(P, P.transpose(0, 2, 1), equal_nan=True), "P != P^T after " + what
    for b in c["untouched"]:
        assert np.array_equal(x[b], c["x0"][b]) and np.array_equal(P[b], start_P(c)[b], equal_nan=True), "filter %d touched by %s" % (b, what)
    return x, P


def check_against_generic(g, c, res, x, P, what):
    """a second batch through M viekf_batch_update calls: same codes and status bits, x and P to assert_close"""
    h = make_gpu(c)
    assert np.array_equal(run_generic(h, c), res), what
    assert np.array_equal(h.get_status(), g.get_status()), (what, h.get_status(), g.get_status())
    xh, Ph = h.get_state(), h.get_covariance()
    print("%s: fused == generic bit for bit: x %s, P %s" % (what, np.array_equal(x, xh, equal_nan=True), np.array_equal(P, Ph, equal_nan=True)))
    assert_close(*mc.nan_split(x, xh), "x against the M-call route, " + what)
    assert_close(*mc.nan_split(P, Ph), "P against the M-call route, " + what)


@pytest.mark.parametrize("N,variant", [(N, vv) for N in bc.SIZES for vv in (0, 1)] + [(5, 2), (5, 3)])
def test_all_five_models_in_one_call(N, variant):
    """ACC, ALT, ATT, POS and VEL in one call: drag 1 / partial 1 (ACC 2-D) and drag 0 / partial 0 (ACC 3-D), a per-filter
    non-diagonal R (r_mode 1) and a shared one"""
    c = bc.case("all5", N, variant)
    g = make_gpu(c)
    res, route = g.update_body(c["entries"])
    assert route == 1
    check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()


@pytest.mark.parametrize("variant", range(len(bc.BODY)))
def test_one_entry_of_each_model_against_update(variant):
    c = bc.case("single", 5, variant)
    g = make_gpu(c)
    res, route = g.update_body(c["entries"])
    assert route == 1 and res.shape == (1, B)
    x, P = check_against_oracle(g, c, res, c["name"])
    check_against_generic(g, c, res, x, P, c["name"])


@pytest.mark.parametrize("N", bc.SIZES)
def test_mixed_script(N):
    """M = 6 in one call: an active row [1, 0, 2, 1, 0], POS 50 m off (gated) in the middle, a NaN in one filter's VEL, and a
    filter that sits the whole call out -- bit for bit untouched"""
    c = bc.case("mixed", N)
    g = make_gpu(c)
    res, route = g.update_body(c["entries"], c["active"])
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    assert not g.get_status().any()
    check_against_generic(g, c, res, x, P, c["name"])
    # a call all of whose entries are gated leaves EVERY filter bit for bit as it is
    mtype, z, R = c["entries"][bc.MIXED_GATED]
    res, route = g.update_body([(mtype, z + 100.0, R)])
    assert route == 1 and (res == orc.MEAS_GATED).all()
    assert np.array_equal(g.get_state(), x) and np.array_equal(g.get_covariance(), P)


@pytest.mark.parametrize("N", [5, 17])
def test_fix_depth_inside_the_chain(N):
    """rho < 0 and rho > 1e2 met by an inactive entry and after an accepted one, more accepted entries behind them: the two
    edits of P(rho, rho) land where later entries subtract from them, the negative-depth bit where it belongs"""
    c = bc.case("fix", N)
    g = make_gpu(c)
    res, route = g.update_body(c["entries"], c["active"])
    assert route == 1
    x, P = check_against_oracle(g, c, res, c["name"])
    st = g.get_status()
    assert list((st & bc.NEG_DEPTH_BIT) != 0) == [True, False, False, False, True] and not (st & ~np.uint32(bc.NEG_DEPTH_BIT)).any(), st
    check_against_generic(g, c, res, x, P, c["name"])


@pytest.mark.parametrize("N", [5, 50])
def test_nan_in_a_body_row_of_P(N):
    """P[2, 7] = NaN in one filter: its gain has a NaN in every entry, the updates are skipped (vi_ekf_meas.cpp:247), the codes
    are 0, the NaN bit is on it and nowhere else"""
    c = bc.case("poison", N)
    g = make_gpu(c)
    res, route = g.update_body(c["entries"])
    assert route == 1 and (res == 0).all()
    x, P = check_against_oracle(g, c, res, c["name"])
    assert np.array_equal(x[bc.POISONED], c["x0"][bc.POISONED]) and np.array_equal(P[bc.POISONED], start_P(c)[bc.POISONED], equal_nan=True)
    st = g.get_status()
    assert list((st & bc.NAN_BIT) != 0) == [b == bc.POISONED for b in range(B)] and not (st & ~np.uint32(bc.NAN_BIT)).any(), st
    check_against_generic(g, c, res, x, P, c["name"])


def test_between_two_resident_steps():
    """N = 50, 48 features tracked: step, step, update_body([ACC, ATT]) on the PACKED P the steps leave, step.  One fused
    launch; the covariance read afterwards is exactly symmetric; rows and columns past the active block are bit for bit what
    the oracle still has there (what the filter was created with)"""
    c = bc.steps_case()
    sc, N, nfeat = c["sc"], c["N"], c["nfeat"]
    g = v.BatchVIEKF(B, N, sc["params"])
    for i in range(nfeat):
        assert (g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan)) == 1).all()
    for s in range(2):
        assert np.array_equal(g.step(sc["u"][s], sc["dt"], c["z"][s], c["slot"], sc["R"]), c["step_codes"][s])
    assert "P packed" in g.describe(), g.describe()
    res, route = g.update_body(c["entries"])
    assert route == 1 and np.array_equal(res, c["codes"])
    assert np.array_equal(g.step(sc["u"][2], sc["dt"], c["z"][2], c["slot"], sc["R"]), c["step_codes"][2])
    x, P = g.get_state(), g.get_covariance()
    assert_close(x, c["x_ref"], "x after step, update_body, step")
    assert_close(P, c["P_ref"], "P after step, update_body, step")
    assert np.array_equal(P, P.transpose(0, 2, 1))
    na = 16 + 3 * nfeat
    assert (P[:, na:, :] == c["P_ref"][:, na:, :]).all() and (P[:, :, na:] == c["P_ref"][:, :, na:]).all()
    assert not g.get_status().any()


def test_per_filter_live_ring_slots():
    """a.si(b) != b: every filter's live state in a ring slot of its own (slots [0, 2, 1, 0, 2] of a ring of 3); against the
    oracle, and bit for bit against a batch that runs the call in its own buffers"""
    c = bc.case("mixed", 5)
    ga, gb = make_gpu(c), make_gpu(c)
    slots = np.array([0, 2, 1, 0, 2], dtype=np.int32)
    ga.history_resize(3)
    capi.check(capi.lib().viekf_batch_snapshot_filters(ga._h, C.c_void_p(slots.ctypes.data), capi.HOST))
    ga.select_filters(slots)
    ra, route = ga.update_body(c["entries"], c["active"])
    assert route == 1
    rb, _ = gb.update_body(c["entries"], c["active"])
    x, P = check_against_oracle(ga, c, ra, c["name"] + ", live slots")
    assert np.array_equal(ra, rb) and np.array_equal(x, gb.get_state()) and np.array_equal(P, gb.get_covariance())
    assert np.array_equal(ga.get_status(), gb.get_status())


def test_more_workgroups_than_compute_units():
    """B = 257, N = 5, M = 2 (the IMU tick): the five filters of the case over and over; filters 0, 1, 255 and 256 (and the
    rest) against the oracle's"""
    c = bc.case("m2", 5)
    nb = 257
    idx = np.arange(nb) % B
    g = make_gpu(c, nb)
    entries = [(mtype, z[idx], R) for mtype, z, R in c["entries"]]
    res, route = g.update_body(entries)
    assert route == 1 and np.array_equal(res, c["codes"][:, idx])
    x, P = g.get_state(), g.get_covariance()
    for k in (0, 1, 255, 256):
        assert_close(x[k], c["x_ref"][k % B], "x of filter %d" % k)
        assert_close(P[k], c["P_ref"][k % B], "P of filter %d" % k)
    assert np.array_equal(x, x[idx]) and np.array_equal(P, P[idx])       # (every copy of a filter came out the same)
    assert not g.get_status().any()


def test_fallback_where_the_lds_layout_does_not_fit():
    """the smallest N whose BodyLds at M = 8 exceeds what the device gives one workgroup: route 0 (M launches of the generic
    kernel issued by the entry point), same parity; one feature fewer: route 1"""
    L = capi.lib()
    limit = C.c_int64(0)
    capi.check(L.viekf_body_lds_limit(0, C.byref(limit)))
    nfb = next(N for N in range(1, 4097) if L.viekf_body_lds_bytes(N, capi.BODY_MAX_M) > limit.value)
    print("LDS per workgroup %d bytes: M = 8 falls back from N = %d (%d bytes)" % (limit.value, nfb, L.viekf_body_lds_bytes(nfb, 8)))
    assert 50 < nfb <= 160, "the headline size must fuse and the fallback must be reachable within the ABI's sizes"
    for N, want in ((nfb, 0), (nfb - 1, 1)):
        c = bc.case("m8", N)
        mah = c["mahal"][~np.isnan(c["mahal"])]
        assert ((mah < 4.0) | (mah > 25.0)).all()      # (the CPU test has checked this at the sizes a 160 KiB device gives)
        g = make_gpu(c)
        res, route = g.update_body(c["entries"])
        assert route == want, (N, route)
        check_against_oracle(g, c, res, c["name"])
        assert not g.get_status().any()


def test_device_pointers():
    """the same call with device pointers (z [M][B][4], R [M][B][9], result on the device): bit for bit the host call"""
    torch = pytest.importorskip("torch")
    c = bc.case("all5", 5, 0)
    g, h = make_gpu(c), make_gpu(c)
    h.use_torch_stream()
    res, route = g.update_body(c["entries"])
    M = len(c["entries"])
    z, R = np.zeros((M, B, 4)), np.zeros((M, B, 9))
    for m, (mtype, zm, Rm) in enumerate(c["entries"]):
        r = Rm.shape[-1]
        z[m, :, :zm.shape[1]] = zm
        R[m, :, :r * r] = Rm.transpose(0, 2, 1).reshape(B, r * r)
    dev = torch.device("cuda:0")
    types = [e[0] for e in c["entries"]]
    rd, route_d = h.update_body((types, [e[1].shape[1] for e in c["entries"]], [e[2].shape[-1] for e in c["entries"]],
                                 torch.tensor(z, device=dev), torch.tensor(R, device=dev)))
    torch.cuda.synchronize()
    assert route_d == route == 1 and np.array_equal(rd.cpu().numpy(), res)
    assert np.array_equal(g.get_state(), h.get_state()) and np.array_equal(g.get_covariance(), h.get_covariance())


def test_refusals():
    """VIEKF_ERR_INVALID, and nothing changed: a feature model, M outside 1 .. 8, a zdim / rdim viekf_batch_update would
    refuse, NULL z or R"""
    c = bc.case("m2", 5)
    g = make_gpu(c)
    L = capi.lib()
    x0, P0 = g.get_state(), g.get_covariance()
    z, R, res, route = np.zeros((9, B, 4)), np.tile(np.eye(3).ravel(), (9, 1)), np.zeros((9, B), dtype=np.int32), C.c_int32(-7)
    p = lambda a: C.c_void_p(a.ctypes.data)
    i32 = lambda *vals: np.array(vals, dtype=np.int32)

    def call(M, types, zdim, rdim, pz=p(z), pR=p(R)):
        return L.viekf_batch_update_body(g._h, M, p(types), p(zdim), p(rdim), pz, pR, 0, None, p(res), C.byref(route), capi.HOST)

    for mtype in (orc.QZETA, orc.FEAT, orc.DEPTH, orc.INV_DEPTH, 7, -1, 10):
        assert call(1, i32(mtype), i32(2), i32(2)) == capi.ERR_INVALID, mtype
    nine = i32(*([orc.POS] * 9))
    three = i32(*([3] * 9))
    assert call(0, nine, three, three) == capi.ERR_INVALID and call(9, nine, three, three) == capi.ERR_INVALID
    assert call(-1, nine, three, three) == capi.ERR_INVALID
    for zd, rd in ((0, 3), (5, 3), (3, 0), (3, 4)):
        assert call(2, i32(orc.POS, orc.POS), i32(3, zd), i32(3, rd)) == capi.ERR_INVALID, (zd, rd)
    assert call(1, i32(orc.POS), i32(3), i32(3), pz=None) == capi.ERR_INVALID
    assert call(1, i32(orc.POS), i32(3), i32(3), pR=None) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
    assert L.viekf_batch_update_body(None, 1, p(i32(orc.POS)), p(i32(3)), p(i32(3)), p(z), p(R), 0, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert route.value == -7
    assert np.array_equal(g.get_state(), x0) and np.array_equal(g.get_covariance(), P0) and not g.get_status().any()
    # and the handle still works
    res2, r2 = g.update_body(c["entries"])
    assert r2 == 1
    check_against_oracle(g, c, res2, c["name"] + " after the refusals")
