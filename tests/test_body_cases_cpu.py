"""CPU checks of the fused body-sensor update's cases (tests/body_cases.py) before anything runs on a GPU:

  * the identity k_update_body_n rests on, restated in numpy: the chain of M updates run on the 16-column panel of P alone
    (with D for the rho diagonals), and ONE deferred trailing application of the applied entries' rank-r downdates to the
    rest of the lower triangle, give what the oracle's M sequential updates give -- x, P and codes, for every case, within
    tests.test_gpu_parity.assert_close (1e-9 of max |ref|, 1e-6 element-wise);
  * the condition on the inputs: every entry's Mahalanobis distance in the oracle's run is below 4 or above 25 (the gate is
    at 9), so a last-bit difference cannot flip a verdict;
  * coverage: the cases reach what they are there for."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import body_cases as bc
from tests import meas_cases as mc
from tests.test_gpu_parity import assert_close

B = bc.B


def _fix_depth(x, D, ln, reset, p0rr):
    """fix_depth_rule on the state x with P(rho, rho) in D -> status bits"""
    flag = 0
    for f in range(ln):
        k = 17 + 5 * f + 4
        if np.isnan(x[k]):
            x[k] = reset
            flag |= bc.NAN_BIT
        if x[k] < 0.0:
            D[f] += (reset - x[k]) ** 2
            x[k] = reset
            flag |= bc.NEG_DEPTH_BIT
        elif x[k] > 1e2:
            D[f] = p0rr
            x[k] = reset
    return flag


def panel_chain(c, b):
    """filter b of case c the kernel's way -> x, P (the active block mirrored from its lower triangle), codes, status bits,
    the number of applied entries and of fix_depth edits"""
    prm = c["params"]
    f = orc.OracleFilter(c["N"]).init(**{k: prm[k] for k in mc.ORACLE_KEYS})      # for h() and boxplus() at a given x
    for i in range(int(c["len"][b])):
        f.init_feature(np.array([300.0, 200.0]), i)
    x, P = c["x0"][b].copy(), c["P0"][b].copy()
    ln = int(c["len"][b])
    nact, n = 16 + 3 * ln, P.shape[0]
    lam = c["lam"] if c["partial"] else np.ones(n)
    L = (lam[:, None] + lam[None, :] - lam[:, None] * lam[None, :])[:nact, :nact]
    low = np.tril(P[:nact, :nact])
    sym = low + np.tril(low, -1).T                                   # what the lower triangle says, read either way
    C = sym[:, :16].copy()                                           # the panel
    rho = 18 + 3 * np.arange(ln)
    D = sym[rho, rho].copy()
    reset, p0rr = 1.0 / (2.0 * prm["min_depth"]), prm["P0_feat"][2]
    codes, applied, flag, fixes = [], [], 0, 0
    hi, lo = np.maximum.outer(np.arange(nact), np.arange(16)), np.minimum.outer(np.arange(nact), np.arange(16))
    for m, (mtype, z, R) in enumerate(c["entries"]):
        act = 1 if c["active"] is None else int(c["active"][m, b])
        z = z[b]
        R = R[b] if R.ndim == 3 else R
        if act == 2:
            codes.append(-1)
            continue
        if np.isnan(z).any():
            codes.append(orc.MEAS_NAN)
            continue
        before = x.copy()
        if act == 0:
            flag |= _fix_depth(x, D, ln, reset, p0rr)
            fixes += int((x != before).sum())
            codes.append(0)
            continue
        r = R.shape[0]
        h, H = f.h(mtype, x)
        assert not H[:r, 16:].any(), "a body model with a non-zero column outside the body block"
        Hb = H[:r, :16]
        res = bc.residual(mtype, z, h)[:r]
        W = C @ Hb.T                                                 # from the panel alone
        Si = np.linalg.inv(Hb @ W[:16] + R)
        if res @ Si @ res > 9.0:
            codes.append(orc.MEAS_GATED)                             # no fix_depth
            continue
        K = W @ Si
        if not (np.isnan(K).any() or np.isnan(Hb).any()):
            dx = np.zeros(n)
            dx[:nact] = lam[:nact] * (K @ res)
            x = f.boxplus(x, dx)
            T = np.einsum("icq,icq->ic", K[hi], W[lo])
            C -= L[:, :16] * T
            D -= L[rho, rho] * np.einsum("fq,fq->f", K[rho], W[rho])
            applied.append((K, W))
        before = x.copy()
        flag |= _fix_depth(x, D, ln, reset, p0rr)
        fixes += int((x != before).sum())
        if np.isnan(x[:17 + 5 * ln]).any():
            flag |= bc.NAN_BIT
        codes.append(0)
    # ONE trailing application to the rest of the lower triangle, in entry order
    T = sym.copy()
    for K, W in applied:
        T -= L * (K @ W.T)
    T[:, :16] = C
    T[rho, rho] = D
    low = np.tril(T)
    Pn = P.copy()
    Pn[:nact, :nact] = low + np.tril(low, -1).T
    return x, Pn, codes, flag, len(applied), fixes


def fallback_n(limit):
    """the smallest N whose LDS layout at M = 8 exceeds `limit` bytes (the layout function itself: it needs no device)"""
    from vi_ekf_amd import capi
    L = capi.lib()
    return next(N for N in range(1, 4097) if L.viekf_body_lds_bytes(N, capi.BODY_MAX_M) > limit)


# (the GPU test takes the fallback size from the device; a workgroup of the MI355X has 160 KiB)
CASES = bc.all_cases() + [("m8", fallback_n(160 * 1024), 0), ("m8", fallback_n(160 * 1024) - 1, 0)]


def test_the_layout_function():
    from vi_ekf_amd import capi
    L = capi.lib()
    for N, M in ((0, 1), (1, 2), (50, 2), (50, 8), (160, 4)):
        n, nxs = 16 + 3 * N, (17 + 5 * N + 1) & ~1
        assert L.viekf_body_lds_bytes(N, M) == 8 * (nxs + 18 * n + N + 6 * n * M + 64)
    assert L.viekf_body_lds_bytes(50, 0) == 0 and L.viekf_body_lds_bytes(50, 9) == 0 and L.viekf_body_lds_bytes(-1, 1) == 0
    assert L.viekf_body_lds_bytes(50, 8) <= 160 * 1024 < L.viekf_body_lds_bytes(fallback_n(160 * 1024), 8)
    assert fallback_n(160 * 1024) == 95


@pytest.mark.parametrize("name,N,variant", CASES)
def test_panel_chain_and_one_trailing_pass_equal_sequential_updates(name, N, variant):
    c = bc.case(name, N, variant)
    for b in range(B):
        x, P, codes, flag, napp, fixes = panel_chain(c, b)
        assert codes == list(c["codes"][:, b]), (c["name"], b, codes, c["codes"][:, b])
        assert_close(*mc.nan_split(x, c["x_ref"][b]), "x of filter %d, %s" % (b, c["name"]))
        assert_close(*mc.nan_split(P, c["P_ref"][b]), "P of filter %d, %s" % (b, c["name"]))
        if b in c["untouched"]:
            assert np.array_equal(c["x_ref"][b], c["x0"][b]) and np.array_equal(c["P_ref"][b], c["P0"][b], equal_nan=True)


@pytest.mark.parametrize("name,N,variant", CASES + [("steps", 50, 0)])
def test_no_entry_is_near_the_gate(name, N, variant):
    c = bc.steps_case() if name == "steps" else bc.case(name, N, variant)
    mah = c["mahal"][~np.isnan(c["mahal"])]
    print("%s: Mahalanobis distances up to %.3g below the gate, from %.3g above it" %
          (name, mah[mah < 9].max(initial=0.0), mah[mah > 9].min(initial=np.inf)))
    assert mah.size and ((mah < 4.0) | (mah > 25.0)).all(), mah
    gated = c["codes"] == orc.MEAS_GATED
    assert ((c["mahal"] > 25.0) == gated).all()


def test_the_cases_reach_what_they_are_for():
    for N in bc.SIZES:
        c = bc.case("mixed", N)
        codes = c["codes"]
        assert (codes[bc.MIXED_GATED][[0, 1, 3, 4]] == orc.MEAS_GATED).all()            # gated in the middle ...
        assert (codes[bc.MIXED_GATED + 1:, [0, 3, 4]] == 0).all()                       # ... accepted entries after it
        assert list(c["active"][bc.MIXED_ACTIVE_ROW]) == [1, 0, 2, 1, 0]                # an inactive and a skipped entry
        assert codes[bc.MIXED_ACTIVE_ROW, 2] == -1 and (codes[:, bc.MIXED_SKIPPED_FILTER] == -1).all()
        assert codes[bc.MIXED_NAN, bc.MIXED_NAN_FILTER] == orc.MEAS_NAN and codes[bc.MIXED_NAN + 1, bc.MIXED_NAN_FILTER] == 0
        assert c["untouched"] == [bc.MIXED_SKIPPED_FILTER]
        for b in (0, 3):                                                                 # the accepted ones really are applied
            assert panel_chain(c, b)[4] == len(bc.MIXED) - 1
        assert panel_chain(c, 4)[4] == len(bc.MIXED) - 2                                 # (inactive, gated)
        assert panel_chain(c, 1)[4] == len(bc.MIXED) - 3                                 # (inactive, gated, NaN)
    for N in (5, 50):                                                                    # the NaN-in-K skip
        c = bc.case("poison", N)
        assert (c["codes"] == 0).all()
        x, P, codes, flag, napp, fixes = panel_chain(c, bc.POISONED)
        assert napp == 0 and np.array_equal(x, c["x0"][bc.POISONED])
        assert np.array_equal(c["x_ref"][bc.POISONED], c["x0"][bc.POISONED])            # the oracle skipped them too
        assert np.array_equal(c["P_ref"][bc.POISONED], c["P0"][bc.POISONED], equal_nan=True)
        assert panel_chain(c, 0)[4] == len(bc.POISON_TYPES)
    for N in (5, 17):                                                                    # fix_depth inside the chain
        c = bc.case("fix", N)
        assert (c["codes"] == 0).all() and c["active"][0, 0] == 0
        reset, p0rr = 1.0 / (2.0 * c["params"]["min_depth"]), c["params"]["P0_feat"][2]
        # rho < 0 in an inactive entry (filter 0) and after an accepted one (filter 4); rho > 1e2 likewise (filters 0 and 1)
        for b, feat, neg in ((0, 0, True), (0, 1, False), (1, 1, False), (4, 2, True)):
            k, d = 17 + 5 * feat + 4, 18 + 3 * feat
            assert c["x0"][b, k] == (-0.3 if neg else 250.0)
            # the edit of P(rho, rho) is there, and the entries after it subtracted from the edited value
            first = c["P0"][b, d, d] + (reset + 0.3) ** 2 if neg else p0rr
            # (filter 4's accepted entry moved rho a little before fix_depth saw it: close to, not below, this figure)
            got = c["P_ref"][b, d, d]
            assert got != first and abs(got - first) < 1e-3 * first and (got < first or b == 4), (b, feat, got, first)
            assert abs(c["x_ref"][b, k] - reset) < 0.2
        for b in (0, 1, 4):
            x, P, codes, flag, napp, fixes = panel_chain(c, b)
            assert fixes >= 1 and napp >= len(bc.FIX_TYPES) - 1                          # at least one MORE accepted entry after it
            assert bool(flag & bc.NEG_DEPTH_BIT) == (b in (0, 4))
    for N in bc.SIZES:                                                                   # every model, both ACC forms
        assert [e[0] for e in bc.case("all5", N, 0)["entries"]] == list(bc.BODY)
        assert bc.case("all5", N, 0)["entries"][0][1].shape == (B, 2) and bc.case("all5", N, 1)["entries"][0][1].shape == (B, 3)
        assert bc.case("all5", N, 0)["entries"][0][2].shape == (B, 2, 2) and bc.case("all5", N, 1)["entries"][0][2].shape == (3, 3)
        assert list(bc.case("all5", N, 0)["len"]) == bc.fill(N)
