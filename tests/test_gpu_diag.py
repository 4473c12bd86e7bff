"""The consistency diagnostics (include/viekf_diag.h, vi_ekf_amd/diag.py) on the device against numpy on the x, P and len that
get_state returns, and against the CPU oracle's boxminus / h.  The states are made dense by fused steps, so P is full and
-- the diagnostics run BEFORE anything mirrors it -- stale above the diagonal.

Tolerances are derived, not measured.  Cholesky is backward stable, ||dA|| <= c m eps ||A||, so with kappa = kappa_2(A)
(numpy.linalg.eigvalsh on the reference side):
    NEES, whitened   |got - ref| <= max(1e-9, 64 m eps kappa) |ref|     (1e-9: the project's parity tolerance; whitened is
                     held to it against max|ref| of the filter, and element-wise on every entry above 1e-6 of that)
    logdet           |got - ref| <= 64 m^2 eps kappa
An indexing or triangle mistake shows as an error of order one."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from vi_ekf_amd import capi, diag, scene
from tests.test_gpu_parity import oracle_params

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
ACC, ALT, ATT, POS, VEL, QZETA, FEAT, DEPTH, INV_DEPTH = 0, 1, 2, 3, 4, 5, 6, 8, 9
BLOCKS = (3, 9, 16)


def make_batch(B, N, lens, steps=2, seed=0):
    """a batch with len_features = lens (ragged allowed) after `steps` fused steps -> (scene, batch, lens, slot)"""
    sc = scene.make_scene(B, N, steps + 2, seed=4000 + 17 * N + seed)
    lens = np.broadcast_to(np.asarray(lens, dtype=np.int32), (B,)).copy()
    g = v.BatchVIEKF(B, N, sc["params"])
    for i in range(int(lens.max())):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan), (lens > i).astype(np.uint8))
    slot = np.where(sc["slot"] < lens[:, None], sc["slot"], -1).astype(np.int32)
    for s in range(steps):
        g.step(sc["u"][s], sc["dt"], sc["z"][s], slot, sc["R"])
    assert (g.get_len_features() == lens).all()
    return sc, g, lens, slot


def oracle_like(sc, N, x, ln):
    """an oracle filter with `ln` active features (boxplus / boxminus / h loop over them), at the state x"""
    f = orc.OracleFilter(N).init(**oracle_params(sc["params"]))
    for i in range(int(ln)):
        f.init_feature(sc["pix"][0, i], i, float("nan"))
    f.x[:] = x
    return f


def perturbed_truth(sc, g, seed):
    """x_true = x [+] dx with dx about half a sigma of P: a healthy error, far from where boxminus is ill-conditioned"""
    r = np.random.default_rng(seed)
    x, P, ln = g.get_state(), g.get_covariance(), g.get_len_features()
    xt = x.copy()
    for b in range(g.B):
        m = 16 + 3 * ln[b]
        dx = np.zeros(g.n)
        dx[:m] = 0.5 * np.sqrt(np.diag(P[b])[:m]) * r.normal(size=m)
        xt[b] = oracle_like(sc, g.N, x[b], ln[b]).boxplus(x[b], dx)
    return xt


def reference(sc, g, x_true):
    """numpy on what get_state returns -> per filter dict(logdet, nees [4], whitened [n], kappa, m)"""
    x, P, ln = g.get_state(), g.get_covariance(), g.get_len_features()
    out = []
    for b in range(g.B):
        m = 16 + 3 * int(ln[b])
        A = P[b, :m, :m]
        w = np.linalg.eigvalsh(A)
        L = np.linalg.cholesky(A)
        e = oracle_like(sc, g.N, x[b], ln[b]).boxminus(x_true[b], x[b])[:m]
        y = np.linalg.solve(L, e)
        wh = np.zeros(g.n)
        wh[:m] = y
        out.append(dict(m=m, kappa=w[-1] / w[0], logdet=2.0 * np.log(np.diag(L)).sum(), whitened=wh,
                        nees=np.array([(y[:p] ** 2).sum() for p in BLOCKS + (m,)])))
    return out


def check_filter(got, b, ref, what):
    m, kappa = ref["m"], ref["kappa"]
    tol = max(1e-9, 64 * m * EPS * kappa)
    print("%s filter %d: m %d kappa %.3e  logdet err %.3e  nees rel err %.3e  whitened err %.3e (max|ref| %.3e)" % (
        what, b, m, kappa, abs(got["logdet"][b] - ref["logdet"]), np.abs(got["nees"][b] / ref["nees"] - 1).max(),
        np.abs(got["whitened"][b] - ref["whitened"]).max(), np.abs(ref["whitened"]).max()))
    assert got["info"][b] == 0, what
    assert abs(got["logdet"][b] - ref["logdet"]) <= 64 * m * m * EPS * kappa, what
    assert (np.abs(got["nees"][b] - ref["nees"]) <= tol * np.abs(ref["nees"])).all(), what
    dw, scale = np.abs(got["whitened"][b] - ref["whitened"]), np.abs(ref["whitened"]).max()
    assert dw.max() <= tol * scale, what
    big = np.abs(ref["whitened"]) > 1e-6 * scale
    assert (dw[big] <= tol * np.abs(ref["whitened"])[big]).all(), what
    assert (got["whitened"][b, m:] == 0.0).all(), what


def test_ragged_sizes_straddle_a_panel_edge():
    """N = 3, len_features 0..3: m = 16, 19, 22, 25 on both sides of the 16-wide panel"""
    sc, g, lens, _ = make_batch(4, 3, [0, 1, 2, 3], seed=1)
    xt = perturbed_truth(sc, g, 1)
    g.step(sc["u"][2], sc["dt"], sc["z"][2], np.full((4, 3), -1, np.int32), sc["R"])   # (a fused propagate: the upper triangle is stale again)
    got = diag.consistency(g, xt)
    ref = reference(sc, g, xt)
    assert [r["m"] for r in ref] == [16, 19, 22, 25]
    for b in range(4):
        check_filter(got, b, ref[b], "ragged")


@pytest.mark.parametrize("N", [12, 50, diag.ONCHIP_MAX_FEATURES, diag.ONCHIP_MAX_FEATURES + 1, 90])
def test_sizes_of_both_paths(N):
    """the headline's m = 166, the last N in LDS and the first in the workspace, and N = 90 with ld padded to 16"""
    sc, g, lens, slot = make_batch(2, N, N, steps=1, seed=2)
    xt = perturbed_truth(sc, g, N)
    g.step(sc["u"][1], sc["dt"], sc["z"][1], slot, sc["R"])
    # x_true belongs to the state before this step: the error is then simply larger, the reference takes the same pair
    got = diag.consistency(g, xt)
    ref = reference(sc, g, xt)
    for b in range(2):
        check_filter(got, b, ref[b], "N = %d" % N)


def test_round_trip_through_boxplus():
    """e = 1e-3 L zeta put in through viekf_batch_boxplus comes back as whitened = 1e-3 zeta and nees = the prefix sums of
    |1e-3 zeta|^2: no reference boxminus or solve involved.

    Body entries.  y[0:16] depends on e[0:16] only (L is lower triangular), and [+] / [-] on the body states are sums,
    differences and one quaternion exp / log: whitened[:, :16], element-wise, and nees[:, 0:3] are held to the module's bound
    max(1e-9, 64 m eps kappa_2(A)) |ref|.

    Feature entries and nees[3].  That bound cannot be met there, and not because of the factorisation: the reference's
    bearing [-] (q_feat_boxminus, math_helper.h:25-43) takes acos of a dot product within theta^2 / 2 of 1, so the angle
    theta_f a feature was moved by comes back with an absolute error of about eps / theta_f -- 1e-4 relative at the 1e-6 rad
    this test moves them by, in the CPU oracle just as on the device.  Bound used instead: |de|_2 <= sqrt(m) max(64 eps
    max(1, |x|_inf), max_f 8 eps / theta_f), so |dy| <= |de|_2 / sqrt(lambda_min(A)), plus the factorisation's
    64 m eps kappa |y|."""
    B, N = 64, 3
    sc, g, lens, _ = make_batch(B, N, 3, seed=3)
    L = capi.lib()
    r = np.random.default_rng(7)
    m = 25
    zeta = r.normal(size=(B, m))
    x, P = g.get_state(), g.get_covariance()
    e = np.stack([1e-3 * np.linalg.cholesky(P[b]) @ zeta[b] for b in range(B)])
    xt = np.empty_like(x)
    p = lambda a: C.c_void_p(a.ctypes.data)
    capi.check(L.viekf_batch_boxplus(g._h, p(x), p(np.ascontiguousarray(e)), p(xt), capi.HOST))
    got = diag.consistency(g, xt)
    worst_body = worst_nees = worst_feat = 0.0
    fails = []
    for b in range(B):
        w = np.linalg.eigvalsh(P[b])
        tol = max(1e-9, 64 * m * EPS * w[-1] / w[0])
        want = 1e-3 * zeta[b]
        body = np.abs(got["whitened"][b, :16] - want[:16]) / np.abs(want[:16])
        nref = np.array([(want[:q] ** 2).sum() for q in BLOCKS])
        nerr = np.abs(got["nees"][b, :3] - nref) / nref
        theta = np.array([np.hypot(e[b, 16 + 3 * f], e[b, 17 + 3 * f]) for f in range(N)])
        de = np.sqrt(m) * max(64 * EPS * max(1.0, np.abs(x[b]).max()), (8 * EPS / theta).max())
        tol_y = de / np.sqrt(w[0]) + 64 * m * EPS * (w[-1] / w[0]) * np.linalg.norm(want)
        ferr = np.abs(got["whitened"][b, 16:m] - want[16:]).max()
        ny = np.linalg.norm(want)
        n3err = abs(got["nees"][b, 3] - ny * ny)
        worst_body, worst_nees, worst_feat = max(worst_body, body.max() / tol), max(worst_nees, nerr.max() / tol), max(worst_feat, ferr / tol_y)
        if not (body.max() <= tol and nerr.max() <= tol and ferr <= tol_y and n3err <= 2 * ny * tol_y + tol_y ** 2 and got["info"][b] == 0):
            fails.append((b, body.max(), nerr.max(), tol, ferr, tol_y, n3err))
    print("round trip, worst error / bound: whitened[:16] %.3e  nees[0:3] %.3e  whitened[16:] (acos bound) %.3e" % (
        worst_body, worst_nees, worst_feat))
    assert not fails, fails


def test_many_passes_below_a_panel():
    """N = 130, n = 406: more rows below a panel than the 8 x 48 one pass of the workgroup holds, so the later passes run -- lanes
    0..15 keep the factored block, the other lanes take further rows -- on the workspace path"""
    N = 130
    sc, g, lens, slot = make_batch(1, N, N, steps=1, seed=4)
    xt = perturbed_truth(sc, g, N)
    g.step(sc["u"][1], sc["dt"], sc["z"][1], slot, sc["R"])
    got = diag.consistency(g, xt)
    ref = reference(sc, g, xt)
    assert ref[0]["m"] == 406
    check_filter(got, 0, ref[0], "N = %d" % N)


def _twins(seed):
    a = make_batch(3, 3, [3, 2, 3], seed=seed)
    b = make_batch(3, 3, [3, 2, 3], seed=seed)
    return a, b


def _feat_args(sc, g, lens):
    r = np.random.default_rng(5)
    slot = np.array([[0, 1, 2], [1, -1, 2], [2, 0, 1]], np.int32)   # filter 1 has two features: slot 2 is not active
    z = sc["pix"][:, :3, :][np.arange(g.B)[:, None], np.maximum(slot, 0)] + r.normal(0, 3.0, (g.B, 3, 2))
    return np.ascontiguousarray(z), slot


def test_read_only_and_stale_upper_triangle():
    """both diagnostics straight after a fused step change nothing, and read the lower triangle only: their outputs equal, bit
    for bit, those computed after the mirror"""
    (sc, g1, lens, slot), (_, g2, _, _) = _twins(11)
    xt = perturbed_truth(sc, g1, 11)
    perturbed_truth(sc, g2, 11)                       # (the same calls on the twin)
    for g in (g1, g2):
        g.step(sc["u"][2], sc["dt"], sc["z"][2], slot, sc["R"])
    z, fslot = _feat_args(sc, g1, lens)
    before = diag.consistency(g1, xt), diag.innovation(g1, FEAT, z, sc["R"], fslot), diag.innovation(g1, POS, xt[:, :3], np.eye(3) * 1e-2)
    s1, s2 = g1.get_status(), g2.get_status()
    x1, P1, l1 = g1.get_state(), g1.get_covariance(), g1.get_len_features()
    x2, P2, l2 = g2.get_state(), g2.get_covariance(), g2.get_len_features()
    assert np.array_equal(s1, s2) and np.array_equal(x1, x2) and np.array_equal(P1, P2) and np.array_equal(l1, l2)
    for g in (g1, g2):                                # P is mirrored now
        after = diag.consistency(g, xt), diag.innovation(g, FEAT, z, sc["R"], fslot), diag.innovation(g, POS, xt[:, :3], np.eye(3) * 1e-2)
        for d0, d1 in zip(before, after):
            for k in d0:
                assert np.array_equal(d0[k], d1[k], equal_nan=True), k
    # and under a participation mask, which the read-only evaluations ignore
    capi.check(capi.lib().viekf_batch_set_active(g1._h, C.c_void_p(np.array([1, 0, 0], np.uint8).ctypes.data), capi.HOST))
    masked = diag.consistency(g1, xt)
    for k in masked:
        assert np.array_equal(masked[k], before[0][k], equal_nan=True), k


def test_per_filter_ring_slots():
    """filter b's live state is ring slot map[b] (viekf_batch_select_filters): the outputs are those of the state that was put
    there, not of the batch's own buffers, which have moved on by then"""
    sc, g, lens, slot = make_batch(3, 3, [3, 2, 3], seed=12)
    xt = perturbed_truth(sc, g, 12)
    g.step(sc["u"][2], sc["dt"], sc["z"][2], slot, sc["R"])
    z, fslot = _feat_args(sc, g, lens)
    d0, i0 = diag.consistency(g, xt), diag.innovation(g, FEAT, z, sc["R"], fslot)
    L = capi.lib()
    ring = np.array([2, 0, 1], np.int32)
    g.history_resize(3)
    capi.check(L.viekf_batch_snapshot_filters(g._h, C.c_void_p(ring.ctypes.data), capi.HOST))
    g.step(sc["u"][3], sc["dt"], sc["z"][3], slot, sc["R"])          # the batch's own buffers move on
    d_moved = diag.consistency(g, xt)
    assert not np.array_equal(d_moved["logdet"], d0["logdet"])
    g.select_filters(ring)
    d1, i1 = diag.consistency(g, xt), diag.innovation(g, FEAT, z, sc["R"], fslot)
    for a, b in ((d0, d1), (i0, i1)):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), k
    g.history_resize(0)


def test_not_positive_definite():
    sc, g, lens, slot = make_batch(3, 3, [3, 2, 3], seed=13)
    xt = perturbed_truth(sc, g, 13)
    x, P = g.get_state(), g.get_covariance()
    P[1, 17, 17] = -1.0
    g.set_state(P=P)
    st0 = g.get_status()
    got = diag.consistency(g, xt)
    assert np.array_equal(g.get_status(), st0)
    assert got["info"].tolist() == [0, 18, 0]
    x, P2, ln = g.get_state(), g.get_covariance(), g.get_len_features()
    assert P2[1, 17, 17] == -1.0
    # filter 1: what lies before the failing pivot is still reported
    A = P2[1, :17, :17]
    Lb = np.linalg.cholesky(A)
    e = oracle_like(sc, 3, x[1], ln[1]).boxminus(xt[1], x[1])
    y = np.linalg.solve(Lb, e[:17])
    w = np.linalg.eigvalsh(A)
    tol = max(1e-9, 64 * 17 * EPS * w[-1] / w[0])
    for k, p in enumerate(BLOCKS):
        ref = (y[:p] ** 2).sum()
        assert np.isfinite(got["nees"][1, k]) and abs(got["nees"][1, k] - ref) <= tol * ref
    assert np.isnan(got["nees"][1, 3]) and np.isnan(got["logdet"][1])
    assert np.abs(got["whitened"][1, :17] - y).max() <= tol * np.abs(y).max()
    assert np.isnan(got["whitened"][1, 17:22]).all() and (got["whitened"][1, 22:] == 0.0).all()
    # the neighbours are untouched by it
    for b in (0, 2):
        xs, m = x, 16 + 3 * int(ln[b])
        A = P2[b, :m, :m]
        w = np.linalg.eigvalsh(A)
        Lb = np.linalg.cholesky(A)
        y = np.linalg.solve(Lb, oracle_like(sc, 3, xs[b], ln[b]).boxminus(xt[b], xs[b])[:m])
        wh = np.zeros(g.n)
        wh[:m] = y
        check_filter(got, b, dict(m=m, kappa=w[-1] / w[0], logdet=2.0 * np.log(np.diag(Lb)).sum(), whitened=wh,
                                  nees=np.array([(y[:p] ** 2).sum() for p in BLOCKS + (m,)])), "next to a failing filter")


def test_argument_rules():
    sc, g, lens, slot = make_batch(2, 3, 3, steps=1, seed=14)
    out = diag.consistency(g)                          # x_true = None: logdet and info only
    assert set(out) == {"logdet", "info"} and np.isfinite(out["logdet"]).all() and (out["info"] == 0).all()
    P = g.get_covariance()
    ref = np.array([np.linalg.slogdet(P[b])[1] for b in range(2)])
    assert np.abs(out["logdet"] - ref).max() <= 64 * 25 * 25 * EPS * np.linalg.cond(P[0])
    L = diag._bind()
    buf = np.zeros(2 * 25)
    p = C.c_void_p(buf.ctypes.data)
    assert L.viekf_diag_consistency(g._h, None, p, None, None, None, capi.HOST) == capi.OK
    assert L.viekf_diag_consistency(g._h, None, p, p, None, None, capi.HOST) == capi.ERR_INVALID      # nees without x_true
    assert L.viekf_diag_consistency(g._h, None, None, None, p, None, capi.HOST) == capi.ERR_INVALID   # whitened without x_true
    assert L.viekf_diag_consistency(g._h, None, None, None, None, None, capi.HOST) == capi.ERR_INVALID
    xt = g.get_state()
    assert L.viekf_diag_consistency(g._h, C.c_void_p(xt.ctypes.data), None, None, None, None, capi.HOST) == capi.ERR_INVALID
    z = np.zeros((2, 2, 3))
    R = np.eye(3)
    with pytest.raises(v.ViekfError):                  # M > 1 for a model without a slot
        diag.innovation(g, POS, z, R)
    with pytest.raises(v.ViekfError):                  # a feature model without slots
        diag.innovation(g, FEAT, np.zeros((2, 2)), np.eye(2))


def _innovation_reference(sc, g, mtype, z, R, slot):
    """r, H P H^T + R and r^T S^-1 r from the oracle's h / H and numpy; z [B][M][zdim], R (rdim, rdim), slot [B][M] or None"""
    x, P, ln = g.get_state(), g.get_covariance(), g.get_len_features()
    B, M, rdim = z.shape[0], z.shape[1], R.shape[0]
    nis = np.full((B, M), np.nan)
    res = np.full((B, M, rdim), np.nan)
    S = np.full((B, M, rdim, rdim), np.nan)
    for b in range(B):
        f = oracle_like(sc, g.N, x[b], ln[b])
        for k in range(M):
            sl = 0 if slot is None else int(slot[b, k])
            if slot is not None and not 0 <= sl < ln[b]:
                continue
            zhat, H = f.h(mtype, x[b], sl)
            if mtype == QZETA:
                r = orc.q_feat_boxminus(z[b, k], zhat)
            elif mtype == ATT:
                r = orc.q_boxminus(z[b, k], zhat)
            else:
                r = z[b, k, :rdim] - zhat[:rdim]
            Hr = H[:rdim]
            S[b, k] = Hr @ P[b] @ Hr.T + R
            res[b, k] = r
            nis[b, k] = r @ np.linalg.solve(S[b, k], r)
    return nis, res, S


def _parity(got, ref, what):
    ok = np.isfinite(ref)
    assert np.array_equal(np.isnan(np.asarray(got)), ~ok), what + ": NaN pattern"
    scale = np.abs(ref[ok]).max()
    d = np.abs(np.asarray(got)[ok] - ref[ok])
    assert d.max() <= 1e-9 * scale, "%s: %.3e vs scale %.3e" % (what, d.max(), scale)
    big = np.abs(ref[ok]) > 1e-9 * scale
    assert (d[big] <= 1e-6 * np.abs(ref[ok])[big]).all(), what


def _cases(sc, g, lens):
    """(name, mtype, z [B][M][zdim], R, slot) with z spread so that the gate opens for some filters and shuts for others"""
    r = np.random.default_rng(21)
    x = g.get_state()
    B = g.B
    zf, fslot = _feat_args(sc, g, lens)
    zf[:, 0] += np.array([[0.0, 0.0], [40.0, -30.0], [3.0, 2.0]])
    depth = 1.0 / x[:, [17 + 4, 17 + 5 + 4]] + np.array([[0.05, 4.0], [3.0, -0.02], [-2.5, 0.3]])
    q = np.stack([orc.q_boxplus(x[b, 6:10], dv) for b, dv in enumerate(np.array([[0.01, -0.02, 0.01], [0.3, 0.1, -0.2], [-0.05, 0.02, 0.15]]))])
    return [
        ("FEAT", FEAT, zf, sc["R"], fslot),
        ("DEPTH", DEPTH, depth[:, :, None], np.array([[0.1]]), np.array([[0, 1]] * B, np.int32)),
        ("POS", POS, (x[:, 0:3] + np.array([[0.01, 0.0, -0.02], [0.3, -0.2, 0.25], [0.05, 0.08, -0.01]]))[:, None, :], np.diag([1e-2, 2e-2, 1e-2]), None),
        ("ATT", ATT, q[:, None, :], np.diag([1e-2, 1e-2, 3e-2]), None),
    ]


def test_innovation_against_the_oracle_and_the_gate():
    sc, g, lens, slot = make_batch(3, 3, [3, 2, 3], seed=15)
    g.step(sc["u"][2], sc["dt"], sc["z"][2], slot, sc["R"])
    cases = _cases(sc, g, lens)
    outs = [diag.innovation(g, mt, z, R, sl) for _, mt, z, R, sl in cases]     # before anything mirrors P
    gated_seen = set()
    for (name, mt, z, R, sl), got in zip(cases, outs):
        nis, res, S = _innovation_reference(sc, g, mt, z, R, sl)
        print(name, "nis ref", nis.tolist(), "got", np.asarray(got["nis"]).tolist())
        _parity(got["nis"], nis, name + " nis")
        _parity(got["residual"], res, name + " residual")
        _parity(got["S"], S, name + " S")
        if name == "FEAT":
            assert np.isnan(got["nis"][1, 1]) and np.isnan(got["nis"][1, 2]) and np.isnan(got["S"][1, 2]).all()
        # the gate of viekf_batch_update on a twin, first measurement of the case
        assert (np.abs(nis[:, 0] - 9.0) > 1e-6).all(), "pick another z: a reference nis sits on the gate"
        _, twin, _, tslot = make_batch(3, 3, [3, 2, 3], seed=15)
        twin.step(sc["u"][2], sc["dt"], sc["z"][2], tslot, sc["R"])
        result = twin.update(mt, z[:, 0], R, None if sl is None else np.ascontiguousarray(sl[:, 0]))
        assert ((result == capi.MEAS_GATED) == (nis[:, 0] > 9.0)).all(), (name, result, nis[:, 0])
        assert ((np.asarray(got["nis"])[:, 0] > 9.0) == (nis[:, 0] > 9.0)).all()
        gated_seen |= set((nis[:, 0] > 9.0).tolist())
    assert gated_seen == {True, False}


def test_device_pointers_equal_host_pointers():
    import torch
    sc, g, lens, slot = make_batch(3, 3, [3, 2, 3], seed=16)
    xt = perturbed_truth(sc, g, 16)
    g.step(sc["u"][2], sc["dt"], sc["z"][2], slot, sc["R"])
    z, fslot = _feat_args(sc, g, lens)
    host = diag.consistency(g, xt), diag.innovation(g, FEAT, z, sc["R"], fslot)
    dev = torch.device("cuda", g.device)
    t = lambda a: torch.as_tensor(a).to(dev).contiguous()
    torch.cuda.synchronize()
    d_c = diag.consistency(g, t(xt))
    d_i = diag.innovation(g, FEAT, t(z), t(sc["R"]), t(fslot))
    g.sync()
    for h, d in zip(host, (d_c, d_i)):
        for k in h:
            assert d[k].is_cuda
            assert np.array_equal(h[k], d[k].cpu().numpy(), equal_nan=True), k
