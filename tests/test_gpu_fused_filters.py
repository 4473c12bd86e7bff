"""viekf_batch_propagate_n_filters_to: the replay after a rewind for filters on independent clocks -- filter b takes k_count[b]
propagates from its live ring slot into dst_slot[b].  On the resident fused kernel that is ONE launch of its multi-propagate
instance with a trip count per workgroup; everywhere else the host steps through viekf_batch_propagate_filters_to.  Either way the
result is, bit for bit, what k_count[b] single viekf_batch_propagate_filters_to launches give."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from tests.helpers import apply_kernel
from tests.test_gpu_parity import assert_close, oracle_params
from vi_ekf_amd import capi, scene

pytestmark = pytest.mark.gpu

KMAX, H = 5, 8


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _plan(B):
    """-> k_count, start slot, destination slot, scratch slot per filter.  Filter 0 takes the full KMAX, filter 1 none; from
    five filters on, filter 4 has a count but no destination (also untouched); the rest draw from {0, 1, 2, 5}."""
    rng = np.random.default_rng(11 + B)
    k = rng.choice([0, 1, 2, 5], size=B).astype(np.int32)
    k[:4] = [5, 0, 2, 1]
    idx = np.arange(B)
    start = (idx % 3).astype(np.int32)
    dst = ((start + 1 + idx % 4) % H).astype(np.int32)
    if B >= 5:
        k[4], dst[4] = 2, -1
    other = np.where((dst + 1) % H == start, (dst + 2) % H, (dst + 1) % H).astype(np.int32)
    return k, start, dst, other


def _inputs(sc, B, k_count):
    """u [KMAX][B][6], dt [KMAX][B]; NaN wherever k >= k_count[b]: those entries must never be read"""
    u = np.stack([sc["u"][1 + k] for k in range(KMAX)])
    dt = np.stack([sc["dt"] * (1.0 + 0.1 * k) for k in range(KMAX)])
    for b in range(B):
        u[k_count[b]:, b, :] = np.nan
        dt[k_count[b]:, b] = np.nan
    return np.ascontiguousarray(u), np.ascontiguousarray(dt)


def _make(sc, B, N, kernel, start, res_instance=None):
    """a batch after one fused step (P dense), every filter's live state in ring slot start[b]; features of NaN depth"""
    g = v.BatchVIEKF(B, N, sc["params"])
    apply_kernel(g, kernel)
    if res_instance is not None:
        g.set_tuning(capi.TUNE_RES_INSTANCE, res_instance)
    for i in range(N):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    g.step(sc["u"][0], sc["dt"], sc["z"][0], sc["slot"], sc["R"])
    g.history_resize(H)
    capi.check(capi.lib().viekf_batch_snapshot_filters(g._h, _p(start), capi.HOST))
    g.select_filters(start)
    return g


def _one_by_one(g, u, dt, k_count, dst, other):
    """KMAX rounds of viekf_batch_propagate_filters_to: a filter's steps by turns into dst / other, the last one into dst"""
    L = capi.lib()
    for k in range(KMAX):
        on = (dst >= 0) & (k < k_count)
        into = np.where(on, np.where((k_count - 1 - k) % 2 == 1, other, dst), -1).astype(np.int32)
        capi.check(L.viekf_batch_propagate_filters_to(g._h, _p(u[k]), _p(dt[k]), _p(into), capi.HOST))


@pytest.mark.parametrize("N,kernel,B", [(6, 0, 7), (50, 2, 5), (60, 0, 5), (30, 1, 5), (90, 0, 4), (50, 0, 600)])
def test_fused_per_filter_counts_equal_single_propagates_bit_for_bit(N, kernel, B):
    sc = scene.make_scene(B, N, KMAX + 1, seed=40 + N)
    k_count, start, dst, other = _plan(B)
    u, dt = _inputs(sc, B, k_count)
    ga, gb = _make(sc, B, N, kernel, start), _make(sc, B, N, kernel, start)
    x0, P0 = ga.get_state(), ga.get_covariance()
    assert np.array_equal(x0, gb.get_state()) and np.array_equal(P0, gb.get_covariance())

    written = ga.propagate_n_filters_to(u, dt, k_count, dst)
    _one_by_one(gb, u, dt, k_count, dst, other)
    fused = "k_step_resident<" in ga.describe()
    print("describe: %s -> intermediates_written %d" % (ga.describe(), written))
    assert written == (0 if fused else 1)

    xa, Pa, xb, Pb = ga.get_state(), ga.get_covariance(), gb.get_state(), gb.get_covariance()
    la, lb = ga.get_len_features(), gb.get_len_features()
    assert np.array_equal(la, lb) and (la == N).all()
    assert np.array_equal(xa, xb)
    for b in range(B):                               # the active block (here: every feature is in use)
        na = 16 + 3 * int(la[b])
        assert np.array_equal(Pa[b, :na, :na], Pb[b, :na, :na]), "filter %d" % b
    assert np.isfinite(xa).all() and np.isfinite(Pa).all()       # none of the NaN inputs past a filter's count was read
    assert np.array_equal(ga.get_status(), gb.get_status())
    moved = (k_count > 0) & (dst >= 0)
    assert np.array_equal(xa[~moved], x0[~moved]) and np.array_equal(Pa[~moved], P0[~moved])     # count 0 / no destination: untouched
    assert all(not np.array_equal(xa[b], x0[b]) for b in np.flatnonzero(moved))
    # every start slot is as it was; the filters that did not move still live there
    ga.select_filters(start)
    assert np.array_equal(ga.get_state(), x0) and np.array_equal(ga.get_covariance(), P0)
    live = np.where(moved, dst, start).astype(np.int32)
    ga.select_filters(live)
    assert np.array_equal(ga.get_state(), xa) and np.array_equal(ga.get_covariance(), Pa)
    # the host's mirror of the live slots moved with the device's: a destination equal to the new live slot is refused
    again = np.where(moved, dst, -1).astype(np.int32)
    L = capi.lib()
    assert L.viekf_batch_propagate_n_filters_to(ga._h, KMAX, _p(u), _p(dt), _p(k_count), _p(again), None, capi.HOST) == capi.ERR_INVALID
    # out of the ring: the whole matrix
    ga.history_resize(0); gb.history_resize(0)
    assert np.array_equal(ga.get_state(), gb.get_state()) and np.array_equal(ga.get_covariance(), gb.get_covariance())
    assert np.array_equal(ga.get_status(), gb.get_status()) and np.array_equal(ga.get_len_features(), gb.get_len_features())


def test_fused_per_filter_counts_vs_oracle():
    """(left to itself a batch of 5 takes the one-workgroup-per-CU instance <3,7>, which the bit-for-bit case above runs; here the
    headline instance <7,3>, row 6 of the instance list, is asked for by index)"""
    N, kernel, B = 50, 2, 5
    sc = scene.make_scene(B, N, KMAX + 1, seed=40 + N)
    k_count, start, dst, _ = _plan(B)
    u, dt = _inputs(sc, B, k_count)
    g = _make(sc, B, N, kernel, start, res_instance=6)
    assert "k_step_resident<7,3>" in g.describe(), g.describe()
    assert g.propagate_n_filters_to(u, dt, k_count, dst) == 0
    x, P = g.get_state(), g.get_covariance()
    for b in range(B):
        f = orc.OracleFilter(N).init(**oracle_params(sc["params"]))
        for i in range(N):
            f.init_feature(sc["pix"][b, i], i, float("nan"))
        f.run_steps(sc["u"][0, b][None], sc["dt"][b], sc["z"][0, b][None], sc["slot"][b], sc["R"])
        for k in range(int(k_count[b]) if dst[b] >= 0 else 0):
            f.propagate(u[k, b], float(dt[k, b]))
        assert_close(x[b], f.x, "x of filter %d (%d propagates)" % (b, k_count[b]))
        assert_close(P[b], f.P, "P of filter %d (%d propagates)" % (b, k_count[b]))


def test_fused_per_filter_counts_refusals():
    """each refused call returns ERR_INVALID and leaves x, P, status and the live slots as they were"""
    B, N = 7, 6
    sc = scene.make_scene(B, N, KMAX + 1, seed=46)
    k_count, start, dst, _ = _plan(B)
    u, dt = _inputs(sc, B, k_count)
    L = capi.lib()

    def call(g, kmax, kc, d, uu=u, dd=dt):
        kc, d = np.ascontiguousarray(kc, dtype=np.int32), np.ascontiguousarray(d, dtype=np.int32)
        return L.viekf_batch_propagate_n_filters_to(g._h, kmax, _p(uu), _p(dd), _p(kc), _p(d), None, capi.HOST)

    # before viekf_batch_select_filters
    g0 = v.BatchVIEKF(B, N, sc["params"])
    for i in range(N):
        g0.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    g0.history_resize(H)
    x0, P0 = g0.get_state(), g0.get_covariance()
    assert call(g0, KMAX, k_count, dst) == capi.ERR_INVALID
    assert np.array_equal(g0.get_state(), x0) and np.array_equal(g0.get_covariance(), P0)

    g = _make(sc, B, N, 0, start)

    def read():
        out = [g.get_state(), g.get_covariance(), g.get_status()]
        for s in range(H):                       # every ring slot of every filter, then back to the live ones
            g.select_filters(np.full(B, s, dtype=np.int32))
            out += [g.get_state(), g.get_covariance()]
        g.select_filters(start)
        return out

    before = read()
    u64, dt64 = np.zeros((65, B, 6)), np.full((65, B), 0.004)
    mask = np.ones(B, dtype=np.uint8); mask[2] = 0
    bad_live = dst.copy(); bad_live[0] = start[0]
    bad_range = dst.copy(); bad_range[2] = H
    bad_count = k_count.copy(); bad_count[3] = KMAX + 1
    neg_count = k_count.copy(); neg_count[3] = -1
    capi.check(L.viekf_batch_set_active(g._h, _p(mask), capi.HOST))
    assert call(g, KMAX, k_count, dst) == capi.ERR_INVALID                    # participation mask set
    capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
    assert call(g, KMAX, k_count, bad_live) == capi.ERR_INVALID               # dst == live
    assert call(g, KMAX, k_count, bad_range) == capi.ERR_INVALID              # slot out of range
    assert call(g, KMAX, bad_count, dst) == capi.ERR_INVALID                  # k_count > Kmax
    assert call(g, KMAX, neg_count, dst) == capi.ERR_INVALID
    assert call(g, 65, k_count, dst, u64, dt64) == capi.ERR_INVALID           # Kmax > 64
    assert call(g, 0, np.zeros(B), dst) == capi.ERR_INVALID
    after = read()
    for a, b in zip(before, after):               # (bytes: a ring slot nobody has written yet may hold anything, NaN included)
        assert a.tobytes() == b.tobytes()
    # the live slots did not move either: the same call, valid, goes through from the start slots
    assert call(g, KMAX, k_count, dst) == capi.OK
    moved = (k_count > 0) & (dst >= 0)
    x = g.get_state()
    assert np.array_equal(x[~moved], before[0][~moved]) and all(not np.array_equal(x[b], before[0][b]) for b in np.flatnonzero(moved))
