"""Participation mask and per-filter ring copies of the C ABI (viekf_batch_set_active, _snapshot_filters / _restore_filters:
what lets filters on independent clocks share a batch) and the covariance block read (viekf_batch_get_cov_block)."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from vi_ekf_amd import capi, scene

pytestmark = pytest.mark.gpu


def _p(a):
    return C.c_void_p(a.ctypes.data)


@pytest.mark.parametrize("N,kernel", [(6, 0), (50, 2), (30, 1), (60, 0), (70, 0), (50, 3), (50, 5)])
def test_masked_filters_are_untouched_and_the_others_unchanged(N, kernel):
    B, steps = 6, 2
    sc = scene.make_scene(B, N, steps, seed=9)
    L = capi.lib()

    def make():
        g = v.BatchVIEKF(B, N, sc["params"])
        from tests.helpers import apply_kernel
        apply_kernel(g, kernel)
        for i in range(N):
            g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        return g

    ga, gb = make(), make()
    x0, P0 = ga.get_state(), ga.get_covariance()
    mask = np.array([1, 0, 1, 1, 0, 1], dtype=np.uint8)
    capi.check(L.viekf_batch_set_active(ga._h, _p(mask), capi.HOST))
    for s in range(steps):
        ga.propagate(sc["u"][s], sc["dt"])
        ga.update_feat(sc["z"][s], sc["slot"], sc["R"])
        ga.step(sc["u"][s], sc["dt"], sc["z"][s], sc["slot"], sc["R"])
        gb.propagate(sc["u"][s], sc["dt"])
        gb.update_feat(sc["z"][s], sc["slot"], sc["R"])
        gb.step(sc["u"][s], sc["dt"], sc["z"][s], sc["slot"], sc["R"])
    capi.check(L.viekf_batch_set_active(ga._h, None, capi.HOST))
    xa, Pa, xb, Pb = ga.get_state(), ga.get_covariance(), gb.get_state(), gb.get_covariance()
    on, off = mask.astype(bool), ~mask.astype(bool)
    assert np.array_equal(xa[off], x0[off]) and np.array_equal(Pa[off], P0[off])          # masked out: bit for bit untouched
    assert np.array_equal(xa[on], xb[on]) and np.array_equal(Pa[on], Pb[on])              # the others: as without a mask
    assert not np.array_equal(xa[on], x0[on])


def test_per_filter_ring_copies_and_cov_block():
    B, N = 4, 8
    sc = scene.make_scene(B, N, 3, seed=4)
    g = v.BatchVIEKF(B, N, sc["params"])
    L = capi.lib()
    for i in range(N):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    g.history_resize(5)
    states = []
    for s in range(3):
        g.step(sc["u"][s], sc["dt"], sc["z"][s], sc["slot"], sc["R"])
        states.append((g.get_state(), g.get_covariance()))
        slot = np.array([s, 4 - s, -1, s], dtype=np.int32)            # every filter its own slot; filter 2 records nothing
        capi.check(L.viekf_batch_snapshot_filters(g._h, _p(slot), capi.HOST))
    # rewind: filter 0 to step 0, filter 1 to step 2 (slot 2), filter 2 stays, filter 3 to step 1
    slot = np.array([0, 2, -1, 1], dtype=np.int32)
    capi.check(L.viekf_batch_restore_filters(g._h, _p(slot), capi.HOST))
    x, P = g.get_state(), g.get_covariance()
    for b, s in ((0, 0), (1, 2), (2, 2), (3, 1)):
        assert np.array_equal(x[b], states[s][0][b]) and np.array_equal(P[b], states[s][1][b])
    bad = np.array([0, 9, 0, 0], dtype=np.int32)
    assert L.viekf_batch_restore_filters(g._h, _p(bad), capi.HOST) == capi.ERR_INVALID
    # a block of P: rows 6..8 (attitude) x columns 0..2 (position), column-major per filter
    blk = np.zeros((B, 3, 3))
    capi.check(L.viekf_batch_get_cov_block(g._h, 6, 0, 3, 3, _p(blk), capi.HOST))
    assert np.array_equal(blk.transpose(0, 2, 1), P[:, 6:9, 0:3])
    assert L.viekf_batch_get_cov_block(g._h, 0, 0, 3, 16 + 3 * N + 1, _p(blk), capi.HOST) == capi.ERR_INVALID


@pytest.mark.parametrize("N,kernel", [(30, 1), (90, 0)])
def test_masked_propagate_keeps_the_other_filters_staleness(N, kernel):
    """Streaming family: a grouped update of filters A leaves their upper triangle stale; a masked propagate of the DISJOINT
    filters B must not clear that (it did, and every whole-P reader then took A's stale upper triangle as valid).
    Compared with the same calls made on two separate batches of the filters A and B."""
    B, M = 6, 5
    sc = scene.make_scene(B, N, 2, seed=21)
    L = capi.lib()

    def make(sel):
        p = sc["params"]
        g = v.BatchVIEKF(len(sel), N, p)
        if kernel:
            g.set_kernel(kernel)
        for i in range(N):
            g.init_feature(sc["pix"][sel, i, :].copy(), np.full(len(sel), np.nan))
        return g

    allf = np.arange(B)
    A, Bm = np.array([0, 2, 3]), np.array([1, 4, 5])
    mA = np.zeros(B, dtype=np.uint8); mA[A] = 1
    mB = np.zeros(B, dtype=np.uint8); mB[Bm] = 1
    g = make(allf)
    g.propagate(sc["u"][0], sc["dt"])                                    # everybody: P no longer diagonal
    capi.check(L.viekf_batch_set_active(g._h, _p(mA), capi.HOST))
    g.update_feat(sc["z"][0][:, :M], sc["slot"][:, :M], sc["R"])          # A: grouped update (M >= 2)
    capi.check(L.viekf_batch_set_active(g._h, _p(mB), capi.HOST))
    g.propagate(sc["u"][1], sc["dt"])                                    # B only
    capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
    P = g.get_covariance()
    x = g.get_state()
    assert (P == P.transpose(0, 2, 1)).all(), "a stale upper triangle was handed out"
    # the same history on separate batches
    ga, gb = make(A), make(Bm)
    ga.propagate(sc["u"][0][A], sc["dt"][A]); gb.propagate(sc["u"][0][Bm], sc["dt"][Bm])
    ga.update_feat(sc["z"][0][A][:, :M], sc["slot"][A][:, :M], sc["R"])
    gb.propagate(sc["u"][1][Bm], sc["dt"][Bm])
    assert np.array_equal(P[A], ga.get_covariance()) and np.array_equal(x[A], ga.get_state())
    assert np.array_equal(P[Bm], gb.get_covariance()) and np.array_equal(x[Bm], gb.get_state())
    # ... and a generic update (reads all of P) after the same sequence agrees as well
    z = np.tile(np.array([0.1, -0.2, 0.3]), (B, 1))
    Rp = np.eye(3) * 0.01
    g.update(capi_type("POS"), z, Rp)
    ga.update(capi_type("POS"), z[A], Rp)
    assert np.array_equal(g.get_covariance()[A], ga.get_covariance())


def capi_type(name):
    return {"ACC": 0, "ALT": 1, "ATT": 2, "POS": 3, "VEL": 4, "QZETA": 5, "FEAT": 6, "DEPTH": 8, "INV_DEPTH": 9}[name]


def test_propagate_to_refuses_a_participation_mask_and_device_slots_are_checked():
    import torch
    B, N = 4, 8
    sc = scene.make_scene(B, N, 1, seed=5)
    g = v.BatchVIEKF(B, N, sc["params"])
    L = capi.lib()
    for i in range(N):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    g.history_resize(3)
    capi.check(L.viekf_batch_select(g._h, 0))
    mask = np.array([1, 0, 1, 1], dtype=np.uint8)
    capi.check(L.viekf_batch_set_active(g._h, _p(mask), capi.HOST))
    u, dt = np.ascontiguousarray(sc["u"][0]), np.ascontiguousarray(sc["dt"])
    assert L.viekf_batch_propagate_to(g._h, _p(u), _p(dt), 1, capi.HOST) == capi.ERR_INVALID
    capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
    capi.check(L.viekf_batch_propagate_to(g._h, _p(u), _p(dt), 1, capi.HOST))
    capi.check(L.viekf_batch_select(g._h, -1))
    # device-resident slot list with an out-of-range entry: nothing is copied for that filter, its INTERNAL flag is raised
    x0, P0 = g.get_state(), g.get_covariance()
    slots = torch.tensor([0, 7, -1, 1], dtype=torch.int32, device="cuda:0")
    capi.check(L.viekf_batch_restore_filters(g._h, C.c_void_p(slots.data_ptr()), capi.DEVICE))
    g.sync()
    st = g.get_status()
    assert st[1] & capi.FLAG_INTERNAL and not (st[[0, 2, 3]] & capi.FLAG_INTERNAL).any()
    x1, P1 = g.get_state(), g.get_covariance()
    assert np.array_equal(x1[1], x0[1]) and np.array_equal(P1[1], P0[1]) and np.array_equal(x1[2], x0[2])


@pytest.mark.parametrize("N,kernel,B", [(6, 0, 7), (50, 2, 5), (30, 1, 5), (60, 0, 5), (90, 0, 4), (50, 0, 600)])
def test_per_filter_live_slots_zero_copy_ring(N, kernel, B):
    """viekf_batch_select_filters / _propagate_filters_to (r04: the zero-copy ring of filters on independent clocks): every filter
    steps from ITS ring slot into ITS next one, rewinds by an index, is updated in its slot -- bit for bit what a batch that keeps
    one live state and is stepped under the same participation masks computes; the slots left behind keep their states; getters and
    set_state work on each filter's own slot; leaving the ring brings every live state home."""
    steps = 4
    sc = scene.make_scene(B, N, steps, seed=21 + N)
    L = capi.lib()
    from tests.helpers import apply_kernel

    def make():
        g = v.BatchVIEKF(B, N, sc["params"])
        apply_kernel(g, kernel)
        for i in range(N):
            g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        return g

    ga, gb = make(), make()
    H = 6
    ga.history_resize(H)
    zero = np.zeros(B, dtype=np.int32)
    capi.check(L.viekf_batch_snapshot_filters(ga._h, _p(zero), capi.HOST))
    capi.check(L.viekf_batch_select_filters(ga._h, _p(zero)))
    assert np.array_equal(ga.get_state(), gb.get_state()) and np.array_equal(ga.get_covariance(), gb.get_covariance())
    live = zero.copy()
    rng = np.random.default_rng(3)
    hist = {}                                       # (filter, slot) -> (x, P) as the reference batch had it then
    xb, Pb = gb.get_state(), gb.get_covariance()
    for b in range(B):
        hist[(b, 0)] = (xb[b].copy(), Pb[b].copy())
    for s in range(steps):
        mask = (rng.uniform(size=B) < 0.7).astype(np.uint8)
        mask[0] = 1
        dst = np.where(mask == 1, (live + 1) % H, -1).astype(np.int32)
        u = np.ascontiguousarray(sc["u"][s]); dt = np.ascontiguousarray(sc["dt"] * (1.0 + 0.1 * s))
        capi.check(L.viekf_batch_propagate_filters_to(ga._h, _p(u), _p(dt), _p(dst), capi.HOST))
        live = np.where(mask == 1, dst, live).astype(np.int32)
        capi.check(L.viekf_batch_set_active(gb._h, _p(mask), capi.HOST))
        gb.propagate(u, dt)
        m2 = (rng.uniform(size=B) < 0.6).astype(np.uint8)     # the frame's updates for some of the filters, in their slots
        m2[0] = 1
        for g in (ga, gb):
            capi.check(L.viekf_batch_set_active(g._h, _p(m2), capi.HOST))
            g.update_feat(sc["z"][s], sc["slot"], sc["R"])
            capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
        xb, Pb = gb.get_state(), gb.get_covariance()
        assert np.array_equal(ga.get_state(), xb) and np.array_equal(ga.get_covariance(), Pb), "step %d" % s
        for b in range(B):
            hist[(b, int(live[b]))] = (xb[b].copy(), Pb[b].copy())
    assert (ga.get_status() == gb.get_status()).all()
    # rewind: every filter to another slot of its own history (an index, no copy); the states are the ones recorded then
    back = np.array([sorted(sl for (bb, sl) in hist if bb == b)[0] for b in range(B)], dtype=np.int32)
    capi.check(L.viekf_batch_select_filters(ga._h, _p(back)))
    xa, Pa = ga.get_state(), ga.get_covariance()
    for b in range(B):
        # (slot 0 is overwritten only if the filter's ring wrapped: H = 6 > steps + 1, it did not)
        assert np.array_equal(xa[b], hist[(b, int(back[b]))][0]) and np.array_equal(Pa[b], hist[(b, int(back[b]))][1])
    capi.check(L.viekf_batch_select_filters(ga._h, _p(live)))
    # set_state on the per-filter slots: only what is given changes
    x_new = ga.get_state()
    x_new[:, 0] += 1.5
    ga.set_state(x=x_new)
    assert np.array_equal(ga.get_state(), x_new) and np.array_equal(ga.get_covariance(), Pb)
    # whole-batch ring calls are refused in this mode; leaving the ring brings every live state home
    assert L.viekf_batch_select(ga._h, 1) == capi.ERR_INVALID
    u = np.ascontiguousarray(sc["u"][0]); dt = np.ascontiguousarray(sc["dt"])
    assert L.viekf_batch_propagate_to(ga._h, _p(u), _p(dt), 1, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_batch_propagate_filters_to(ga._h, _p(u), _p(dt), _p(live), capi.HOST) == capi.ERR_INVALID   # (dst == live)
    ga.history_resize(0)
    assert np.array_equal(ga.get_state(), x_new) and np.array_equal(ga.get_covariance(), Pb)
    ga.propagate(u, dt); gb.set_state(x=x_new); gb.propagate(u, dt)
    assert np.array_equal(ga.get_state(), gb.get_state()) and np.array_equal(ga.get_covariance(), gb.get_covariance())


def test_propagate_filters_to_refuses_a_participation_mask():
    """viekf_batch_propagate_filters_to launches under a mask of its own (dst_slot[b] >= 0): a mask the caller set with
    viekf_batch_set_active would be ignored and a filter it masked out stepped anyway.  Refused like propagate_to: ERR_INVALID,
    and x, P, status and the live slot map are what they were; after set_active(NULL) the same call goes through."""
    B, N, H = 7, 6, 4
    sc = scene.make_scene(B, N, 2, seed=27)
    L = capi.lib()
    g = v.BatchVIEKF(B, N, sc["params"])
    for i in range(N):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    g.history_resize(H)
    for s in (2, 3):                                 # slots 2 and 3: the state before the step
        capi.check(L.viekf_batch_snapshot_filters(g._h, _p(np.full(B, s, dtype=np.int32)), capi.HOST))
    g.step(sc["u"][0], sc["dt"], sc["z"][0], sc["slot"], sc["R"])
    live = (np.arange(B) % 2).astype(np.int32)      # slots 0 and 1: the state after it, the live ones
    capi.check(L.viekf_batch_snapshot_filters(g._h, _p(live), capi.HOST))
    capi.check(L.viekf_batch_select_filters(g._h, _p(live)))
    dst = (live + 2).astype(np.int32)
    dst[3] = -1

    def read():
        """x, P, status of the live slots, and x, P of the destination slots (selected and selected back)"""
        out = [g.get_state(), g.get_covariance(), g.get_status()]
        capi.check(L.viekf_batch_select_filters(g._h, _p(dst)))
        out += [g.get_state(), g.get_covariance()]
        capi.check(L.viekf_batch_select_filters(g._h, _p(live)))
        return out

    before = read()
    assert not np.array_equal(before[0], before[3])
    mask = np.array([1, 0, 1, 1, 0, 1, 1], dtype=np.uint8)      # filters 1 and 4 masked out, with dst_slot >= 0
    capi.check(L.viekf_batch_set_active(g._h, _p(mask), capi.HOST))
    u, dt = np.ascontiguousarray(sc["u"][1]), np.ascontiguousarray(sc["dt"])
    assert L.viekf_batch_propagate_filters_to(g._h, _p(u), _p(dt), _p(dst), capi.HOST) == capi.ERR_INVALID
    capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
    after = read()
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    capi.check(L.viekf_batch_propagate_filters_to(g._h, _p(u), _p(dt), _p(dst), capi.HOST))
    x, P = g.get_state(), g.get_covariance()
    moved = dst >= 0
    assert np.array_equal(x[~moved], before[0][~moved]) and np.array_equal(P[~moved], before[1][~moved])
    assert all(not np.array_equal(x[b], before[0][b]) for b in np.flatnonzero(moved))
    # the moved filters now live in their destination slots: selecting the old live slots shows the states left there
    capi.check(L.viekf_batch_select_filters(g._h, _p(live)))
    assert np.array_equal(g.get_state(), before[0]) and np.array_equal(g.get_covariance(), before[1])
