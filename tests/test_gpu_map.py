"""The device-resident landmark map (include/viekf_map.h, vi_ekf_amd.LandmarkMap) against its restatement tests/map_ref.py by
the tolerance of tests/test_gpu_parity.py (max|d| <= 1e-9 max|ref| per array and 1e-6 element-wise, integers and the NaN
pattern exact) -- and against itself where the claim is bit for bit: device pointers against host pointers, the query on a
packed P against the query on the canonical one, a resumed store against the store it resumes, entries of features that are
no longer tracked.  The restatement is fed the device's own x, P, nodes and id tables: what is held to it here is the map's
geometry and its store rules; the intake has tests/test_gpu_frame.py and the node graph tests/test_gpu_node.py."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import map_ref as MR
from tests import sim_ref as R
from tests.test_frame_ref_cpu import SCRIPT
from tests.test_gpu_frame import RESIDENT, STREAMING, _batch, _params, frame, hover, noise, same_bits, script_frames, state
from tests.test_gpu_node import cuda, host, random_edges
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

LIVE = ("pos_node", "cov_node", "pos_global", "cov_global")
STORE = ("ids", "pos", "cov", "n_obs", "node_count")
ERR = ("err_node", "nees", "info", "err_global")
Q_B_C, P_B_C = np.asarray(orc.EKF_YAML["q_b_c"], float), np.asarray(orc.EKF_YAML["p_b_c"], float)


def close_nan(got, ref, what):
    """the NaN pattern exactly, the rest by assert_close"""
    got, ref = np.asarray(host(got)), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (what, np.isnan(got).sum(), np.isnan(ref).sum())
    m = ~np.isnan(ref)
    if m.any():
        assert_close(got[m], ref[m], what)


def bits(d, keys):
    return [host(d[k]) for k in keys]


def device_inputs(g, fi=None, ng=None):
    """what the restatement is fed: the device's own state, id table and nodes"""
    x, P, ln = state(g)
    tab, tl = fi.tracked() if fi is not None else (np.full((g.B, g.N), -1, np.int32), ln.copy())
    st = ng.get() if ng is not None else dict(node=None, true_node=None, count=None)
    return dict(x=x, P=P, ln=ln, tab=tab, tl=tl, node=st["node"], true_node=st["true_node"], count=st["count"])


def live_against_ref(mp, ref, d, what):
    out = mp.landmarks()
    rout = ref.landmarks(d["x"], d["P"], d["ln"], d["node"])
    for k in LIVE:
        close_nan(out[k], rout[k], "%s %s" % (what, k))
    for b in range(mp.batch.B):                              # slots past len are NaN in every output
        assert all(np.isnan(out[k][b, d["ln"][b]:]).all() for k in LIVE), (what, b)
    return out


def store_against_ref(mp, ref, what):
    st, rst = mp.get(), ref.get()
    for k in ("ids", "n_obs", "node_count"):
        assert np.array_equal(st[k], rst[k]), (what, k, st[k], rst[k])
    for k in ("pos", "cov"):
        assert np.array_equal(st[k][st["ids"] < 0], rst[k][rst["ids"] < 0]), (what, k)       # empty entries: zeros
        if (st["ids"] >= 0).any():
            assert_close(st[k][st["ids"] >= 0], rst[k][rst["ids"] >= 0], "%s store %s" % (what, k))
    return st


def error_against_ref(mp, ref, d, lm, fids, lmi, what, conv=None):
    conv = conv or (lambda a: a)
    err = mp.error(conv(lm), conv(fids), conv(lmi))
    rerr = ref.error(d["x"], d["P"], d["ln"], d["tab"], d["tl"], lm, fids, lmi, d["node"], d["true_node"])
    assert np.array_equal(host(err["info"]), rerr["info"]), (what, host(err["info"]), rerr["info"])
    for k in ("err_node", "nees", "err_global"):
        close_nan(err[k], rerr[k], "%s %s" % (what, k))
    return err


def field(rng, L):
    """a landmark field of the test's own and the landmark a feature id stands for"""
    return rng.normal(0.0, 3.0, (L, 3)), (lambda ids: np.where(ids >= 0, (ids * 7 + 3) % L, -1).astype(np.int32))


# ---- scripted frames ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [STREAMING, RESIDENT])
def test_scripted_frames_against_the_restatement(family):
    """B = 5, N = 8, M = 10, the twelve frames of test_frame_ref_cpu.SCRIPT with use_keyframe_reset on (resets at frames 2, 3,
    6, 8, 11; filter 3 sits two frames out) and three propagates before each.  After every frame the four live outputs, the
    store (capacity 16) and the error against the restatement; a map fed device pointers agrees bit for bit with one fed host
    pointers; entries of features that were dropped keep their bits across later frames and resets."""
    import vi_ekf_amd as v
    B, N, M, K, cap, L = 5, 8, 10, 3, 16, 40
    p = _params(use_keyframe_reset=True)
    g = _batch(B, N, p, family)
    fi, ng = v.FrameIntake(g), v.NodeGraph(g)
    mh, md, ref = v.LandmarkMap(g, fi, ng, cap), v.LandmarkMap(g, fi, ng, cap), MR.BatchMapRef(B, N, Q_B_C, P_B_C, cap)
    rng = np.random.default_rng(7)
    lm, lm_of = field(rng, L)
    Rm = noise(B, M, 2)
    resets = kept = 0
    for k, rows in enumerate(SCRIPT):
        u, dt = hover(K, B, 100 + k)
        g.step_n(u, dt, None, None, None)
        z, ids, depth = frame(rng, B, M, rows)
        active = np.ones(B, np.uint8)
        active[3] = k not in (2, 3)
        out = fi.intake(z, ids, Rm, depth=depth, active=active)
        xt = rng.normal(0.0, 1.0, (B, 12))
        xt[:, 6:10] /= np.linalg.norm(xt[:, 6:10], axis=1, keepdims=True)
        ng.update(out, x_true=xt)
        before = mh.get()
        mh.update()
        md.update()
        d = device_inputs(g, fi, ng)
        ref.update(d["x"], d["P"], d["ln"], d["tab"], d["tl"], d["node"], d["count"])
        what = "frame %d" % k
        live = live_against_ref(mh, ref, d, what)
        st = store_against_ref(mh, ref, what)
        err = error_against_ref(mh, ref, d, lm, ids, lm_of(ids), what)
        # device pointers: the same bits
        ld, sd = md.landmarks(device=True), md.get(device=True)
        ed = md.error(cuda(lm), cuda(ids), cuda(lm_of(ids)))
        assert all(t.is_cuda for t in list(ld.values()) + list(sd.values()) + list(ed.values()))
        assert same_bits(bits(ld, LIVE), bits(live, LIVE)) and same_bits(bits(sd, STORE), bits(st, STORE))
        assert same_bits(bits(ed, ERR), bits(err, ERR))
        # an entry whose feature is not tracked now keeps every bit
        for b in range(B):
            tracked = set(d["tab"][b, :d["ln"][b]].tolist())
            for e in range(cap):
                if before["ids"][b, e] >= 0 and before["ids"][b, e] not in tracked and st["ids"][b, e] == before["ids"][b, e]:
                    assert all(np.array_equal(st[key][b, e], before[key][b, e]) for key in STORE), (k, b, e)
                    kept += 1
            assert set(st["ids"][b][st["n_obs"][b] > before["n_obs"][b]].tolist()) <= tracked
        resets += int(out["did_reset"].sum())
    assert resets >= 15 and kept > 30
    st = mh.get()
    assert (st["ids"] >= 0).sum(axis=1).min() >= 10 and st["node_count"].max() >= 4 and st["n_obs"].max() >= 4
    assert g.get_status().max() < 8


# ---- tables wider than a wave, partially filled ------------------------------------------------------------------------------
@pytest.mark.parametrize("N,family", [(77, RESIDENT), (150, STREAMING), (300, STREAMING)])
def test_wide_partially_filled_tables(N, family):
    """B = 3 with len_features 0, 1 and N, N past one wave (N = 77: workgroups of 128), past two (N = 150: of 256) and past the
    largest workgroup (N = 300: the lanes loop): slots past len are NaN, a store smaller than N (capacity 64: ids 3 j + 5 share a residue 64 slots apart, three ways at N = 150),
    a landmark field per vehicle and a frame longer than the table"""
    import vi_ekf_amd as v
    B, cap, L, M = 3, 64, 300, N + 3
    p = _params(use_keyframe_reset=True)
    g = _batch(B, N, p, family)
    rng = np.random.default_rng(11)
    lens = [0, 1, N]
    tab = np.full((B, N), -1, np.int32)
    for j in range(N):
        px = np.stack([rng.uniform(40.0, 600.0, B), rng.uniform(40.0, 440.0, B)], axis=1)
        g.init_feature(px, np.full(B, 1.0 + 0.05 * j), np.array([j < n for n in lens], np.uint8))
    for b in range(B):
        tab[b, :lens[b]] = 3 * np.arange(lens[b]) + 5 + 1000 * b
    u, dt = hover(2, B, 3)
    g.step_n(u, dt, None, None, None)
    assert g.get_len_features().tolist() == lens
    fi = v.FrameIntake(g)
    fi.set_tracked(tab)
    mp, ref = v.LandmarkMap(g, fi, None, cap), MR.BatchMapRef(B, N, Q_B_C, P_B_C, cap)
    d = device_inputs(g, fi)
    live = live_against_ref(mp, ref, d, "wide")
    assert np.isnan(live["pos_node"][0]).all() and np.isnan(live["pos_node"][1, 1:]).all() and not np.isnan(live["cov_global"][2]).any()
    for k in range(2):
        mp.update()
        ref.update(d["x"], d["P"], d["ln"], d["tab"], d["tl"])
        st = store_against_ref(mp, ref, "wide store %d" % k)
    assert (st["ids"][0] == -1).all() and (st["ids"][1] >= 0).sum() == 1 and (st["ids"][2] >= 0).all()
    assert st["ids"][2].min() - 2005 == 3 * (N - cap) and st["n_obs"][2].tolist() == [2] * cap      # the larger ids hold the entries
    lm = rng.normal(0.0, 3.0, (B, L, 3))
    fids = np.full((B, M), -1, np.int32)
    for b in range(B):
        fids[b, :lens[b]] = tab[b, :lens[b]][::-1]
    lmi = np.where(fids >= 0, fids % (L + 20) - 10, -1).astype(np.int32)      # some below 0, some past L
    err = error_against_ref(mp, ref, d, lm, fids, lmi, "wide error")
    assert np.isnan(err["nees"][2]).sum() > 0 and np.isfinite(err["nees"][2]).sum() > N // 2


# ---- a packed P ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,inst", [(12, 0), (50, -1)])
def test_query_on_a_packed_P(N, inst):
    """B = 3, resident family.  A fused step_n leaves P PACKED (N = 12 on instance <2,1>, N = 50 on <3,7>): the query then and
    the query after get_covariance() agree bit for bit, with host and with device pointers, and with the restatement; x, the
    lower triangle of P, len_features and the status flags are what a twin batch that was never queried holds"""
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, M = 3, 6
    p = _params(use_keyframe_reset=True)
    rng = np.random.default_rng(31)
    z0, _, _ = frame(rng, B, N, list(range(N)), spread=0)
    u, dt = hover(4, B, 5)
    zs = np.stack([z0[:, j] + rng.normal(0.0, 0.5, (B, 2)) for j in range(M)], axis=1)
    slot = np.tile(np.arange(M, dtype=np.int32), (B, 1))
    ga, gb = _batch(B, N, p, RESIDENT), _batch(B, N, p, RESIDENT)
    for g in (ga, gb):
        if inst >= 0:
            g.set_tuning(capi.TUNE_RES_INSTANCE, inst)
        for j in range(N):
            g.init_feature(z0[:, j].copy(), np.full(B, np.nan))
        g.step_n(u, dt, zs, slot, noise(B, M, 0))
    assert "P packed" in ga.describe(), ga.describe()
    ng = v.NodeGraph(ga)
    for _ in range(2):                                       # the node away from the identity
        ng.update(np.ones(B, np.uint8), random_edges(rng, B))
    mp, ref = v.LandmarkMap(ga, None, ng), MR.BatchMapRef(B, N, Q_B_C, P_B_C)
    q1 = mp.landmarks()                                      # P as the launch left it
    qd = mp.landmarks(device=True)
    d = device_inputs(ga, None, ng)                          # (get_covariance: canonical from here on)
    status = ga.get_status()
    q2 = mp.landmarks()
    assert same_bits(bits(q1, LIVE), bits(q2, LIVE)) and same_bits(bits(qd, LIVE), bits(q1, LIVE))
    assert not np.isnan(q1["cov_global"]).any()
    xb, Pb, lb = state(gb)
    assert np.array_equal(d["x"], xb) and np.array_equal(np.tril(d["P"]), np.tril(Pb)) and np.array_equal(d["ln"], lb)
    assert np.array_equal(status, gb.get_status())
    live_against_ref(mp, ref, d, "packed")
    mp.update()                                              # capacity 0: legal, and nothing to do
    assert mp.get()["ids"].shape == (B, 0)


# ---- the store ---------------------------------------------------------------------------------------------------------------
def _tracked_batch(B, N, table, seed):
    """a batch whose filters hold the features of `table` ([B][N], -1 padded: the same length in every filter)"""
    import vi_ekf_amd as v
    g = _batch(B, N, _params(use_keyframe_reset=True))
    rng = np.random.default_rng(seed)
    n = int((table[0] >= 0).sum())
    for j in range(n):
        g.init_feature(np.stack([rng.uniform(60.0, 580.0, B), rng.uniform(60.0, 420.0, B)], axis=1), np.full(B, 2.0 + j))
    u, dt = hover(3, B, seed)
    g.step_n(u, dt, None, None, None)
    fi = v.FrameIntake(g)
    fi.set_tracked(table)
    return g, fi


def test_larger_id_wins_a_shared_residue():
    """capacity 4 with ids {1, 5, 9} in filter 0 (and {9, 5, 1}, {5, 9, 1} in the others: the order of the slots does not
    matter): entry 1 holds id 9 after each of three calls, with the same position and covariance bits, n_obs counting up; the
    other ids were not written"""
    import vi_ekf_amd as v
    B, N, cap = 3, 4, 4
    table = np.array([[1, 5, 9, -1], [9, 5, 1, -1], [5, 9, 1, -1]], np.int32)
    g, fi = _tracked_batch(B, N, table, 51)
    mp, ref = v.LandmarkMap(g, fi, None, cap), MR.BatchMapRef(B, N, Q_B_C, P_B_C, cap)
    d = device_inputs(g, fi)
    live = mp.landmarks()
    first = None
    for k in range(3):
        mp.update()
        ref.update(d["x"], d["P"], d["ln"], d["tab"], d["tl"])
        st = store_against_ref(mp, ref, "call %d" % k)
        assert st["ids"].tolist() == [[-1, 9, -1, -1]] * B and st["n_obs"].tolist() == [[0, k + 1, 0, 0]] * B
        first = first or st
        assert same_bits(bits(st, ("ids", "pos", "cov", "node_count")), bits(first, ("ids", "pos", "cov", "node_count")))
    for b in range(B):                                       # what is stored is the live query's global landmark of id 9's slot
        j = table[b].tolist().index(9)
        assert np.array_equal(st["pos"][b, 1], live["pos_global"][b, j]) and np.array_equal(st["cov"][b, 1], live["cov_global"][b, j])


def test_get_reset_set_resumes_bit_for_bit_and_a_stale_table_is_left_alone():
    import vi_ekf_amd as v
    B, N, cap = 3, 6, 4                                      # capacity < N
    t0 = np.array([[0, 1, 2, 3, 4, -1]] * B, np.int32) + np.array([[0], [10], [20]], np.int32) * (np.arange(N) < 5)
    g, fi = _tracked_batch(B, N, t0, 53)
    ma, mb = v.LandmarkMap(g, fi, None, cap), v.LandmarkMap(g, fi, None, cap)
    ref = MR.BatchMapRef(B, N, Q_B_C, P_B_C, cap)
    d = device_inputs(g, fi)
    for _ in range(2):
        ma.update()
        ref.update(d["x"], d["P"], d["ln"], d["tab"], d["tl"])
    saved = store_against_ref(ma, ref, "capacity < N")
    assert saved["ids"][0].tolist() == [4, 1, 2, 3]          # id 4 took id 0's entry
    t1 = t0.copy()
    t1[:, 0] = [7, 17, 27]                                    # another id in slot 0: its entry restarts
    fi.set_tracked(t1)
    mb.update()                                              # (something to forget)
    mb.reset()
    assert (mb.get()["ids"] == -1).all() and not mb.get()["pos"].any() and not mb.get()["n_obs"].any()
    mb.set(**saved)
    assert same_bits(bits(mb.get(), STORE), bits(saved, STORE))
    u, dt = hover(2, B, 54)
    g.step_n(u, dt, None, None, None)
    ma.update()
    mb.update()
    assert same_bits(bits(ma.get(), STORE), bits(mb.get(), STORE))
    st = ma.get()
    assert st["ids"][0].tolist() == [4, 1, 2, 7] and st["n_obs"][0].tolist() == [3, 3, 3, 1]
    mb.set(n_obs=np.full((B, cap), 9, np.int32))             # one array alone: the others keep every bit
    s2 = mb.get()
    assert (s2["n_obs"] == 9).all() and same_bits(bits(s2, ("ids", "pos", "cov", "node_count")), bits(st, ("ids", "pos", "cov", "node_count")))
    sd = ma.get(device=True)
    assert all(sd[k].is_cuda for k in STORE) and same_bits(bits(sd, STORE), bits(st, STORE))
    # a feature started behind the intake's back: the table is stale, the store keeps every bit and the error is NaN
    assert g.init_feature(np.tile([320.0, 240.0], (B, 1)), np.full(B, np.nan)).all()
    ma.update()
    assert same_bits(bits(ma.get(), STORE), bits(st, STORE))
    lm = np.zeros((8, 3))
    err = ma.error(lm, t1, np.where(t1 >= 0, 1, -1).astype(np.int32))
    assert np.isnan(err["err_node"]).all() and np.isnan(err["nees"]).all() and not err["info"].any()
    assert not np.isnan(ma.landmarks()["pos_node"][:, :N]).any()       # (the live query does not use the table)


# ---- the error ---------------------------------------------------------------------------------------------------------------
def test_error_of_the_true_state_is_zero():
    """B = 3, N = 8: the filter's state is set to the simulator's true state of the features the camera reports.  The landmark
    error is zero by assert_close's measure: l_true - err against l_true (1e-9 of the largest landmark coordinate; a landmark's z
    is exactly 0 and falls under the per-array bound).  A P9 that is not positive definite gives info naming the pivot and a NaN
    nees for that slot only; an id absent from the frame, or a landmark index outside the field, gives NaN and info 0."""
    import vi_ekf_amd as v
    B, N = 3, 8
    p = _params(use_keyframe_reset=True)
    per = {k: R.LOOP[k][:B] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    bs = v.BatchSimulator(B, p, max_features=N, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5, **per)
    lm = R.jittered_landmarks(77)
    bs.set_landmarks(lm)
    bs.step(40)
    z, ids, cnt, dep, lmi = bs.camera(N)
    assert cnt.min() >= 6, cnt
    g = _batch(B, N, p)
    g.set_state(x=np.nan_to_num(host(bs.truth_state(ids))), len_features=cnt)
    fi = v.FrameIntake(g)
    fi.set_tracked(ids)
    mp, ref = v.LandmarkMap(g, fi), MR.BatchMapRef(B, N, Q_B_C, P_B_C)
    err = mp.error(lm, ids, lmi)
    m = lmi >= 0                                             # (the slots the camera filled: the filters' features)
    assert np.array_equal(m, np.arange(N)[None, :] < cnt[:, None])
    lt = lm[np.maximum(lmi, 0)]
    assert_close((lt - err["err_node"])[m], lt[m], "err_node of the truth")
    assert_close((lt - err["err_global"])[m], lt[m], "err_global of the truth")
    assert not err["info"].any() and (err["nees"][m] < 1e-12).all() and np.isnan(err["nees"][~m]).all()
    assert_close(mp.landmarks()["pos_node"][m], lt[m], "l of the truth")
    nan0 = int(np.isnan(err["nees"]).sum())
    # not positive definite: filter 1, slot 2
    P = g.get_covariance()
    r = 16 + 3 * 2
    P[1, r + 1, r + 1] = -50.0
    g.set_state(P=P)
    d = device_inputs(g, fi)
    bad = mp.error(lm, ids, lmi)
    rbad = ref.error(d["x"], d["P"], d["ln"], d["tab"], d["tl"], lm, ids, lmi)
    assert bad["info"][1, 2] in (1, 2, 3) and np.array_equal(bad["info"], rbad["info"]) and np.count_nonzero(bad["info"]) == 1
    assert np.isnan(bad["nees"][1, 2]) and np.isnan(bad["nees"]).sum() == nan0 + 1
    assert np.array_equal(bad["err_node"], err["err_node"], equal_nan=True)
    assert np.array_equal(np.delete(bad["nees"].ravel(), N + 2), np.delete(err["nees"].ravel(), N + 2), equal_nan=True)
    # an id that is not in the frame, a landmark below 0 and one past the field
    f2, l2 = ids.copy(), lmi.copy()
    f2[0, list(ids[0]).index(d["tab"][0, 3])] = -1
    l2[1, list(ids[1]).index(d["tab"][1, 0])] = -1
    l2[2, list(ids[2]).index(d["tab"][2, 5])] = lm.shape[0]
    gone = mp.error(lm, f2, l2)
    for b, j in ((0, 3), (1, 0), (2, 5)):
        assert np.isnan(gone["err_node"][b, j]).all() and np.isnan(gone["err_global"][b, j]).all() and np.isnan(gone["nees"][b, j])
        assert gone["info"][b, j] == 0
    assert np.isnan(gone["err_node"]).sum() == 3 * nan0 + 9 and np.count_nonzero(gone["info"]) == 1


# ---- ring slots -------------------------------------------------------------------------------------------------------------
def test_per_filter_live_slots_are_followed():
    """B = 3 with a history ring and select_filters, a different slot per filter: the map reads the filters where they live
    (the batch's own buffers hold the state from before the frames)"""
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, N, M, cap = 3, 8, 10, 16
    p = _params(use_keyframe_reset=True)
    g = _batch(B, N, p)
    g.history_resize(4)
    live = np.array([2, 0, 3], np.int32)
    capi.check(capi.lib().viekf_batch_snapshot_filters(g._h, C.c_void_p(live.ctypes.data), capi.HOST))
    g.select_filters(live)
    fi, ng = v.FrameIntake(g), v.NodeGraph(g)
    mp, ref = v.LandmarkMap(g, fi, ng, cap), MR.BatchMapRef(B, N, Q_B_C, P_B_C, cap)
    lm, lm_of = field(np.random.default_rng(3), 30)
    filled = 0
    for k, (z, ids, depth, active, Rm) in enumerate(script_frames(B, N, M, 19, count=6)):
        out = fi.intake(z, ids, Rm, depth=depth, active=active)
        ng.update(out)
        mp.update()
        d = device_inputs(g, fi, ng)
        ref.update(d["x"], d["P"], d["ln"], d["tab"], d["tl"], d["node"], d["count"])
        out_live = live_against_ref(mp, ref, d, "frame %d" % k)
        store_against_ref(mp, ref, "frame %d" % k)
        error_against_ref(mp, ref, d, lm, ids, lm_of(ids), "frame %d" % k)
        filled += int((~np.isnan(out_live["pos_global"][:, :, 0])).sum())
    assert filled > 60 and (mp.get()["ids"] >= 0).sum() > 20


# ---- closed loop ----------------------------------------------------------------------------------------------------------
def test_closed_loop_with_nothing_crossing_to_the_host():
    """sim_ref.LOOP, B = 4, N = 8, 2 s at 250 / 25 Hz with use_keyframe_reset on: BatchSimulator.step -> step_n -> camera ->
    FrameIntake.intake -> NodeGraph.update -> LandmarkMap.update -> LandmarkMap.error, every array between the calls a CUDA
    tensor.  On every frame the device's error and store agree with the restatement fed the device's own state; after t = 1 s
    the worst |err_node| over features whose store entry has n_obs >= 5 stays inside map_ref.LOOP_MAP_BOUND = 2.75 m, twice the
    1.375 m the restated stack measures on the CPU (tests/test_map_ref_cpu.py)."""
    import torch
    import vi_ekf_amd as v
    B, N, cap = 4, MR.LOOP_MAP_N, MR.LOOP_MAP_CAPACITY
    p = MR.loop_map_params()
    per = {k: R.LOOP[k] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    bs = v.BatchSimulator(B, p, max_features=N, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5, **per)
    lm = R.jittered_landmarks(77)
    bs.set_landmarks(lm)
    lm_dev = cuda(lm)
    g = v.BatchVIEKF(B, N, dict(p, name="map"))
    fi, ng = v.FrameIntake(g), v.NodeGraph(g)
    mp, ref = v.LandmarkMap(g, fi, ng, cap), MR.BatchMapRef(B, N, p["q_b_c"], p["p_b_c"], cap)
    R_pix = torch.diag(torch.tensor([10.0, 10.0], dtype=torch.float64)).cuda()
    dt = torch.full((10, B), bs.dt, dtype=torch.float64, device="cuda")
    worst, counted = np.zeros(B), 0
    for f in range(int(round(MR.LOOP_MAP_TMAX * 25))):
        u = bs.step(10, device=True)
        g.step_n(u, dt, None, None, None)
        z, ids, cnt, dep, lmk = bs.camera(N, device=True)
        out = fi.intake(z, ids, R_pix)
        tracked, _ = fi.tracked(device=True)
        ng.update(out, x_true=bs.truth_state(tracked))
        mp.update()
        err = mp.error(lm_dev, ids, lmk)
        st = mp.get(device=True)
        assert u.is_cuda and z.is_cuda and lmk.is_cuda and all(err[k].is_cuda for k in ERR) and all(st[k].is_cuda for k in STORE)
        # the test's own look at the results, not part of the loop
        d = device_inputs(g, fi, ng)
        ref.update(d["x"], d["P"], d["ln"], d["tab"], d["tl"], d["node"], d["count"])
        store_against_ref(mp, ref, "frame %d" % f)
        rerr = ref.error(d["x"], d["P"], d["ln"], d["tab"], d["tl"], lm, host(ids), host(lmk), d["node"], d["true_node"])
        assert np.array_equal(host(err["info"]), rerr["info"]) and not rerr["info"].any(), f
        for k in ("err_node", "nees", "err_global"):
            close_nan(err[k], rerr[k], "frame %d %s" % (f, k))
        if bs.t > 1.0:
            e, sid, nobs = host(err["err_node"]), host(st["ids"]), host(st["n_obs"])
            for b in range(B):
                for j in range(d["ln"][b]):
                    at = d["tab"][b, j] % cap
                    if sid[b, at] == d["tab"][b, j] and nobs[b, at] >= MR.LOOP_MAP_MIN_OBS:
                        assert not np.isnan(e[b, j]).any(), (f, b, j)
                        worst[b] = max(worst[b], np.abs(e[b, j]).max())
                        counted += 1
    print("closed loop with a map, worst |err_node| after t = 1 s over n_obs >= %d: %s m (%d slot-frames); bound %.3f"
          % (MR.LOOP_MAP_MIN_OBS, np.round(worst, 4), counted, MR.LOOP_MAP_BOUND))
    assert counted > 4 * 50 and (worst > 0).all()
    assert (worst < MR.LOOP_MAP_BOUND).all(), (worst, MR.LOOP_MAP_BOUND)
    assert g.get_status().max() < 8 and (host(mp.get()["ids"]) >= 0).sum(axis=1).min() >= N


# ---- argument rules -------------------------------------------------------------------------------------------------------
def test_argument_rules():
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, map as vmap
    B, N = 2, 4
    g, g2 = _batch(B, N, _params()), _batch(B, N, _params())
    fi, ng, fi2, ng2 = v.FrameIntake(g), v.NodeGraph(g), v.FrameIntake(g2), v.NodeGraph(g2)
    for bad in (-1, 4097):
        with pytest.raises(v.ViekfError) as e:
            v.LandmarkMap(g, fi, ng, bad)
        assert e.value.code == capi.ERR_INVALID and "4096" in str(e.value)
    with pytest.raises(v.ViekfError) as e:                   # a store needs the intake's id table
        v.LandmarkMap(g, None, ng, 8)
    assert e.value.code == capi.ERR_INVALID and "frame intake" in str(e.value)
    for kw in (dict(frame=fi2), dict(node=ng2), dict(frame=fi2, node=ng)):
        with pytest.raises(v.ViekfError) as e:
            v.LandmarkMap(g, **kw)
        assert e.value.code == capi.ERR_INVALID and "another batch" in str(e.value)
    v.LandmarkMap(g, fi, ng, 4096).close()
    mp, m0 = v.LandmarkMap(g, fi, ng, 4), v.LandmarkMap(g)
    L, h = vmap._bind(), mp._h
    buf = np.zeros((B, N, 6))
    ptr = C.c_void_p(buf.ctypes.data)
    ibuf = np.zeros((B, 8), np.int32)
    iptr = C.c_void_p(ibuf.ctypes.data)
    assert L.viekf_map_create(g._h, None, None, 0, None) == capi.ERR_INVALID
    assert L.viekf_map_landmarks(h, None, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert b"at least one" in L.viekf_last_error()
    assert L.viekf_map_landmarks(h, ptr, None, None, None, 7) == capi.ERR_INVALID
    assert L.viekf_map_landmarks(h, None, None, None, ptr, capi.HOST) == capi.OK          # any one output is enough
    assert L.viekf_map_get(h, None, None, None, None, None, 7) == capi.ERR_INVALID
    assert L.viekf_map_get(h, None, None, None, None, None, capi.HOST) == capi.OK         # NULL skips an array: all five
    for M in (0, -3, 4097):
        assert L.viekf_map_error(h, ptr, 0, 4, iptr, iptr, M, ptr, None, None, None, capi.HOST) == capi.ERR_INVALID
        assert b"4096" in L.viekf_last_error()
    assert L.viekf_map_error(h, ptr, 0, 4, iptr, iptr, 8, None, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_map_error(h, None, 0, 4, iptr, iptr, 8, ptr, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_map_error(h, ptr, 0, 0, iptr, iptr, 8, ptr, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_map_error(h, ptr, 0, 4, iptr, iptr, 8, ptr, None, None, None, 7) == capi.ERR_INVALID
    assert L.viekf_map_error(h, ptr, 0, 4, iptr, iptr, 8, ptr, None, None, None, capi.HOST) == capi.OK
    assert L.viekf_map_error(m0._h, ptr, 0, 4, iptr, iptr, 8, ptr, None, None, None, capi.HOST) == capi.ERR_INVALID      # no intake
    assert b"frame intake" in L.viekf_last_error()
    only = mp.landmarks(want=("pos_global",))
    assert list(only) == ["pos_global"] and only["pos_global"].shape == (B, N, 3)
    assert m0.get()["ids"].shape == (B, 0) and m0.landmarks()["cov_node"].shape == (B, N, 6)
    lm = np.zeros((5, 3))
    with pytest.raises(ValueError, match="mix"):
        mp.error(cuda(lm), ibuf, ibuf)
    with pytest.raises(ValueError, match="mix"):
        mp.set(ids=np.zeros((B, 4), np.int32), n_obs=torch.zeros((B, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        mp.error(lm, ibuf, ibuf[:, :7])
    with pytest.raises(ValueError, match="shape"):
        mp.error(np.zeros((B + 1, 5, 3)), ibuf, ibuf)
    with pytest.raises(ValueError, match="shape"):
        mp.set(pos=np.zeros((B, 4, 6)))
    with pytest.raises(ValueError, match="lm_true"):
        mp.error(np.zeros(3), ibuf, ibuf)
    # a participation mask is ignored: every call is read-only on the batch
    mask = np.array([1, 0], np.uint8)
    capi.check(capi.lib().viekf_batch_set_active(g._h, C.c_void_p(mask.ctypes.data), capi.HOST))
    assert mp.landmarks()["pos_node"].shape == (B, N, 3) and L.viekf_map_update(h) == capi.OK
    capi.check(capi.lib().viekf_batch_set_active(g._h, None, capi.HOST))
    # a destroyed batch: the map refuses to go on, and its own tables can still be released
    g.close()
    with pytest.raises(ValueError, match="closed"):
        mp.landmarks()
    with pytest.raises(ValueError, match="closed"):
        v.LandmarkMap(g)
    mp.close()
    with pytest.raises(ValueError, match="closed"):
        mp.get()
