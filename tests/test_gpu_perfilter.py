"""Per-filter parameter sets on the GPU (viekf_batch_set_params_filters / BatchVIEKF.set_params): one batch whose filters have a
camera, extrinsics, noise and start state each equals, bit for bit, the batches of one created with those sets, and the oracle
run with them, through every kernel family; the shared set is bit for bit what it was; reset, getters and the drag switch;
the modules that read the set through the batch; the ring routes and the sequencer; the refusals.
The cases and their conditions: tests/perfilter_cases.py, tests/test_perfilter_cases_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from tests import hetero_cases as hc
from tests import perfilter_cases as pc
from tests.test_gpu_parity import assert_close
from vi_ekf_amd import capi

pytestmark = pytest.mark.gpu

NAN = float("nan")
# id -> (N, B, nonunit, kernel family of set_kernel, tunings, what describe() must name, what it must not)
CONFIGS = {
    "N3-stream": (3, 3, None, 1, (), ("k_propagate_",), ("k_step_resident",)),
    "N3-resident": (3, 3, None, 2, (), ("k_step_resident",), ()),
    "N12": (12, 5, None, 0, (), ("k_step_resident",), ()),
    "N50-zu": (50, 4, None, 0, (("TUNE_RES_INSTANCE", 6),), ("k_step_resident<7,3> ZU",), ()),
    "N50-general": (50, 4, 2, 0, (("TUNE_RES_INSTANCE", 6),), ("k_step_resident<7,3>",), (" ZU",)),
    "N77-two-service-waves": (77, 3, None, 0, (), ("k_step_resident<8,6>", "2 service waves"), ()),
    "N90-wide": (90, 3, None, 0, (), ("k_propagate_wide", "k_update_feat_panelsvc"), ()),
    "N48-tiles-single": (48, 5, None, 0, (("TUNE_TILES", 2),), ("k_step_tiles<",), ()),
    "N48-tiles-pair": (48, 5, None, 0, (("TUNE_TILES", 3),), ("k_step_tiles_pair",), ()),
}
ORACLE_CONFIGS = ("N3-stream", "N3-resident", "N12", "N50-zu", "N50-general", "N90-wide")
_RUNS = {}


def _configure(g, kernel, tunings):
    for key, val in tunings:
        g.set_tuning(getattr(capi, key), val)
    if kernel:
        g.set_kernel(kernel)


def _make(c, kernel=0, tunings=(), rows=None):
    """the batch of case c (or of its filters `rows`), every filter on its own set and at its own x0 / P0"""
    params = c["params"] if rows is None else [c["params"][b] for b in rows]
    g = v.BatchVIEKF(len(params), c["N"], list(params))
    _configure(g, kernel, tunings)
    return g


def _script(g, c):
    """the script of tests/perfilter_cases.py on the batch g -> everything the calls return and the final state"""
    B, N, nf = g.B, c["N"], c["nf"]
    o = dict(x0=g.get_state(), P0=g.get_covariance())
    for i in range(nf):
        assert (g.init_feature(c["pix"][:, i, :].copy(), np.full(B, NAN)) == 1).all()
    o["A"] = g.step_n(c["u"][0:2], c["dtA"], c["zA"], c["slotA"], c["R"]).copy()
    o["B"] = g.step_n(c["u"][2:4], c["dtB"], c["zB"], c["slotB"], c["R"]).copy()
    o["body"] = g.update_body(c["body"])[0].T.copy()
    o["depth"] = g.update_depths(orc.DEPTH, c["dz"], c["dslot"], c["dR"])[0].copy()
    o["pixvel"] = g.update_pixel_vels(c["pz"], c["pslot"], c["gyro"], c["pR"])[0].copy()
    o["init"] = g.init_feature(c["pix"][:, N - 1, :].copy(), np.full(B, NAN)).reshape(B, 1).copy()
    o["len_kept"] = g.keep_features(c["keep"]).copy()
    o["edge"] = g.keyframe_reset()
    g.propagate(c["u"][4], c["dt"])
    o.update(x=g.get_state(), P=g.get_covariance(), len=g.get_len_features(), status=g.get_status())
    return o


def _same(got, ref, b, what):
    """filter 0 of a batch of one against filter b of the mixed batch, bit for bit (NaNs in the same places)"""
    for k in ref:
        assert np.array_equal(got[k][0], ref[k][b], equal_nan=True), "%s, filter %d: %s differs" % (what, b, k)


def _mixed(name):
    if name not in _RUNS:
        N, B, nonunit, kernel, tunings, names, absent = CONFIGS[name]
        c = pc.case(N, B, nonunit)
        g = _make(c, kernel, tunings)
        d = g.describe()
        assert all(s in d for s in names) and not any(s in d for s in absent), d
        _RUNS[name] = (c, d, _script(g, c))
        g.close()
    return _RUNS[name]


def _ones_tunings(mixed_describe, tunings):
    """a batch of one gets the mixed batch's kernels: never the unit-Lambda instances where the mixed batch cannot use them"""
    if "k_step_resident" in mixed_describe and " ZU" not in mixed_describe:
        return tuple(tunings) + (("TUNE_UNIT_LAMBDA", 0),)
    return tuple(tunings)


# ---- 1. one batch with B sets == B batches of one --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_mixed_batch_equals_batches_of_one(name):
    N, B, nonunit, kernel, tunings, names, absent = CONFIGS[name]
    c, d, mixed = _mixed(name)
    for b in range(B):
        g1 = _make(c, kernel, _ones_tunings(d, tunings), rows=[b])
        assert g1.describe() == d, (g1.describe(), d)
        _same(_script(g1, pc.one(c, b)), mixed, b, name)
        g1.close()
    assert (mixed["status"] == 0).all()


def test_large_batch_filters_beyond_256():
    """B = 300 > 256: an index kept in eight bits, or a set read at b mod 256, shows at filters 255 / 256 / 299"""
    c = pc.tiled(pc.case(12, 5), 300)
    g = _make(c)
    d = g.describe()
    row = [i for i in range(len(hc.res_rows())) if hc.row_name(i) in d]
    assert len(row) == 1, d
    mixed = _script(g, c)
    g.close()
    for b in (0, 1, 255, 256, 299):
        g1 = _make(c, 0, (("TUNE_RES_INSTANCE", row[0]),), rows=[b])      # (the instance a batch of 300 gets, not a batch of one's)
        assert g1.describe() == d
        _same(_script(g1, pc.one(c, b)), mixed, b, "B = 300")
        g1.close()


# ---- 2. against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ORACLE_CONFIGS)
def test_mixed_batch_against_the_oracle(name):
    c, d, o = _mixed(name)
    for k in ("A", "B", "body", "depth", "pixvel", "init"):
        assert np.array_equal(o[k], c["codes"][k]), k
    assert np.array_equal(o["len"], c["len_ref"]) and np.array_equal(o["len_kept"], c["len_kept"])
    assert np.array_equal(o["x0"], c["x0_ref"]) and np.array_equal(o["P0"], c["P0_ref"])
    assert_close(o["x"], c["x_ref"], "x")
    assert_close(o["P"], c["P_ref"], "P")
    assert_close(o["edge"], c["edge_ref"], "edge")
    assert (o["status"] == 0).all()


# ---- 3. nothing changes for the shared set ---------------------------------------------------------------------------------
@pytest.mark.parametrize("N,tunings", [(50, (("TUNE_RES_INSTANCE", 6),)), (90, ())])
def test_shared_set_is_bit_for_bit_what_it_was(N, tunings):
    """B copies of the creation set, and then NULL, between two step_n calls (N = 50: P is packed there)"""
    c = pc.case(N, 4 if N == 50 else 3)
    B = c["B"]
    shared = c["params"][1]
    outs, descs = [], []
    for mode in ("never", "copies", "copies-then-null"):
        g = v.BatchVIEKF(B, N, shared)
        _configure(g, 0, tunings)
        descs.append([g.describe()])
        for i in range(c["nf"]):
            g.init_feature(c["pix"][:, i, :].copy(), np.full(B, NAN))
        rA = g.step_n(c["u"][0:2], c["dtA"], c["zA"], c["slotA"], c["R"]).copy()
        if N == 50:
            assert "P packed" in g.describe()
        if mode != "never":
            g.set_params([shared] * B)
        if mode == "copies-then-null":
            g.set_params(None)
        descs[-1].append(g.describe())
        rB = g.step_n(c["u"][2:4], c["dtB"], c["zB"], c["slotB"], c["R"]).copy()
        g.propagate(c["u"][4], c["dt"])
        outs.append(dict(A=rA, B=rB, x=g.get_state(), P=g.get_covariance(), len=g.get_len_features(), status=g.get_status()))
        g.close()
    for o, d in zip(outs[1:], descs[1:]):
        assert d == descs[0], (d, descs[0])
        for k in outs[0]:
            assert np.array_equal(o[k], outs[0][k]), k


# ---- 4. reset, getters, drag switch ------------------------------------------------------------------------------------------
def _assert_params_equal(got, want):
    want = capi.Params.from_dict(want).to_dict() if isinstance(want, dict) else want.to_dict()
    got = got.to_dict()
    for k in capi.Params.ARRAYS:
        assert np.array_equal(got[k], want[k]), k
    for k in capi.Params.SCALARS:
        assert got[k] == want[k], k


def test_reset_and_getters():
    c = pc.case(12, 5)
    B, N = c["B"], c["N"]
    g = v.BatchVIEKF(B, N, c["params"][0])
    g.set_params(c["params"])
    # the live state is not touched by the call ...
    assert np.array_equal(g.get_state(), np.tile(c["x0_ref"][0], (B, 1)))
    g.step_n(c["u"][0:2], c["dtA"], None, None, None)
    g.reset()                                   # ... the next reset puts filter b at its own x0 and diag(P0 | P0_feat ...)
    assert np.array_equal(g.get_state(), c["x0_ref"]) and np.array_equal(g.get_covariance(), c["P0_ref"])
    assert (g.get_len_features() == 0).all() and (g.get_status() == 0).all()
    for b in range(B):
        _assert_params_equal(g.params_of(b), c["params"][b])
    created = capi.Params()
    capi.check(capi.lib().viekf_batch_get_params(g._h, C.byref(created)))
    _assert_params_equal(created, c["params"][0])
    g.set_params(None)                          # back to the creation set: getter and reset follow
    for b in range(B):
        _assert_params_equal(g.params_of(b), c["params"][0])
    g.reset()
    assert np.array_equal(g.get_state(), np.tile(c["x0_ref"][0], (B, 1)))
    g.close()
    # the list form of the constructor: created with entry 0, given the list, reset
    g = v.BatchVIEKF(B, N, c["params"])
    assert np.array_equal(g.get_state(), c["x0_ref"]) and np.array_equal(g.get_covariance(), c["P0_ref"])
    g.close()


def test_drag_switch_reaches_every_filter():
    """sets with the drag term off, switched on at run time: ACC then has zdim = 2 and every filter's set must say so"""
    c = pc.case(12, 5)
    B, N = c["B"], c["N"]
    off = [dict(p, use_drag_term=False) for p in c["params"]]

    def run(g, cc):
        g.set_drag_term(1)
        for i in range(cc["nf"]):
            g.init_feature(cc["pix"][:, i, :].copy(), np.full(g.B, NAN))
        rA = g.step_n(cc["u"][0:2], cc["dtA"], cc["zA"], cc["slotA"], cc["R"]).copy()
        rb = g.update_body(cc["body"][:1])[0].T.copy()          # ACC, z [B][2]
        g.propagate(cc["u"][4], cc["dt"])                       # (the drag term of the dynamics)
        return dict(A=rA, body=rb, x=g.get_state(), P=g.get_covariance())

    g = v.BatchVIEKF(B, N, off)
    mixed = run(g, c)
    assert all(g.params_of(b).use_drag_term == 1 for b in range(B))
    assert (mixed["body"] == 0).all()
    g.close()
    for b in range(B):
        g1 = v.BatchVIEKF(1, N, off[b])
        _same(run(g1, pc.one(c, b)), mixed, b, "drag switch")
        g1.close()


# ---- 5. the modules that read the set through the batch ------------------------------------------------------------------------
def _module_outputs(g, c):
    """frame intake with new features, the landmark map's live query, the innovation and the read-only hooks on the batch g"""
    B, N = g.B, c["N"]
    L = capi.lib()
    o = {}
    fi = v.FrameIntake(g)
    M = 5
    ids = np.tile(np.arange(M, dtype=np.int32), (B, 1))
    out = fi.intake(np.ascontiguousarray(c["pix"][:, :M, :]), ids, c["R"])          # every id is new: init_features
    o["intake_result"], o["tracked"] = out["result"], fi.tracked()[0]
    g.step_n(c["u"][0:2], c["dtA"], np.ascontiguousarray(c["pix"][:, :M, :] + 0.3), ids, c["R"])
    lm = v.LandmarkMap(g, fi, None, 16)
    live = lm.landmarks(want=("pos_node", "cov_node"))
    o["lm_pos"], o["lm_cov"] = live["pos_node"], live["cov_node"]
    slot = np.full(B, 2, dtype=np.int32)
    inn = v.innovation(g, orc.FEAT, np.ascontiguousarray(c["pix"][:, 2, :] + 1.0), c["R"], slot=slot)
    o["nis"], o["residual"], o["S"] = inn["nis"], inn["residual"], inn["S"]
    o["h_feat"] = g.eval_h(orc.FEAT, slot)
    o["h_acc"] = g.eval_h(orc.ACC)
    n = g.n
    xdot, A, G = np.zeros((B, n)), np.zeros((B, n, n)), np.zeros((B, 6, n))
    u = np.ascontiguousarray(c["u"][4])
    p = lambda a: C.c_void_p(a.ctypes.data)
    capi.check(L.viekf_batch_eval_jacobians(g._h, None, p(u), p(xdot), p(A), p(G), capi.HOST))
    o["xdot"], o["A"], o["G"] = xdot, A, G
    o["xdot_hook"] = g.eval_xdot(u)             # (rotates u by the filter's q_b_u)
    o["x"], o["P"] = g.get_state(), g.get_covariance()
    del lm, fi
    return o


def test_modules_that_read_the_set_through_the_batch():
    N, B = 8, 4
    c, _ = pc.inputs(N, B)
    g = _make(c)
    mixed = _module_outputs(g, c)
    g.close()
    assert (mixed["tracked"][:, :5] == np.arange(5)).all() and np.isfinite(mixed["lm_pos"][:, :5]).all()
    for b in range(B):
        g1 = _make(c, rows=[b])
        _same(_module_outputs(g1, pc.one(c, b)), mixed, b, "modules")
        g1.close()
    for k in ("lm_pos", "nis", "h_feat", "xdot", "xdot_hook"):      # (the sets differ: so do these)
        assert not np.array_equal(mixed[k][1], mixed[k][0], equal_nan=True), k


# ---- 6. ring routes and the sequencer ------------------------------------------------------------------------------------------
def _ring_route(g, c, n_route, live, kc):
    """per-filter live slots: filter b starts at ring position live[b] and steps through positions of its own"""
    B = g.B
    L = capi.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    for i in range(c["nf"]):
        g.init_feature(c["pix"][:, i, :].copy(), np.full(B, NAN))
    g.history_resize(4)
    live = np.asarray(live, dtype=np.int32)
    capi.check(L.viekf_batch_snapshot_filters(g._h, p(live), capi.HOST))
    g.select_filters(live)
    g.set_params(c["params"])                   # (legal under select_filters: the sets are no part of a ring slot)
    res = []
    if n_route:
        dst = ((live + 2) % 4).astype(np.int32)
        g.propagate_n_filters_to(np.ascontiguousarray(c["u"][0:2]), c["dtA"], np.asarray(kc, dtype=np.int32), dst)
        live = dst
    for k in (2, 3):
        dst = ((live + 1) % 4).astype(np.int32)
        u, dt = np.ascontiguousarray(c["u"][k]), np.ascontiguousarray(c["dtB"][k - 2])
        capi.check(L.viekf_batch_propagate_filters_to(g._h, p(u), p(dt), p(dst), capi.HOST))
        live = dst
        res.append(g.update_feat(c["zA" if k == 2 else "zB"], c["slotA" if k == 2 else "slotB"], c["R"]).copy())
    return dict(rA=res[0], rB=res[1], x=g.get_state(), P=g.get_covariance(), len=g.get_len_features(), status=g.get_status())


@pytest.mark.parametrize("n_route", [False, True])
def test_per_filter_live_slots_with_distinct_sets(n_route):
    """select_filters, propagate_filters_to and (n_route) propagate_n_filters_to with one or two propagates per filter"""
    c3 = pc.tiled_rows(pc.case(12, 5), [0, 1, 2])
    live, kc = [0, 1, 2], [1, 2, 1]
    g = v.BatchVIEKF(3, 12, c3["params"])
    mixed = _ring_route(g, c3, n_route, live, kc)
    g.close()
    assert (mixed["status"] == 0).all() and (mixed["rA"] == 0).all()
    for b in range(3):
        c1 = pc.one(c3, b)
        g1 = v.BatchVIEKF(1, 12, c1["params"])
        _same(_ring_route(g1, c1, n_route, [live[b]], [kc[b]]), mixed, b, "ring route")
        g1.close()


def test_independent_sequencer_over_three_sets():
    """delayed frames, so that every filter rewinds and replays its stored inputs -- rotated on the host by ITS q_b_u"""
    from tests.test_gpu_sequencer import _feed
    N, steps = 5, 20
    base = dict(orc.EKF_YAML, keyframe_overlap_threshold=0.8)
    sets = [pc.draw(base, b) for b in range(3)]
    sources = [dict(seed=41, clock0=0.0, dt_imu=0.004, delay=0.011, alt_every=0),
               dict(seed=42, clock0=500.0, dt_imu=0.005, delay=0.03, alt_every=7),
               dict(seed=43, clock0=-20.0, dt_imu=0.004, delay=0.0105, alt_every=0)]
    g = v.BatchVIEKF(3, N, sets)
    sg = v.SeqVIEKF(g, state_hist=32, meas_hist=64, independent=True)
    gens = [_feed(sg, [b], 3, N, steps=steps, **src) for b, src in enumerate(sources)]
    live = list(range(3))
    while live:
        for b in list(live):
            try:
                if next(gens[b])[0] == "frame":
                    sg.handle_measurements()
            except StopIteration:
                live.remove(b)
    x_all, P_all, tracked = g.get_state(), g.get_covariance(), sg.tracked_features()
    assert not np.array_equal(x_all[0], x_all[1])
    for b, src in enumerate(sources):
        g1 = v.BatchVIEKF(1, N, sets[b])
        s1 = v.SeqVIEKF(g1, state_hist=32, meas_hist=64, independent=True)
        for ev in _feed(s1, [0], 1, N, steps=steps, **src):
            if ev[0] == "frame":
                s1.handle_measurements()
        assert np.array_equal(g1.get_state()[0], x_all[b]), "filter %d: state differs from its own sequencer of one" % b
        assert np.array_equal(g1.get_covariance()[0], P_all[b]), "filter %d: covariance differs" % b
        assert s1.tracked_features()[0] == tracked[b]
        del s1
        g1.close()
    del sg
    g.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_batch_unchanged():
    c = pc.case(12, 5)
    B, N = c["B"], c["N"]
    L = capi.lib()
    g = v.BatchVIEKF(B, N, c["params"])
    for i in range(c["nf"]):
        g.init_feature(c["pix"][:, i, :].copy(), np.full(B, NAN))
    g.step_n(c["u"][0:2], c["dtA"], c["zA"], c["slotA"], c["R"])

    def snapshot():
        sets = [g.params_of(b).to_dict() for b in range(B)]
        flat = np.array([np.concatenate([np.ravel(d[k]) for k in capi.Params.ARRAYS + capi.Params.SCALARS]) for d in sets])
        return (g.get_state(), g.get_covariance(), g.get_len_features(), g.get_status(), g.describe(), flat)

    def unchanged(before):
        now = snapshot()
        return all(np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b for a, b in zip(before, now))

    before = snapshot()
    kot = capi.Params.from_dict(c["params"][0]).keyframe_overlap_threshold
    for field in ("use_drag_term", "use_partial_update", "use_keyframe_reset", "keyframe_overlap_threshold"):
        bad = [dict(p) for p in c["params"]]
        bad[3][field] = 0.5 * kot if field == "keyframe_overlap_threshold" else not c["params"][0][field]
        with pytest.raises(v.ViekfError) as e:
            g.set_params(bad)
        assert e.value.code == capi.ERR_INVALID and "filter 3" in str(e.value) and field in str(e.value), str(e.value)
        assert unchanged(before)
    # the structural fields follow the run-time drag switch: the CURRENT value is the batch's
    g.set_drag_term(0)
    with pytest.raises(v.ViekfError) as e:
        g.set_params(c["params"])
    assert e.value.code == capi.ERR_INVALID and "use_drag_term" in str(e.value)
    g.set_params([dict(p, use_drag_term=False) for p in c["params"]])
    g.set_drag_term(1)
    assert unchanged(before)
    out = capi.Params()
    for filt in (-1, B, B + 1000):
        assert L.viekf_batch_get_params_filter(g._h, filt, C.byref(out)) == capi.ERR_INVALID
        assert b"range" in L.viekf_last_error()
    assert L.viekf_batch_get_params_filter(g._h, 0, None) == capi.ERR_INVALID
    arr = (capi.Params * B)(*[capi.Params.from_dict(p) for p in c["params"]])
    assert L.viekf_batch_set_params_filters(None, arr) == capi.ERR_INVALID
    assert L.viekf_batch_get_params_filter(None, 0, C.byref(out)) == capi.ERR_INVALID
    with pytest.raises(ValueError):
        g.set_params(c["params"][:B - 1])
    assert unchanged(before)
    # ... and the batch goes on as one that was never refused anything
    rB = g.step_n(c["u"][2:4], c["dtB"], c["zB"], c["slotB"], c["R"]).copy()
    ref = v.BatchVIEKF(B, N, c["params"])
    for i in range(c["nf"]):
        ref.init_feature(c["pix"][:, i, :].copy(), np.full(B, NAN))
    ref.step_n(c["u"][0:2], c["dtA"], c["zA"], c["slotA"], c["R"])
    assert np.array_equal(rB, ref.step_n(c["u"][2:4], c["dtB"], c["zB"], c["slotB"], c["R"]))
    assert np.array_equal(g.get_state(), ref.get_state()) and np.array_equal(g.get_covariance(), ref.get_covariance())
    ref.close()
    g.close()
