"""GPU parity at the BASELINE batch sizes: filters of EVERY dispatch round against the oracle.

The small parity tests (tests/test_gpu_parity.py, B <= 12) only ever exercise the first workgroup
that lands on a CU.  The headline runs 1024 workgroups over 256 CUs (four rounds; a later workgroup
starts on LDS / registers that still hold a previous filter's data), and the two- and four-per-CU
instances <2,1>, <2,2> and <3,2> are only picked when the batch exceeds the CU count.  Here the HIP path runs the full batch
and a strided sample of filters -- first, last and the ones either side of a round boundary -- is
compared with the CPU oracle on the same seeded inputs, with the same bar as test_gpu_parity.py.

Reference behaviour compared: propagate (vi_ekf.cpp:262-318) + N sequential FEAT updates
(vi_ekf_meas.cpp:196-278) per step.
"""
import os

import numpy as np
import pytest

import vi_ekf_amd as v
from oracle import oracle as orc
from vi_ekf_amd import scene
from tests import hetero_cases as hc
from tests.test_gpu_parity import assert_close, oracle_params

pytestmark = pytest.mark.gpu


def oracle_subset(sc, N, steps, which):
    """the oracle on filters `which` of the scene, all host threads -> x, P, res [len(which)][steps][M]"""
    fs = []
    for b in which:
        f = orc.OracleFilter(N).init(**oracle_params(sc["params"]))
        for i in range(N):
            f.init_feature(sc["pix"][b, i], i, float("nan"))
        fs.append(f)
    u = np.ascontiguousarray(sc["u"][:steps, which].transpose(1, 0, 2))
    z = np.ascontiguousarray(sc["z"][:steps, which].transpose(1, 0, 2, 3))
    threads = max(1, min(len(which), os.cpu_count() or 1, 16))
    res = orc.run_steps_mt(fs, threads, u, float(sc["dt"][0]), z, sc["slot"][which], sc["R"])
    return np.stack([f.x.copy() for f in fs]), np.stack([f.P.copy() for f in fs]), res


def expected_instance(B, N):
    """what describe() must name for an automatic batch on this device: the row of kResInst that setup_resident's rule picks
    (the table itself, read by tests/hetero_cases.py, and the device's CU count), or the streaming family past its last row"""
    import torch
    row = hc.auto_row(N, B, torch.cuda.get_device_properties(0).multi_processor_count)
    return hc.row_name(row) if row >= 0 else "k_propagate_"


def run_full(B, N, steps, which, kernel=0, seed=None, tune=()):
    sc = scene.make_scene(B, N, steps, seed=4000 + N if seed is None else seed)
    g = v.BatchVIEKF(B, N, sc["params"])
    if kernel:
        g.set_kernel(kernel)
    for key, value in tune:
        g.set_tuning(key, value)
    if kernel == 0:
        assert g.describe().startswith(expected_instance(B, N)), (g.describe(), expected_instance(B, N))
    for i in range(N):
        ok = g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
        assert (ok == 1).all()
    res = np.zeros((steps, B, N), dtype=np.int32)
    for s in range(steps):
        res[s] = g.step(sc["u"][s], sc["dt"], sc["z"][s], sc["slot"], sc["R"])
    which = np.asarray(which)
    x_ref, P_ref, res_ref = oracle_subset(sc, N, steps, which)
    assert (res[:, which].transpose(1, 0, 2) == res_ref).all(), "meas_result codes differ"
    x = g.get_state()
    P = g.get_covariance()
    assert_close(x[which], x_ref, "x of filters %s" % list(which))
    assert_close(P[which], P_ref, "P of filters %s" % list(which))
    st = g.get_status()
    assert (st & (1 | 2 | 8) == 0).all(), "NaN / blow-up / internal flags raised: %s" % np.unique(st)
    # every filter ran the same kind of step: P symmetric and finite everywhere, not only in the sample
    assert np.isfinite(x).all() and np.isfinite(P).all()
    assert (P == P.transpose(0, 2, 1)).all()
    return g


def test_headline_batch_every_dispatch_round():
    """B=1024, N=50 (BASELINE configs[2]): the headline instance, two workgroups per CU, two rounds over 256 CUs"""
    run_full(1024, 50, 3, [0, 255, 256, 511, 700, 1023])


@pytest.mark.parametrize("N", [12, 20, 25])
def test_two_per_cu_instance_beyond_one_round(N):
    """B=600 > 256 CUs: by the table, on a 256-CU device N = 12 runs on <2,1> (four 128-thread workgroups per CU: 600 > 2 x 256),
    N = 20 on <2,2> and N = 23 .. 25 on <3,2> (192 threads), both two workgroups per CU; run_full asserts the instance that
    describe() names against the table and the device's CU count"""
    run_full(600, N, 4, [0, 1, 255, 256, 511, 512, 598, 599])


def test_config1_batch256_n25():
    """BASELINE configs[1]: B=256, N=25"""
    run_full(256, 25, 4, [0, 1, 127, 128, 254, 255])


def test_wide_p_full_batch():
    """BASELINE configs[4]: B=1024, N=150, P in HBM (MFMA propagate + grouped update), one step"""
    run_full(1024, 150, 1, [0, 1023])


def test_two_service_waves_full_batch():
    """B=1024, N=64: the <6,6> instance with the body lanes on a second service wave (N + 14 > 64)"""
    run_full(1024, 64, 2, [0, 255, 256, 1023])


def test_two_filters_per_workgroup_sizes_between():
    """B=1024 at feature counts either side of the instance boundaries"""
    run_full(1024, 26, 2, [0, 300, 1023])     # <4,3>
    run_full(1024, 38, 2, [0, 511, 1023])     # <4,3>, its last size
    run_full(1024, 39, 2, [0, 256, 1023])     # <5,3>
    run_full(1024, 43, 2, [0, 255, 1023])     # <5,3>, its last size
    run_full(1024, 44, 2, [0, 700, 1023])     # <6,3>
    run_full(1024, 47, 2, [0, 256, 1023])     # <6,3>, its last size
    run_full(1024, 48, 2, [0, 256, 1023])     # <7,3>, its first
    run_full(1024, 49, 2, [0, 512, 1023])


@pytest.mark.parametrize("N", [1, 3, 12, 15])
def test_four_per_cu_instance_small_filters(N):
    """B=1024 > 2 x 256 CUs, N <= 15: the <2,1> instance (ONE worker wave + the service wave, four 128-thread workgroups per CU;
    the reference's own sizes: NUM_FEATURES 12, include/vi_ekf.h:39-45)"""
    run_full(1024, N, 3, [0, 1, 255, 256, 511, 512, 767, 1022, 1023])


def test_features_on_both_service_waves_full_batch():
    """B=1024, N=70: the <7,6> instance (features 64.. on the body wave's lanes; the measurement list crosses the 64 per launch)"""
    run_full(1024, 70, 2, [0, 255, 256, 1023])


@pytest.mark.parametrize("N", [12, 50, 70])
def test_general_lambda_instances_full_batch(N):
    """the same batches on the general-Lambda instances (what a parameter file with lambda_feat[0:2] != 1 selects)"""
    from vi_ekf_amd import capi
    g = run_full(1024, N, 2, [0, 255, 256, 1023], tune=[(capi.TUNE_UNIT_LAMBDA, 0)])
    assert " ZU" not in g.describe()


@pytest.mark.parametrize("N,group", [(85, 0), (85, 16), (85, 24), (100, 0), (100, 16), (90, 24), (85, -1), (100, -1), (160, 0)])
def test_wide_p_group_sizes(N, group):
    """the grouped update at the sizes between the families: the look-ahead kernel (groups of 16, the default where its LDS layout
    fits: N <= 154), r03's kernel with forced group sizes 24 / 32 and with its own choice (group = -1: VIEKF_TUNE_PANEL_SERVICE = 0
    -> 32 at N = 85, 24 at N = 100), N = 160 where only r03's kernel fits; more measurements than one group: x, P (whole, mirrored
    from the lower triangle) and codes against the oracle, P == P^T bit for bit"""
    from vi_ekf_amd import capi
    tune = []
    if group > 0:
        tune.append((capi.TUNE_BLOCK_GROUP, group))
    if group < 0:
        tune.append((capi.TUNE_PANEL_SERVICE, 0))
    g = run_full(64, N, 2, [0, 31, 63], tune=tune)
    d = g.describe()
    if group in (0, 16) and N <= 154:
        assert "k_update_feat_panelsvc<512,16>" in d, d
    elif group > 0:
        assert "k_update_feat_blocked<512,%d>" % group in d, d
    elif N == 160:
        assert "k_update_feat_blocked<512,16>" in d, d
    else:
        assert "k_update_feat_blocked<512,%d>" % (32 if N == 85 else 24) in d, d


# ---- the OTHER routes bench.py times, at the size it times them: the multi-propagate instance of the headline kernel
# (viekf_batch_step_n / _propagate_n_to), the out-of-place ring store (P_out != P) and the per-filter zero-copy ring of the
# independent-clock sequencer (viekf_batch_select_filters / _propagate_filters_to), B = 1024, N = 50, filters of every dispatch
# round against the ORACLE (vo_propagate + the updates; reference vi_ekf.cpp:262-318, vi_ekf_meas.cpp:196-278), not against
# another HIP route: a fault shared by a fused route and its HIP twin would pass a HIP-vs-HIP comparison.
HEADLINE_SAMPLE = [0, 255, 256, 511, 700, 1023]     # first, last and either side of a dispatch round


def _headline_batch(steps, seed):
    B, N = 1024, 50
    sc = scene.make_scene(B, N, steps, seed=seed)
    g = v.BatchVIEKF(B, N, sc["params"])
    for i in range(N):
        assert (g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan)) == 1).all()
    assert g.describe().startswith("k_step_resident<7,3>"), g.describe()
    return sc, g


def _oracle_filters(sc, N, which):
    fs = []
    for b in which:
        f = orc.OracleFilter(N).init(**oracle_params(sc["params"]))
        for i in range(N):
            f.init_feature(sc["pix"][b, i], i, float("nan"))
        fs.append(f)
    return fs


def _check_sample(g, fs, which, what):
    """x and P of the sample against the oracle filters fs; no flag, finite and P == P^T bit for bit over the WHOLE batch"""
    x, P = g.get_state(), g.get_covariance()
    assert_close(x[which], np.stack([f.x for f in fs]), "x, " + what)
    assert_close(P[which], np.stack([f.P for f in fs]), "P, " + what)
    assert (g.get_status() & (1 | 2 | 8) == 0).all(), what
    assert np.isfinite(x).all() and np.isfinite(P).all(), what
    assert (P == P.transpose(0, 2, 1)).all(), "P != P^T somewhere in the batch, " + what


def _oracle_frame(fs, which, z, slot, R, res, what):
    """the frame's FEAT updates on every oracle filter of the sample; their codes against the batch's, bit for bit"""
    for j, b in enumerate(which):
        for m in range(slot.shape[1]):
            r = fs[j].update(orc.FEAT, z[b, m], R, True, int(slot[b, m]))
            assert r == res[b, m], "meas_result code of filter %d, update %d: %d vs the oracle's %d (%s)" % (b, m, res[b, m], r, what)


@pytest.mark.parametrize("K", [8, 9])
def test_step_n_headline_batch_vs_oracle(K):
    """viekf_batch_step_n (cadence_250_30.fused in bench.py): K IMU samples + the frame's 50 updates in ONE launch of the
    multi-propagate instance k_step_resident<7,3,MP>, two frames in a row, with uneven dt"""
    which = np.asarray(HEADLINE_SAMPLE)
    sc, g = _headline_batch(2 * K, 7100 + K)
    fs = _oracle_filters(sc, 50, which)
    dt = np.tile(sc["dt"], (K, 1)) * np.linspace(0.8, 1.2, K)[:, None]
    for fr in range(2):
        u = np.ascontiguousarray(sc["u"][fr * K:(fr + 1) * K])
        res = g.step_n(u, dt, sc["z"][fr], sc["slot"], sc["R"])
        for j, b in enumerate(which):
            for k in range(K - 1):
                fs[j].propagate(u[k, b], dt[k, b])
            ref = fs[j].run_steps(u[K - 1, b][None], dt[K - 1, b], sc["z"][fr, b][None], sc["slot"][b], sc["R"])[0]
            assert (res[b] == ref).all(), "meas_result codes differ (filter %d, frame %d)" % (b, fr)
    _check_sample(g, fs, which, "step_n K=%d" % K)


def test_propagate_n_to_headline_batch_vs_oracle():
    """viekf_batch_propagate_n_to (the sequencer's closing replay): K = 8 propagates into ring slots 1..8 in ONE launch of the
    same instance, only the last slot written (*intermediates_written == 0: not the one-by-one fallback); then the frame's
    updates IN that slot"""
    import ctypes as C
    from vi_ekf_amd import capi
    K = 8
    which = np.asarray(HEADLINE_SAMPLE)
    sc, g = _headline_batch(K, 7200)
    fs = _oracle_filters(sc, 50, which)
    L = capi.lib()
    g.history_resize(K + 2)
    g.snapshot(0)
    capi.check(L.viekf_batch_select(g._h, 0))
    u = np.ascontiguousarray(sc["u"][:K])
    dt = np.ascontiguousarray(np.tile(sc["dt"], (K, 1)) * (1.0 + 0.05 * np.arange(K))[:, None])
    slots = np.arange(1, K + 1, dtype=np.int32)
    written = C.c_int32(-1)
    p = lambda a: C.c_void_p(a.ctypes.data)
    capi.check(L.viekf_batch_propagate_n_to(g._h, K, p(u), p(dt), p(slots), C.byref(written), capi.HOST))
    assert written.value == 0
    for j, b in enumerate(which):
        for k in range(K):
            fs[j].propagate(u[k, b], dt[k, b])
    _check_sample(g, fs, which, "propagate_n_to K=8, slot 8")
    res = g.update_feat(sc["z"][0], sc["slot"], sc["R"])
    _oracle_frame(fs, which, sc["z"][0], sc["slot"], sc["R"], res, "ring slot 8")
    _check_sample(g, fs, which, "updates in ring slot 8")
    g.history_resize(0)
    _check_sample(g, fs, which, "after leaving the ring")


def test_propagate_to_ring_slot_headline_batch_vs_oracle():
    """viekf_batch_propagate_to: the out-of-place store of the fused kernel (P read from slot i, written to slot i + 1,
    viekf_resident_worker.hpp: P_out != P) through three slots at B = 1024, N = 50; the slot left behind still holds its state"""
    import ctypes as C
    from vi_ekf_amd import capi
    which = np.asarray(HEADLINE_SAMPLE)
    sc, g = _headline_batch(3, 7300)
    fs = _oracle_filters(sc, 50, which)
    L = capi.lib()
    g.history_resize(4)
    g.snapshot(0)
    capi.check(L.viekf_batch_select(g._h, 0))
    p = lambda a: C.c_void_p(a.ctypes.data)
    dt = np.ascontiguousarray(sc["dt"])
    kept = None
    for k in range(3):
        u = np.ascontiguousarray(sc["u"][k])
        capi.check(L.viekf_batch_propagate_to(g._h, p(u), p(dt), k + 1, capi.HOST))
        for j, b in enumerate(which):
            fs[j].propagate(u[b], dt[b])
        _check_sample(g, fs, which, "propagate_to slot %d" % (k + 1))
        if k == 0:
            kept = [f.clone() for f in fs]
    capi.check(L.viekf_batch_select(g._h, 1))       # rewind: slot 1 was read by the second call, never written again
    _check_sample(g, kept, which, "slot 1 after two more propagates")


def test_per_filter_ring_headline_batch_vs_oracle():
    """viekf_batch_select_filters / _propagate_filters_to (the independent-clock sequencer's zero-copy ring) at B = 1024, N = 50:
    every filter starts on ITS ring position (slot b % 18: the six sample filters on six different slots), three steps of
    propagate_filters_to in which some filters (sample ones among them) stay put, each followed by the frame's updates in the
    per-filter slots; then a rewind of every sample filter to an earlier slot of its own history, and the way home"""
    import ctypes as C
    from vi_ekf_amd import capi
    B, H, steps = 1024, 18, 3
    which = np.asarray(HEADLINE_SAMPLE)
    sc, g = _headline_batch(steps, 7400)
    fs = _oracle_filters(sc, 50, which)
    L = capi.lib()
    p = lambda a: C.c_void_p(a.ctypes.data)
    live = (np.arange(B) % H).astype(np.int32)
    assert len(set(live[which].tolist())) == len(which)
    g.history_resize(H)
    capi.check(L.viekf_batch_snapshot_filters(g._h, p(live), capi.HOST))
    capi.check(L.viekf_batch_select_filters(g._h, p(live)))
    _check_sample(g, fs, which, "per-filter slots b % 18")
    hist = {(j, int(live[b])): fs[j].clone() for j, b in enumerate(which)}      # (sample index, slot) -> the oracle's state there
    stay = {0: [255, 700], 1: [1023], 2: [0, 511]}                               # sample filters that do not propagate in step s
    rng = np.random.default_rng(11)
    for s in range(steps):
        dst = np.where(rng.uniform(size=B) < 0.8, (live + 1) % H, -1).astype(np.int32)
        dst[which] = (live[which] + 1) % H
        dst[stay[s]] = -1
        u = np.ascontiguousarray(sc["u"][s])
        dt = np.ascontiguousarray(sc["dt"] * (1.0 + 0.1 * s))
        capi.check(L.viekf_batch_propagate_filters_to(g._h, p(u), p(dt), p(dst), capi.HOST))
        live = np.where(dst >= 0, dst, live).astype(np.int32)
        for j, b in enumerate(which):
            if dst[b] >= 0:
                fs[j].propagate(u[b], dt[b])
        _check_sample(g, fs, which, "propagate_filters_to, step %d" % s)
        res = g.update_feat(sc["z"][s], sc["slot"], sc["R"])
        _oracle_frame(fs, which, sc["z"][s], sc["slot"], sc["R"], res, "per-filter ring, step %d" % s)
        _check_sample(g, fs, which, "updates in the per-filter slots, step %d" % s)
        for j, b in enumerate(which):
            hist[(j, int(live[b]))] = fs[j].clone()
    # rewind: sample filter j to an earlier slot of its own history (an index, no copy); the others stay where they are
    back = np.full(B, -1, dtype=np.int32)
    kept = []
    for j, b in enumerate(which):
        mine = [sl for (jj, sl) in hist if jj == j and sl != live[b]]
        assert mine, "filter %d has no earlier slot" % b
        back[b] = mine[j % len(mine)]
        kept.append(hist[(j, int(back[b]))])
    capi.check(L.viekf_batch_select_filters(g._h, p(back)))
    _check_sample(g, kept, which, "rewound to an earlier slot")
    capi.check(L.viekf_batch_select_filters(g._h, p(live)))
    _check_sample(g, fs, which, "back on the live slots")
    g.history_resize(0)                             # leaving the ring brings every live state home
    _check_sample(g, fs, which, "after leaving the ring")
