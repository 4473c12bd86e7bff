"""The PIXEL_VEL model of tests/pixvel_ref.py (the numpy statement of csrc/viekf_pixvel_model.hpp) on the CPU: against the
oracle's own dynamics and h_feat, its Jacobian against central differences, against the independent kinematics of
vi_ekf_amd/sim.py, the flow by id and the intake step on ragged lists, the cases' own conditions and the LDS layout."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import np_twin as tw
from oracle import oracle as orc
from tests import pixvel_cases as pc
from tests import pixvel_ref as pr
from tests.helpers import jac_fixture, make_oracle, make_twin

FD_TOL = 1e-3          # tests/properties.py::_htest: |a - d| <= max(tol |a|, tol)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fixture(N, seed, drag):
    """jac_fixture's random state and camera, with a q_b_u that is not the identity and a unit q_b_c"""
    p, pix, dep, u = jac_fixture(N, seed)
    p = dict(p, use_drag_term=drag)
    r = np.random.default_rng(seed + 1)
    q = np.array([0.9, 0.0, 0.0, 0.0]) + r.uniform(-0.3, 0.3, 4)
    p["q_b_u"] = q / np.linalg.norm(q)
    p["q_b_c"] = p["q_b_c"] / np.linalg.norm(p["q_b_c"])
    return p, pix, dep, u


def thr(a):
    return max(FD_TOL * np.linalg.norm(a), FD_TOL)


@pytest.mark.parametrize("N", [1, 3, 12])
@pytest.mark.parametrize("drag", [True, False])
def test_model_against_the_oracles_dynamics_and_h_feat(N, drag):
    """the pixel is h_feat(q_zeta(t)) and the state moves by f(x, u) dt: the central difference of OracleFilter.h(FEAT) along
    x [+] (+- eps f) is zhat + O(eps^2).  Halving eps shrinks the disagreement by four until round-off takes over"""
    p, pix, dep, u = fixture(N, 500 + N, drag)
    f, t = make_oracle(N, p, pix, dep), make_twin(N, p, pix, dep)
    gyro = u[3:6]
    ub = pr.body_input(t, gyro)
    ub[0:3] = tw.rota(t.q_b_u, u[0:3])                         # (the accelerometer moves the state, not the bearing)
    xd, _, _ = f.dynamics(f.x, ub)
    for i in range(N):
        zhat, _ = pr.h_pixel_vel(t, f.x.copy(), i, gyro)
        errs = []
        for eps in (4e-3, 2e-3, 1e-3, 5e-4):
            hp, _ = f.h(orc.FEAT, f.boxplus(f.x, eps * xd), i)
            hm, _ = f.h(orc.FEAT, f.boxplus(f.x, -eps * xd), i)
            errs.append(np.abs((hp[:2] - hm[:2]) / (2 * eps) - zhat).max())
        print("N %d drag %d slot %d: |zhat| %.3e, disagreement at eps = 4e-3 .. 5e-4: %s" % (N, drag, i, np.abs(zhat).max(), errs))
        for a, b in zip(errs, errs[1:]):
            if a > 1e-6 * max(np.abs(zhat).max(), 1.0):        # (below that round-off dominates the difference)
                assert b / a <= 0.35, (i, errs)
        assert min(errs) <= thr(zhat), (i, errs, zhat)


@pytest.mark.parametrize("N", [1, 3, 12])
@pytest.mark.parametrize("drag", [True, False])
def test_jacobian_against_central_differences(N, drag):
    p, pix, dep, u = fixture(N, 600 + N, drag)
    t = make_twin(N, p, pix, dep)
    gyro = u[3:6]
    I, eps = np.eye(t.n), 1e-6
    for i in range(N):
        _, H = pr.h_pixel_vel(t, t.x, i, gyro)
        d = np.zeros_like(H)
        for k in range(t.n):
            zp, _ = pr.h_pixel_vel(t, t.boxplus(t.x, I[:, k] * eps), i, gyro)
            zm, _ = pr.h_pixel_vel(t, t.boxplus(t.x, -I[:, k] * eps), i, gyro)
            d[:, k] = (zp - zm) / (2 * eps)
        nine = [3, 4, 5, 12, 13, 14, 16 + 3 * i, 17 + 3 * i, 18 + 3 * i]
        rest = [k for k in range(t.n) if k not in nine]
        assert (H[:, rest] == 0.0).all() and (np.abs(H[:, nine]) > 0).all()
        err = np.abs(H - d).max()
        print("N %d drag %d slot %d: |H| %.3e, max |H - fd| %.3e" % (N, drag, i, np.linalg.norm(H), err))
        assert err <= thr(H), (i, err, thr(H))
        # the bearing block is not Hb times Aff's own block: the error-state dynamics carry a transport term
        _, A, _ = t.dynamics(t.x, pr.body_input(t, gyro))
        _, Hf = t.h_feat(t.x, i)
        r0 = 16 + 3 * i
        naive = Hf[:, r0:r0 + 2] @ A[r0:r0 + 2, r0:r0 + 2]
        assert np.abs(naive - d[:, r0:r0 + 2]).max() > 10 * thr(H)


def test_model_against_the_simulators_kinematics():
    """vi_ekf_amd/sim.py integrates the vehicle and projects landmarks without any of the filter's code: the central difference
    of noise-free pixels at ticks k -+ s against zhat at the true state of tick k, for s = 1 and 2.  The rates are constant
    within a tick and jump between ticks, so the pixel velocity at tick k has a left and a right value; the central difference
    gives their mean, and so does the model (it is linear in omega) with the mean of the two gyro samples.
    The simulator integrates a tick in four explicit Euler steps: the position moves with the velocity at a step's start, which
    shifts the flow it produces by half a step against the continuous model -- first order in the step, the same at both
    spacings, and at 1 ms steps larger than the second-order term looked for.  So the five ticks the differences span are
    integrated with the simulator's own step function at 1 / 256 of its step (controls held per tick as ever)."""
    FINE = 256
    from vi_ekf_amd import scene, sim
    p = dict(scene.EKF_YAML)
    s = sim.Simulator(p, num_features=8, seed=3)
    K0 = 600                                                   # t = 2.4 s: on the circle, every axis moving
    track, hist = None, {}
    for k in range(1, K0 + 3):
        s._control()
        w_next = s.imu(noise=False)[3:6] if k - 1 == K0 else None
        if w_next is not None:
            hist["gyro_after"] = w_next
        if k >= K0 - 2:                                        # the five ticks the differences span: integrated finely
            dt, s.dt = s.dt, s.dt / FINE
            for _ in range(FINE):
                s._step_truth()
            s.dt = dt
        else:
            s._step_truth()
        s.k, s.t = k, k * s.dt
        if k == K0 - 2:
            pix, _, vis = s.project()
            track = [i for i in np.argsort(np.linalg.norm(pix - s.c, axis=1)) if vis[i]][:12]
        if track is not None:
            pix, depth, vis = s.project(track)
            assert vis.all()
            hist[k] = pix
            if k == K0:
                hist["gyro_before"] = s.imu(noise=False)[3:6]
                hist["state"] = s.state()
                hist["pc"] = np.array([sim.q_rotp(s.q_b_c, sim.q_rotp(s.q, s.landmarks[i] - s.pos) - s.p_b_c) for i in track])
    N = len(track)
    prm = {k: p[k] for k in ("x0", "P0", "Qx", "lam", "Qu", "P0_feat", "Qx_feat", "lam_feat", "cam_center", "focal_len", "q_b_c",
                             "p_b_c", "q_b_u", "min_depth", "use_drag_term", "use_partial_update")}
    t = tw.TwinFilter(N, **prm)
    st = hist["state"]
    x = np.zeros(t.nx)
    x[0:3], x[3:6], x[6:10] = st[0:3], st[7:10], st[3:7]
    x[10:13], x[13:16], x[16] = s.accel_bias_, s.gyro_bias_, s.mu
    for i in range(N):
        d = np.linalg.norm(hist["pc"][i])
        x[17 + 5 * i:21 + 5 * i] = tw.from_two_unit_vectors(tw.E_Z, hist["pc"][i] / d)
        x[21 + 5 * i] = 1.0 / d
    t.len = N
    gyro = 0.5 * (hist["gyro_before"] + hist["gyro_after"])
    res = {}
    for sp in (1, 2):
        flow = (hist[K0 + sp] - hist[K0 - sp]) / (2 * sp * s.dt)
        zh = np.array([pr.h_pixel_vel(t, x, i, gyro)[0] for i in range(N)])
        res[sp] = np.abs(flow - zh).max(axis=1)
        print("spacing +-%d ticks: flow up to %.1f px/s, residual per feature %s" % (sp, np.abs(flow).max(), np.round(res[sp], 5)))
    assert np.abs(flow).max() > 5.0                            # (the vehicle moves)
    assert np.median(res[1] / res[2]) <= 0.35, (res[1], res[2])
    assert res[1].max() <= 1e-3 * np.abs(flow).max()           # signs and frames: a flipped term is of the size of the flow


def test_pixel_flow_and_intake_step_on_ragged_lists():
    nan = np.nan
    ids_prev = np.array([[4, 7, 7, -1, 9], [1, 2, 3, 4, 5]], np.int32)
    z_prev = np.arange(20, dtype=np.float64).reshape(2, 5, 2)
    z_prev[1, 2, 0] = nan                                       # id 3 of filter 1 has a NaN coordinate in the earlier frame
    ids = np.array([[7, 5, 9, -1, 4, 7, 11], [5, 3, 8, 1, -1, -1, 2]], np.int32)      # M_prev = 5, M = 7
    z = 100.0 + np.arange(28, dtype=np.float64).reshape(2, 7, 2)
    z[1, 6, 1] = np.inf                                         # id 2 of filter 1: not finite now
    dt = np.array([0.04, 0.05])
    zd = pr.pixel_flow(z_prev, ids_prev, z, ids, dt)
    assert np.array_equal(zd[0, 0], (z[0, 0] - z_prev[0, 1]) / 0.04)           # id 7 repeats in ids_prev: the first match
    assert np.array_equal(zd[0, 5], (z[0, 5] - z_prev[0, 1]) / 0.04)           # ... and in ids: each entry gets its flow
    assert np.isnan(zd[0, 1]).all() and np.isnan(zd[0, 6]).all()               # ids that appeared
    assert np.isnan(zd[0, 3]).all()                                            # padding (-1 never matches a -1)
    assert np.array_equal(zd[0, 2], (z[0, 2] - z_prev[0, 4]) / 0.04) and np.array_equal(zd[0, 4], (z[0, 4] - z_prev[0, 0]) / 0.04)
    assert np.array_equal(zd[1, 0], (z[1, 0] - z_prev[1, 4]) / 0.05) and np.array_equal(zd[1, 3], (z[1, 3] - z_prev[1, 0]) / 0.05)
    assert np.isnan(zd[1, 1]).all() and np.isnan(zd[1, 6]).all() and np.isnan(zd[1, 2]).all()
    # the intake step: which entries measure, their order and codes
    p, pix, dep, u = fixture(3, 41, True)
    twins = [make_twin(3, p, pix, dep) for _ in range(2)]
    for t in twins:
        t.P = t.P * 1e-2
    tables = [[7, 4, 9], [5, 1, 3]]                             # slot order
    feat = np.array([[0, 0, 1, -1, 4, 3, 0], [0, 0, 4, 2, -1, -1, 0]], np.int32)
    gyro = np.tile(u[3:6], (2, 1))
    flow = np.zeros((2, 7, 2))
    for b in range(2):
        for i in range(7):
            gid = int(ids[b, i])
            flow[b, i] = pr.h_pixel_vel(twins[b], twins[b].x, tables[b].index(gid), gyro[b])[0] + 2.0 if gid in tables[b] else 3.0
    flow[1, 1] = nan                                            # no flow for id 3
    before = [t.x.copy() for t in twins]
    res = pr.intake_pixel_vel(twins, tables, ids, flow, feat, gyro, np.eye(2) * 100.0, 1e-4)
    # filter 0: 7 (queued), 5 (not tracked: INVALID), 9 (FEAT gated: still measured), pad, 4 (NEW_FEATURE: none), 7 again
    # (FEAT answered INVALID for the repeat: none), 11 (not in the table: INVALID)
    assert list(res[0]) == [0, 3, 0, -1, -1, -1, 3], res
    assert list(res[1]) == [0, -1, -1, -1, -1, -1, 3], res      # 5 measured; 3 has no flow; 8 new; 1 had a NaN pixel; 2 not tracked
    res1 = res[1].copy()
    assert not np.array_equal(twins[0].x, before[0])
    res = pr.intake_pixel_vel(twins, tables, ids, flow, feat, gyro, np.eye(2) * 100.0, 0.0, active=np.array([1, 0]), stale=(0,))
    assert list(res[0]) == [3, 3, 3, -1, 3, 3, 3] and (res[1] == -1).all() and res1[0] == 0


@pytest.mark.parametrize("name,N,variant", [("once", 1, 0), ("once", 3, 1), ("once", 12, 2), ("once", 12, 3), ("once", 3, 4),
                                            ("repeat", 2, 0), ("mixed", 12, 0), ("mixed", 12, 1), ("fix", 3, 0), ("fix", 12, 1),
                                            ("poison", 12, 0)])
def test_cases_reach_what_they_are_for(name, N, variant):
    c = pc.case(name, N, variant)
    codes = c["codes"]
    assert np.isfinite(c["x_ref"]).all()
    P = np.delete(c["P_ref"], c["poisoned"], axis=0) if c["poisoned"] is not None else c["P_ref"]
    assert np.isfinite(P).all() and np.abs(P - P.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(P).max()
    if name in ("once", "repeat"):
        assert set(np.unique(codes)) <= {-1, 0, 3} and (codes == 0).sum() >= 2 and not (codes == 1).any()
        assert (codes[3] != 0).all() and 3 in c["untouched"]                   # the filter without features
        assert np.abs(c["x_ref"][0, 3:6] - c["x0"][0, 3:6]).max() > 1e-6       # the velocity is corrected
    if name == "repeat":
        assert c["slot"].shape[1] == 70 and (c["len"] == [2, 0, 1, 0, 1]).all()
    if name == "mixed":
        assert (codes[:, pc.MIXED_GATED][[0, 1]] == 1).all()
        assert codes[pc.MIXED_NAN_FILTER, pc.MIXED_NAN] == 2 and (codes[pc.MIXED_SKIPPED_FILTER] == -1).all()
        assert set(np.unique(codes[pc.MIXED_GYRO_NAN_FILTER])) <= {2, 3}
        assert pc.MIXED_SKIPPED_FILTER in c["untouched"] and pc.MIXED_GYRO_NAN_FILTER in c["untouched"]
        assert (codes[0] == 0).sum() >= 5 and (codes[1] == 0).sum() >= 4
    if name == "fix":
        reset = 1.0 / (2.0 * c["params"]["min_depth"])
        assert c["x0"][pc.FIX_NEG_FILTER, 21 + 5 * (N - 1)] < 0 and c["x0"][pc.FIX_BIG_FILTER, 21 + 5] > 1e2
        assert (codes[pc.FIX_NEG_FILTER] == 0).all()
        # repaired to 1 / (2 min_depth), then moved by the later entries' corrections
        assert 0 < c["x_ref"][pc.FIX_NEG_FILTER, 21 + 5 * (N - 1)] < 2 * reset
        d = 18 + 3 * (N - 1)
        assert c["P_ref"][pc.FIX_NEG_FILTER, d, d] != c["P0"][pc.FIX_NEG_FILTER, d, d]
    if name == "poison":
        i, j = pc.POISON_AT
        assert np.isnan(c["P0"][pc.POISONED, i, j]) and i < 16 + 3 * c["len"][pc.POISONED]
        assert (codes[pc.POISONED][c["slot"][pc.POISONED] < c["len"][pc.POISONED]] >= 0).all()


def test_lds_bytes_against_the_layout():
    """viekf_pixvel_lds_bytes against the layout it states: 8 (nx' + 5 n + 32), the sections in order and disjoint"""
    from vi_ekf_amd import capi
    L = capi.lib()
    for N in (0, 1, 2, 3, 12, 50, 77, 100, 500, 4096):
        nx, n = 17 + 5 * N, 16 + 3 * N
        nxs = (nx + 1) & ~1
        assert L.viekf_pixvel_lds_bytes(N) == 8 * (nxs + 5 * n + 32), N
    assert L.viekf_pixvel_lds_bytes(-1) == 0 and L.viekf_pixvel_lds_bytes(4097) == 0
    text = open(os.path.join(ROOT, "vi_ekf_amd", "csrc", "viekf_pixvel_lds.hpp")).read()
    assert "xs(0), W(nxs), K(W + 2 * n), lam(K + 2 * n), sm(lam + n), total(sm + kSmall)" in text and "kSmall = 32" in text
    assert L.viekf_pixvels_lds_bytes(50, 50) == 8 * (268 + 166 + 50 + 9 * 166 + 32 + 200 + 2 * 166 * 50)
    assert capi.PIXVELS_MAX_M == 256 and "VIEKF_PIXVELS_MAX_M 256" in open(os.path.join(ROOT, "include", "viekf_pixvel.h")).read()
