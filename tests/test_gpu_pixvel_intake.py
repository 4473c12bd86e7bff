"""FrameIntake.intake_pixel_vel (viekf_frame_intake_pixel_vel, include/viekf_pixvel.h) behind FrameIntake.intake of the same
frame and vi_ekf_amd.pixel_flow between two frames, on device pointers, against tests/pixvel_ref.py: which entries are
measurements, their codes, and x and P.  Three frames with a lost id, a new id, a repeated id, a gated FEAT, a NaN pixel, an
inactive filter and a stale table.  Then the closed loop: simulator -> step_n -> intake -> pixel_flow -> intake_pixel_vel."""
import numpy as np
import pytest

from oracle import np_twin
from oracle import oracle as orc
from tests import frame_ref as F
from tests import meas_cases as mc
from tests import pixvel_ref as PR
from tests.test_gpu_frame import _batch, _params, active_block, against_ref, close, frame, noise, same_bits, state

pytestmark = pytest.mark.gpu

B, N, M = 3, 8, 8
INACTIVE = 1
ROWS = ([0, 1, 2, 3, 4, 5],                      # frame 1: every id new
        [0, 1, 2, 3, 5, 7, 1, -1],               # frame 2: id 4 lost, id 7 new, id 1 repeated
        [0, 1, 2, 3, 5, 7, -1, -1])              # frame 3
FAR, NANPIX = (2,), (1,)                         # frame 2: entry 2 is 300 px off (FEAT gated), entry 1 has a NaN pixel
GYRO_VAR = 1e-4


def twins_of(ref, p):
    """numpy twins at the restated filters' states (P: lower triangle mirrored, what the device holds), and their id tables"""
    prm = {k: p[k] for k in mc.ORACLE_KEYS}
    ts = []
    for r in ref.r:
        t = np_twin.TwinFilter(N, **prm)
        low = np.tril(r.f.P)
        t.x, t.P, t.len = r.f.x.copy(), low + np.tril(low, -1).T, int(r.f.len_features)
        ts.append(t)
    return ts, [list(r.tracked()) for r in ref.r]


def flow_R():
    R = np.zeros((B, M, 2, 2))
    for b in range(B):
        for i in range(M):
            R[b, i] = [[900.0 + 10 * i, 5.0 * b], [5.0 * b, 1200.0 + 7 * i]]
    return R


def compare(g, ts, what, only=None):
    x, P, ln = state(g)
    rx, rP = np.stack([t.x for t in ts]), np.stack([t.P for t in ts])
    rl = [t.len for t in ts]
    x, P = active_block(x, P, rl)
    rx, rP = active_block(rx, rP, rl)
    sel = list(range(len(ts))) if only is None else list(only)
    assert np.array_equal(ln[sel], np.array(rl)[sel])
    assert close(x[sel], rx[sel]) and close(P[sel], rP[sel]), (what, np.abs(x[sel] - rx[sel]).max(), np.abs(P[sel] - rP[sel]).max())
    assert np.array_equal(P, P.transpose(0, 2, 1))


def test_three_frames():
    import torch
    import vi_ekf_amd as v
    t = lambda a: None if a is None else torch.tensor(a, device="cuda:0")
    p = _params(use_keyframe_reset=False)
    g, ref = _batch(B, N, p), F.BatchFrameRef(B, N, p, 0.8)
    fi = v.FrameIntake(g)
    rng = np.random.default_rng(41)
    Rm, Rf = noise(B, M, 0), flow_R()
    u = np.zeros((10, B, 6))                                    # 25 Hz frames at a 250 Hz IMU
    u[:, :, 2] = -9.80665
    u[:, :, 3:6] = rng.normal(0.0, 0.05, (10, B, 3))
    dt = np.full((10, B), 0.004)
    dt_frame = np.full(B, 0.04)
    z1, ids1, _ = frame(rng, B, M, ROWS[0])
    against_ref(fi.intake(z1, ids1, Rm), fi, g, ref.intake(z1, ids1, Rm), ref, "frame 1")
    active = np.ones(B, np.uint8)
    active[INACTIVE] = 0
    zp, idp = z1, ids1
    for k in (1, 2):
        g.step_n(u, dt, None, None, None)
        ref.propagate(u, dt)
        z, ids, _ = frame(rng, B, M, ROWS[k], FAR if k == 1 else (), NANPIX if k == 1 else ())
        dz, dids, dact = t(z), t(ids), t(active)
        out = fi.intake(dz, dids, t(Rm), active=dact)
        rout = ref.intake(z, ids, Rm, active=active)
        o = {kk: out[kk].cpu().numpy() for kk in out}
        against_ref(o, fi, g, rout, ref, "frame %d" % (k + 1))
        fres = o["result"]
        # the flow between the two frames, by id, on the device
        g.use_torch_stream()
        dzd = v.pixel_flow(g, t(zp), t(idp), dz, dids, t(dt_frame))
        torch.cuda.synchronize()
        zd = dzd.cpu().numpy()
        assert np.array_equal(zd, PR.pixel_flow(zp, idp, z, ids, dt_frame), equal_nan=True)
        gyro = np.ascontiguousarray(u[9][:, 3:6])
        ts, tabs = twins_of(ref, p)
        stale = ()
        if k == 2:                                             # a feature started behind the intake's back: filter 0's table is stale
            px = np.tile(np.array([500.0, 300.0]), (B, 1))
            assert g.init_feature(px, np.full(B, np.nan), np.array([1, 0, 0], np.uint8))[0] == 1
            stale = (0,)
        before = state(g)
        res = fi.intake_pixel_vel(out, dids, dzd, t(gyro), t(Rf), GYRO_VAR, True, dact).cpu().numpy()
        want = PR.intake_pixel_vel(ts, tabs, ids, zd, fres, gyro, Rf, GYRO_VAR, True, active, stale)
        assert np.array_equal(res, want), (k, res, want)
        live = [b for b in range(B) if b != INACTIVE and b not in stale]
        for b in range(B):
            for i in range(M):
                if b in live:
                    assert (res[b, i] != -1) == PR.is_measurement(int(ids[b, i]), int(fres[b, i]), zd[b, i]), (b, i)
        assert (res[INACTIVE] == -1).all() and (res[live] == 0).sum() >= 3 * len(live)
        after = state(g)
        assert all(np.array_equal(a[INACTIVE], c[INACTIVE]) for a, c in zip(before, after))
        if k == 1:
            assert (fres[live][:, list(FAR)] == orc.MEAS_GATED).all() and (res[live][:, list(FAR)] == orc.MEAS_GATED).all()   # 7500 px/s
            assert (fres[live][:, list(NANPIX)] == orc.MEAS_NAN).all() and (res[live][:, list(NANPIX)] == -1).all()
            assert (fres[live] == orc.MEAS_NEW_FEATURE).any() and (fres[live] == orc.MEAS_INVALID).any()
            compare(g, ts, "after intake_pixel_vel, frame 2")
            for r, tt in zip(ref.r, ts):                       # the restated filters go on from the updated state
                r.f.x[:] = tt.x
                r.f.P[:] = tt.P
        else:
            assert (res[0][ids[0] >= 0] == orc.MEAS_INVALID).all() and (res[0][ids[0] < 0] == -1).all()
            assert all(np.array_equal(a[0], c[0]) for a, c in zip(before, after))
            compare(g, ts, "after intake_pixel_vel, frame 3", only=(1, 2))
        assert g.get_status().max() < 8
        zp, idp = z, ids
    # use_pixel_vel = 0: inactive measurements -- fix_depth only, nothing to fix: bit for bit
    before = state(g)
    res = fi.intake_pixel_vel(fres, ids, zd, gyro, Rf[0, 0], GYRO_VAR, False, active)
    assert set(np.unique(res[2])) == {-1, 0} and (res[INACTIVE] == -1).all() and same_bits(before, state(g))


def test_argument_rules():
    import ctypes as C
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    g = _batch(2, 5, _params())
    fi = v.FrameIntake(g)
    L, h = capi.lib(), fi._h
    ids, zd, fr, R, gy = np.zeros((2, 4), np.int32), np.full((2, 4, 2), 3.0), np.zeros((2, 4), np.int32), np.eye(2) * 100.0, np.zeros((2, 3))
    p = lambda a: C.c_void_p(a.ctypes.data)
    before = state(g)
    f = L.viekf_frame_intake_pixel_vel
    assert f(h, 0, p(ids), p(zd), p(fr), p(gy), p(R), 0, 0.0, 1, None, None, capi.HOST) == capi.ERR_INVALID
    assert f(h, capi.PIXVELS_MAX_M + 1, p(ids), p(zd), p(fr), p(gy), p(R), 0, 0.0, 1, None, None, capi.HOST) == capi.ERR_INVALID
    for k in range(5):
        a = [p(ids), p(zd), p(fr), p(gy), p(R)]
        a[k] = None
        assert f(h, 4, a[0], a[1], a[2], a[3], a[4], 0, 0.0, 1, None, None, capi.HOST) == capi.ERR_INVALID, k
    assert f(h, 4, p(ids), p(zd), p(fr), p(gy), p(R), 3, 0.0, 1, None, None, capi.HOST) == capi.ERR_INVALID
    assert f(h, 4, p(ids), p(zd), p(fr), p(gy), p(R), 0, -1.0, 1, None, None, capi.HOST) == capi.ERR_INVALID
    assert f(h, 4, p(ids), p(zd), p(fr), p(gy), p(R), 0, 0.0, 1, None, None, 7) == capi.ERR_INVALID
    assert same_bits(before, state(g))
    res = fi.intake_pixel_vel(fr, ids, zd, gy, R)                        # host arrays; no id is tracked: INVALID
    assert res.shape == (2, 4) and (res == orc.MEAS_INVALID).all() and same_bits(before, state(g))


# ---- closed loop ----------------------------------------------------------------------------------------------------------
# The bound on the velocity NEES e^T P_vv^-1 e: chi-square with 3 degrees of freedom exceeds 25.9 with probability 1e-5.  The run
# looks at 8 filters on 13 frames, so a consistent filter leaves it with probability about 1e-3.
NEES_BOUND = 25.9


def _fly(with_pixel_vel):
    import torch
    import vi_ekf_amd as v
    Bc, Nc, frames = 8, 12, 25                                         # 1 s at 250 / 25 Hz
    p = _params(use_keyframe_reset=False)
    bs = v.BatchSimulator(Bc, p, max_features=Nc, seed=np.arange(1, Bc + 1))
    g = _batch(Bc, Nc, p)
    g.use_torch_stream()
    fi = v.FrameIntake(g)
    R_pix = torch.diag(torch.tensor([10.0, 10.0], dtype=torch.float64)).cuda()
    # the flow's noise: two pixel errors of 0.5 px over 0.04 s, 17.7 px/s -- and the difference is the velocity half a frame ago,
    # which at these accelerations is of the same size: 30 px/s
    R_flow = torch.diag(torch.tensor([900.0, 900.0], dtype=torch.float64)).cuda()
    dt = torch.full((10, Bc), bs.dt, dtype=torch.float64, device="cuda")
    dt_frame = torch.full((Bc,), 10 * bs.dt, dtype=torch.float64, device="cuda")
    zp = idp = None
    nees, applied = [], 0
    for f in range(frames):
        u = bs.step(10, device=True)
        g.step_n(u, dt, None, None, None)
        z, ids, cnt, dep, _ = bs.camera(Nc, device=True)
        out = fi.intake(z, ids, R_pix)
        if with_pixel_vel and zp is not None:
            zdot = v.pixel_flow(g, zp, idp, z, ids, dt_frame)
            gyro = u[9, :, 3:6].contiguous()
            res = fi.intake_pixel_vel(out, ids, zdot, gyro, R_flow, 1e-4)
            assert zdot.is_cuda and res.is_cuda
            applied += int((res == 0).sum().item())
        zp, idp = z, ids
        if bs.t > 0.5:                                         # (the test's own look at the state, not part of the loop)
            x, P, (st, _) = g.get_state(), g.get_covariance(), bs.truth()
            e = x[:, 3:6] - st[:, 7:10]
            nees.append([e[b] @ np.linalg.solve(P[b, 3:6, 3:6], e[b]) for b in range(Bc)])
    x, (st, _) = g.get_state(), bs.truth()
    tracked, ln = fi.tracked(device=True)
    diag = v.consistency(g, bs.truth_state(tracked))
    g.sync()
    assert (diag["info"].cpu().numpy() == 0).all() and np.isfinite(diag["nees"].cpu().numpy()).all()
    P = g.get_covariance()
    return dict(nees=np.array(nees), verr=np.linalg.norm(x[:, 3:6] - st[:, 7:10], axis=1), status=g.get_status(), x=x, applied=applied,
                vsigma=np.sqrt(np.trace(P[:, 3:6, 3:6], axis1=1, axis2=2)))


def test_closed_loop():
    """B = 8, N = 12, 1 s of flight at the simulator's defaults, every array between the calls a CUDA tensor.  The run without the
    pixel-velocity step is held to the bound first; the run with it stays inside the same bound, ends with a velocity error that
    (the mean over the eight filters of |v - v_true|) is not larger, and raises no NaN, blow-up or negative-depth bit."""
    base = _fly(False)
    print("without PIXEL_VEL: worst velocity NEES %.3f, |v error| at the end %s" % (base["nees"].max(), np.round(base["verr"], 4)))
    assert base["nees"].max() <= NEES_BOUND and not base["status"].any()
    run = _fly(True)
    print("with PIXEL_VEL:    worst velocity NEES %.3f, |v error| at the end %s, %d entries applied"
          % (run["nees"].max(), np.round(run["verr"], 4), run["applied"]))
    assert run["applied"] >= 8 * 12 * 12
    assert not np.isnan(run["x"][:, :17]).any() and not run["status"].any()
    assert run["nees"].max() <= NEES_BOUND
    # The error at the end: each filter's is ONE draw of its noise, of the size of its own standard deviation, so the sign of
    # the difference of two such draws is not determined per filter.  Asserted: the mean over the eight filters is not larger,
    # and no filter ends more than three of its own standard deviations (sqrt trace P_vv) above its error in the other run.
    assert run["verr"].mean() <= base["verr"].mean()
    assert (run["verr"] <= base["verr"] + 3.0 * run["vsigma"]).all(), (run["verr"], base["verr"], run["vsigma"])
