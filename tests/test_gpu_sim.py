"""The batched flight simulator (include/viekf_sim.h, vi_ekf_amd.BatchSimulator) against the numpy restatement
tests/sim_ref.py, by the project's parity rule: max|d| <= 1e-9 max|ref| per array, integers bit-exact --
truth, IMU stream, feature lists, frames, the true state in the filter's layout -- and its outputs as the inputs of the
existing entry points: step_n, KLTTracker.load_image, SeqVIEKF, diag.consistency."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import sim_ref as R

pytestmark = pytest.mark.gpu

TICKS, EVERY = 1000, 10            # 4 s at 250 Hz, a frame every 10 ticks
SIGMAS = dict(accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5)
QUIET = dict(accel_sigma=0.0, gyro_sigma=0.0, pix_sigma=0.0)


def _params(**kw):
    p = dict(orc.EKF_YAML)
    p["use_keyframe_reset"] = False
    p.update(kw)
    return p


def _sim(B, params, cfg=None, lm=None, **kw):
    import vi_ekf_amd as v
    per = {} if cfg is None else {k: cfg[k] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    bs = v.BatchSimulator(B, params, **per, **kw)
    if lm is not None:
        bs.set_landmarks(lm)
    return bs


def close(a, ref, rel=1e-9):
    """the parity rule, NaN padding in the same places"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape and np.array_equal(np.isnan(a), np.isnan(ref))
    if not np.isfinite(ref).any():
        return True
    return np.nanmax(np.abs(a - ref)) <= rel * np.nanmax(np.abs(ref))


@functools.lru_cache(maxsize=None)
def landmarks():
    return R.jittered_landmarks(77)


@functools.lru_cache(maxsize=None)
def five():
    """the five vehicles of sim_ref.FIVE flown once on the CPU for 4 s: truth and t per tick, the IMU sample with and
    without noise (noise never feeds back into the truth), and a frame every 10 ticks for N = 8 and N = 12"""
    p, lm = _params(), landmarks()
    fly = R.vehicles(R.FIVE, p, 8, lm)
    cams = {N: R.vehicles(R.FIVE, p, N, lm) for N in (8, 12)}
    B = len(fly)
    out = dict(u=np.empty((TICKS + 1, B, 6)), u_quiet=np.empty((TICKS + 1, B, 6)), state=np.empty((TICKS + 1, B, 13)),
               t=np.empty((TICKS + 1, B)), frames={N: [] for N in cams})
    for k in range(TICKS + 1):
        for b, s in enumerate(fly):
            if k:                                        # (advance(1) without its own imu() call)
                s._control()
                s._step_truth()
                s.k += 1
                s.t = s.k * s.dt
            out["u"][k, b], out["u_quiet"][k, b], out["state"][k, b], out["t"][k, b] = s.imu(), s.imu(noise=False), s.state(), s.t
        if k and k % EVERY == 0:
            for N, cs in cams.items():
                fr = []
                for s, c in zip(fly, cs):
                    c.copy_truth_from(s)
                    fr.append(c.camera_padded(N))
                out["frames"][N].append([np.stack([f[i] for f in fr]) for i in range(5)])
    out["next_id"] = {N: [c.next_feat_id for c in cs] for N, cs in cams.items()}
    return out


# -- step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise", [False, True])
def test_step_truth_and_imu(noise):
    ref = five()
    bs = _sim(5, _params(), R.FIVE, landmarks(), max_features=12, **(SIGMAS if noise else QUIET))
    uref = ref["u"] if noise else ref["u_quiet"]
    assert close(bs.imu(), uref[0])                      # sim.imu() before the first run()
    assert np.array_equal(bs.imu(), bs.imu())            # sampling a tick twice gives the same sample
    us, sts, ts = [], [], []
    for i in range(50):
        us.append(bs.step(10))
        st, t = bs.truth()
        sts.append(st)
        ts.append(t)
    assert bs.tick == 500
    u, st, t = np.concatenate(us), np.stack(sts), np.stack(ts)
    assert close(u, uref[1:501])
    assert close(st, ref["state"][10:501:10])
    assert close(t, ref["t"][10:501:10], rel=1e-15)
    if noise:
        assert np.abs(u - ref["u_quiet"][1:501]).max() > 0.1     # (and the noise is there)


def test_step_k_is_k_steps_of_one():
    a = _sim(5, _params(), R.FIVE, landmarks(), **SIGMAS)
    b = _sim(5, _params(), R.FIVE, landmarks(), **SIGMAS)
    for i in range(3):
        ua = a.step(10)
        ub = np.concatenate([b.step(1) for _ in range(10)])
        assert np.array_equal(ua, ub)
        assert np.array_equal(a.truth()[0], b.truth()[0]) and np.array_equal(a.truth()[1], b.truth()[1])
    a.reset()
    c = _sim(5, _params(), R.FIVE, landmarks(), **SIGMAS)
    assert np.array_equal(a.step(7), c.step(7))          # reset starts the same flight again


def test_device_imu_stream_feeds_step_n_as_it_is():
    """u written with VIEKF_DEVICE is the u of viekf_batch_step_n / _propagate_n_to: no copy, no re-layout"""
    import torch
    import vi_ekf_amd as v
    B, N, K = 5, 4, 10
    bs = _sim(B, _params(), R.FIVE, landmarks(), **SIGMAS)
    u = bs.step(K, device=True)
    assert u.is_cuda and tuple(u.shape) == (K, B, 6) and u.dtype == torch.float64 and u.is_contiguous()
    dt = torch.full((K, B), bs.dt, dtype=torch.float64, device=u.device)
    g, h = v.BatchVIEKF(B, N, _params()), v.BatchVIEKF(B, N, _params())
    torch.cuda.synchronize()                             # (dt was filled on torch's stream, the batch runs on its own)
    g.step_n(u, dt, None, None, None)
    g.sync()
    h.step_n(u.cpu().numpy(), dt.cpu().numpy(), None, None, None)
    assert np.array_equal(g.get_state(), h.get_state()) and np.array_equal(g.get_covariance(), h.get_covariance())
    assert not np.array_equal(g.get_state()[:, :10], np.tile(np.asarray(_params()["x0"], float)[:10], (B, 1)))
    b2 = _sim(B, _params(), R.FIVE, landmarks(), **SIGMAS)
    assert np.array_equal(u.cpu().numpy(), b2.step(K))   # the device route writes what the host route writes


# -- camera ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [8, 12])
def test_camera_frames(N):
    ref = five()
    assert max(ref["next_id"][N]) > N                    # (a vehicle lost features and re-acquired them under new ids)
    bs = _sim(5, _params(), R.FIVE, landmarks(), max_features=12, **SIGMAS)
    for f in range(TICKS // EVERY):
        bs.step(EVERY)
        z, ids, cnt, dep, lm = bs.camera(N)
        rz, rids, rcnt, rdep, rlm = ref["frames"][N][f]
        assert np.array_equal(cnt, rcnt), f
        assert np.array_equal(ids, rids) and np.array_equal(lm, rlm), f
        assert close(z, rz) and close(dep, rdep), f
    z2 = bs.camera(N)[0]
    assert np.array_equal(z, z2)                         # the same tick again: the same pixel noise


# -- batch independence ------------------------------------------------------------------------------------------------------
def test_a_vehicle_does_not_depend_on_its_batch():
    B, same = 300, (0, 150, 299)
    seed = np.arange(1, B + 1, dtype=np.uint64)
    radius = 0.35 + 0.004 * np.arange(B)
    period = 6.0 + 0.01 * np.arange(B)
    ab = np.tile([0.05, -0.04, 0.03], (B, 1)) * np.linspace(0.5, 1.5, B)[:, None]
    gb = np.tile([0.004, -0.003, 0.002], (B, 1)) * np.linspace(1.5, 0.5, B)[:, None]
    one = dict(seed=[2 ** 33 + 5], radius=[0.9], period=[7.0], accel_bias=[[0.02, 0.01, -0.03]], gyro_bias=[[0.001, -0.002, 0.003]])
    for s in same:
        seed[s], radius[s], period[s], ab[s], gb[s] = one["seed"][0], one["radius"][0], one["period"][0], one["accel_bias"][0], one["gyro_bias"][0]
    big = _sim(B, _params(), dict(seed=seed, radius=radius, period=period, accel_bias=ab, gyro_bias=gb), landmarks(), **SIGMAS)
    small = _sim(1, _params(), one, landmarks(), **SIGMAS)
    for rnd in range(3):
        ub, us = big.step(10), small.step(10)
        zb, ib, cb, db, lb = big.camera(8)
        zs, is_, cs, ds, ls = small.camera(8)
        frames = [(big.render(w, h, depth=True), small.render(w, h, depth=True)) for (w, h) in ((70, 50), (160, 120))]
        for s in same:
            assert np.array_equal(ub[:, s], us[:, 0]), (rnd, s)
            assert np.array_equal(zb[s], zs[0], equal_nan=True) and np.array_equal(ib[s], is_[0]) and cb[s] == cs[0]
            assert np.array_equal(db[s], ds[0], equal_nan=True) and np.array_equal(lb[s], ls[0])
            for (gb_, ds_) in frames:
                assert np.array_equal(gb_[0][s], ds_[0][0]) and np.array_equal(gb_[1][s], ds_[1][0])
        assert not np.array_equal(ub[:, 1], ub[:, 0])    # (other vehicles fly something else)
    assert cs[0] == 8


def test_per_vehicle_landmark_fields_and_device_outputs():
    """one landmark field per vehicle ([B][L][3]) gives every vehicle what a simulator of its own with that field gives;
    camera() into device tensors gives the bytes of the host route"""
    B = 3
    fields = np.stack([R.jittered_landmarks(100 + b) for b in range(B)])
    cfg = {k: v[:B] for k, v in R.FIVE.items()}
    many = _sim(B, _params(), cfg, fields, **SIGMAS)
    ones = [_sim(1, _params(), {k: v[b:b + 1] for k, v in cfg.items()}, fields[b], **SIGMAS) for b in range(B)]
    for rnd in range(3):
        many.step(10)
        out = many.camera(8)
        img = many.render(70, 50, depth=True)
        for b, o in enumerate(ones):
            o.step(10)
            for x, y in zip(out, o.camera(8)):
                assert np.array_equal(x[b], y[0], equal_nan=True), (rnd, b)
            for x, y in zip(img, o.render(70, 50, depth=True)):
                assert np.array_equal(x[b], y[0])
    assert not np.array_equal(out[4][0], out[4][1])      # (the fields differ, and so do the landmarks picked)
    many.set_landmarks(fields[0])                        # back to one field for all
    assert np.array_equal(many.camera(8)[4][1], _sim(1, _params(), {k: v[1:2] for k, v in cfg.items()}, fields[0], **SIGMAS).camera(8)[4][0])
    many.step(10)
    dev = many.camera(8, device=True)
    host = many.camera(8)
    assert all(d.is_cuda for d in dev)
    for d, h in zip(dev, host):
        assert np.array_equal(d.cpu().numpy(), h, equal_nan=True)


# -- render ------------------------------------------------------------------------------------------------------------------
TWO = dict(seed=[1, 2], radius=[0.35, 1.2], period=[8.0, 6.0], accel_bias=[[0.05, -0.04, 0.03]] * 2, gyro_bias=[[0.004, -0.003, 0.002]] * 2)


@pytest.mark.parametrize("W,H", [(640, 480), (70, 50)])
def test_render_every_pixel(W, H):
    """70 x 50 is no multiple of the 64 x 16 tile nor of four pixels per thread (pairs are stored), with a ragged last row of
    tiles; the image centre moves with the size.  t = 0 and mid-flight."""
    p = _params(cam_center=[W * 0.5 - 4.2, H * 0.5 + 1.1])
    lm = landmarks()
    refs = R.vehicles(TWO, p, 8, lm)
    bs = _sim(2, p, TWO, lm, **SIGMAS)
    for K in (0, 300):
        if K:
            bs.step(K)
            for r in refs:
                r.advance(K)
        assert close(bs.truth()[0], np.stack([r.state() for r in refs]))
        img, dmm = bs.render(W, H, depth=True)
        only = bs.render(W, H)
        assert img.shape == (2, H, W) and img.dtype == np.uint8 and dmm.dtype == np.float32 and np.array_equal(only, img)
        for b, r in enumerate(refs):
            val, rng, hit = r.render_values(W, H)
            assert hit.all() and rng.max() <= 10e3       # every ray hits the ground within 10 m: fp64 error << 1e-6 there
            err = np.abs(img[b].astype(np.float64) - val)
            assert err.max() <= 0.5 + 1e-6, (K, b, err.max())
            assert (np.abs(dmm[b].astype(np.float64) - rng) <= 2.0 ** -23 * rng).all()
            assert img[b].std() > 5.0                    # (a textured image)


def test_render_rays_that_miss():
    """pitched by 93.4 degrees: the horizon crosses the image -- grey 30 and +inf exactly where the reference misses"""
    p = _params(cam_center=[35.0, 25.0], x0=[0, 0, -2, 0, 0, 0, np.cos(0.815), 0, np.sin(0.815), 0, 0, 0, 0, 0, 0, 0, 0.1])
    lm = landmarks()
    refs = R.vehicles(TWO, p, 8, lm)
    bs = _sim(2, p, TWO, lm)
    img, dmm = bs.render(70, 50, depth=True)
    for b, r in enumerate(refs):
        val, rng, hit = r.render_values(70, 50)
        assert hit.any() and not hit.all()
        assert (img[b][~hit] == 30).all() and np.isposinf(dmm[b][~hit]).all()
        assert np.isfinite(dmm[b][hit]).all()
        near = hit & (rng <= 10e3)
        assert (np.abs(img[b].astype(np.float64) - val)[near] <= 0.5 + 1e-6).all()


# -- truth state -------------------------------------------------------------------------------------------------------------
def test_truth_state_in_the_filters_layout():
    """Features initialised by viekf_batch_init_feature from noise-free pixels and depths are the true features.  The camera
    has square pixels here: init_feature scales the pixel's y by f_y / f_x (vi_ekf_feat.cpp:17), which is the true bearing
    only then (tests/test_sim_ref_cpu.py has the yaml's camera: up to 1e-3 rad of initialisation error, not truth)."""
    import vi_ekf_amd as v
    B, N = 5, 8
    p = _params(focal_len=[611.1864013671875, 611.1864013671875])
    lm = landmarks()
    bs = _sim(B, p, R.FIVE, lm, max_features=N, **QUIET)
    refs = R.vehicles(R.FIVE, p, N, lm, **QUIET)
    bs.step(100)
    z, ids, cnt, dep, _ = bs.camera(N)
    assert (cnt == N).all()
    g = v.BatchVIEKF(B, N, p)
    for j in range(N):
        assert g.init_feature(np.ascontiguousarray(z[:, j]), np.ascontiguousarray(dep[:, j])).all()
    x = g.get_state()
    xt = bs.truth_state(ids)
    assert xt.shape == (B, g.nx)
    for b in range(B):
        for j in range(N):
            f = slice(17 + 5 * j, 21 + 5 * j)
            assert np.abs(orc.q_feat_boxminus(xt[b, f], x[b, f])).max() <= 1e-9
            assert abs(xt[b, 21 + 5 * j] - x[b, 21 + 5 * j]) <= 1e-12 * abs(x[b, 21 + 5 * j])
    st, _ = bs.truth()
    assert np.array_equal(xt[:, 0:3], st[:, 0:3]) and np.array_equal(xt[:, 3:6], st[:, 7:10]) and np.array_equal(xt[:, 6:10], st[:, 3:7])
    assert np.array_equal(xt[:, 10:13], np.asarray(R.FIVE["accel_bias"])) and np.array_equal(xt[:, 13:16], np.asarray(R.FIVE["gyro_bias"]))
    assert (xt[:, 16] == 0.1).all()
    # against the restatement
    for r in refs:
        r.advance(100)
        r._camera()
    assert close(xt, np.stack([r.truth_state(ids[b]) for b, r in enumerate(refs)]))
    # the same call with the yaml's camera (f_x != f_y), which the comparison with init_feature above cannot use
    py = _params()
    by, ry = _sim(2, py, TWO, lm, max_features=N, **QUIET), R.vehicles(TWO, py, N, lm, **QUIET)
    by.step(100)
    idy = by.camera(N)[1]
    for r in ry:
        r.advance(100)
        r._camera()
    assert close(by.truth_state(idy), np.stack([r.truth_state(idy[b]) for b, r in enumerate(ry)]))
    # fly on until the widest circle has dropped some of these ids: their slots turn into five NaNs
    for _ in range(60):
        bs.step(10)
        ids2 = bs.camera(N)[1]
    gone = np.array([[i not in ids2[b] for i in ids[b]] for b in range(B)])
    assert gone.any() and not gone.all()
    asked = ids.copy()
    asked[0, 0] = -1
    gone[0, 0] = True
    xt2 = bs.truth_state(asked)
    feat = xt2[:, 17:].reshape(B, N, 5)
    assert np.isnan(feat[gone]).all() and np.isfinite(feat[~gone]).all() and np.isfinite(xt2[:, :17]).all()
    out = v.consistency(g, xt2)
    assert (out["info"] == 0).all() and np.isfinite(out["nees"][:, :3]).all() and np.isfinite(out["logdet"]).all()
    # the device route gives the same numbers
    import torch
    xd = bs.truth_state(torch.as_tensor(asked).cuda())
    assert xd.is_cuda and np.array_equal(xd.cpu().numpy(), xt2, equal_nan=True)


# -- frames to the tracker, on the device -----------------------------------------------------------------------------------
def test_rendered_frames_feed_the_tracker_on_the_device():
    import vi_ekf_amd as v
    B, W, H, MF = 2, 640, 480, 12
    bs = _sim(B, _params(), TWO, landmarks(), **SIGMAS)
    dev, host = v.KLTTracker(B, W, H, max_features=MF, radius=30), v.KLTTracker(B, W, H, max_features=MF, radius=30)
    for f in range(3):
        if f:
            bs.step(10)
        img, dmm = bs.render(W, H, depth=True, device=True)
        assert img.is_cuda and dmm.is_cuda
        fd, idd, cd = dev.load_image(img)
        assert fd.is_cuda
        fh, idh, ch = host.load_image(img.cpu().numpy())
        assert np.array_equal(fd.cpu().numpy(), fh, equal_nan=True) and np.array_equal(idd.cpu().numpy(), idh)
        assert np.array_equal(cd.cpu().numpy(), ch) and (ch > 0).all()
        zd = dev.sample_depth(dmm, 1.5)
        zh = host.sample_depth(dmm.cpu().numpy(), 1.5)
        assert np.array_equal(zd.cpu().numpy(), zh, equal_nan=True) and np.isfinite(zh).any()
        assert np.array_equal(img.cpu().numpy(), bs.render(W, H))       # (and the host route renders the same bytes)


# -- closed loop --------------------------------------------------------------------------------------------------------------
def test_closed_loop_through_the_sequencer():
    """four vehicles on different trajectories and seeds drive four filters of one SeqVIEKF for 2 s (250 Hz IMU, 25 Hz frames,
    N = 8); after t = 1 s every filter stays inside the bounds of test_sim_end_to_end.py's sequencer test, and the
    simulator's true state makes the consistency diagnostics finite.  tests/test_sim_ref_cpu.py flies the same scenario
    through the restated stack."""
    import vi_ekf_amd as v
    B, N, p = 4, 8, _params()
    bs = _sim(B, p, R.LOOP, landmarks(), max_features=N, **SIGMAS)
    g = v.BatchVIEKF(B, N, dict(p, keyframe_overlap_threshold=0.8, name="sim"))
    sg = v.SeqVIEKF(g, state_hist=64, meas_hist=200)
    R_pix = np.diag([10.0, 10.0])
    sg.propagate_state(bs.imu(), 0.0)                    # vi_ekf_test.cpp:57
    worst = np.zeros((B, 3))
    ids = None
    for f in range(50):
        u = bs.step(10)
        for i in range(10):
            sg.propagate_state(u[i], (bs.tick - 10 + i + 1) * bs.dt)
        z, ids, cnt, dep, _ = bs.camera(N)
        sg.handle_measurements()
        sg.keep_only_features(ids)
        sg.add_frame(bs.t, z, R_pix, ids)                # (a NaN-padded slot answers MEAS_NAN)
        sg.handle_measurements()
        if bs.t > 1.0:
            x, (st, _) = g.get_state(), bs.truth()
            assert not np.isnan(x[:, :17]).any()
            for b in range(B):
                e = [np.abs(x[b, 0:3] - st[b, 0:3]).max(), np.abs(x[b, 3:6] - st[b, 7:10]).max(),
                     np.degrees(np.abs(orc.q_boxminus(x[b, 6:10], st[b, 3:7])).max())]
                worst[b] = np.maximum(worst[b], e)
    assert (worst < np.array(R.LOOP_BOUNDS)).all(), worst
    assert (worst > 0).all() and (cnt == N).all()
    x = g.get_state()
    ln = g.get_len_features()
    assert not np.isnan(np.concatenate([x[b, :17 + 5 * ln[b]] for b in range(B)])).any()
    tracked = sg.tracked_features()
    slots = np.full((B, N), -1, np.int32)
    for b in range(B):
        slots[b, :len(tracked[b])] = tracked[b]          # the filter's slot order, which need not be the camera's
    out = v.consistency(g, bs.truth_state(slots))
    assert (out["info"] == 0).all() and np.isfinite(out["nees"]).all() and np.isfinite(out["logdet"]).all()


# -- argument rules -----------------------------------------------------------------------------------------------------------
def test_argument_rules():
    import vi_ekf_amd as v
    from vi_ekf_amd import capi, simbatch
    bs = _sim(2, _params(), max_features=8)
    L, h = bs._L, bs._h
    buf = np.zeros(2 * 64 * 64 * 8, np.uint8)
    ptr = C.c_void_p(buf.ctypes.data)

    def refused(rc, word):
        assert rc == capi.ERR_INVALID and word in L.viekf_last_error().decode(), (rc, L.viekf_last_error())

    refused(L.viekf_sim_step(h, 1, None, capi.HOST), "null")
    refused(L.viekf_sim_imu(h, None, capi.HOST), "null")
    refused(L.viekf_sim_camera(h, 8, None, ptr, ptr, None, None, capi.HOST), "null")
    refused(L.viekf_sim_camera(h, 8, ptr, ptr, None, None, None, capi.HOST), "null")
    refused(L.viekf_sim_render(h, 64, 64, None, None, capi.HOST), "null")
    refused(L.viekf_sim_get_truth(h, None, None, capi.HOST), "null")
    refused(L.viekf_sim_truth_state(h, None, 0, None, capi.HOST), "null")
    refused(L.viekf_sim_set_landmarks(h, None, 0, capi.HOST), "null")
    refused(L.viekf_sim_camera(h, 9, ptr, ptr, ptr, None, None, capi.HOST), "num_features")
    refused(L.viekf_sim_camera(h, 0, ptr, ptr, ptr, None, None, capi.HOST), "num_features")
    refused(L.viekf_sim_truth_state(h, ptr, 9, ptr, capi.HOST), "max_features")
    refused(L.viekf_sim_step(h, 0, ptr, capi.HOST), "K must")
    refused(L.viekf_sim_step(h, -3, ptr, capi.HOST), "K must")
    refused(L.viekf_sim_render(h, 63, 64, ptr, None, capi.HOST), "even")     # pixels are stored in pairs
    refused(L.viekf_sim_render(h, 2, 64, ptr, None, capi.HOST), "width")
    refused(L.viekf_sim_render(h, 64, 64, ptr, None, 7), "where")
    import torch
    t = torch.zeros(2 * 6 + 2, dtype=torch.float64, device="cuda")           # a device u that is 8- but not 16-byte aligned
    odd = C.c_void_p(t.data_ptr() + 8)
    refused(L.viekf_sim_imu(h, odd, capi.DEVICE), "aligned")
    refused(L.viekf_sim_step(h, 1, odd, capi.DEVICE), "aligned")
    with pytest.raises(v.ViekfError) as e:
        v.BatchSimulator(2, _params(), grid=(-3.0, 0.2, 33))                # L = 1089 > 1024
    assert e.value.code == capi.ERR_INVALID and "1024" in str(e.value)
    assert bs.tick == 0 and np.isfinite(bs.step(1)).all()                    # nothing of this moved the simulator
    assert bs.render(66, 64).shape == (2, 64, 66)                            # an even width that is no multiple of four
    assert sorted(simbatch.SIM_SYMBOLS) == sorted(set(simbatch.SIM_SYMBOLS))
