"""tests/sim_ref.py, the numpy restatement the batched simulator (include/viekf_sim.h) is tested against, on its own: it is
sim.Simulator where no noise is drawn, its Philox is the standard one, its normals have the moments of normals, its
renderer restates render() to the bit, and the closed loop the GPU test flies stays inside the bounds on the CPU."""
import ctypes as C
import os
import re

import numpy as np

from oracle import oracle as orc
from oracle import seq_oracle as so
from tests import sim_ref as R
from vi_ekf_amd import capi, sim as S, simbatch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _params():
    p = dict(orc.EKF_YAML)
    p["use_keyframe_reset"] = False
    return p


def test_without_noise_the_restatement_is_the_simulator():
    """all sigmas 0: truth, IMU, pixels and ids equal sim.Simulator's over 2 s, with features lost and re-acquired"""
    N = 8
    kw = dict(num_features=N, seed=5, tmax=2.0, radius=1.5, period=4.0, cam_rate=12.5, accel_sigma=0.0, gyro_sigma=0.0, pix_sigma=0.0)
    a, b = S.Simulator(_params(), **kw), R.RefSimulator(_params(), **kw)
    la, lb = [], []
    for s, log in ((a, la), (b, lb)):
        s.register_imu_cb(lambda t, z, Rm, log=log, s=s: log.append(("imu", t, z.copy(), s.state().copy())))
        s.register_feat_cb(lambda t, z, ids, Rm, log=log: log.append(("feat", t, z.copy(), list(ids))))
    assert np.array_equal(a.imu(), b.imu())
    for x, y in zip(a.project(), S.Simulator.project(b)):      # (the restated projection is the inherited one)
        assert np.array_equal(x, y)
    while a.run():
        assert b.run()
    assert not b.run() and len(la) == len(lb) == 500 + 25
    for ea, eb in zip(la, lb):
        assert ea[0] == eb[0] and ea[1] == eb[1]
        assert np.array_equal(ea[2], eb[2])
        if ea[0] == "imu":
            assert np.array_equal(ea[3], eb[3])
        else:
            assert ea[3] == eb[3]
    assert a.next_feat_id == b.next_feat_id and a.next_feat_id > N      # (features were lost and re-acquired)
    # advance() is run() without the callbacks
    c = R.RefSimulator(_params(), **kw)
    u = c.advance(500)
    assert np.array_equal(u, np.stack([e[2] for e in lb if e[0] == "imu"])) and np.array_equal(c.state(), b.state())


def test_philox_known_answers():
    """philox4x32-10.  The first two are the vectors of Random123's kat_vectors file (zero counter and key; all ones); all
    four were confirmed against an independent implementation, at::Philox4_32 of ATen/core/PhiloxRNGEngine.h as shipped
    with torch (seed = key, offset = counter words 0 1, subsequence = counter words 2 3) -- except the all-ones vector,
    which that engine's offset arithmetic cannot address and which is quoted from the vector file."""
    kat = [
        ((0, 0), (0, 0, 0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
        ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
        ((0x299f31d0, 0xa4093822), (0, 0, 0x13198a2e, 0x243f6a88), "c0331b72 e6786def 907dfd7c c9230399"),
        ((7, 0), (0, 0, 5, 9), "ac8c7d1d 74ea9c8d 5e2b9ec5 252469d7"),
    ]
    for key, ctr, want in kat:
        assert " ".join("%08x" % int(w) for w in R.philox4x32_10(key, ctr)) == want, (key, ctr)
    # vectorised over counters and keys = one at a time
    blk = np.arange(5, dtype=np.uint64)
    w = R.philox4x32_10((3, 4), (9, 1, blk, 0))
    for i in range(5):
        assert [int(x[i]) for x in w] == [int(x) for x in R.philox4x32_10((3, 4), (9, 1, i, 0))]


def test_uniforms_are_inside_the_open_interval():
    z, o = np.uint32(0), np.uint32(0xffffffff)
    assert R.uniform53(z, z) == 2.0 ** -54 and R.uniform53(o, o) == 1.0 - 2.0 ** -54
    assert np.isfinite(np.sqrt(-2.0 * np.log(R.uniform53(z, z))))


def test_moments_of_the_restated_normals():
    """98,304 draws (256 vehicles x 64 ticks x 6): mean within 5 / sqrt(n), variance within 5 sqrt(2 / n), lag-one
    correlation across consecutive ticks within 5 / sqrt(n).  The seeds are those the GPU tests use (b + 1, and the
    scenario seeds of sim_ref); the GPU inherits the result through its parity with the restatement."""
    for seeds in (np.arange(1, 257, dtype=np.uint64), np.array((R.FIVE["seed"] + R.LOOP["seed"]) * 32, dtype=np.uint64)[:256] + np.repeat(np.arange(32, dtype=np.uint64) * 1000, 8)):
        n = R.imu_normals(seeds[:, None], np.arange(1, 65, dtype=np.uint64)[None, :])      # [256][64][6]
        assert n.shape == (256, 64, 6)
        cnt = n.size
        assert abs(n.mean()) < 5.0 / np.sqrt(cnt)
        assert abs(n.var() - 1.0) < 5.0 * np.sqrt(2.0 / cnt)
        lag = (n[:, 1:, :] * n[:, :-1, :]).mean()
        assert abs(lag) < 5.0 / np.sqrt(n[:, 1:, :].size)
        # pixel noise: another stream of the same generator
        px = np.stack(R.normal_pair(seeds[:, None], 10, R.STREAM_PIX, np.arange(192, dtype=np.uint64)[None, :]))
        assert abs(px.mean()) < 5.0 / np.sqrt(px.size) and abs(px.var() - 1.0) < 5.0 * np.sqrt(2.0 / px.size)


def test_noise_is_addressed_not_drawn():
    """the same tick sampled twice gives the same sample (the stated difference from sim.py); another tick, seed or
    landmark gives another"""
    s = R.RefSimulator(_params(), num_features=6, seed=3)
    assert np.array_equal(s.imu(), s.imu())
    z1, ids1, _ = s._camera()
    z2, ids2, _ = s._camera()
    assert np.array_equal(z1, z2) and ids1 == ids2
    u0 = s.imu()
    s.advance(1)
    assert not np.array_equal(u0, s.imu())
    assert not np.array_equal(R.imu_normals(3, 0), R.imu_normals(4, 0))
    assert not np.array_equal(R.imu_normals(3, 0), R.imu_normals(3 + 2 ** 32, 0))     # (the high half of the seed is key too)


def test_restated_render_is_render():
    """render_values() rounds to render()'s image and depth bit for bit, at t = 0 and mid-flight, with and without misses"""
    p = _params()
    s = R.RefSimulator(p, num_features=6, seed=2, radius=0.9)
    for K in (0, 300):
        s.advance(K)
        for (w, h) in ((70, 50), (160, 120)):
            img, dmm = s.render(w, h, depth=True)
            val, rng, hit = s.render_values(w, h)
            assert np.array_equal(np.clip(np.rint(val), 0, 255).astype(np.uint8), img)
            assert np.array_equal(rng.astype(np.float32), dmm) and np.array_equal(hit, np.isfinite(dmm))
    # pitched by 93.4 degrees with the image centre moved into the small frame: the horizon crosses the image
    tilted = dict(p, cam_center=[35.0, 25.0], x0=[0, 0, -2, 0, 0, 0, np.cos(0.815), 0, np.sin(0.815), 0, 0, 0, 0, 0, 0, 0, 0.1])
    s = R.RefSimulator(tilted, seed=2)
    img, dmm = s.render(70, 50, depth=True)
    val, rng, hit = s.render_values(70, 50)
    assert hit.any() and not hit.all()
    assert np.array_equal(np.clip(np.rint(val), 0, 255).astype(np.uint8), img) and np.array_equal(rng.astype(np.float32), dmm)
    assert (img[~hit] == 30).all()


def test_truth_state_is_what_init_feature_gives_for_a_square_pixel_camera():
    """the bearing of the true state is from_two_unit_vectors(e_z, p_c / |p_c|).  VIEKF::init_feature scales the pixel's y
    by f_y / f_x (vi_ekf_feat.cpp:17), which is the true bearing only for f_x == f_y: with a square-pixel camera the
    oracle's init_feature from the noise-free pixel gives the same quaternion; with the yaml's camera (f_y / f_x - 1 =
    6e-4) it differs by up to 1e-3 rad, which is the reference's initialisation error and not part of the truth."""
    N = 6
    for fy, bound_lo, bound_hi in ((611.1864013671875, 0.0, 1e-12), (611.5557861328125, 1e-6, 2e-3)):
        p = dict(_params(), focal_len=[611.1864013671875, fy])
        s = R.RefSimulator(p, num_features=N, seed=4, pix_sigma=0.0)
        s.advance(100)
        z, ids, depth = s._camera()
        x = s.truth_state(ids + [-1, 12345])
        assert x.size == 17 + 5 * (N + 2) and np.isnan(x[17 + 5 * N:]).all()
        f = orc.OracleFilter(N).init(**p)
        worst = 0.0
        for j in range(N):
            assert f.init_feature(z[j], j, depth[j])
            qf, rho = f.x[17 + 5 * j: 21 + 5 * j], f.x[21 + 5 * j]
            worst = max(worst, np.abs(orc.q_feat_boxminus(x[17 + 5 * j: 21 + 5 * j], qf)).max())
            assert abs(rho - x[21 + 5 * j]) <= 1e-12 * abs(rho)
        assert bound_lo <= worst <= bound_hi, (fy, worst)
        assert np.array_equal(x[0:3], s.pos) and np.array_equal(x[3:6], s.vel) and np.array_equal(x[6:10], s.q)
        assert np.array_equal(x[10:13], s.accel_bias_) and np.array_equal(x[13:16], s.gyro_bias_) and x[16] == 0.1


def test_closed_loop_scenario_stays_inside_the_bounds_on_the_cpu():
    """the CPU twin of tests/test_gpu_sim.py's closed loop: the four vehicles of sim_ref.LOOP, N = 8, 2 s at 250 / 25 Hz,
    through the restated sequencer; after t = 1 s every vehicle stays inside 0.6 m, 0.4 m/s, 2.5 degrees"""
    N, p = 8, _params()
    lm = R.jittered_landmarks(77)
    for sim in R.vehicles(R.LOOP, p, N, lm, tmax=2.0):
        o = so.SeqOracle(orc.OracleFilter(N).init(**p), 0.8, state_hist=64)

        def feat_cb(t, pix, ids, Rm, o=o):
            o.handle_measurements()
            o.keep_only_features(list(ids))
            for i, gid in enumerate(ids):
                o.add_measurement(t, pix[i], orc.FEAT, Rm, True, gid, float("nan"))
            o.handle_measurements()

        sim.register_imu_cb(lambda t, z, Rm, o=o: o.propagate_state(z, t))
        sim.register_feat_cb(feat_cb)
        o.propagate_state(sim.imu(), sim.t)
        worst = np.zeros(3)
        while sim.run():
            if sim.k % 10 == 0 and sim.t > 1.0:
                st, x = sim.state(), o.f.x
                e = [np.abs(x[0:3] - st[0:3]).max(), np.abs(x[3:6] - st[7:10]).max(),
                     np.degrees(np.abs(orc.q_boxminus(x[6:10], st[3:7])).max())]
                worst = np.maximum(worst, e)
        assert not np.isnan(o.f.x).any() and not o.log
        assert (worst < np.array(R.LOOP_BOUNDS)).all(), (sim.seed, worst)
        assert sim.next_feat_id >= N


# -- C ABI without a device -----------------------------------------------------------------------------------------------
def declared_sim_symbols():
    txt = open(os.path.join(ROOT, "include", "viekf_sim.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(viekf_sim_[a-z_0-9]+)\s*\(", txt)))


def test_header_and_library_agree():
    syms = declared_sim_symbols()
    assert sorted(simbatch.SIM_SYMBOLS) == syms and len(syms) == 15
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    assert L.viekf_abi_version() == 1
    cfg = simbatch.SimConfig()
    assert simbatch._bind().viekf_sim_config_default(C.byref(cfg)) == capi.OK
    assert (cfg.imu_rate, cfg.grid_origin, cfg.grid_pitch, cfg.grid_n, cfg.win_u_max, cfg.win_min_depth) == (250.0, -3.0, 0.22, 28, 625.0, 0.2)


def test_argument_validation_without_device():
    L = simbatch._bind()
    out = C.c_void_p()
    p = capi.Params.from_dict(_params())
    cfg = simbatch.SimConfig()
    L.viekf_sim_config_default(C.byref(cfg))
    assert L.viekf_sim_create(4, C.byref(p), C.byref(cfg), 0, None) == capi.ERR_INVALID
    assert L.viekf_sim_create(4, None, C.byref(cfg), 0, C.byref(out)) == capi.ERR_INVALID
    assert L.viekf_sim_create(0, C.byref(p), C.byref(cfg), 0, C.byref(out)) == capi.ERR_INVALID
    cfg.grid_n = 33                                  # L = 1089 > 1024
    assert L.viekf_sim_create(4, C.byref(p), C.byref(cfg), 0, C.byref(out)) == capi.ERR_INVALID
    assert b"1024" in L.viekf_last_error() and not out.value
    assert L.viekf_sim_config_default(None) == capi.ERR_INVALID
    assert L.viekf_sim_destroy(None) == capi.ERR_INVALID
    assert L.viekf_sim_reset(None) == capi.ERR_INVALID
    assert L.viekf_sim_sync(None) == capi.ERR_INVALID
    assert L.viekf_sim_step(None, 1, None, 0) == capi.ERR_INVALID
    assert L.viekf_sim_imu(None, None, 0) == capi.ERR_INVALID
    assert L.viekf_sim_camera(None, 8, None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_sim_render(None, 640, 480, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_sim_get_truth(None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_sim_truth_state(None, None, 0, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
