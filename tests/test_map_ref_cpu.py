"""tests/map_ref.py, the restatement the device-resident landmark map (include/viekf_map.h) is tested against, on its own:
its Jacobian is the derivative of l(x [+] d) for np_twin's boxplus by central differences, Sigma is symmetric positive
definite, l of the simulator's true state IS the landmark, the store keeps its rules, and the restated stack flies the closed
loop of tests/test_gpu_map.py on the CPU, which fixes that test's bound.  And the C ABI without a device."""
import os
import re

import numpy as np

from oracle import np_twin as tw
from oracle import oracle as orc
from tests import map_ref as MR
from tests import sim_ref as R
from vi_ekf_amd import capi, map as vmap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q_B_C, P_B_C = np.asarray(orc.EKF_YAML["q_b_c"], float), np.asarray(orc.EKF_YAML["p_b_c"], float)


def unit(rng, n=4):
    v = rng.normal(0.0, 1.0, n)
    return v / np.linalg.norm(v)


def random_state(rng, N, depth=(1.0, 10.0)):
    """pos and velocity a few metres, attitude and bearings random unit quaternions, depths uniform in `depth`"""
    x = np.zeros(17 + 5 * N)
    x[0:6] = rng.normal(0.0, 2.0, 6)
    x[6:10] = unit(rng)
    x[10:17] = rng.normal(0.0, 0.1, 7)
    for j in range(N):
        x[17 + 5 * j:21 + 5 * j] = unit(rng)
        x[21 + 5 * j] = 1.0 / rng.uniform(*depth)
    return x


def random_spd(rng, n, scale=0.05):
    A = rng.normal(0.0, scale, (n, n))
    return A @ A.T + 1e-4 * np.eye(n)


def test_jacobian_is_the_derivative_for_the_filters_own_boxplus():
    """N = 3, depths 1 .. 10 m, attitudes and bearings random: the analytic J against central differences of
    l(TwinFilter.boxplus(x, d)) with h = 1e-6, within 1e-6 of the largest entry of J (truncation and round-off at that step are
    below 1e-9 relative for these depths).  Also with the camera away from the body (a q_b_c and p_b_c that are not trivial)."""
    rng = np.random.default_rng(5)
    N, h = 3, 1e-6
    p = dict(orc.EKF_YAML)
    worst = 0.0
    for trial in range(40):
        q_b_c, p_b_c = (Q_B_C, P_B_C) if trial % 2 == 0 else (unit(rng), rng.normal(0.0, 0.3, 3))
        f = tw.TwinFilter(N, **dict(p, q_b_c=q_b_c, p_b_c=p_b_c))
        f.len = N
        x = random_state(rng, N)
        for j in range(N):
            J = MR.jacobian(x, j, f.q_b_c, f.p_b_c)
            Jfd = np.zeros((3, 9))
            for c, col in enumerate(MR.idx9(j)):
                d = np.zeros(f.n)
                d[col] = h
                Jfd[:, c] = (MR.landmark(f.boxplus(x, d), j, f.q_b_c, f.p_b_c) - MR.landmark(f.boxplus(x, -d), j, f.q_b_c, f.p_b_c)) / (2 * h)
            # no other column of the error state moves l
            for col in (3, 9, 15, 16 + 3 * ((j + 1) % N)):
                d = np.zeros(f.n)
                d[col] = h
                assert np.array_equal(MR.landmark(f.boxplus(x, d), j, f.q_b_c, f.p_b_c), MR.landmark(x, j, f.q_b_c, f.p_b_c))
            rel = np.abs(J - Jfd).max() / np.abs(J).max()
            worst = max(worst, rel)
            assert rel <= 1e-6, (trial, j, rel, J, Jfd)
    print("analytic J against central differences, worst relative to max|J|: %.3e" % worst)


def test_sigma_is_symmetric_positive_definite():
    rng = np.random.default_rng(6)
    N = 3
    for _ in range(20):
        x, P = random_state(rng, N), random_spd(rng, 16 + 3 * N)
        node = np.concatenate([rng.normal(0.0, 1.0, 3), unit(rng)])
        for j in range(N):
            S = MR.sigma(x, P, j, Q_B_C, P_B_C)
            assert np.allclose(S, S.T, rtol=0, atol=1e-15 * np.abs(S).max()) and np.linalg.eigvalsh(S).min() > 0
            _, Sg = MR.to_global(node, MR.landmark(x, j, Q_B_C, P_B_C), S)
            assert np.allclose(np.linalg.eigvalsh(Sg), np.linalg.eigvalsh(S), rtol=1e-9)     # a rotation of Sigma
            info, nees = MR.cholesky3(S, np.array([0.1, -0.2, 0.3]))
            e = np.array([0.1, -0.2, 0.3])
            assert info == 0 and abs(nees - e @ np.linalg.solve(S, e)) <= 1e-9 * nees
    # only the lower triangle of P is read
    P2 = P + np.triu(rng.normal(0.0, 1.0, P.shape), 1)
    assert np.array_equal(MR.sigma(x, P2, 1, Q_B_C, P_B_C), MR.sigma(x, P, 1, Q_B_C, P_B_C))
    # a matrix that is not positive definite names its pivot
    assert MR.cholesky3(np.diag([1.0, -1.0, 1.0]), np.ones(3))[0] == 2 and np.isnan(MR.cholesky3(np.diag([1.0, -1.0, 1.0]), np.ones(3))[1])
    assert MR.cholesky3(np.diag([np.nan, 1.0, 1.0]), np.ones(3))[0] == 1


def test_landmark_of_the_true_state_is_the_landmark():
    """x = RefSimulator.truth_state (the restatement of viekf_sim_truth_state) of the tracked features: l is the landmark the
    feature was drawn from to 1e-12 m, and MapRef.error against the field is zero to the same"""
    N, p = 8, dict(orc.EKF_YAML)
    lm = R.jittered_landmarks(77)
    seen = 0
    for sim in R.vehicles(R.LOOP, p, N, lm, tmax=2.0):
        for _ in range(3):
            sim.advance(40)
            z, ids, n, depth, lmi = sim.camera_padded()
            xt = sim.truth_state(ids[:n])
            mp = MR.MapRef(N, sim.q_b_c, sim.p_b_c)
            P = random_spd(np.random.default_rng(n), 16 + 3 * N)
            for j in range(n):
                assert np.abs(MR.landmark(xt, j, sim.q_b_c, sim.p_b_c) - lm[lmi[j]]).max() <= 1e-12, (j, lmi[j])
                seen += 1
            x = np.zeros(17 + 5 * N)
            x[:xt.size] = xt
            table = np.full(N, -1, np.int32)
            table[:n] = ids[:n]
            err = mp.error(x, P, n, table, n, lm, ids, lmi)
            assert np.abs(err["err_node"][:n]).max() <= 1e-12 and np.abs(err["err_global"][:n]).max() <= 1e-12
            assert (err["info"] == 0).all() and (err["nees"][:n] < 1e-18).all() and np.isnan(err["err_node"][n:]).all()
    assert seen >= 4 * 3 * 6


def _store_case(rng, N=6):
    x, P = random_state(rng, N), random_spd(rng, 16 + 3 * N)
    return x, P


def test_store_rules():
    """eviction restarts n_obs, the larger id wins a shared residue, entries of untracked features keep every bit, a stale table
    leaves the store untouched, an invalid rho does not enter"""
    rng = np.random.default_rng(8)
    N, cap = 6, 4
    x, P = _store_case(rng, N)
    mp = MR.MapRef(N, Q_B_C, P_B_C, cap)
    node = np.concatenate([rng.normal(0.0, 1.0, 3), unit(rng)])
    # ids 1, 5, 9 share residue 1; id 2 alone; slot 4 has a rho that is not valid; slot 5 is past len
    x[21 + 5 * 4] = -0.5
    table = np.array([1, 9, 5, 2, 7, 11], np.int32)
    mp.update(x, P, 5, table, 5, node, 3)
    assert mp.ids.tolist() == [-1, 9, 2, -1] and mp.n_obs.tolist() == [0, 1, 1, 0] and mp.node_count.tolist() == [0, 3, 3, 0]
    lg, Sg = MR.to_global(node, MR.landmark(x, 1, Q_B_C, P_B_C), MR.sigma(x, P, 1, Q_B_C, P_B_C))
    assert np.array_equal(mp.pos[1], lg) and np.array_equal(mp.cov[1], MR.tri(Sg))
    mp.update(x, P, 5, table, 5, node, 3)
    mp.update(x, P, 5, table, 5, node, 4)
    assert mp.ids.tolist() == [-1, 9, 2, -1] and mp.n_obs.tolist() == [0, 3, 3, 0] and mp.node_count.tolist() == [0, 4, 4, 0]
    # a stale table: nothing moves
    before = [a.copy() for a in (mp.ids, mp.pos, mp.cov, mp.n_obs, mp.node_count)]
    mp.update(x + 1.0, P, 5, table, 4, node, 9)
    assert all(np.array_equal(a, b) for a, b in zip(before, (mp.ids, mp.pos, mp.cov, mp.n_obs, mp.node_count)))
    # feature 9 is lost, 5 takes its entry: n_obs restarts; 2 is no longer tracked and keeps every bit
    keep2 = (mp.pos[2].copy(), mp.cov[2].copy())
    x2 = x.copy()
    x2[17:17 + 5 * 2] = np.concatenate([x[17 + 5 * 0:22 + 5 * 0], x[17 + 5 * 2:22 + 5 * 2]])
    table2 = np.array([1, 5, -1, -1, -1, -1], np.int32)
    mp.update(x2, P, 2, table2, 2, node, 5)
    assert mp.ids.tolist() == [-1, 5, 2, -1] and mp.n_obs.tolist() == [0, 1, 3, 0] and mp.node_count.tolist() == [0, 5, 4, 0]
    assert np.array_equal(mp.pos[2], keep2[0]) and np.array_equal(mp.cov[2], keep2[1])
    # capacity 0 holds nothing and does nothing
    m0 = MR.MapRef(N, Q_B_C, P_B_C, 0)
    m0.update(x, P, 5, table, 5)
    assert m0.ids.size == 0
    # the live query: NaN past len and for the invalid rho
    out = mp.landmarks(x, P, 5, node)
    assert np.isnan(out["pos_node"][[4, 5]]).all() and np.isnan(out["cov_global"][[4, 5]]).all() and not np.isnan(out["pos_global"][:4]).any()


def test_loop_through_the_restated_stack():
    """sim_ref.LOOP with resets on, N = 8, 2 s at 250 / 25 Hz through RefSimulator -> oracle propagate -> FrameRef -> NodeRef ->
    MapRef: the stores fill (no vehicle loses a feature or resets on these small circles), every tracked slot that is in the frame
    factors, and the worst |err_node| after t = 1 s over features with n_obs >= 5 is the figure map_ref.LOOP_MAP_MEASURED states.
    The restatement alone satisfies LOOP_MAP_BOUND (twice that figure), which is the bound of the GPU test."""
    res = MR.fly_loop_map()
    worst = max(r["worst"] for r in res)
    print("sim_ref.LOOP with resets on through the restated stack: resets", [r["resets"] for r in res], "store entries",
          [r["entries"] for r in res], "slot-frames counted", [r["counted"] for r in res])
    print("worst |err_node| after t = 1 s over n_obs >= %d: %.4f m per vehicle %s; worst landmark NEES %.3f"
          % (MR.LOOP_MAP_MIN_OBS, worst, ["%.4f" % r["worst"] for r in res], max(r["nees_worst"] for r in res)))
    for r in res:
        assert r["bad"] == 0 and r["counted"] > 50 and r["entries"] >= MR.LOOP_MAP_N and r["worst"] > 0
    m = MR.LOOP_MAP_MEASURED
    assert 0.99 * m <= worst <= m, (worst, m)                # the stated figure IS what this prints, rounded up
    assert MR.LOOP_MAP_BOUND == 2.0 * m and worst < MR.LOOP_MAP_BOUND


# -- C ABI without a device -----------------------------------------------------------------------------------------------
def test_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "viekf_map.h")).read()
    nocom = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_map_[a-z_0-9]+)\s*\(", nocom)))
    assert sorted(vmap.MAP_SYMBOLS) == syms and len(syms) == 8
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vi_ekf_amd", "libviekf_hip.so")], capture_output=True, text=True, check=True)
    exported = sorted(ln.split()[-1] for ln in out.stdout.splitlines() if re.search(r"\bviekf_map_", ln))
    assert exported == syms, exported                        # exactly the declared ones
    assert int(re.search(r"#define\s+VIEKF_MAP_MAX_CAPACITY\s+(\d+)", txt).group(1)) == vmap.MAX_CAPACITY
    assert L.viekf_abi_version() == 1
    # include/viekf.h itself got no new symbol
    assert "viekf_map" not in open(os.path.join(ROOT, "include", "viekf.h")).read()


def test_header_is_plain_c11(tmp_path):
    """tests/c/map_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    import subprocess
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "map_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "map_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "map header ok" in out.stdout, out.stderr


def test_null_handles_are_refused():
    L = vmap._bind()
    assert L.viekf_map_create(None, None, None, 0, None) == capi.ERR_INVALID
    assert L.viekf_map_destroy(None) == capi.ERR_INVALID
    assert L.viekf_map_reset(None) == capi.ERR_INVALID
    assert L.viekf_map_landmarks(None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_map_update(None) == capi.ERR_INVALID
    assert L.viekf_map_get(None, None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_map_set(None, None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_map_error(None, None, 0, 1, None, None, 1, None, None, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
