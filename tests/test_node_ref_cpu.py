"""tests/node_ref.py, the restatement the device-resident node graph (include/viekf_node.h) is tested against, on its own:
its node is SeqOracle._node_update's (the line-by-line restatement of the reference), the truth in the node frame is the reset
applied to the truth, and the restated stack flies the resetting closed loop of tests/test_gpu_node.py on the CPU, which
fixes that test's bounds."""
import os
import re

import numpy as np

from oracle import np_twin as tw
from oracle import oracle as orc
from oracle import seq_oracle as so
from tests import frame_ref as F
from tests import node_ref as NR
from tests.test_frame_ref_cpu import SCRIPT, _params, _pix
from vi_ekf_amd import capi, node

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hover(f, k, steps=3):
    rng = np.random.default_rng(40 + k)
    for _ in range(steps):
        u = np.array([0.0, 0.0, -9.80665, 0.0, 0.0, 0.0]) + rng.normal(0.0, 0.05, 6)
        f.propagate(u, 0.004)


def test_node_is_seq_oracles_node_update():
    """the twelve frames of test_frame_ref_cpu.SCRIPT (resets at frames 2, 3, 6, 8, 11), a few propagates between them so that
    the edges are not trivial: the restated node, covariance, global pose and global covariance against SeqOracle fed the same
    edges, and the trail holds the nodes before each move"""
    N, p = 8, _params(use_keyframe_reset=True)
    ref = F.FrameRef(orc.OracleFilter(N).init(**p), 0.8)
    o = so.SeqOracle(ref.f, 0.8, state_hist=4)            # (the same filter: get_global_pose / _cov read its x and P)
    nd = NR.NodeRef(trail_capacity=8)
    Rm = np.diag([10.0, 10.0])
    resets, before = [], []
    for k, ids in enumerate(SCRIPT):
        _hover(ref.f, k)
        out = ref.intake(np.array([_pix(g) for g in ids]).reshape(-1, 2), ids, Rm)
        node0 = nd.node.copy()
        nd.update(out["did_reset"], out["edges"])
        if out["did_reset"]:
            resets.append(k)
            before.append(nd.trail_nodes[(nd.count - 1) % 8].copy())
            assert np.array_equal(before[-1], node0) and np.array_equal(nd.trail_edges[(nd.count - 1) % 8], out["edges"])
            o._node_update(out["edges"])
        else:
            assert np.array_equal(nd.node, node0)           # a filter that did not reset keeps its node
        assert np.array_equal(nd.node, o.node) and np.array_equal(nd.node_cov, o.node_cov), k
        assert np.array_equal(nd.global_pose(ref.f.x), o.get_global_pose()), k
        assert np.array_equal(nd.global_cov(ref.f.P), o.get_global_cov()), k
    assert resets == [2, 3, 6, 8, 11] and nd.count == 5
    assert np.abs(nd.node[:3]).max() > 0 and np.abs(nd.node_cov).max() > 0
    assert abs(np.linalg.norm(nd.node[3:]) - 1.0) < 1e-12
    assert np.allclose(nd.node_cov, nd.node_cov.T, rtol=0, atol=1e-18)


def test_relative_truth_right_after_a_reset_is_the_reset_applied_to_the_truth():
    """position 0 and attitude from_euler(roll, pitch, 0), to 1e-12; every other column is copied; and a truth that has moved
    on is seen from the node frame"""
    rng = np.random.default_rng(3)
    nd = NR.NodeRef()
    for _ in range(20):
        xt = rng.normal(0.0, 1.0, 17 + 5 * 3)
        xt[6:10] = NR.from_euler(*rng.uniform([-0.6, -0.6, -3.1], [0.6, 0.6, 3.1]))
        edge = np.concatenate([rng.normal(0, 1, 3), NR.from_euler(0, 0, rng.uniform(-3, 3)), np.eye(3).ravel() * 0.01, [0.02]])
        nd.update(1, edge, xt)
        xr = nd.relative_truth(xt)
        roll, pitch, yaw = NR.euler_of(xt[6:10])
        assert np.abs(xr[0:3]).max() <= 1e-12
        assert np.abs(xr[6:10] - NR.from_euler(roll, pitch, 0.0)).max() <= 1e-12
        keep = [i for i in range(xt.size) if not (i < 3 or 6 <= i < 10)]
        assert np.array_equal(xr[keep], xt[keep])
        # later: the truth has moved by d in the inertial frame and turned by dq in the body frame
        d, dq = rng.normal(0, 1, 3), tw.qexp(rng.normal(0, 0.3, 3))
        x2 = xt.copy()
        x2[0:3] += d
        x2[6:10] = tw.qmul(xt[6:10], dq)
        xr2 = nd.relative_truth(x2)
        qy = NR.from_euler(0.0, 0.0, yaw)
        assert np.abs(xr2[0:3] - tw.rotp(qy, d)).max() <= 1e-12
        assert np.abs(xr2[6:10] - tw.qmul(NR.from_euler(roll, pitch, 0.0), dq)).max() <= 1e-12
        # the estimate in the node frame and the node compose to the global pose: node * relative = global
        assert np.abs(so.xform_mul(nd.true_node, np.concatenate([xr2[0:3], xr2[6:10]])) - np.concatenate([x2[0:3], x2[6:10]])).max() <= 1e-12


def test_loop_kfr_through_the_restated_stack():
    """LOOP_KFR, N = 8, 3 s at 250 / 25 Hz, threshold 0.8: the vehicles reset (6, 7, 6, 7 times), 21 - 23 feature ids are handed
    out, nothing is NaN, no Cholesky factorisation of P's pose blocks or of the global covariance fails, and the worst errors
    are the figures node_ref.LOOP_KFR_MEASURED states -- LOOP_KFR_BOUNDS, twice that, are the bounds of the GPU test"""
    res = NR.fly_loop_kfr()
    worst = np.max([r["worst"] for r in res], axis=0)
    nees = max(r["nees"] for r in res)
    print("LOOP_KFR through the restated stack: resets per vehicle", [len(r["reset_frames"]) for r in res],
          "ids handed out", [r["next_feat_id"] for r in res])
    print("worst errors after t = 1 s: global %.4f m %.4f deg, relative to the true node %.4f m %.4f deg; global NEES %.4f"
          % (worst[0], worst[1], worst[2], worst[3], nees))
    for r in res:
        assert len(r["reset_frames"]) >= 5 and r["reset_frames"] == sorted(set(r["reset_frames"]))
        assert 21 <= r["next_feat_id"] <= 23
        assert not r["nan"] and r["chol_failures"] == 0
    rec = NR.loop_kfr_recorded()
    assert rec["reset_frames"] == [r["reset_frames"] for r in res] and rec["next_feat_id"] == [r["next_feat_id"] for r in res]
    m = NR.LOOP_KFR_MEASURED
    got = dict(global_m=worst[0], global_deg=worst[1], relative_m=worst[2], relative_deg=worst[3], nees=nees)
    for k, v in got.items():
        assert 0.99 * m[k] <= v <= m[k], (k, v, m[k])           # the stated figures ARE what this prints, rounded up
        assert NR.LOOP_KFR_BOUNDS[k] == 2.0 * m[k]
    assert nees <= 5.82


# -- C ABI without a device -----------------------------------------------------------------------------------------------
def test_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "viekf_node.h")).read()
    nocom = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_node_[a-z_0-9]+)\s*\(", nocom)))
    assert sorted(node.NODE_SYMBOLS) == syms and len(syms) == 10
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    assert int(re.search(r"#define\s+VIEKF_NODE_MAX_TRAIL\s+(\d+)", txt).group(1)) == node.MAX_TRAIL
    assert L.viekf_abi_version() == 1


def test_header_is_plain_c11(tmp_path):
    """tests/c/node_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    import subprocess
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "node_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "node_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "node header ok" in out.stdout, out.stderr


def test_null_handles_are_refused():
    L = node._bind()
    assert L.viekf_node_create(None, 0, None) == capi.ERR_INVALID
    assert L.viekf_node_destroy(None) == capi.ERR_INVALID
    assert L.viekf_node_reset(None) == capi.ERR_INVALID
    assert L.viekf_node_update(None, None, None, None, 0, 0) == capi.ERR_INVALID
    assert L.viekf_node_global(None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_node_relative_truth(None, None, None, 17, 0) == capi.ERR_INVALID
    assert L.viekf_node_global_error(None, None, 17, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_node_get(None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_node_set(None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_node_trail(None, None, None, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
