"""The fused step loads its launch constants in batches: the ownership words of a thread's blocks once per use site (block load,
local transforms + contraction offsets, update-loop indices, canonical store), Qx of the diagonal blocks ahead of the propagate's
barrier, sqrt(Qu) and Qx of the body rows from LDS.  None of it changes a value, so what the moved loads feed is pinned here:

 * viekf_batch_step_n against the same propagates and step as separate launches, BIT FOR BIT (np.array_equal on x, P, len, status
   and result codes): the preloaded words live inside the multi-propagate loop.  Each case with P packed between launches and with
   P canonical -- the latter takes the canonical load and the chunked canonical store;
 * one propagate-only launch with a non-uniform Qx (body rows all different, the three rows of a feature different) and a
   non-uniform Qu against the CPU oracle, with the tolerance tests/test_gpu_parity.py applies to a propagate (its assert_close,
   imported: TOL = 1e-9 of max|ref| and 1e-6 element-wise, test_gpu_parity.py:18-30).  The parameter set has ONE Qx_feat triple
   for all features (as the reference, vi_ekf.cpp:139-144), so Qx cannot differ between features through the API;
   What catches what: the bit-for-bit cases catch a wrong sqrt(Qu) staging (the multi-propagate kernels read it from memory,
   the others from LDS); a wrong body-row Qx staging or a wrong diagonal Qx triple is caught by THIS case alone, since both
   sides of the bit-for-bit cases read Qx the same way.  So Qx (1e-4 .. 1.6e-3) and Qx_feat (1e-5 .. 3e-5) stay at least four
   orders of magnitude above assert_close's floor of 1e-9 max|P| (max|P| is about 4): a mis-indexed row cannot hide under it;
 * a filter with fewer features than slots (47 of 50): the inactive blocks, and the lanes that own nothing, bit for bit as the
   canonical run leaves them.
"""
import numpy as np
import pytest

from tests.helpers import make_oracle
from tests.test_gpu_packed_p import I_1_7, I_2_1, I_5_6_2, I_7_3, Rec, same
from tests.test_gpu_parity import assert_close, oracle_params
import vi_ekf_amd as v
from vi_ekf_amd import capi, scene

pytestmark = pytest.mark.gpu

# (B, N, instance): the headline instance, its ragged tile row and unowned lanes (N = 48), one worker wave, seven worker waves,
# two service waves, features on the body wave (N = 65: the automatic instance)
CASES = [(3, 50, I_7_3), (3, 48, I_7_3), (2, 12, I_2_1), (2, 25, I_1_7), (2, 51, I_5_6_2), (1, 65, None)]
NONUNIFORM = dict(Qx=[1e-4 * (1 + k) for k in range(16)], Qx_feat=[1e-5, 2e-5, 3e-5], Qu=[0.5, 1.0, 2.0, 2e-4, 4e-4, 8e-4])
K = 3


def _dt(sc):
    return np.ascontiguousarray(np.tile(sc["dt"], (K, 1)))


def fused(r, meas=True):
    sc = r.sc
    for s in (0, K):
        u = np.ascontiguousarray(sc["u"][s:s + K])
        if meas:
            r.read(r.g.step_n(u, _dt(sc), r.z[s + K - 1], sc["slot"], sc["R"]).copy())
        else:
            r.g.step_n(u, _dt(sc), None, None, None)
            r.read()


def separate(r, meas=True):
    sc = r.sc
    for s in (0, K):
        for k in range(K - 1 if meas else K):
            r.g.propagate(sc["u"][s + k], sc["dt"])
        if meas:
            r.read(r.step(s + K - 1))
        else:
            r.read()


@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("B,N,inst", CASES)
def test_step_n_equals_separate_launches(B, N, inst, packed):
    a = Rec(B, N, packed=packed, inst=inst, seed=100 + N, params=NONUNIFORM)
    fused(a)
    b = Rec(B, N, packed=packed, inst=inst, seed=100 + N, params=NONUNIFORM)
    separate(b)
    assert "k_step_resident" in a.g.describe(), a.g.describe()
    same(a, b)
    res = np.concatenate([np.asarray(r[4]).ravel() for r in a.log])
    assert (res == 0).any(), "the scene has no accepted update"


@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("B,N,inst", CASES)
def test_step_n_without_measurements_equals_propagates(B, N, inst, packed):
    a = Rec(B, N, packed=packed, inst=inst, seed=200 + N, params=NONUNIFORM)
    fused(a, meas=False)
    b = Rec(B, N, packed=packed, inst=inst, seed=200 + N, params=NONUNIFORM)
    separate(b, meas=False)
    same(a, b)


@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("B,N,inst", CASES)
def test_propagate_only_launch_with_nonuniform_qx_and_qu(B, N, inst, packed):
    sc = scene.make_scene(B, N, 1, seed=300 + N, params=NONUNIFORM)
    g = v.BatchVIEKF(B, N, sc["params"])
    if inst is not None:
        g.set_tuning(capi.TUNE_RES_INSTANCE, inst)
    g.set_tuning(capi.TUNE_PACKED_P, packed)
    for i in range(N):
        g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan))
    assert "k_step_resident" in g.describe(), g.describe()
    fs = [make_oracle(N, oracle_params(sc["params"]), sc["pix"][b]) for b in range(B)]
    g.propagate(sc["u"][0], sc["dt"])
    for b in range(B):
        fs[b].propagate(sc["u"][0, b], sc["dt"][b])
    assert_close(g.get_state(), np.stack([f.x for f in fs]), "x")
    assert_close(g.get_covariance(), np.stack([f.P for f in fs]), "P")


def test_inactive_slots_as_the_canonical_run_leaves_them():
    B, N, nfeat = 2, 50, 47
    out = []
    for packed, script in ((1, fused), (0, fused), (1, separate)):
        r = Rec(B, N, packed=packed, inst=I_7_3, seed=147, params=NONUNIFORM)
        keep = np.ones((B, N), dtype=np.uint8)
        keep[:, nfeat:] = 0
        r.g.keep_features(keep)
        assert (r.g.get_len_features() == nfeat).all()
        r.read()
        script(r)
        r.read(r.step(2 * K))
        out.append(r)
    same(out[0], out[1])
    same(out[0], out[2])
    P = out[0].log[-1][1]
    d = 16 + 3 * nfeat
    assert np.isfinite(P).all() and (np.diagonal(P[:, d:, d:], axis1=1, axis2=2) > 0).all()
