"""The fused step's sweeps with MORE than four blocks per thread rotate their operand reads under the multiply-adds
(res_rotating_reads, viekf_resident_common.hpp): block ia + 2's rows are read into the operand buffer block ia just released.  No
arithmetic changes; what can go wrong is the pipeline itself -- a block swept with another block's rows (buffer parity at an odd
and at an even block count), the prologue (blocks 0 and 1) and the epilogue (the last two blocks, read but nothing behind them),
threads that own nothing in their upper slots, and the update that does not run: it reads no operand, must leave P as it is and
the update after it must read fresh rows.  So, on every instance with more than four blocks per thread that a small batch can be
put on, and on <4,3> as the control that keeps all its operands in flight:

 * one fused step (propagate + M updates, M = 1, 2 and N) against the CPU oracle, unit Lambda and general Lambda on the bearing
   components, with the helper and tolerance of tests/test_gpu_parity.py (assert_close: 1e-9 of max|ref|, 1e-6 element-wise); result
   codes exactly.  The scene is tests/test_gpu_packed_p.py's (Rec): with M = N fix_depth fires inside the updates;
 * the same with three inactive slots (len_features < N);
 * a measurement that the gate rejects BETWEEN two that run, in every filter, and a NaN pixel in one;
 * step_n with K = 3 (the multi-propagate kernels' contraction) bit for bit against two propagates and a step, as
   tests/test_gpu_lifecycle.py does at its own sizes.
B = 3: more than one workgroup.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import make_oracle
from tests.test_gpu_packed_p import GENERAL_LAMBDA, I_5_6_2, I_7_3, Rec, same
from tests.test_gpu_parity import assert_close, oracle_params
from tests.test_gpu_setup_under_load import fused, separate

pytestmark = pytest.mark.gpu

# rows of the resident dispatch table (viekf_instance_rows.hpp; the index VIEKF_TUNE_RES_INSTANCE takes)
I_4_3, I_5_3, I_6_3 = 3, 4, 5
B = 3
# (instance, N, its name): N = 26 is <7,3>'s smallest -- most threads own nothing in their upper slots
CASES = [(I_5_3, 39, "<5,3>"), (I_6_3, 44, "<6,3>"), (I_7_3, 26, "<7,3>"), (I_7_3, 50, "<7,3>"), (I_5_6_2, 51, "<5,6>"),
         (I_4_3, 26, "<4,3>")]
IDS = ["%s-N%d" % (c[2], c[1]) for c in CASES]
LAMBDAS = {"unit": None, "general": GENERAL_LAMBDA}


def _rec(inst, N, name, lam="unit", nfeat=None):
    r = Rec(B, N, packed=True, inst=inst, seed=100 + N, params=LAMBDAS[lam], steps=11)
    d = r.g.describe()
    assert d.startswith("k_step_resident" + name), d
    assert (" ZU" in d) == (lam == "unit"), d
    if nfeat is not None:
        keep = np.ones((B, N), dtype=np.uint8)
        keep[:, nfeat:] = 0
        r.g.keep_features(keep)
        assert (r.g.get_len_features() == nfeat).all()
    return r


def _oracle_step(r, x0, P0, u, z, slot, nfeat=None):
    """one propagate and the listed updates on one oracle filter per batch entry, started from (x0, P0) -> x, P, codes"""
    sc = r.sc
    R = np.asarray(sc["R"]).reshape(2, 2)
    xs, Ps, codes = [], [], np.zeros(slot.shape, dtype=np.int32)
    for b in range(r.B):
        f = make_oracle(r.N, oracle_params(sc["params"]), sc["pix"][b][:nfeat])
        f.x[:] = x0[b]
        f.P[:] = P0[b]
        f.propagate(u[b], float(sc["dt"][b]))
        for m, sl in enumerate(slot[b]):
            if not 0 <= sl < f.len_features:
                codes[b, m] = 3
            elif np.isnan(z[b, m]).any():
                codes[b, m] = 2
            else:
                codes[b, m] = f.update(orc.FEAT, z[b, m], R, True, f.feature_ids[sl])
        xs.append(f.x.copy())
        Ps.append(f.P.copy())
    return np.stack(xs), np.stack(Ps), codes


def _step_and_compare(r, z, slot, nfeat=None):
    sc = r.sc
    x0, P0 = r.g.get_state(), r.g.get_covariance()
    z, slot = np.ascontiguousarray(z), np.ascontiguousarray(slot)
    xr, Pr, cr = _oracle_step(r, x0, P0, sc["u"][0], z, slot, nfeat)
    codes = r.g.step(sc["u"][0], sc["dt"], z, slot, sc["R"]).copy()
    assert np.array_equal(codes, cr), (codes, cr)
    assert_close(r.g.get_state(), xr, "x")
    assert_close(r.g.get_covariance(), Pr, "P")
    return codes


@pytest.mark.parametrize("M", ["1", "2", "N"])
@pytest.mark.parametrize("lam", ["unit", "general"])
@pytest.mark.parametrize("inst,N,name", CASES, ids=IDS)
def test_one_step_against_the_oracle(inst, N, name, lam, M):
    r = _rec(inst, N, name, lam)
    M = N if M == "N" else int(M)
    codes = _step_and_compare(r, r.z[0][:, :M], r.sc["slot"][:, :M])
    assert (codes == 0).any(), codes
    if M == N:
        assert ((r.g.get_status() & 4) != 0).any(), "no filter took the negative-depth branch: fix_depth is not exercised"


@pytest.mark.parametrize("inst,N,name", CASES, ids=IDS)
def test_inactive_slots(inst, N, name):
    nfeat = N - 3
    r = _rec(inst, N, name, nfeat=nfeat)
    codes = _step_and_compare(r, r.z[0], r.sc["slot"], nfeat)
    assert (codes == 3).sum() == 3 * B and (codes == 0).any()


@pytest.mark.parametrize("lam", ["unit", "general"])
@pytest.mark.parametrize("inst,N,name", CASES, ids=IDS)
def test_gated_between_two_that_run_and_a_nan_pixel(inst, N, name, lam):
    """measurement 1 is rejected by the gate in every filter, measurements 0 and 2 run; filter 1 has a NaN pixel further on"""
    r = _rec(inst, N, name, lam)
    z = r.sc["z"][0] + np.random.default_rng(5).normal(0.0, 1.5, r.sc["z"][0].shape)
    z[:, 1, 0] += 5000.0
    z[1, 4, 1] = np.nan
    codes = _step_and_compare(r, z, r.sc["slot"])
    assert (codes[:, 1] == 1).all() and (codes[:, 0] == 0).all() and (codes[:, 2] == 0).all(), codes[:, :3]
    assert codes[1, 4] == 2 and (codes[[0, 2], 4] == 0).all()
    assert ((r.g.get_status() & 4) != 0).any(), "no filter took the negative-depth branch: fix_depth is not exercised"


@pytest.mark.parametrize("inst,N,name", CASES, ids=IDS)
def test_step_n_equals_two_propagates_and_a_step(inst, N, name):
    a, b = _rec(inst, N, name), _rec(inst, N, name)
    fused(a)
    separate(b)
    same(a, b)
    assert (np.asarray(a.log[-1][4]) == 0).any(), "the scene has no accepted update"
