"""The fused step runs the propagate's set-up while the global loads of its register blocks of P are still in flight: the part of
P that lives in LDS (body columns, body block) is loaded and written FIRST, in both forms of P, then the block loads are issued
and first waited for behind the set-up's last barrier (B3p) -- or, in a launch without a propagate, before the first column
extraction.  No arithmetic changes, so what the moved wait feeds is pinned here on every kind of launch:

 * against the CPU oracle with the tolerances tests/test_gpu_parity.py applies (assert_close, imported: 1e-9 of max|ref| and
   1e-6 element-wise), after each leg of one script: the first fused step after set_state (canonical load), a fused step that
   loads what a fused step stored (packed load where P is kept packed), a propagate-only launch, an update-only launch
   (update_feat) and step_n with K = 3.  Reading P converts it to the canonical form, so a leg that is to LOAD a packed image is
   preceded by a fused step that is not read (the oracle runs it too).  A set-up that reads the body columns or the body block
   before they are in LDS is wrong in both forms alike: these legs catch it;
 * BIT FOR BIT (same, imported): the script with P packed between launches against the script with P canonical -- an ordering
   error in one form only -- and step_n against K - 1 propagates and a step as separate launches;
 * a filter with 47 of 50 features: bit for bit between the two forms and between step_n and separate launches.
"""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import make_oracle
from tests.test_gpu_packed_p import I_1_7, I_2_1, I_5_6_2, I_7_3, Rec, same
from tests.test_gpu_parity import assert_close, oracle_params

pytestmark = pytest.mark.gpu

# (B, N, instance): the headline instance, its ragged tile row and threads without a diagonal block (N = 48), one worker wave,
# seven worker waves (an instance that keeps the old order), two service waves, features on the body wave (N = 65: automatic)
CASES = [(3, 50, I_7_3), (3, 48, I_7_3), (2, 12, I_2_1), (2, 25, I_1_7), (2, 51, I_5_6_2), (1, 65, None)]
K = 3
STEPS = 11
LEGS = ("first step", "second step", "propagate", "update_feat", "step_n")


def _ktile(sc):
    return np.ascontiguousarray(np.tile(sc["dt"], (K, 1)))


def script(r):
    """the five legs on the batch; a record after each"""
    g, sc = r.g, r.sc
    r.read(r.step(0))                                                   # canonical load (set_state wrote P)
    r.step(1)
    r.read(r.step(2))                                                   # loads what step 1 stored
    r.step(3)
    g.propagate(sc["u"][4], sc["dt"])                                   # propagate-only launch
    r.read()
    r.step(5)
    r.read(g.update_feat(r.z[6], sc["slot"], sc["R"]).copy())           # update-only launch
    r.step(7)
    r.read(g.step_n(np.ascontiguousarray(sc["u"][8:8 + K]), _ktile(sc), r.z[10], sc["slot"], sc["R"]).copy())


def oracle_script(r, x0, P0):
    """the same calls on one oracle filter per batch entry, started from the state the batch was given -> records (x, P, codes)"""
    sc = r.sc
    R = np.asarray(sc["R"]).reshape(2, 2)
    fs = []
    for b in range(r.B):
        f = make_oracle(r.N, oracle_params(sc["params"]), sc["pix"][b])
        f.x[:] = x0[b]
        f.P[:] = P0[b]
        fs.append(f)

    def updates(s):
        out = np.zeros((r.B, sc["slot"].shape[1]), dtype=np.int32)
        for b, f in enumerate(fs):
            ids = f.feature_ids
            for m, sl in enumerate(sc["slot"][b]):
                out[b, m] = f.update(orc.FEAT, r.z[s][b, m], R, True, ids[sl]) if 0 <= sl < f.len_features else 3
        return out

    def prop(s):
        for b, f in enumerate(fs):
            f.propagate(sc["u"][s, b], float(sc["dt"][b]))

    def step(s):
        prop(s)
        return updates(s)

    def rec(codes=None):
        log.append((np.stack([f.x.copy() for f in fs]), np.stack([f.P.copy() for f in fs]), codes))

    log = []
    rec(step(0))
    step(1)
    rec(step(2))
    step(3)
    prop(4)
    rec()
    step(5)
    rec(updates(6))
    step(7)
    prop(8)
    prop(9)
    rec(step(10))
    return log


@functools.lru_cache(maxsize=None)
def gpu_run(B, N, inst, packed):
    r = Rec(B, N, packed=packed, inst=inst, seed=100 + N, steps=STEPS)
    r.start = (r.g.get_state(), r.g.get_covariance())
    script(r)
    r.desc = r.g.describe()
    return r


@functools.lru_cache(maxsize=None)
def oracle_run(B, N, inst):
    r = gpu_run(B, N, inst, 0)
    return oracle_script(r, *r.start)


@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("B,N,inst", CASES)
def test_every_kind_of_launch_against_the_oracle(B, N, inst, packed):
    r = gpu_run(B, N, inst, packed)
    assert "k_step_resident" in r.desc and ("P packed" in r.desc) == bool(packed), r.desc
    ref = oracle_run(B, N, inst)
    assert len(r.log) == len(ref) == len(LEGS)
    for leg, (x, P, _, _, codes), (xr, Pr, cr) in zip(LEGS, r.log, ref):
        if cr is not None:
            assert np.array_equal(codes, cr), "%s: result codes" % leg
        assert_close(x, xr, "x after %s" % leg)
        assert_close(P, Pr, "P after %s" % leg)
    codes = np.concatenate([np.asarray(rec[4]).ravel() for rec in r.log if rec[4] is not None])
    assert (codes == 0).any() and (codes == 1).any(), "the scene has no accepted or no gated update"


@pytest.mark.parametrize("B,N,inst", CASES)
def test_packed_equals_canonical_bit_for_bit(B, N, inst):
    same(gpu_run(B, N, inst, 1), gpu_run(B, N, inst, 0))


def fused(r):
    sc = r.sc
    r.step(0)                                                           # (unread: the next launch loads what this one stored)
    r.read(r.g.step_n(np.ascontiguousarray(sc["u"][1:1 + K]), _ktile(sc), r.z[K], sc["slot"], sc["R"]).copy())


def separate(r):
    sc = r.sc
    r.step(0)
    for k in range(K - 1):
        r.g.propagate(sc["u"][1 + k], sc["dt"])
    r.read(r.step(K))


@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("B,N,inst", CASES)
def test_step_n_equals_separate_launches(B, N, inst, packed):
    a = Rec(B, N, packed=packed, inst=inst, seed=100 + N, steps=STEPS)
    fused(a)
    b = Rec(B, N, packed=packed, inst=inst, seed=100 + N, steps=STEPS)
    separate(b)
    same(a, b)
    assert (np.asarray(a.log[-1][4]) == 0).any(), "the scene has no accepted update"


def test_47_of_50_features():
    B, N, nfeat = 2, 50, 47
    out = []
    for packed, legs in ((1, (script, fused)), (0, (script, fused)), (1, (separate,))):
        for leg in legs:
            # (process noise on the feature rows, as tests/test_gpu_step_serial_loads.py sets it: the inactive slots receive it too)
            r = Rec(B, N, packed=packed, inst=I_7_3, seed=147, steps=STEPS, params=dict(Qx_feat=[1e-5, 2e-5, 3e-5]))
            keep = np.ones((B, N), dtype=np.uint8)
            keep[:, nfeat:] = 0
            r.g.keep_features(keep)
            assert (r.g.get_len_features() == nfeat).all()
            r.read()
            leg(r)
            out.append(r)
    same(out[0], out[2])       # the five legs: packed against canonical
    same(out[1], out[3])       # step_n: packed against canonical
    same(out[1], out[4])       # step_n against separate launches
    P = out[0].log[-1][1]
    d = 16 + 3 * nfeat
    assert np.isfinite(P).all() and (np.diagonal(P[:, d:, d:], axis1=1, axis2=2) > 0).all()
    codes = np.asarray(out[0].log[1][4])
    assert (codes[:, :nfeat] == 0).any(), "the scene has no accepted update"
