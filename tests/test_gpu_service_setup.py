"""The single-propagate kernels of the instances <6,3>, <7,3> and <5,6> evaluate the body-only part of the propagate's set-up
(Phi_bb / M_bb, Psi P_bb, T16, Gs_b, Pi, Xi) on the service wave (res_service_setup, viekf_resident_common.hpp); their
multi-propagate kernels keep the old order, where the worker waves do it across one more barrier.  (<4,3>, the fourth instance
that runs the set-up under the load of P, was built and measured with the new order too and is gated off; its cases stay, so that
they are there when the gate is changed.)  Every element is the same expression on the same operands in both, so the two orders
must agree BIT FOR BIT.

Which launch runs which kernel: `step`, `propagate` and `step_n` with K = 1 launch the single-propagate kernel (new order), `step_n`
with K >= 2 the multi-propagate kernel (old order) -- launch_resident picks the flavour by K > 1.  So each case advances the same
start twice by TWO propagates and one frame of updates along three routes,

  A  propagate, step                    (single-propagate kernel twice: new order)
  B  propagate, step_n with K = 1       (the same kernels through the other entry point)
  C  step_n with K = 2                  (multi-propagate kernel: old order)

and asserts x, P, len, status and the result codes equal bit for bit between all three -- C against A is the equality step_n
promises (tests/test_gpu_setup_under_load.py pins it for the default settings), and here it sets the old order against the new.
Route A is also held to the CPU oracle with the tolerance of the parity cases (assert_close of tests/test_gpu_parity.py: 1e-9 of
max|ref| per array and 1e-6 element-wise).

Each of the four instances is forced (TUNE_RES_INSTANCE) at the smallest and the largest N it serves, B = 3.  The settings vary
over the cases so that every instance sees both values of each: fewer live features than slots (the inactive slots take the Phi = I
branch), use_partial_update off / on with the reference's lambda_feat = [1, 1, x] (both run the unit-Lambda kernels) / on with
lambda != 1 on the bearing components (the general-Lambda kernels), the drag term on / off, P packed / canonical on entry (where
the packed image does not fit -- <7,3> at N = 26 -- the library stays canonical); dt always differs between the filters and from
the default.  One case does the same for launches without updates
(`propagate` against step_n with every measurement skipped).
"""
import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import make_oracle
from tests.test_gpu_packed_p import GENERAL_LAMBDA, I_5_6_2, I_7_3, Rec, same
from tests.test_gpu_parity import assert_close, oracle_params

pytestmark = pytest.mark.gpu

I_4_3, I_6_3 = 3, 5   # rows of the resident dispatch table (viekf_instance_rows.hpp), beside the two imported ones
B = 3
DT_SCALE = np.array([1.0, 0.5, 1.7])   # dt differs between the filters (and from the scene's default but for filter 0)
STEPS = 4                              # two rounds of (propagate, propagate + updates)

# settings: (inactive slots, partial update: 0 off / 1 on, unit Lambda / 2 on, general Lambda, use_drag_term, packed)
S_A = (3, 1, 1, 1)
S_B = (1, 0, 0, 0)
S_C = (0, 2, 0, 0)
S_D = (2, 2, 1, 1)
# (instance, N, settings): smallest and largest N of each instance, two settings each
CASES = [(I_4_3, 26, S_A), (I_4_3, 26, S_B), (I_4_3, 38, S_C), (I_4_3, 38, S_D),
         (I_6_3, 44, S_D), (I_6_3, 44, S_C), (I_6_3, 47, S_B), (I_6_3, 47, S_A),
         (I_7_3, 26, S_C), (I_7_3, 26, S_D), (I_7_3, 50, S_A), (I_7_3, 50, S_B),
         (I_5_6_2, 51, S_B), (I_5_6_2, 51, S_A), (I_5_6_2, 57, S_D), (I_5_6_2, 57, S_C)]
KERNEL = {I_4_3: "k_step_resident<4,3", I_6_3: "k_step_resident<6,3", I_7_3: "k_step_resident<7,3", I_5_6_2: "k_step_resident<5,6"}


def make(inst, N, settings, seed_off=0):
    idle, partial, drag, packed = settings
    # (process noise on every row, as tests/test_gpu_parity.py sets it for the partial-feature case: inactive slots receive it too)
    params = dict(use_partial_update=int(partial != 0), use_drag_term=drag, Qx=[1e-4] * 16, Qx_feat=[1e-5, 2e-5, 3e-5])
    if partial == 2:
        params.update(GENERAL_LAMBDA)
    r = Rec(B, N, packed=packed, inst=inst, seed=300 + N + seed_off, steps=STEPS, params=params)
    r.sc["dt"] = r.sc["dt"] * DT_SCALE
    # outliers on LIVE slots (measurement m belongs to slot N - 1 - m; Rec's own sit on slot N - 1, which may be inactive here)
    r.z[1, :, idle + 1, 0] += 5000.0
    r.z[3, 1, idle + 2, 1] -= 5000.0
    if idle:
        keep = np.ones((B, N), dtype=np.uint8)
        keep[:, N - idle:] = 0
        r.g.keep_features(keep)
        assert (r.g.get_len_features() == N - idle).all()
    r.start = (r.g.get_state(), r.g.get_covariance())
    if packed:   # reading P left it canonical: one launch that changes nothing (no propagate, every measurement skipped) packs it
        skip = np.full_like(r.sc["slot"], -1)
        r.g.update_feat(r.z[0], skip, r.sc["R"])
    r.desc0 = r.g.describe()
    return r


def _dt(sc, K):
    return np.ascontiguousarray(np.tile(sc["dt"], (K, 1)))


def route_a(r, slot=None):
    sc = r.sc
    for s in (0, 2):
        r.g.propagate(sc["u"][s], sc["dt"])
        r.read(r.g.step(sc["u"][s + 1], sc["dt"], r.z[s + 1], sc["slot"] if slot is None else slot, sc["R"]).copy())


def route_b(r):
    sc = r.sc
    for s in (0, 2):
        r.g.propagate(sc["u"][s], sc["dt"])
        r.read(r.g.step_n(np.ascontiguousarray(sc["u"][s + 1:s + 2]), _dt(sc, 1), r.z[s + 1], sc["slot"], sc["R"]).copy())


def route_c(r, slot=None):
    sc = r.sc
    for s in (0, 2):
        r.read(r.g.step_n(np.ascontiguousarray(sc["u"][s:s + 2]), _dt(sc, 2), r.z[s + 1], sc["slot"] if slot is None else slot,
                          sc["R"]).copy())


def oracle_route(r, with_updates=True):
    """two rounds of (propagate, propagate, updates) on one oracle filter per batch entry, from the state the batch started from"""
    sc = r.sc
    R = np.asarray(sc["R"]).reshape(2, 2)
    nlive = int(r.g.get_len_features()[0])
    log = []
    fs = []
    for b in range(B):
        f = make_oracle(r.N, oracle_params(sc["params"]), sc["pix"][b][:nlive])
        f.x[:] = r.start[0][b]
        f.P[:] = r.start[1][b]
        fs.append(f)
    for s in (0, 2):
        codes = np.zeros((B, sc["slot"].shape[1]), dtype=np.int32)
        for b, f in enumerate(fs):
            f.propagate(sc["u"][s, b], float(sc["dt"][b]))
            f.propagate(sc["u"][s + 1, b], float(sc["dt"][b]))
            ids = f.feature_ids
            for m, sl in enumerate(sc["slot"][b]):
                if with_updates:
                    codes[b, m] = f.update(orc.FEAT, r.z[s + 1][b, m], R, True, ids[sl]) if 0 <= sl < f.len_features else 3
        log.append((np.stack([f.x.copy() for f in fs]), np.stack([f.P.copy() for f in fs]), codes))
    return log


@functools.lru_cache(maxsize=None)
def run_a(inst, N, settings):
    r = make(inst, N, settings)
    route_a(r)
    r.desc = r.g.describe()
    return r


@pytest.mark.parametrize("inst,N,settings", CASES)
def test_new_order_equals_old_order_bit_for_bit(inst, N, settings):
    a = run_a(inst, N, settings)
    assert KERNEL[inst] in a.desc and (" ZU" in a.desc) == (settings[1] != 2), a.desc
    if not settings[3]:
        assert "P canonical" in a.desc, a.desc
    elif (inst, N) != (I_7_3, 26):
        assert "P packed" in a.desc, a.desc
    b = make(inst, N, settings)
    route_b(b)
    c = make(inst, N, settings)
    route_c(c)
    same(a, b)
    same(a, c)
    codes = np.concatenate([np.asarray(rec[4]).ravel() for rec in a.log])
    assert (codes == 0).any() and (codes == 1).any(), "the scene has no accepted or no gated update"
    if settings[0]:
        assert (codes == 3).any(), "no measurement of an inactive slot"


@pytest.mark.parametrize("inst,N,settings", CASES)
def test_new_order_against_the_oracle(inst, N, settings):
    a = run_a(inst, N, settings)
    ref = oracle_route(a)
    nx = 17 + 5 * (N - settings[0])
    assert len(a.log) == len(ref) == 2
    for k, ((x, P, _, _, codes), (xr, Pr, cr)) in enumerate(zip(a.log, ref)):
        assert np.array_equal(codes, cr), "round %d: result codes" % k
        assert_close(x[:, :nx], xr[:, :nx], "x after round %d" % k)
        assert_close(P, Pr, "P after round %d" % k)


def test_propagate_only_launches():
    """no updates: `propagate` twice (single-propagate kernel, new order) against step_n with K = 2 and every measurement skipped
    (multi-propagate kernel, old order), bit for bit, and against the oracle"""
    inst, N, settings = I_7_3, 50, S_A
    a = make(inst, N, settings, seed_off=1)
    sc = a.sc
    for s in (0, 2):
        a.g.propagate(sc["u"][s], sc["dt"])
        a.g.propagate(sc["u"][s + 1], sc["dt"])
        a.read()
    assert KERNEL[inst] in a.g.describe()
    c = make(inst, N, settings, seed_off=1)
    skip = np.full_like(sc["slot"], -1)
    for s in (0, 2):
        c.g.step_n(np.ascontiguousarray(sc["u"][s:s + 2]), _dt(sc, 2), c.z[s + 1], skip, sc["R"])
        c.read()
    same(a, c)
    ref = oracle_route(a, with_updates=False)
    nx = 17 + 5 * (N - settings[0])
    for k, ((x, P, _, _, _), (xr, Pr, _)) in enumerate(zip(a.log, ref)):
        assert_close(x[:, :nx], xr[:, :nx], "x after round %d" % k)
        assert_close(P, Pr, "P after round %d" % k)
