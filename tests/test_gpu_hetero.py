"""The fused step, the streaming family and the tile family on inputs that differ PER FILTER: dt [B], a non-diagonal R in all
three modes ((2,2), (B,2,2), (B,M,2,2)), a slot list permuted per filter and the ragged batch len = [N, N - 3, 1, 0, N - 1] in
ONE launch.  Every other parity test of the hot path takes its inputs from vi_ekf_amd/scene.py::make_scene, which is uniform
over the batch in exactly those places: a kernel reading dt_all[0], a transposed R, filter 0's slot row or a wrong r_stride
passes them all.  The case, its script of four calls (step, update_feat, step_n with K = 3, propagate) and the reasons for its
inputs are in tests/hetero_cases.py; tests/test_hetero_cases_cpu.py checks on the CPU that no entry is near the gate, that
the case reaches what it is for and that each of those mistakes moves x or P by at least 1000 x the bound used here.

The reference is the CPU oracle, per filter, one call after the other.  Result codes are compared exactly after every call;
x (each filter's active part) and P (whole) only at the end of the script, with tests.test_gpu_parity.assert_close, so that a
packed P carries between the fused launches; P == P^T bit for bit; no NaN, blow-up or internal bit in the status word.
Every route asserts through describe() that it runs what it names.  B = 5: more than one workgroup, and in the paired tile
kernel filters (0, 1) of len N and N - 3 and (2, 3) of len 1 and 0 share a workgroup while filter 4 is alone in the last."""
import numpy as np
import pytest

import vi_ekf_amd as v
from tests import hetero_cases as hc
from tests.test_gpu_body import start_P
from tests.test_gpu_parity import assert_close
from vi_ekf_amd import capi

pytestmark = pytest.mark.gpu

B = hc.B
ROUTES = hc.resident_routes() + hc.STREAM_ROUTES


def make_batch(c, kernel, tune, names):
    """a batch on the route (tunings first), at the case's start state: the oracle's x, P and len, written with set_state"""
    g = v.BatchVIEKF(B, c["N"], c["params"])
    if kernel in (3, 5):
        g.set_tuning(capi.TUNE_TILES, 2 if kernel == 3 else 3)
    elif kernel:
        g.set_kernel(kernel)
    for key, value in tune:
        g.set_tuning(getattr(capi, key), value)
    d = g.describe()
    for name in names:
        assert name in d, d
    if names[0].startswith("k_step"):
        assert d.startswith(names[0]), d
    g.set_state(x=c["x0"], P=start_P(c), len_features=c["len"])
    assert g.describe() == d
    return g


def run_script(g, c, what):
    c0, c1, c2 = c["calls"]
    u, dt = c["u"], c["dt"]
    calls = (("step", lambda: g.step(u[0], dt, c0["z"], c0["slot"], c0["R"])),
             ("update_feat", lambda: g.update_feat(c1["z"], c1["slot"], c1["R"])),
             ("step_n", lambda: g.step_n(np.ascontiguousarray(u[1:4]), c["dt3"], c2["z"], c2["slot"], c2["R"])))
    for k, (name, call) in enumerate(calls):
        codes = call()
        bad = np.argwhere(codes != c["codes"][k])
        assert bad.size == 0, "%s, %s: codes differ at (filter, entry) %s: %s vs the oracle's %s" % (
            what, name, bad[:8].tolist(), codes[tuple(bad[:8].T)], c["codes"][k][tuple(bad[:8].T)])
    g.propagate(u[4], dt)
    x, P = g.get_state(), g.get_covariance()
    for b in range(B):
        na = 17 + 5 * int(c["len"][b])
        assert_close(x[b, :na], c["x_ref"][b, :na], "%s: x of filter %d (len %d)" % (what, b, c["len"][b]))
    for b in range(B):
        assert_close(P[b], c["P_ref"][b], "%s: P of filter %d (len %d)" % (what, b, c["len"][b]))
    assert_close(P, c["P_ref"], what + ": P")
    assert np.array_equal(P, P.transpose(0, 2, 1)), what + ": P != P^T"
    st = g.get_status()
    assert (st & (capi.FLAG_NAN | capi.FLAG_BLOWING_UP | capi.FLAG_INTERNAL) == 0).all(), (what, st)
    assert np.array_equal(g.get_len_features(), c["len"])


@pytest.mark.parametrize("r_mode", [0, 1, 2])
@pytest.mark.parametrize("route,N,kernel,tune,names", ROUTES, ids=[r[0] for r in ROUTES])
def test_script_on_every_route(route, N, kernel, tune, names, r_mode):
    """the resident family -- every row of kResInst forced at its nmax, rows from nmin 26 also at their nmin, <2,1> and <1,7>
    also at N = 5 -- and the streaming family: every propagate and every update kernel it has.

    Measured on an MI355X over the 120 cases of this file: result codes equal everywhere; P within 1.3e-14 of max |ref| and
    2.0e-8 element-wise; x within 3.0e-12 of max |ref| and 1.5e-7 element-wise.  The start state is away from zero
    (hetero_cases.X0_AWAY): from the scene's own hover at the origin the attitude's vector part and the biases are what
    hundreds of increments of either sign leave, and one such residue (the yaw component, 2.5e-8 after increments summing to
    9.4e-4) missed the element-wise bar by 1.19e-6 while every array agreed to 5e-13 in norm -- hetero_cases.cancelled()
    states when the bar can be asked of an element, and tests/test_hetero_cases_cpu.py holds every case to it."""
    c = hc.case(N, r_mode)
    run_script(make_batch(c, kernel, tune, names), c, "%s r_mode %d" % (route, r_mode))


@pytest.mark.parametrize("r_mode", [0, 1, 2])
@pytest.mark.parametrize("route,N,kernel,tune,names", hc.TILE_ROUTES, ids=[r[0] for r in hc.TILE_ROUTES])
def test_script_on_the_tile_family(route, N, kernel, tune, names, r_mode):
    """N = 46 and 50, one filter per workgroup and the paired form: there two filters of DIFFERENT size loop in step"""
    c = hc.case(N, r_mode)
    run_script(make_batch(c, kernel, tune, names), c, "%s r_mode %d" % (route, r_mode))


@pytest.mark.parametrize("r_mode", [1, 2])
@pytest.mark.parametrize("route,N,M,kernel,tune,names", hc.CHUNKED_ROUTES, ids=[r[0] for r in hc.CHUNKED_ROUTES])
def test_chunked_lists_with_their_own_R(route, N, M, kernel, tune, names, r_mode):
    """more measurements than one fused launch holds: the later chunks read z, slot, the codes and R at an offset (d_R + rsm m0
    with the filter stride still 4 M).  Slots drawn per filter from -1 .. N - 1, R per filter and per entry"""
    c = hc.case(N, r_mode, M)
    assert c["M"] == M > 64
    run_script(make_batch(c, kernel, tune, names), c, "%s r_mode %d" % (route, r_mode))
