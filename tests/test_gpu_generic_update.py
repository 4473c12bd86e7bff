"""k_update_generic (every measurement that is not a hot-path FEAT update goes through it: viekf_batch_update) and the
lifecycle kernels next to it -- k_init_feature, k_keep_features, k_keyframe_reset -- against the CPU oracle where a column
stride can be told from a row count and a feature count from a capacity: odd n and padded ld (N = 5: n = 31, ld = 32; 77: 247 /
248; 83: 265 / 272), filters of len N, N - 3, 1, 0 and N - 1 in ONE launch, a per-filter R with off-diagonal terms, both values
of use_partial_update, active = 0 / 1 / 2, fix_depth after an accepted update, the NaN-in-K skip, and per-filter live ring slots.

The form P is in when an update arrives: reading P (get_covariance) brings it to the full form, and run_script reads it after
every call but one.  So every update but one finds a full P.  The exception is the QZETA update of every filter's last feature
that follows the script's `propagate` entry: nothing reads or converts P between the two, so that update enters through
viekf_batch_update's own conversion -- from the fused kernel's packed image where the batch keeps one (whole-batch mode, the
on-chip family; asserted through describe() at N = 50), from a lower-triangle-only P otherwise (the matrix-core propagate at
N = 83, the streaming family, per-filter mode, which is never packed).  Without that conversion every case here fails at that
update.  The comparison after QZETA checks the propagate as well.

The script of calls and the reasons for its inputs are in tests/meas_cases.py; tests/test_meas_cases_cpu.py checks on the CPU
that the oracle accepts what it is meant to accept and that a second fp64 reference, run over the same script, agrees with
it, which is what the tolerance here (assert_close of tests/test_gpu_parity.py, unchanged) rests on."""
import ctypes as C

import numpy as np
import pytest

import vi_ekf_amd as v
from vi_ekf_amd import capi
from tests import meas_cases as mc
from tests.helpers import apply_kernel
from tests.test_gpu_parity import assert_close

pytestmark = pytest.mark.gpu

B = mc.B
NAN_BIT, NEG_DEPTH_BIT = 1, 4


def make_gpu(sc, N, kernel=0):
    """a batch at the warm state the script starts from: all N features, two steps of min(N, 8) FEAT updates"""
    g = apply_kernel(v.BatchVIEKF(B, N, sc["params"]), kernel)
    for i in range(N):
        assert (g.init_feature(sc["pix"][:, i, :].copy(), np.full(B, np.nan)) == 1).all()
    for s in range(2):
        z, slot = mc.warm_inputs(sc, N, s)
        assert (g.step(sc["u"][s], sc["dt"], z, slot, sc["R"]) == 0).all()
    return g


def apply_gpu(g, kind, a):
    if kind == "update":
        return g.update(a["mtype"], a["z"], a["R"], a["slot"], a["active"])
    if kind == "init_feature":
        return g.init_feature(a["pix"].copy(), a["depth"], a["mask"])
    if kind == "keep_features":
        return g.keep_features(a["keep"])
    if kind == "keyframe_reset":
        return g.keyframe_reset(a["mask"])
    if kind == "propagate":
        return g.propagate(a["u"], a["dt"])
    if kind == "poison_P":
        P = g.get_covariance()
        P[a["b"], a["i"], a["j"]] = P[a["b"], a["j"], a["i"]] = np.nan
        return g.set_state(P=P)
    raise ValueError(kind)


def _rel(got, ref):
    got, ref = mc.nan_split(got, ref)
    return np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-300)


def run_script(gs, fs, script, tag):
    """every script entry on the batches gs and on the oracle filters fs; gs[0] against the oracle after every call, gs[1:]
    bit for bit against gs[0].  After `propagate` nothing is read on the device, and before a call x and P are read only when
    the call has filters to leave untouched (the update after the propagate has none): that update meets P as the propagate
    left it, and the comparison after it covers both."""
    g = gs[0]
    worst = {"x": 0.0, "P": 0.0}
    status = {}
    after_propagate = False
    for kind, a in script:
        what = "%s: %s" % (tag, a["label"])
        if a["untouched"]:
            x0, P0 = g.get_state(), g.get_covariance()
        rets = [apply_gpu(h, kind, a) for h in gs]
        ref = mc.apply_oracle(fs, kind, a)
        if kind == "propagate":
            after_propagate = True
            continue
        if after_propagate:
            assert kind == "update" and not a["untouched"], "the call after the propagate must not have P read before it"
            after_propagate = False
        x, P = g.get_state(), g.get_covariance()
        xr, Pr = np.stack([f.x for f in fs]), np.stack([f.P for f in fs])
        worst["x"], worst["P"] = max(worst["x"], _rel(x, xr)), max(worst["P"], _rel(P, Pr))
        print("%-60s x %.2e  P %.2e" % (what, _rel(x, xr), _rel(P, Pr)))
        if kind == "keyframe_reset":
            assert_close(rets[0], ref, "edge, " + what)
        elif ref is not None:
            assert np.array_equal(rets[0], ref), (what, rets[0], ref)          # result codes, ok, new_len: bit-exact
        if kind in ("update", "init_feature", "keep_features"):
            exp = a["expect"]
            got = {b: int(c) for b, c in enumerate(rets[0]) if c != 0 or kind != "update"}
            assert got == exp, (what, got, exp)
        assert (g.get_len_features() == mc.lens(fs)).all(), what
        assert_close(*mc.nan_split(x, xr), "x after " + what)
        assert_close(*mc.nan_split(P, Pr), "P after " + what)
        if kind == "update":       # exactly symmetric: the grouped FEAT kernels that follow read one triangle only
            assert np.array_equal(P, P.transpose(0, 2, 1), equal_nan=True), "P != P^T after " + what
        for b in a["untouched"]:
            assert np.array_equal(x[b], x0[b], equal_nan=True) and np.array_equal(P[b], P0[b], equal_nan=True), \
                "filter %d touched by %s" % (b, what)
        for h, r in zip(gs[1:], rets[1:]):
            assert r is None or np.array_equal(rets[0], r), what
            assert np.array_equal(x, h.get_state(), equal_nan=True), "x of the two batches after " + what
            assert np.array_equal(P, h.get_covariance(), equal_nan=True), "P of the two batches after " + what
        status[a["label"]] = g.get_status()
    print("%s: GPU vs oracle max rel err x %.2e, P %.2e" % (tag, worst["x"], worst["P"]))
    return status


def check_status(status, gs):
    """the negative-depth bit on the filters fix_depth reset, the NaN bit on the poisoned one, neither anywhere else"""
    neg = np.array([b in mc.NEG_DEPTH_FILTERS for b in range(B)])
    nan = np.arange(B) == mc.POISONED
    before = status["init_feature with depth NaN"]
    assert not (before & (NEG_DEPTH_BIT | NAN_BIT)).any(), before
    st = status["INV_DEPTH that drives rho negative"]
    assert (((st & NEG_DEPTH_BIT) != 0) == neg).all() and not (st & NAN_BIT).any(), st
    for label in ("NaN into P", "ALT on a P with a NaN", "POS after the reset"):
        st = status[label]
        assert (((st & NEG_DEPTH_BIT) != 0) == neg).all() and (((st & NAN_BIT) != 0) == nan).all(), (label, st)
    for h in gs[1:]:
        assert (h.get_status() == gs[0].get_status()).all()


@pytest.mark.parametrize("N,partial,drag,kernel", [c + (0,) for c in mc.CASES] + [(5, 1, 1, 1)])
def test_script_against_the_oracle(N, partial, drag, kernel):
    """the script call by call on a BatchVIEKF and on the oracle: result codes, ok and new_len bit-exact, x, P and the keyframe
    edges to assert_close, len equal, P == P^T bit for bit after every update, every filter a call must not touch (gated, NaN in
    z, invalid slot, active == 2, masked, ok == 0, the skipped update on a P with a NaN) bit for bit what it was, and the
    status bits.  kernel = 1 forces the streaming family (the warm steps then leave a plain full P)."""
    sc, fs, script = mc.cached(N, partial, drag)
    g = make_gpu(sc, N, kernel)
    print(g.describe())
    if N == 50:        # the headline size keeps P packed between fused launches: the update after the propagate unpacks it
        assert "P packed" in g.describe(), g.describe()
    assert_close(g.get_state(), np.stack([f.x for f in fs]), "x after the warm steps")
    assert_close(g.get_covariance(), np.stack([f.P for f in fs]), "P after the warm steps")
    status = run_script([g], fs, script, "N=%d partial=%d drag=%d kernel=%d" % (N, partial, drag, kernel))
    check_status(status, [g])


@pytest.mark.parametrize("N", [5, 83])
def test_per_filter_live_slots(N):
    """a.si(b) != b: every filter's live state in a ring slot of its own (slots [0, 2, 1, 0, 2] of a ring of 3).  The same calls
    against the oracle as above, and bit for bit against a second batch that runs them in its own buffers."""
    sc, fs, script = mc.cached(N, 1, 1)
    ga, gb = make_gpu(sc, N), make_gpu(sc, N)
    L = capi.lib()
    slots = np.array([0, 2, 1, 0, 2], dtype=np.int32)
    ga.history_resize(3)
    capi.check(L.viekf_batch_snapshot_filters(ga._h, C.c_void_p(slots.ctypes.data), capi.HOST))
    ga.select_filters(slots)
    assert np.array_equal(ga.get_state(), gb.get_state()) and np.array_equal(ga.get_covariance(), gb.get_covariance())
    status = run_script([ga, gb], fs, script, "N=%d live slots" % N)
    check_status(status, [ga, gb])
