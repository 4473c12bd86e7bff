"""The conditions tests/meas_cases.py promises, checked on the CPU for every (N, partial, drag) the GPU test runs: the script's
result codes are exactly the designated ones (so none of its updates is gated or skipped by accident), the negative-depth
case really takes fix_depth's reset, every P stays finite but the one poisoned on purpose -- and the numpy twin, a second and
independent reference, runs the WHOLE script from its own warm state, never re-seeded from the oracle, and agrees with the
oracle after every call to the bar the GPU is held to (assert_close of tests/test_gpu_parity.py).  That agreement over the
script is what the GPU tolerance rests on: inputs on which two fp64 references part, in one call or by amplification
across calls, would be too ill-conditioned to hold a kernel to."""
import numpy as np
import pytest

from oracle import np_twin, oracle as orc
from tests import meas_cases as mc
from tests.test_gpu_parity import assert_close

B = mc.B


def _rel(a, b):
    a, b = mc.nan_split(a, b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _twin_call(t, kind, a, b):
    """script entry on the twin of filter b -> the call's result for filter b"""
    if kind == "update":
        act = 1 if a["active"] is None else int(a["active"][b])
        sl = int(a["slot"][b]) if a["slot"] is not None else 0
        R = a["R"][b] if a["R"].ndim == 3 else a["R"]
        return t.update(a["mtype"], a["z"][b], R, sl, bool(act))
    if kind == "init_feature":
        return int(t.init_feature(a["pix"][b], float(a["depth"][b])))
    if kind == "keep_features":
        for s in reversed(range(t.len)):          # (from the back: the slots in front of a dropped one keep their numbers)
            if not a["keep"][b, s]:
                t.clear_feature(s)
        return t.len
    if kind == "keyframe_reset":
        return t.keyframe_reset_edge()
    if kind == "propagate":
        t.propagate(a["u"][b], float(a["dt"][b]))
        return None
    raise ValueError(kind)


@pytest.mark.parametrize("N,partial,drag", mc.CASES)
def test_script_conditions_and_twin_agreement(N, partial, drag):
    sc, fs, script = mc.cached(N, partial, drag)
    prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
    twins = []
    for b in range(B):          # the twin's own warm state: all N features, the two warm steps
        t = np_twin.TwinFilter(N, **prm)
        for i in range(N):
            t.init_feature(sc["pix"][b, i])
        for s in range(2):
            z, slot = mc.warm_inputs(sc, N, s)
            t.propagate(sc["u"][s, b], sc["dt"][b])
            for m in range(slot.shape[1]):
                assert t.update_feat(z[b, m], sc["R"], int(slot[b, m])) == 0
        assert_close(t.x, fs[b].x, "twin x after the warm steps, filter %d" % b)
        assert_close(t.P, fs[b].P, "twin P after the warm steps, filter %d" % b)
        twins.append(t)
    rho0 = 1.0 / (2.0 * prm["min_depth"])
    worst = {"x": 0.0, "P": 0.0}
    poisoned = set()
    seen = set()
    for kind, a in script:
        what = a["label"]
        before = [(f.x.copy(), f.P.copy(), f.len_features) for f in fs]
        ret = mc.apply_oracle(fs, kind, a)
        # the designated results, and no other
        if kind == "update":
            seen.add(a["mtype"])
            assert {b: int(c) for b, c in enumerate(ret) if c != 0} == a["expect"], (what, ret)
        elif kind in ("init_feature", "keep_features"):
            assert {b: int(c) for b, c in enumerate(ret)} == a["expect"], (what, ret)
        for b in a["untouched"]:
            assert np.array_equal(fs[b].x, before[b][0], equal_nan=True), (what, b)
            assert np.array_equal(fs[b].P, before[b][1], equal_nan=True), (what, b)
        if kind == "poison_P":
            poisoned.add(a["b"])
            twins[a["b"]].P[a["i"], a["j"]] = twins[a["b"]].P[a["j"], a["i"]] = np.nan
            continue
        for b in range(B):
            assert np.isfinite(fs[b].x).all(), (what, b)
            assert np.isfinite(fs[b].P).all() == (b not in poisoned), (what, b)
        # the twin, from wherever the script so far has taken it
        for b in range(B):
            if kind == "update" and ret[b] not in (orc.MEAS_SUCCESS, orc.MEAS_GATED):
                continue        # (skipped, invalid slot, NaN in z: decided before the filter is looked at)
            if kind in ("init_feature", "keyframe_reset") and a["mask"] is not None and not a["mask"][b]:
                continue
            t = twins[b]
            tr = _twin_call(t, kind, a, b)
            if kind == "keyframe_reset":
                assert_close(tr, ret[b], "twin edge, %s, filter %d" % (what, b))
            elif kind != "propagate":
                assert tr == ret[b], (what, b, tr, ret[b])
            assert t.len == fs[b].len_features
            for nm, got, ref in (("x", t.x, fs[b].x), ("P", t.P, fs[b].P)):
                assert_close(*mc.nan_split(got, ref), "twin %s, %s, filter %d" % (nm, what, b))
                worst[nm] = max(worst[nm], _rel(got, ref))
        if what == "INV_DEPTH that drives rho negative":
            # accepted, rho < 0, reset to rho0 with (rho0 - rho)^2 added to P_rr: the closed form for a fresh feature,
            # P_rr = P0_feat[2], R = 0.01, lambda_rho = lam_feat[2]
            P0, R, l = prm["P0_feat"][2], 0.01, (prm["lam_feat"][2] if partial else 1.0)
            K = P0 / (P0 + R)
            rho = rho0 + l * K * (-3.0 * rho0)
            assert rho < 0.0
            Pn = P0 + (2 * l - l * l) * (P0 * R / (P0 + R) - P0) + (rho0 - rho) ** 2
            assert abs(Pn - (0.264 if partial else 0.946)) < 1e-3
            for b in mc.NEG_DEPTH_FILTERS:
                d = 18 + 3 * int(a["slot"][b])
                assert before[b][1][d, d] == P0 and before[b][0][21 + 5 * int(a["slot"][b])] == rho0
                assert fs[b].x[21 + 5 * int(a["slot"][b])] == rho0
                assert fs[b].P[d, d] != before[b][1][d, d] and abs(fs[b].P[d, d] - Pn) < 1e-12
    assert seen == {orc.ACC, orc.ALT, orc.ATT, orc.POS, orc.VEL, orc.QZETA, orc.DEPTH, orc.INV_DEPTH, orc.FEAT}
    assert poisoned == {mc.POISONED}
    print("twin vs oracle over the script, N = %d partial = %d drag = %d: max rel err x %.2e, P %.2e" % (N, partial, drag, worst["x"], worst["P"]))


def test_the_ragged_fill_is_what_it_says():
    for N in (5, 50, 77, 83):
        keep = mc.first_keep(N)
        assert list(keep.sum(axis=1)) == mc.fill(N) == [N, N - 3, 1, 0, N - 1]
        assert keep[1, 0] and keep[1, N - 1] and not keep[4, (N - 1) // 2]      # from the middle outwards
