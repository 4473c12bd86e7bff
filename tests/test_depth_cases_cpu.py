"""CPU checks of the cases of a frame's DEPTH updates in one launch (tests/depth_cases.py) before anything runs on a GPU:

  * the identity k_update_depths rests on, restated in numpy (depth_cases.chain): every entry's column taken from the START
    P's lower triangle and brought up to date left-looking with the W and S^-1 of the entries applied before it, D riding
    along for the rho diagonals, and ONE trailing pass -- gives what the oracle's M sequential updates give (x, P and codes,
    within tests.test_gpu_parity.assert_close), and EXACTLY what the element-wise sequential formula
    P_ij -= L_ij (K[max(i,j)] W[min(i,j)]) gives entry by entry;
  * the condition on the inputs: every distance that reaches the gate is below 4 or above 25 (the gate is at 9), and above
    25 exactly where the code is GATED, so a last-bit difference cannot flip a verdict;
  * coverage: the cases reach what the GPU tests rely on.

A filter with a NaN in P is the one place where the oracle is NOT the reference: its dense P H^T meets the NaN in every entry
(0 * NaN) and skips them all, while viekf_batch_update forms W from the one column H names.  The contract is the latter; the
poisoned filter is held to the sequential formula alone, here and on the GPU (against the M-call route)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import depth_cases as dc
from tests import meas_cases as mc
from tests.test_gpu_parity import assert_close

B = dc.B
CASES = dc.all_cases()


def poisoned(name, b):
    return name == "poison" and b == dc.POISONED


@pytest.mark.parametrize("name,N,variant", CASES)
def test_left_looking_chain_and_one_trailing_pass_equal_sequential_updates(name, N, variant):
    c = dc.case(name, N, variant)
    for b in range(B):
        x, P, codes, flag, napp, fixes, mah = dc.chain(c, b, True)
        xs, Ps, codes_s, flag_s, napp_s, fixes_s, mah_s = dc.chain(c, b, False)
        # the element-wise sequential formula: exactly
        assert np.array_equal(x, xs) and np.array_equal(P, Ps, equal_nan=True), (c["name"], b)
        assert list(codes) == list(codes_s) and (flag, napp, fixes) == (flag_s, napp_s, fixes_s) and mah == mah_s
        assert list(codes) == list(c["codes"][b]), (c["name"], b, codes, c["codes"][b])
        if poisoned(name, b):
            continue
        assert_close(*mc.nan_split(x, c["x_ref"][b]), "x of filter %d, %s" % (b, c["name"]))
        assert_close(*mc.nan_split(P, c["P_ref"][b]), "P of filter %d, %s" % (b, c["name"]))
        if b in c["untouched"]:
            assert np.array_equal(c["x_ref"][b], c["x0"][b]) and np.array_equal(c["P_ref"][b], c["P0"][b], equal_nan=True)


@pytest.mark.parametrize("name,N,variant", CASES)
def test_no_entry_is_near_the_gate(name, N, variant):
    c = dc.case(name, N, variant)
    mah = c["mahal"][~np.isnan(c["mahal"])]
    print("%s: Mahalanobis distances up to %.3g below the gate, from %.3g above it" %
          (c["name"], mah[mah < 9].max(initial=0.0), mah[mah > 9].min(initial=np.inf)))
    assert mah.size and ((mah < 4.0) | (mah > 25.0)).all(), mah
    assert ((c["mahal"] > 25.0) == (c["codes"] == orc.MEAS_GATED)).all()
    if name not in ("neg", "mixed"):
        assert (mah < 0.25).all()                              # honest entries: the noise is within half a sigma
    if name == "poison":                                       # the poisoned filter applies what the oracle skipped
        d = np.array(dc.chain(c, dc.POISONED, True)[6])
        assert d.size == c["slot"].shape[1] and (d < 4.0).all(), d
    if name == "mixed":                                        # the second call: every entry gated, far above 25
        z, codes, d = dc.all_gated(c)
        reached = codes == orc.MEAS_GATED
        assert reached.any() and (d[reached] > 25.0).all() and np.isnan(d[~reached]).all()


def test_no_entry_behind_the_fused_steps_is_near_the_gate():
    c = dc.steps_case()
    assert (c["codes"] == 0).all() and (c["mahal"] < 0.25).all() and c["slot"].shape == (B, c["nfeat"])
    assert all(sorted(row) == list(range(c["nfeat"])) for row in c["slot"])


def test_the_cases_reach_what_they_are_for():
    for N in dc.SIZES:                                         # every slot once
        for v, (partial, r_mode, order) in enumerate(dc.ONCE_VARIANTS):
            c = dc.case("once", N, v)
            assert c["slot"].shape == (B, N) and list(c["len"]) == dc.fill(N) and c["mtype"] == orc.DEPTH
            assert (c["partial"], c["r_mode"], c["order"]) == (partial, r_mode, order)
            assert np.asarray(c["R"]).shape == ((), (B,), (B, N))[r_mode]
            for b in range(B):
                row = c["slot"][b]
                want = np.where(row < 0, -1, np.where(row >= c["len"][b], orc.MEAS_INVALID, 0))
                assert list(c["codes"][b]) == list(want)
                assert sorted(row[row >= 0]) == [s for s in range(N) if s in row]      # a permutation (less the -1)
            assert (c["slot"][dc.ONCE_SKIP_FILTER] == -1).sum() == 1
            if N > 1:
                assert (c["codes"] == orc.MEAS_INVALID).any() and (c["codes"] == 0).any()
            assert dc.chain(c, 0, True)[4] == N                                         # all of them applied
    for N in (5, 17):
        assert dc.case("once_inv", N, 0)["mtype"] == orc.INV_DEPTH and dc.case("once_inv", N, 1)["order"] == 1
    for v in (0, 1):                                           # M past a wave and past N, a slot three times
        c = dc.case("repeat", dc.REPEAT_N, v)
        assert c["slot"].shape == (B, dc.REPEAT_M) and dc.REPEAT_M > 64 > dc.REPEAT_N and c["order"] == v
        for b in range(B):
            assert list(np.flatnonzero(c["slot"][b] == dc.REPEAT_SLOT)) == list(dc.REPEAT_AT)
        assert (c["codes"][0] == 0).all() and dc.chain(c, 0, True)[4] == dc.REPEAT_M
        assert len(set(c["slot"][0])) < dc.REPEAT_M                                    # slots repeat
    for N in dc.MIXED_SIZES:                                   # mixed script
        c = dc.case("mixed", N, N % 2)
        codes, a = c["codes"], c["active"]
        assert set(a[dc.MIXED_ACTIVE_FILTER]) == {0, 1, 2}                              # 0, 1 and 2 within one row
        assert list(codes[dc.MIXED_ACTIVE_FILTER, :4]) == [0, 0, -1, orc.MEAS_GATED]
        assert codes[0, dc.MIXED_GATED] == codes[4, dc.MIXED_GATED] == orc.MEAS_GATED   # gated in the middle ...
        assert (codes[[0, 4], dc.MIXED_GATED + 1:] == 0).all()                          # ... accepted entries after it
        assert codes[dc.MIXED_NAN_FILTER, dc.MIXED_NAN] == orc.MEAS_NAN
        assert (codes[dc.MIXED_SKIPPED_FILTER] == -1).all() and dc.MIXED_SKIPPED_FILTER in c["untouched"]
        assert dc.chain(c, 0, True)[4] == dc.MIXED_M - 3 and dc.chain(c, 4, True)[4] == dc.MIXED_M - 2
    for N in (5, 17):                                          # fix_depth inside the chain
        c = dc.case("fix", N)
        assert c["active"][0, 0] == 0 and (c["codes"][[0, 4]] == 0).all()
        reset, p0rr = 1.0 / (2.0 * c["params"]["min_depth"]), c["params"]["P0_feat"][2]
        for b, feat, neg in ((0, 0, True), (0, 1, False), (1, 1, False), (4, 2, True)):
            k, d = 17 + 5 * feat + 4, 18 + 3 * feat
            assert c["x0"][b, k] == (-0.3 if neg else 250.0)
            assert feat in c["slot"][b][1:]                                             # an entry ON the edited diagonal follows
            first = c["P0"][b, d, d] + (reset + 0.3) ** 2 if neg else p0rr
            assert c["P_ref"][b, d, d] < first                                          # ... and subtracted from the edited value
        for b in (0, 1, 4):
            x, P, codes, flag, napp, fixes, mah = dc.chain(c, b, True)
            assert fixes >= 1 and napp >= 2
            assert bool(flag & dc.NEG_DEPTH_BIT) == (b in dc.FIX_NEG_FILTERS)
        c = dc.case("neg", N)                                  # an INV_DEPTH drives rho negative; the same slot again
        assert c["mtype"] == orc.INV_DEPTH and list(c["slot"][0]) == [dc.NEG_SLOT, 0, dc.NEG_SLOT]
        for b in range(B):
            x, P, codes, flag, napp, fixes, mah = dc.chain(c, b, True)
            assert bool(flag & dc.NEG_DEPTH_BIT) == (b in dc.NEG_FILTERS), (b, flag)
            if b in dc.NEG_FILTERS:
                assert napp == 3 and fixes == 1 and (c["codes"][b] == 0).all()
                d = 18 + 3 * dc.NEG_SLOT
                assert c["x0"][b, 17 + 5 * dc.NEG_SLOT + 4] == 0.004 and abs(c["x_ref"][b, 17 + 5 * dc.NEG_SLOT + 4] - reset) < 0.1
    for N in (5, 50):                                          # a NaN in P that one entry's column meets
        c = dc.case("poison", N)
        b = dc.POISONED
        col = 18 + 3 * dc.POISON_SLOT
        assert np.isnan(c["P0"][b, col, dc.POISON_ROW]) and np.isnan(c["P0"][b]).sum() == 2
        assert list(c["slot"][b]).count(dc.POISON_SLOT) == 1 and (c["codes"][b] == 0).all()
        x, P, codes, flag, napp, fixes, mah = dc.chain(c, b, True)
        assert napp == c["slot"].shape[1] - 1                                           # that entry skipped, the others applied
        assert not np.array_equal(x, c["x0"][b]) and np.isnan(P).sum() == 2 and not np.isnan(x).any() and flag == 0
        assert np.array_equal(c["x_ref"][b], c["x0"][b])                                # (the oracle skipped them all)
