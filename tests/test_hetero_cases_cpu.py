"""CPU checks of the per-filter case of the fused and streaming steps (tests/hetero_cases.py) before anything runs on a GPU,
with the oracle alone, for the N of every route of tests/test_gpu_hetero.py:

  * no verdict near the gate: every entry that reaches the gate has an oracle Mahalanobis distance below 4 or above 25 (the
    gate is at 9: the margin of tests/test_body_cases_cpu.py), so a last-bit difference cannot flip a result code;
  * the case reaches what it is for: every call's codes contain 0, 1, 3 and -1, code 2 appears in filter 1, len is
    [N, N - 3, 1, 0, N - 1] and the empty filter gets only 3 and -1; no compared element of the reference x is the residue
    of increments that cancel (hetero_cases.cancelled);
  * the inputs are not degenerate: with one input made uniform at a time -- dt := dt[0]; R := R of filter 0; R := R of
    measurement 0; R without its off-diagonal; slot := slot[0] with z unchanged -- x or P of every affected filter moves by at
    least 1e-6 of max |ref|, 1000 x the bound of tests.test_gpu_parity.assert_close: a kernel that makes that mistake cannot
    pass the GPU test.  A filter is affected if its input changed and, for the R and slot substitutions, it has at least one
    accepted update; every other filter must not move at all.  The move is taken at the end of the script, where the GPU
    test compares; above N = 77 after its first two calls (the oracle's dense update costs 13 ms at n = 316 and 50 ms at
    n = 496).  The first update of a fresh feature hardly reads R (H P H^T is 3700 px^2 against R of 10): it is the second
    and third call, on features measured before, that R moves."""
import numpy as np
import pytest

from tests import hetero_cases as hc

B = hc.B
CASES = hc.all_cases()
IDS = ["N%d-r%d%s" % (N, rm, "-M%d" % M if M else "") for N, rm, M in CASES]
BAR = 1e-6
MOVES = {}      # substitution -> the smallest move seen, for the summary line


def test_the_header_is_read_as_the_library_reports_it():
    """res_rows() parses viekf_instance_rows.hpp; the library reports (RB, NW, nmin, nmax) of its compiled table"""
    from tests.test_resmap_cpu import INSTANCES
    rows = hc.res_rows()
    assert [(r[0], r[1], r[3], r[4]) for r in rows] == list(INSTANCES)
    assert all(r[2] in (1, 2) and r[5] in (40, 80, 160) for r in rows)


def test_the_routes_are_the_ones_the_table_implies():
    rows = hc.res_rows()
    routes = hc.resident_routes()
    assert len(routes) == len(rows) + sum(r[3] >= 26 for r in rows) + 2
    assert {(r[4][0], r[1]) for r in routes} >= {("k_step_resident<2,1>", 5), ("k_step_resident<1,7>", 5)}
    two_waves = sorted(r[1] for r in routes if rows[r[3][0][1]][2] == 2)
    assert two_waves == [51, 51, 57, 65, 67, 72, 73, 77]
    # every forced row holds its size: the feature range and the blocks
    for _, N, _, tune, _ in routes:
        rb, nw, ns, nmin, nmax, kb = rows[tune[0][1]]
        assert nmin <= N <= nmax and N * (N + 1) // 2 <= rb * nw * 64
    # what a 256-CU device picks by itself (tests/test_gpu_fullbatch.py)
    assert [hc.row_name(hc.auto_row(N, 600, 256)) for N in (12, 20, 25)] == ["k_step_resident<2,1>", "k_step_resident<2,2>", "k_step_resident<3,2>"]
    assert hc.row_name(hc.auto_row(50, 1024, 256)) == "k_step_resident<7,3>" and hc.row_name(hc.auto_row(25, 256, 256)) == "k_step_resident<1,7>"


@pytest.mark.parametrize("N,r_mode,M", CASES, ids=IDS)
def test_no_verdict_near_the_gate(N, r_mode, M):
    c = hc.case(N, r_mode, M)
    for k in range(3):
        mah, codes = c["mahal"][k], c["codes"][k]
        at_gate = ~np.isnan(mah)
        assert (at_gate == ((codes == 0) | (codes == 1))).all()
        m = mah[at_gate]
        assert m.size and ((m < 4.0) | (m > 25.0)).all(), m
        assert ((mah > 25.0) == (codes == 1)).all()
    m = np.concatenate([a[~np.isnan(a)] for a in c["mahal"]])
    print("N = %d r_mode %d: Mahalanobis distances up to %.3g below the gate, from %.3g above it" % (N, r_mode, m[m < 9].max(), m[m > 9].min()))


@pytest.mark.parametrize("N,r_mode,M", CASES, ids=IDS)
def test_the_case_reaches_what_it_is_for(N, r_mode, M):
    c = hc.case(N, r_mode, M)
    assert list(c["len"]) == [N, N - 3, 1, 0, N - 1] and c["M"] == (M or hc.list_len(N))
    assert c["x0"].shape == (B, 17 + 5 * N) and c["P0"].shape == (B, 16 + 3 * N, 16 + 3 * N)
    assert np.isfinite(c["x_ref"]).all() and np.isfinite(c["P_ref"]).all()
    assert not hc.cancelled(c), "an element of the reference is what its increments cancel to: %s" % hc.cancelled(c)
    for k, cl in enumerate(c["calls"]):
        codes = c["codes"][k]
        assert set(np.unique(codes)) == {-1, 0, 1, 2, 3}, np.unique(codes)
        assert (codes[hc.NAN_FILTER] == 2).sum() == 1 and (codes[[0, 2, 3, 4]] != 2).all()
        assert set(np.unique(codes[3])) <= {-1, 3} and (codes[3] == 3).any()
        assert (codes[[0, 1, 4], hc.GATED_ENTRY] != 0).all() and codes[0, hc.GATED_ENTRY] == 1
        assert (codes[0, hc.GATED_ENTRY + 1:] == 0).any() and (codes[hc.NAN_FILTER, np.argmax(codes[hc.NAN_FILTER] == 2):] == 0).any() \
            or N == 5       # accepted entries BEHIND the gated one and the NaN one (filter 1 has two features at N = 5)
        R = cl["R"]
        assert R.shape == {0: (2, 2), 1: (B, 2, 2), 2: (B, c["M"], 2, 2)}[r_mode]
        R2 = R.reshape(-1, 2, 2)
        assert (R2[:, 0, 1] == R2[:, 1, 0]).all() and (R2[:, 0, 1] != 0.0).all() and (R2[:, 0, 0] != R2[:, 1, 1]).all()
        assert (np.linalg.eigvalsh(R2) >= 8.0 - 1e-12).all()
        slot = cl["slot"]
        assert all(not np.array_equal(slot[0], slot[b]) for b in range(1, B))
        one = np.flatnonzero(slot[hc.ONE_FEATURE_FILTER] == 0)       # the one-feature filter's slot, elsewhere than in filter 0's list
        assert len(one) and (slot[0, one] != 0).all() and (codes[hc.ONE_FEATURE_FILTER, one] == 0).any()
        assert (np.abs(R2[:, 0, 1]) >= hc.R_SPREAD).all() and (np.abs(R2[:, 0, 0] - R2[:, 1, 1]) >= hc.R_SPREAD).all()
        if M is None:                                                # the structured list
            for b in range(B):
                s = sorted(slot[b].tolist())
                assert s[0] == -1 and s[-1] == N + 2 and len(set(s)) == c["M"] - 1
                assert len(set(s[1:-1])) == c["M"] - 3 and 0 <= s[1] and s[-2] < N
                assert c["M"] < N + 3 or set(s[1:-1]) == set(range(N))
        else:
            assert (slot >= -1).all() and (slot < N).all() and c["M"] > (80 if N > 64 else 64)      # more than a fused launch holds
    assert len(set(c["dt"].tolist())) == B and np.array_equal(c["dt3"], hc.dt3_of(c["dt"])) and (c["dt3"][2] > c["dt3"][0]).all()


def _move(x, P, ref_x, ref_P, ln):
    """per filter: the larger of the relative moves of x (active part) and P"""
    out = np.zeros(B)
    for b in range(B):
        na = 17 + 5 * int(ln[b])
        out[b] = max(np.abs(x[b, :na] - ref_x[b, :na]).max() / np.abs(ref_x[b, :na]).max(), np.abs(P[b] - ref_P[b]).max() / np.abs(ref_P[b]).max())
    return out


@pytest.mark.parametrize("N,r_mode,M", CASES, ids=IDS)
def test_the_inputs_are_not_degenerate(N, r_mode, M):
    c = hc.case(N, r_mode, M)
    upto = 4 if N <= hc.LAST_RESIDENT_N else 2
    if upto < 4:
        codes, _, x_ref, P_ref = hc.run(c, upto=upto)
        codes = codes[:upto]
    else:
        x_ref, P_ref, codes = c["x_ref"], c["P_ref"], c["codes"]
    accepted = np.stack([(k == 0).any(axis=1) for k in codes]).any(axis=0)
    past_0 = np.stack([(k[:, 1:] == 0).any(axis=1) for k in codes]).any(axis=0)      # (measurement 0 keeps its own R)
    assert list(accepted) == [True, True, True, False, True]
    not0 = np.arange(B) != 0

    def diag_only(R):
        return R * np.eye(2)

    def of_filter_0(R):
        return np.broadcast_to(R[0], R.shape)

    def of_measurement_0(R):
        return np.broadcast_to(R[:, :1], R.shape)

    subs = [("dt := dt[0]", dict(dt=np.full(B, c["dt"][0])), not0),
            ("off-diagonal dropped", dict(R=diag_only), accepted),
            ("slot := slot[0]", dict(slot=lambda s: np.tile(s[0], (B, 1))), accepted & not0)]
    if r_mode >= 1:
        subs.append(("R := R of filter 0", dict(R=of_filter_0), accepted & not0))
    if r_mode == 2:
        subs.append(("R := R of measurement 0", dict(R=of_measurement_0), past_0))
    runs = hc.run_many(c, [kw for _, kw, _ in subs], upto)
    for (name, kw, affected), (_, _, x, P, _) in zip(subs, runs):
        mv = _move(x, P, x_ref, P_ref, c["len"])
        print("N = %d r_mode %d, %s: moves %s of filters %s" % (N, r_mode, name, " ".join("%.2e" % m for m in mv[affected]), np.flatnonzero(affected)))
        MOVES[name] = min(MOVES.get(name, np.inf), mv[affected].min())
        assert (mv[affected] >= BAR).all(), (name, mv)
        assert (mv[~affected] == 0.0).all(), (name, mv)      # (filter 0 keeps its inputs; the empty filter reads no R and no slot)


def test_the_smallest_moves():
    """(a line for the log: the smallest move per substitution over every case above; it runs after them)"""
    for name, v in sorted(MOVES.items()):
        print("smallest move, %s: %.2e" % (name, v))
    assert all(v >= BAR for v in MOVES.values())
