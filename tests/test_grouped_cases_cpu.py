"""The cases of tests/test_gpu_grouped.py held to their conditions, on the CPU: from the oracle's codes and the Python model of
the grouped kernels' window and scan (tests/grouped_cases.py::groups), for every route's group size."""
import numpy as np
import pytest

from tests import grouped_cases as gc

CASES = sorted({(r[1], r[4]) for r in gc.ROUTES})


def test_the_routes_are_the_six_of_the_table():
    assert [(r[1], r[2], r[3]) for r in gc.ROUTES] == [
        (20, (), "k_update_feat_panelsvc<512,16>"),
        (20, (("TUNE_PANEL_SERVICE", 0), ("TUNE_BLOCK_GROUP", 16)), "k_update_feat_blocked<512,16>"),
        (20, (("TUNE_PANEL_SERVICE", 0), ("TUNE_BLOCK_GROUP", 24)), "k_update_feat_blocked<512,24>"),
        (20, (("TUNE_PANEL_SERVICE", 0), ("TUNE_BLOCK_GROUP", 32)), "k_update_feat_blocked<512,32>"),
        (78, (), "k_update_feat_panelsvc<512,16>"),
        (78, (("TUNE_PANEL_SERVICE", 0),), "k_update_feat_blocked<512,16>")]
    for _, N, _, _, _, padded in gc.ROUTES:     # dense columns: the stride is below the tile rows' 16 ceil(n / 16); padded: equal
        n = 16 + 3 * N
        assert (gc.cov_ld(N) == (n + 15) // 16 * 16) == padded and gc.cov_ld(N) == {20: 76, 78: 256}[N]


def test_the_model_of_window_and_scan():
    """cap, repeat, window end, list end, and a window without a group, on lists small enough to follow by hand"""
    assert gc.groups([0, 1, 2, 3], 2) == [(0, 2, 2, "cap"), (2, 4, 2, "cap")]
    assert gc.groups([0, 1, 0, 2], 4, 8) == [(0, 2, 2, "repeat"), (2, 4, 2, "end")]
    assert gc.groups([5, -1, -1, -1, -1, -1, 6], 2, 4) == [(0, 4, 1, "window"), (4, 7, 1, "end")]
    assert gc.groups([-1, -1, -1, -1, 3], 2, 4) == [(0, 4, 0, "window"), (4, 5, 1, "end")]


@pytest.mark.parametrize("N,BG", CASES)
def test_the_lists_reach_what_they_are_for(N, BG):
    c = gc.case(N, BG)
    M, BWIN, full = c["slot"].shape[1], 2 * BG, min(BG, c["nfeat"])
    assert M >= 3 * BWIN
    assert np.isfinite(c["x_ref"]).all() and np.isfinite(c["P_ref"]).all()
    for b in range(gc.B):
        adm = gc.admissible(c["slot"][b], c["z"][b], c["nfeat"])
        assert np.array_equal(adm >= 0, (c["codes"][b] == 0) | (c["codes"][b] == 1))
        assert set(c["codes"][b].tolist()) == {-1, 0, 1, 2, 3}, (b, set(c["codes"][b].tolist()))
        gs = gc.groups(adm, BG)
        assert gs[-1][1] == M and all(g[1] == h[0] for g, h in zip(gs, gs[1:]))
        first = gs[0]                                                                # (a)
        assert first[2] == full and first[3] == ("cap" if BG <= c["nfeat"] else "repeat"), first
        assert any(w == "repeat" and 1 < k < full for _, _, k, w in gs)               # (b)
        assert any(k == 0 and e - s == BWIN for s, e, k, _ in gs)                     # (c): a whole window, no group
        run = max(len(t) for t in "".join("x" if a < 0 else " " for a in adm).split())
        assert run >= BWIN
        assert any(w == "window" and 0 < k < BG and e - s == BWIN for s, e, k, w in gs)   # (d)
        gated = np.flatnonzero(c["codes"][b] == 1)                                    # (e): applied entries of its group on both sides
        assert len(gated) == 1
        s, e = next((s, e) for s, e, _, _ in gs if s <= gated[0] < e)
        assert (c["codes"][b, s:gated[0]] == 0).any() and (c["codes"][b, gated[0] + 1:e] == 0).any()
        last = gs[-1]                                                                 # (f)
        assert last[3] == "end" and 0 < last[2] < BG and last[1] - last[0] < BWIN and adm[M - 1] >= 0
        # the three kinds of inadmissible entry, all inside the run of (c)
        assert (c["slot"][b] < 0).any() and (c["what"][b] == 2).any() and (c["slot"][b] >= c["N"]).any()
        assert ((c["slot"][b] >= c["nfeat"]) & (c["slot"][b] < c["N"])).any()


def test_the_filters_differ():
    for N, BG in CASES:
        c = gc.case(N, BG)
        assert not np.array_equal(c["slot"][0], c["slot"][1]) and not np.array_equal(c["slot"][1], c["slot"][2])
