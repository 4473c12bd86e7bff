"""The two grouped wide-P update kernels (vi_ekf_amd/csrc/viekf_kernels_grouped.hpp) where their window, scan, panel load and
epilogue could drift apart: k_update_feat_panelsvc and k_update_feat_blocked at every group size, on dense columns (N = 20,
ld = 76) and on padded ones (N = 78, ld = 256), on the lists of tests/grouped_cases.py -- a full group, a group closed by a
repeated slot, a whole window without a group, a group cut by a window's end, a gated entry in mid-group, a list ending
inside a group; B = 3 filters with their own lists.  One propagate, then update_feat alone.  The oracle applies the entries
one by one: codes bit for bit, x and P with tests.test_gpu_parity.assert_close.  tests/test_grouped_cases_cpu.py holds the
lists to those conditions."""
import numpy as np
import pytest

import vi_ekf_amd as v
from tests import grouped_cases as gc
from tests.test_gpu_parity import assert_close
from vi_ekf_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("route,N,tune,name,BG,padded", gc.ROUTES, ids=[r[0] for r in gc.ROUTES])
def test_grouped_update_routes_vs_oracle(route, N, tune, name, BG, padded):
    c = gc.case(N, BG)
    g = v.BatchVIEKF(gc.B, N, c["params"])
    g.set_kernel(1)
    for key, value in tune:
        g.set_tuning(getattr(capi, key), value)
    assert name in g.describe(), g.describe()
    for i in range(c["nfeat"]):
        assert (g.init_feature(c["pix"][:, i, :].copy(), np.full(gc.B, np.nan)) == 1).all()
    g.propagate(c["u"], c["dt"])
    codes = g.update_feat(c["z"], c["slot"], c["R"])
    assert g.describe().count(name) == 1
    bad = np.argwhere(codes != c["codes"])
    assert bad.size == 0, "%s: codes differ at (filter, entry) %s: %s vs the oracle's %s" % (
        route, bad[:8].tolist(), codes[tuple(bad[:8].T)], c["codes"][tuple(bad[:8].T)])
    x, P = g.get_state(), g.get_covariance()
    print("%s: max |x - ref| / max |ref| %.3e, P %.3e" % (route, np.abs(x - c["x_ref"]).max() / np.abs(c["x_ref"]).max(),
                                                          np.abs(P - c["P_ref"]).max() / np.abs(c["P_ref"]).max()))
    assert_close(x, c["x_ref"], route + ": x")
    assert_close(P, c["P_ref"], route + ": P")
