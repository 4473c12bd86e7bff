"""The lane pass of the fused-step kernel's block ownership map (vi_ekf_amd/csrc/viekf_resmap.cpp: build_resmap).

The kernels that publish a feature's column pair with one store body per wave (res_merged_publish, viekf_fused_lds.hpp) rely on a
worker thread not holding two blocks with a common feature: build_resmap's last pass permutes lanes inside each (slot, wave) group
until none does, or as few as it reaches, and the library reports what is left per worker wave (viekf_debug_resmap_repeats).  A
(thread, feature) repeat is counted here from the map itself -- over the threads and the features, the number of the thread's
owned blocks that hold the feature, less one -- and must equal the library's count for every dispatch-table row and every N of its
range.  The headline instance <7,3> is left without any for N = 46 .. 49 and with at most one per wave at N = 50.  The map's other
invariants stay with tests/test_resmap_cpu.py.  Pure host arithmetic, no GPU.
"""
import ctypes as C

import numpy as np
import pytest

from vi_ekf_amd import capi
from tests.test_resmap_cpu import INSTANCES, build


def reported(n, rb, nw):
    fn = capi.lib().viekf_debug_resmap_repeats
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    out = np.full(nw, -1, dtype=np.int32)
    rc = fn(n, rb, nw, C.c_void_p(out.ctypes.data))
    return rc, out


def recount(m, n, nw):
    """(thread, feature) repeats per worker wave, from the map [rb][64 nw]"""
    owned = (m >> 16) != 0
    I, J = m & 0xFF, (m >> 8) & 0xFF
    per_wave = np.zeros(nw, dtype=np.int64)
    for t in range(m.shape[1]):
        held = np.zeros(256, dtype=np.int64)
        for a in range(m.shape[0]):
            if owned[a, t]:
                held[I[a, t]] += 1
                if J[a, t] != I[a, t]:
                    held[J[a, t]] += 1
        per_wave[t // 64] += np.maximum(held - 1, 0).sum()
    return per_wave


@pytest.mark.parametrize("rb,nw,n_min,n_max", INSTANCES)
def test_reported_repeats_are_the_maps(rb, nw, n_min, n_max):
    for n in range(n_min, n_max + 1):
        rc_map, m = build(n, rb, nw)
        assert rc_map > 0
        total, per_wave = reported(n, rb, nw)
        mine = recount(m, n, nw)
        assert total == mine.sum() and (per_wave == mine).all(), "N=%d <%d,%d>: library %s, map %s" % (n, rb, nw, per_wave, mine)


@pytest.mark.parametrize("n", [46, 47, 48, 49])
def test_headline_instance_has_no_repeat_below_fifty(n):
    rc, m = build(n, 7, 3)
    assert rc > 0 and recount(m, n, 3).sum() == 0
    assert reported(n, 7, 3)[0] == 0


def test_headline_map_has_at_most_one_repeat_per_wave():
    rc, m = build(50, 7, 3)
    mine = recount(m, 50, 3)
    assert rc == 7 and (mine <= 1).all() and mine.sum() <= 3
    total, per_wave = reported(50, 7, 3)
    assert total <= 3 and (per_wave <= 1).all()


def test_refused_sizes_report_failure():
    assert reported(52, 7, 3)[0] < 0
