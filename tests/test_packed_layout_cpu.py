"""Host-side invariants of the packed image of P (vi_ekf_amd/csrc/viekf_instance_rows.hpp: ResPack).

Between two fused launches a filter's n * ld doubles of the P buffer may hold the kernel's own image: every worker thread's
block registers in 16-byte pairs, then the LDS-resident body columns and body block.  A wrong offset rule would let two values
share a place, or write past the filter's P.  Checked here through the library's own rule (viekf_debug_packed_layout) and its
own ownership map (viekf_debug_build_resmap), for every instance row and every feature count of its range -- pure host
arithmetic, no GPU.
"""
import ctypes as C

import numpy as np
import pytest

from vi_ekf_amd import capi

from .test_resmap_cpu import INSTANCES, build


def layout(n, rb, nw):
    fn = capi.lib().viekf_debug_packed_layout
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    fn.restype = C.c_int
    elem = np.full((9 * rb, 64 * nw), -1, dtype=np.int32)
    info = np.zeros(5, dtype=np.int32)
    assert fn(n, rb, nw, C.c_void_p(elem.ctypes.data), C.c_void_p(info.ctypes.data)) == 0
    return elem, dict(pbc=int(info[0]), pbb=int(info[1]), total=int(info[2]), nld=int(info[3]), fits=bool(info[4]))


@pytest.mark.parametrize("rb,nw,n_min,n_max", INSTANCES)
def test_offsets_distinct_inside_the_filters_p_and_aligned(rb, nw, n_min, n_max):
    tw = 64 * nw
    for n in range(n_min, n_max + 1):
        rc, m = build(n, rb, nw)
        assert rc > 0
        elem, L = layout(n, rb, nw)
        owned = np.repeat((m >> 16) != 0, 9, axis=0)          # [9 rb][tw]: register q = 9 slot + element of thread t
        offs = np.concatenate([elem[owned], np.arange(L["pbc"], L["pbc"] + 48 * n), np.arange(L["pbb"], L["pbb"] + 256)])
        assert len(np.unique(offs)) == len(offs)              # owned registers, Pbc and Pbb pairwise distinct
        # (the unowned registers are stored too: they must not land on anything either)
        assert len(np.unique(elem)) == elem.size and elem.max() < L["pbc"] <= L["pbb"] and L["pbb"] + 256 == L["total"]
        assert offs.min() >= 0
        assert (elem.max() < L["nld"] and L["total"] <= L["nld"]) == L["fits"]   # inside n * ld exactly where the host says "fits"
        assert L["fits"] == (9 * rb * tw + 48 * n + 256 <= L["nld"])              # the size the design states
        # the 16-byte pairs: registers (q, q + 1), q even, of one thread are adjacent and start on an even offset; so do Pbc / Pbb
        npair = (9 * rb) // 2
        even = elem[0:2 * npair:2]
        assert (even % 2 == 0).all() and (elem[1:2 * npair:2] == even + 1).all()
        assert L["pbc"] % 2 == 0 and L["pbb"] % 2 == 0 and L["nld"] % 2 == 0
        # lanes of a pair are 16 bytes apart: a wave instruction covers 1 KB contiguous
        assert (np.diff(even, axis=1) == 2).all()


def test_headline_image_is_about_half_the_matrix():
    _, L = layout(50, 7, 3)
    assert L["total"] == 14752 and L["nld"] == 27556 and L["fits"]


def test_small_filter_on_a_wide_instance_does_not_fit():
    _, L = layout(1, 2, 1)
    assert L["total"] == 1456 and L["nld"] == 19 * 20 and not L["fits"]
