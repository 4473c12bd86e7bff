"""LDS bank-conflict cycles of the worker waves' operand reads, computed from the block ownership map on the CPU (no GPU).

Every block (I, J) of a worker thread reads, with ds_read_b128 (16 bytes per lane), the rows 16 + 3 I + r of K, the rows
16 + 3 J + s of W (update sweep: [n][2] doubles, 16 bytes per row) and the Z records of rows 3 I + r and 3 J + s (propagate
contraction: ZS = 26 doubles per row, 16 bytes at 2 k).  The hardware serves the instruction in four groups of 16 lanes,
{0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; a byte address a sits on bank (a / 4) mod 64; lanes with the same
address share one access; every further distinct address on a busy bank costs one more cycle.  A lane without a block reads
block (0, 0).  Prints the extra cycles per workgroup, summed over waves, slots in use and rows: for one update sweep (K and W
rows) and for one trip k of the contraction (Z records of I and of J).

  PYTHONPATH=. python tools/resmap_conflicts.py N RB NW     (VIEKF_LIB=... picks another build of the library, e.g. the parent's)
"""
import ctypes as C
import sys

import numpy as np

from vi_ekf_amd import capi

GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS = GROUPS + [[l + 32 for l in g] for g in GROUPS]
ZS = 26


def extra_cycles(addr):
    """addr[64]: byte address of each lane's 16-byte read -> conflict cycles of the wave instruction"""
    extra = 0
    for g in GROUPS:
        per_bank = {}
        for a in {int(addr[l]) for l in g}:
            for d in range(4):
                bank = (a // 4 + d) % 64
                per_bank[bank] = per_bank.get(bank, 0) + 1
        extra += max(per_bank.values()) - 1
    return extra


def main():
    n, rb, nw = (int(x) for x in sys.argv[1:4])
    fn = capi.lib().viekf_debug_build_resmap
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    fn.restype = C.c_int
    m = np.zeros(rb * 64 * nw, dtype=np.int32)
    used = fn(n, rb, nw, C.c_void_p(m.ctypes.data))
    assert used > 0
    m = m.reshape(rb, 64 * nw)
    I, J = m & 0xFF, (m >> 8) & 0xFF
    tot = {"K rows": 0, "W rows": 0, "Z records of I": 0, "Z records of J": 0}
    for a in range(used):
        for w in range(nw):
            sl = slice(64 * w, 64 * w + 64)
            for r in range(3):
                tot["K rows"] += extra_cycles(16 * (16 + 3 * I[a, sl] + r))
                tot["W rows"] += extra_cycles(16 * (16 + 3 * J[a, sl] + r))
                tot["Z records of I"] += extra_cycles(8 * ZS * (3 * I[a, sl] + r))
                tot["Z records of J"] += extra_cycles(8 * ZS * (3 * J[a, sl] + r))
    reads = 3 * used * nw
    print("N=%d <%d,%d> slots in use %d: %d ds_read_b128 per operand kind (4 cycles each when conflict-free)" % (n, rb, nw, used, reads))
    for k, v in tot.items():
        print("  %-16s %4d extra cycles" % (k, v))


if __name__ == "__main__":
    main()
