"""The cases of the two GROUPED wide-P update kernels (k_update_feat_panelsvc, k_update_feat_blocked<512, 16 | 24 | 32>:
vi_ekf_amd/csrc/viekf_kernels_grouped.hpp), shared by the CPU check of their own conditions (tests/test_grouped_cases_cpu.py)
and the GPU test (tests/test_gpu_grouped.py).  Plain numpy and the oracle: no GPU code, no pytest.

Both kernels stage a WINDOW of BWIN = 2 BG entries of a filter's measurement list, decide each entry's admission there (code
-1 for slot < 0, 3 for a slot the filter does not track, 2 for a NaN pixel), scan the window into a GROUP -- up to BG admissible
entries with distinct slots; a repeated slot closes the group and opens the next; so does the window's end -- and start the next
window where the scan stopped.  groups() below is that window and scan in Python.  A measurement list exercises the places where
the two kernels' statements of it could drift apart:

  (a) a run of BG distinct admissible slots: a full group (at N = 20 a filter tracks 18 features, so a group of 24 or 32 cannot
      fill: there the run is all 18 and a repeat closes it; tests/hetero_cases.py fills groups of 32 at N = 85 and 24 at N = 100)
  (b) a repeated slot inside what would otherwise be one group
  (c) 2 BWIN consecutive inadmissible entries -- slot -1, a NaN pixel, slots at and past the filter's feature count in turn --
      so that a whole window forms no group
  (d) admissible entries every fourth entry only: a group ends at a window's end with fewer than BG
  (e) one entry 5000 px off, gated, in the middle of a group
  (f) the list ends inside a group.

B = 3 filters with their own slot permutation and pixel noise; every filter tracks NFEAT(N) = N - 2 of its N slots.  One
propagate, then update_feat alone.  The reference is the oracle applying the entries one by one."""
import numpy as np

from oracle import oracle as orc
from tests import meas_cases as mc
from vi_ekf_amd import scene

B = 3
_CASES = {}

# (id, N, tunings, kernel name in describe(), BG, padded columns): set_kernel(1) on every route (at N = 20 the batch would
# otherwise run the fused step); padded = the column stride of P is a multiple of 16 (N > 77, cov_ld of viekf_host.hpp)
ROUTES = [
    ("N20-panelsvc", 20, (), "k_update_feat_panelsvc<512,16>", 16, False),
    ("N20-blocked16", 20, (("TUNE_PANEL_SERVICE", 0), ("TUNE_BLOCK_GROUP", 16)), "k_update_feat_blocked<512,16>", 16, False),
    ("N20-blocked24", 20, (("TUNE_PANEL_SERVICE", 0), ("TUNE_BLOCK_GROUP", 24)), "k_update_feat_blocked<512,24>", 24, False),
    ("N20-blocked32", 20, (("TUNE_PANEL_SERVICE", 0), ("TUNE_BLOCK_GROUP", 32)), "k_update_feat_blocked<512,32>", 32, False),
    ("N78-panelsvc", 78, (), "k_update_feat_panelsvc<512,16>", 16, True),
    ("N78-blocked", 78, (("TUNE_PANEL_SERVICE", 0),), "k_update_feat_blocked<512,16>", 16, True),
]


def nfeat(N):
    return N - 2


def cov_ld(N):
    """the column stride of P (viekf_host.hpp)"""
    n = 16 + 3 * N
    return (n + 15) & ~15 if N > 77 else (n + 1) & ~1


def groups(adm, BG, BWIN=None):
    """window and scan of the grouped kernels.  adm: per entry the slot where the entry is admissible, else -1.
    -> [(first entry of the window, entry the scan stopped at, measurements in the group, why it closed)], why being
    "cap", "repeat", "window" (the window's end) or "end" (the list's end)"""
    BWIN, M, m, out = BWIN or 2 * BG, len(adm), 0, []
    while m < M:
        mend, seen, mm, why = min(M, m + BWIN), set(), m, None
        while mm < mend and len(seen) < BG:
            if adm[mm] >= 0:
                if adm[mm] in seen:
                    why = "repeat"
                    break
                seen.add(adm[mm])
            mm += 1
        why = why or ("cap" if len(seen) == BG else ("end" if mend == M else "window"))
        out.append((m, mm, len(seen), why))
        m = mm
    return out


def admissible(slot, z, ln):
    """per entry: the slot where the kernels admit the entry, else -1"""
    ok = (slot >= 0) & (slot < ln) & ~np.isnan(z).any(axis=-1)
    return np.where(ok, slot, -1)


def _list(r, N, BG):
    """one filter's list -> slot [M], what [M] (0 plain, 1 the 5000 px entry, 2 a NaN pixel)"""
    L, BWIN = nfeat(N), 2 * BG
    p = r.permutation(L)
    slot, what = [], []

    def add(s, w=0):
        slot.append(int(s))
        what.append(w)

    for s in p[:min(BG, L)]:                       # (a)
        add(s)
    q = r.permutation(L)
    for s in list(q[:5]) + [q[2]]:                 # (b): q[2] a second time closes the group q[0..4] (or the run of (a), at BG > L)
        add(s)
    add(q[5]); add(q[6], 1); add(q[7]); add(q[8])  # (e): the group q[2], q[5], [q[6] gated], q[7], q[8], ...
    for k in range(2 * BWIN):                      # (c); the group of (e) ends at its window's end inside this run
        kind = k % 4
        if kind == 0:
            add(-1)
        elif kind == 1:
            add(p[k % L], 2)
        elif kind == 2:
            add(L + (k // 4) % (N - L))            # a slot of the batch that this filter does not track
        else:
            add(N + 2)
    t = r.permutation(L)
    for k in range(BWIN + BWIN // 2):              # (d): one admissible entry in four
        if k % 4 == 0:
            add(t[(k // 4) % L])
        else:
            add(-1 if k % 4 != 2 else N + 1)
    add(N - 1)                                     # (f): not admissible, then three distinct slots and the end
    for s in r.permutation(L)[:3]:
        add(s)
    return np.array(slot, dtype=np.int32), np.array(what)


def case(N, BG):
    """-> dict: N, BG, nfeat, params, pix, u [B, 6], dt [B], z [B, M, 2], slot [B, M], R, what [B, M], codes [B, M] (the
    oracle's), x_ref, P_ref (after the propagate and the list)"""
    key = (N, BG)
    if key not in _CASES:
        sc = scene.make_scene(B, N, 1, seed=8100 + 10 * N + BG)
        r = np.random.default_rng(8200 + 10 * N + BG)
        L = nfeat(N)
        lists = [_list(r, N, BG) for _ in range(B)]
        slot, what = np.stack([l[0] for l in lists]), np.stack([l[1] for l in lists])
        M = slot.shape[1]
        z = np.stack([sc["pix"][b, np.clip(slot[b], 0, N - 1)] for b in range(B)]) + r.normal(0.0, 0.5, (B, M, 2))
        z[what == 1, 0] += 5000.0
        z[what == 2, 1] = np.nan
        prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
        R = np.asarray(sc["R"], dtype=np.float64).reshape(2, 2)
        codes = np.zeros((B, M), dtype=np.int32)
        fs = []
        for b in range(B):
            f = orc.OracleFilter(N).init(**prm)
            for i in range(L):
                assert f.init_feature(sc["pix"][b, i], i)
            f.propagate(sc["u"][0][b], float(sc["dt"][b]))
            for m in range(M):
                s = int(slot[b, m])
                if not 0 <= s < f.len_features:
                    codes[b, m] = -1 if s < 0 else orc.MEAS_INVALID
                elif np.isnan(z[b, m]).any():
                    codes[b, m] = orc.MEAS_NAN
                else:
                    codes[b, m] = f.update(orc.FEAT, z[b, m], R, True, f.feature_ids[s])
            fs.append(f)
        c = dict(N=N, BG=BG, nfeat=L, params=sc["params"], pix=sc["pix"], u=np.ascontiguousarray(sc["u"][0]), dt=sc["dt"],
                 z=np.ascontiguousarray(z), slot=np.ascontiguousarray(slot), R=R, what=what, codes=codes,
                 x_ref=np.stack([f.x.copy() for f in fs]), P_ref=np.stack([f.P.copy() for f in fs]))
        for a in c.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]
