"""The case of the fused and streaming steps on inputs that DIFFER PER FILTER, shared by the CPU check of its own conditions
(tests/test_hetero_cases_cpu.py) and the GPU test (tests/test_gpu_hetero.py).  Plain numpy and the oracle: no GPU code, no
pytest.

vi_ekf_amd/scene.py::make_scene gives every filter of a batch the same dt, one shared diagonal R, the same slot row and the
same feature count -- exactly where a kernel indexes per filter or per measurement.  case(N, r_mode, M) is ONE script of four
calls on the ragged batch of tests/meas_cases.py (B = 5, len = [N, N - 3, 1, 0, N - 1] clipped at 0):

  1. step(u[0], dt, z0, slot0, R0)      2. update_feat(z1, slot1, R1)      3. step_n(u[1:4], dt3, z2, slot2, R2)
  4. propagate(u[4], dt)

with dt[b] = DT (0.5 + 0.25 b), dt3[k, b] = dt[b] (1 + 0.1 k), the scene's u (it differs per filter already), and for each
measured call its own list and its own R = 2 A A^T + 8 I, A ~ N(0, 1): SPD, not diagonal, unequal diagonal entries, of shape
(2, 2), (B, 2, 2) or (B, M, 2, 2) for r_mode 0, 1, 2.  A list (M = None) has M = N + 3 entries per filter, permuted per filter:
a permutation of the N slots, one -1, one slot N + 2 and one repeated slot; above N = 77 it has M = 43 (40 distinct slots and
the three extras) and from N = 150 M = 20: the dense oracle at n = 496 is the cost.  With M given the slots are drawn per
filter from -1 .. N - 1 (the lists longer than one fused launch holds).  z is the slot's scene pixel plus N(0, 0.5) noise; entry 1 of every filter is
5000 px off (gated where it reaches the gate -- it is put on a slot below N, so in filter 0 it always does) and one entry of
filter 1 has a NaN pixel.

The start state (x0, P0, len) is the oracle's: the body at X0_AWAY (no component at zero: with the scene's own hover at the
origin, identity attitude and zero biases, many products of the dynamics and of the Jacobians vanish, and the small states are
residues of cancelling increments -- see cancelled()); filter b gets len[b] features through init_feature from the scene's pixels.
The reference is OracleFilter.propagate and OracleFilter.update(FEAT, z, R_bm, True, feature_ids[slot]) per filter, one by
one; the codes -1 (slot < 0), 3 (slot not tracked) and 2 (NaN pixel) are the C ABI's own answers, decided before the filter
is looked at, in the kernels' order (tests/test_gpu_rotating_reads.py::_oracle_step, tests/meas_cases.py::apply_oracle).

case(...) -> dict: N, r_mode, M, params, x0, P0, len, u [5, B, 6], dt [B], dt3 [3, B], calls (three dicts z [B, M, 2],
slot [B, M], R), codes (three [B, M]), mahal (three [B, M]: the oracle's Mahalanobis distance of every entry that reached the
gate, NaN elsewhere), x_ref, P_ref (after call 4), travel [B, nx] (the sum of |x_after - x_before| over every propagate and
accepted update: an element far smaller than its travel is what its increments cancel to).  run(c, dt=, R=, slot=) and
run_many rerun the oracle with one input replaced (the sensitivity check of the CPU test)."""
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import oracle as orc
from tests import meas_cases as mc
from vi_ekf_amd import scene

B = mc.B
LAST_RESIDENT_N = 77
WIDE_M, WIDEST_M = 43, 20
GATED_ENTRY, NAN_FILTER, ONE_FEATURE_FILTER = 1, 1, 2
R_SPREAD = 0.5
# The start state of the body, away from zero in every component (the scene's own x0 is a hover at the origin with identity
# attitude and zero biases: there the attitude's vector part, the biases and the horizontal position are what hundreds of
# increments of either sign happen to leave -- see cancelled()).  Position, velocity, unit attitude, b_a, b_g, mu.
_Q0 = np.array([1.0, 0.05, -0.04, 0.03])
X0_AWAY = np.concatenate([[0.3, -0.2, -2.0], [0.1, -0.05, 0.02], _Q0 / np.linalg.norm(_Q0), [0.02, -0.03, 0.01], [0.08, -0.06, 0.05], [0.1]])
NOISE_FLOOR, CANCEL_BODY, CANCEL_FEATURE = 1e-9, 1e3, 1e6      # assert_close's floor; see cancelled()
_CASES = {}


def fill(N):
    """the ragged feature counts, clipped at 0"""
    return [max(v, 0) for v in mc.fill(N)]


def list_len(N):
    """N + 3 on chip; 43 above (as the wide tests cap M); 20 from N = 150 (n >= 466), where one dense update of the oracle takes
    50 ms: still more than one group of 16 in every kernel that groups"""
    return N + 3 if N <= LAST_RESIDENT_N else (WIDE_M if N < 150 else WIDEST_M)


def r_of(R, b, m):
    """the R of measurement m of filter b, whatever the mode"""
    return R if R.ndim == 2 else (R[b] if R.ndim == 3 else R[b, m])


def _spd(r, lead):
    """R = 2 A A^T + 8 I, A ~ N(0, 1); an A whose R comes out nearly diagonal or with nearly equal diagonal entries (less than
    R_SPREAD apart) is drawn again, so that every single R tells a transposition, a swapped diagonal and a dropped
    off-diagonal apart"""
    A = r.normal(0.0, 1.0, lead + (2, 2))
    while True:
        R = 2.0 * (A @ np.swapaxes(A, -1, -2)) + 8.0 * np.eye(2)
        weak = (np.abs(R[..., 0, 1]) < R_SPREAD) | (np.abs(R[..., 0, 0] - R[..., 1, 1]) < R_SPREAD)
        if not weak.any():
            return R
        A[weak] = r.normal(0.0, 1.0, (int(weak.sum()), 2, 2))


def _list(r, N, M, drawn):
    """one filter's slot list"""
    if drawn:
        lst = r.integers(-1, N, size=M)
    else:
        slots = r.permutation(N)[:M - 3]
        if 0 not in slots:      # (a list shorter than N: slot 0, the only one the one-feature filter tracks, is in it)
            slots[r.integers(len(slots))] = 0
        lst = r.permutation(np.concatenate([slots, [-1, N + 2, slots[r.integers(len(slots))]]]))
    if not 0 <= lst[GATED_ENTRY] < N:      # the entry that is 5000 px off sits on a slot of the filter's table
        j = next(j for j in range(M) if j != GATED_ENTRY and 0 <= lst[j] < N)
        lst[[GATED_ENTRY, j]] = lst[[j, GATED_ENTRY]]
    return lst.astype(np.int32)


def _lists(r, N, M, drawn):
    """the B lists of one call.  The one-feature filter measures slot 0 only: its list has it at an entry that is not the
    gated one and where filter 0's list has another slot, or reading filter 0's row would change nothing for it"""
    slot = [_list(r, N, M, drawn) for _ in range(B)]
    while True:
        mine, theirs = np.flatnonzero(slot[ONE_FEATURE_FILTER] == 0), np.flatnonzero(slot[0] == 0)
        if len(set(mine) - {GATED_ENTRY}) and not set(mine) & set(theirs):
            return np.stack(slot)
        slot[ONE_FEATURE_FILTER] = _list(r, N, M, drawn)


def _call(r, sc, N, M, r_mode, ln, drawn):
    slot = _lists(r, N, M, drawn)
    z = np.stack([sc["pix"][b, np.clip(slot[b], 0, N - 1)] for b in range(B)]) + r.normal(0.0, 0.5, (B, M, 2))
    z[:, GATED_ENTRY, 0] += 5000.0
    ok = [m for m in range(M) if m != GATED_ENTRY and 0 <= slot[NAN_FILTER, m] < ln[NAN_FILTER]]
    if ok:
        z[NAN_FILTER, ok[0], 1] = np.nan
    R = _spd(r, {0: (), 1: (B,), 2: (B, M)}[r_mode])
    return dict(z=np.ascontiguousarray(z), slot=np.ascontiguousarray(slot), R=R)


def mahalanobis(f, z, R, gid):
    """r^T (H P H^T + R)^-1 r of the FEAT measurement z of feature gid on the oracle filter f, before the update"""
    h, H = f.h(orc.FEAT, None, gid)
    res = z - h[:2]
    S = H[:2] @ f.P @ H[:2].T + R
    return float(res @ np.linalg.solve(S, res))


def _updates(f, b, call, R, slot, codes, mah, moved=None):
    for m in range(slot.shape[1]):
        sl, z = int(slot[b, m]), call["z"][b, m]
        if not 0 <= sl < f.len_features:
            codes[b, m] = -1 if sl < 0 else orc.MEAS_INVALID
        elif np.isnan(z).any():
            codes[b, m] = orc.MEAS_NAN
        else:
            Rbm, gid = r_of(R, b, m), f.feature_ids[sl]
            mah[b, m] = mahalanobis(f, z, Rbm, gid)
            codes[b, m] = f.update(orc.FEAT, z, Rbm, True, gid)
            if moved:
                moved()


def dt3_of(dt):
    return np.ascontiguousarray(dt[None, :] * (1.0 + 0.1 * np.arange(3))[:, None])


def _run_filter(c, b, dt, Rs, sls, upto):
    """filter b through the script -> its rows of the three codes and distances, x, P"""
    M, u, dt3 = c["M"], c["u"], dt3_of(dt)
    codes, mah = np.zeros((3, 1, M), dtype=np.int32), np.full((3, 1, M), np.nan)
    f = c["start"][b].clone()
    travel, last = np.zeros(f.nx), [f.x.copy()]

    def moved():
        travel[:] += np.abs(f.x - last[0])
        last[0] = f.x.copy()

    f.propagate(u[0, b], float(dt[b]))
    moved()
    for k in range(min(upto, 3)):
        if k == 2:
            for kp in range(3):
                f.propagate(u[1 + kp, b], float(dt3[kp, b]))
                moved()
        call = dict(z=c["calls"][k]["z"][b][None])
        _updates(f, 0, call, _row(Rs[k], b), sls[k][b][None], codes[k], mah[k], moved)
    if upto >= 4:
        f.propagate(u[4, b], float(dt[b]))
        moved()
    return codes[:, 0], mah[:, 0], f.x.copy(), f.P.copy(), travel


def _row(R, b):
    """filter b's part of R, shaped so that r_of(., 0, m) finds it"""
    return R if R.ndim == 2 else R[b][None]


def run_many(c, variants, upto=4):
    """the script on clones of the case's start filters, once per variant -- a dict with any of dt (another dt [B]), R, slot
    (functions of a call's R / slot giving the one to use instead) -> per variant: codes, mahal (three [B, M] each), x, P.
    upto: stop after that many calls.  The filters are independent and the oracle's calls leave the interpreter, so they run
    on a few host threads"""
    jobs = []
    for v in variants:
        dt = np.asarray(v.get("dt", c["dt"]), dtype=np.float64)
        Rs = [v["R"](cl["R"]) if "R" in v else cl["R"] for cl in c["calls"]]
        sls = [v["slot"](cl["slot"]) if "slot" in v else cl["slot"] for cl in c["calls"]]
        jobs += [(c, b, dt, Rs, sls, upto) for b in range(B)]
    with ThreadPoolExecutor(max_workers=max(1, min(8, os.cpu_count() or 1))) as pool:
        done = list(pool.map(lambda j: _run_filter(*j), jobs))
    out = []
    for i in range(len(variants)):
        rows = done[B * i:B * (i + 1)]
        out.append(([np.stack([r[0][k] for r in rows]) for k in range(3)], [np.stack([r[1][k] for r in rows]) for k in range(3)],
                    np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]), np.stack([r[4] for r in rows])))
    return out


def run(c, upto=4, **variant):
    return run_many(c, [variant], upto)[0][:4]



def cancelled(c):
    """The elements of the reference x that the element-wise bar cannot be asked of.  tests.test_gpu_parity.assert_close holds
    an array to 1e-9 of its largest element and every element above the noise floor (1e-9 of the largest) to 1e-6 of itself.
    x[i] is the sum of its increments -- travel[i] = sum |x_after - x_before| over every propagate and accepted update --
    and two fp64 implementations agree on an element no better than on its increments times travel / |x|:

      * a BODY element is moved by gains made of the small cross-covariances between the body and the measured feature.
        The kernels propagate P block by block, the oracle as a dense Phi P Phi^T; they agree to a few ulp of max |P|, which
        is 1e-10 .. 1e-9 of such a cross-covariance and so of the increment (measured on an MI355X: 3e-10 on the gyro
        bias, the same on the resident and the streaming kernels).  Where the increments cancel to less than a thousandth
        of their absolute sum (1e-6 / 1e-9), the bar asks more than agreement in norm gives;
      * a FEATURE element is moved by its own update, whose gain is made of the feature's own 3 x 3 block (exact to
        rounding); what differs is the residual z - zhat, a few ulp of a pixel coordinate of up to 640 against residuals
        of 0.1 .. 1 px: 1e-12 of the increment, which allows a cancellation of 1e6.  (The fourth component of a bearing
        quaternion IS such a residue by construction: init_feature makes it zero.)

    -> [(filter, index)] of the elements of the active parts beyond these; a case must have none
    (tests/test_hetero_cases_cpu.py), hence X0_AWAY"""
    out = []
    for b in range(B):
        na = 17 + 5 * int(c["len"][b])
        x = np.abs(c["x_ref"][b, :na])
        allowed = np.where(np.arange(na) < 17, CANCEL_BODY, CANCEL_FEATURE)
        out += [(b, int(i)) for i in np.flatnonzero((x > NOISE_FLOOR * x.max()) & (c["travel"][b, :na] > allowed * x))]
    return out


def case(N, r_mode, M=None):
    key = (N, r_mode, M)
    if key not in _CASES:
        drawn = M is not None
        Mc = M if drawn else list_len(N)
        sc = scene.make_scene(B, N, 5, 5100 + 7 * N + r_mode, params=dict(x0=X0_AWAY.tolist()))
        ln = np.array(fill(N), dtype=np.int32)
        prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
        fs = [orc.OracleFilter(N).init(**prm) for _ in range(B)]
        for b in range(B):
            for i in range(ln[b]):
                assert fs[b].init_feature(sc["pix"][b, i], i)
        assert list(mc.lens(fs)) == list(ln)
        dt = scene.DT * (0.5 + 0.25 * np.arange(B))
        c = dict(N=N, r_mode=r_mode, M=Mc, params=sc["params"], start=fs, len=ln, u=sc["u"], dt=dt, dt3=dt3_of(dt),
                 x0=np.stack([f.x.copy() for f in fs]), P0=np.stack([f.P.copy() for f in fs]))
        r = np.random.default_rng(6100 + 13 * N + r_mode + (1000 * Mc if drawn else 0))
        c["calls"] = [_call(r, sc, N, Mc, r_mode, ln, drawn) for _ in range(3)]
        c["codes"], c["mahal"], c["x_ref"], c["P_ref"], c["travel"] = run_many(c, [{}])[0]
        for a in [c["x0"], c["P0"], c["x_ref"], c["P_ref"], dt, c["dt3"]] + c["codes"] + [v for cl in c["calls"] for v in cl.values()]:
            a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


# ---- the rows of the resident dispatch table, read from the header that states them -----------------------------------
_ROWS_HPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "vi_ekf_amd", "csrc", "viekf_instance_rows.hpp")


def res_rows():
    """(RB, NW, NS, nmin, nmax, max_lds_kb) of every row of kResInst (viekf_instance_rows.hpp), in its order: the index is what
    VIEKF_TUNE_RES_INSTANCE takes.  tests/test_hetero_cases_cpu.py holds this reading against the library's own report."""
    rows = []
    with open(_ROWS_HPP) as fh:
        for line in fh:
            if re.match(r"#define VIEKF_RES_LIST_\d+\(X\)", line):
                rows += [tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+), (\d+), (\d+), (\d+)\)", line)]
    return rows


def auto_row(N, batch, cus):
    """the row setup_resident (viekf_dispatch.hpp) picks for a batch of `batch` filters of N features on a device of `cus` CUs:
    the first row that holds N -- its feature range and its N (N + 1) / 2 blocks on RB * 64 NW places --, a row of two (four)
    workgroups per CU only for a batch beyond one (two) per CU.  (The LDS bound is what nmax states.)"""
    for i, (rb, nw, ns, nmin, nmax, kb) in enumerate(res_rows()):
        if not nmin <= N <= nmax or N * (N + 1) // 2 > rb * nw * 64 or N > nw * 64:
            continue
        if kb <= 80 and batch <= cus:
            continue
        if kb <= 40 and batch <= 2 * cus:
            continue
        return i
    return -1


def row_name(i):
    rb, nw = res_rows()[i][:2]
    return "k_step_resident<%d,%d>" % (rb, nw)


# ---- the routes of the GPU test: (id, N, kernel of tests.test_gpu_parity.make_gpu, tunings, what describe() names) ----------
def resident_routes():
    out = []
    for i, (rb, nw, ns, nmin, nmax, kb) in enumerate(res_rows()):
        sizes = [nmax] + ([nmin] if nmin >= 26 else []) + ([5] if i in (0, 7) else [])
        for N in sizes:
            out.append(("res%d-%d.%d-N%d" % (i, rb, nw, N), N, 0, (("TUNE_RES_INSTANCE", i),), (row_name(i),)))
    return out


STREAM_ROUTES = [
    ("stream-N5", 5, 1, (), ("k_propagate_wide", "k_update_feat_panelsvc")),
    ("stream-N5-plain", 5, 1, (("TUNE_STREAM_MFMA", 0),), ("k_propagate_stream + k_update_feat_stream",)),
    ("stream-N17", 17, 1, (), ("k_propagate_wide", "k_update_feat_panelsvc")),
    ("stream-N17-blocked", 17, 1, (("TUNE_PANEL_SERVICE", 0),), ("k_propagate_wide", "k_update_feat_blocked<512,16>")),
    ("stream-N51-r02", 51, 1, (("TUNE_STREAM_MFMA", 2),), ("k_propagate_stream + k_update_feat_panelsvc",)),
    ("stream-N85-blocked", 85, 1, (("TUNE_PANEL_SERVICE", 0),), ("k_propagate_wide", "k_update_feat_blocked<512,32>")),
    ("stream-N100-blocked", 100, 1, (("TUNE_PANEL_SERVICE", 0),), ("k_propagate_wide", "k_update_feat_blocked<512,24>")),
    ("stream-N150", 150, 1, (), ("k_propagate_wide", "k_update_feat_panelsvc")),
    ("stream-N160", 160, 1, (), ("k_propagate_wide", "k_update_feat_blocked<512,16>")),
]
TILE_ROUTES = [("tiles-N%d-%s" % (N, "pair" if k == 5 else "single"), N, k, (), ("k_step_tiles_pair" if k == 5 else "k_step_tiles<",))
               for N in (46, 50) for k in (3, 5)]
# (id, N, M, kernel, tunings, names): more measurements than one fused launch holds
CHUNKED_ROUTES = [("auto-N12-M70", 12, 70, 0, (), ("k_step_resident",)),
                  ("res6-7.3-N50-M130", 50, 130, 0, (("TUNE_RES_INSTANCE", 6),), ("k_step_resident<7,3>",)),
                  ("tiles-N50-pair-M130", 50, 130, 5, (), ("k_step_tiles_pair",))]


def all_cases():
    """(N, r_mode, M) of every case the GPU test runs, for the CPU test"""
    sizes = sorted({r[1] for r in resident_routes() + STREAM_ROUTES + TILE_ROUTES})
    return [(N, rm, None) for N in sizes for rm in (0, 1, 2)] + [(r[1], rm, r[2]) for r in CHUNKED_ROUTES for rm in (1, 2)]
