"""The cases of the fused body-sensor update (BatchVIEKF.update_body, include/viekf_body.h), shared by the CPU check of their
own conditions and of the identity the kernel rests on (tests/test_body_cases_cpu.py) and by the GPU test
(tests/test_gpu_body.py).  Plain numpy and the oracle: no GPU code, no pytest.

A case is ONE call: M entries (mtype, z [B, zdim], R) on the ragged batch of tests/meas_cases.py -- B = 5 filters with
len = [N, N - 3, 1, 0, N - 1] clipped at 0 -- from a start state (x0, P0, len) the GPU test writes with set_state.  The start
state is the oracle's: all N features, two warm steps of min(N, 8) FEAT updates (P dense), the ragged keep_features, then the
case's own preparation (rho written into x, a NaN into P).  The entries are written while they run on clones of those
filters: every z is the oracle's prediction at the state the entry will meet, plus seeded noise.  The reference for
everything -- x, P, result codes -- is OracleFilter.update applied entry by entry (meas_cases.apply_oracle).

case(name, N) -> dict: N, params, x0, P0, len, entries, active ([M, B] or None), codes [M, B], x_ref, P_ref, mahal [M, B]
(the oracle's Mahalanobis distance of every entry that reached the gate, NaN elsewhere), untouched (filters the call must
leave bit for bit) and what the case is there to reach (`reaches`, checked on the CPU)."""
import numpy as np

from oracle import oracle as orc
from tests import meas_cases as mc
from vi_ekf_amd import scene

B = mc.B
SIZES = (1, 5, 16, 17, 50)          # n = 19, 31 (odd, one pad row), 64 / 67 (the wave boundary of the column walk), 166 (n = ld)
BODY = (orc.ACC, orc.ALT, orc.ATT, orc.POS, orc.VEL)
NOISE = {orc.ACC: 0.1, orc.ALT: 0.05, orc.ATT: 0.02, orc.POS: 0.05, orc.VEL: 0.05}
POISONED = mc.POISONED
NAN_BIT, NEG_DEPTH_BIT = 1, 4
_WARM, _CASES = {}, {}


def fill(N):
    """the ragged feature counts, clipped at 0 (N = 1: [1, 0, 1, 0, 0])"""
    return [max(v, 0) for v in mc.fill(N)]


def rdim(mtype, drag):
    return {orc.ACC: 2 if drag else 3, orc.ALT: 1, orc.ATT: 3, orc.POS: 3, orc.VEL: 3}[mtype]


def warm(N, partial, drag):
    """the scene and the warm, ragged oracle filters (shared: run clones)"""
    key = (N, partial, drag)
    if key not in _WARM:
        sc = scene.make_scene(B, N, 2, 4100 + 7 * N + 2 * partial + drag, params=dict(use_partial_update=partial, use_drag_term=drag))
        fs = mc.make_filters(sc, N)
        for s in range(2):
            z, slot = mc.warm_inputs(sc, N, s)
            for b in range(B):
                fs[b].run_steps(sc["u"][s, b][None], sc["dt"][b], z[b][None], slot[b], sc["R"])
        mc.apply_oracle(fs, "keep_features", dict(keep=mc.first_keep(N)))
        assert list(mc.lens(fs)) == fill(N)
        _WARM[key] = (sc, fs)
    sc, fs = _WARM[key]
    return sc, [f.clone() for f in fs]


def predict(f, mtype, drag, r):
    """the oracle's prediction of a body measurement at f's state, plus noise"""
    x, s = f.x, NOISE[mtype]
    if mtype == orc.ACC:
        if drag:
            return x[10:12] - x[16] * x[3:5] + r.normal(0, s, 2)
        return f.h(orc.ACC)[0][:3] + r.normal(0, s, 3)
    if mtype == orc.ALT:
        return -x[2:3] + r.normal(0, s, 1)
    if mtype == orc.ATT:
        return orc.q_boxplus(x[6:10], r.normal(0, s, 3))
    return x[{orc.POS: 0, orc.VEL: 3}[mtype]:][:3] + r.normal(0, s, 3)


def residual(mtype, z, h):
    return orc.q_boxminus(z, h[:4]) if mtype == orc.ATT else z - h[:len(z)]


def mahalanobis(f, mtype, z, R):
    """r^T (H P H^T + R)^-1 r of the oracle filter f, before the update"""
    h, H = f.h(mtype)
    k = R.shape[0]
    res = residual(mtype, z, h)[:k]
    S = H[:k] @ f.P @ H[:k].T + R
    return float(res @ np.linalg.solve(S, res))


def _build(N, partial, drag, types, per_filter_R, seed, active=None, prepare=None, tweak=None):
    sc, fs = warm(N, partial, drag)
    if prepare:
        prepare(fs)
    x0, P0, ln = np.stack([f.x.copy() for f in fs]), np.stack([f.P.copy() for f in fs]), mc.lens(fs)
    r = np.random.default_rng(seed)
    M = len(types)
    entries, codes, mah = [], np.zeros((M, B), dtype=np.int32), np.full((M, B), np.nan)
    act = None if active is None else np.asarray(active, dtype=np.uint8)
    for m, mtype in enumerate(types):
        z = np.stack([predict(fs[b], mtype, drag, r) for b in range(B)])
        if tweak:
            tweak(m, z)
        d = rdim(mtype, drag)
        R = mc._spd(r, d) if per_filter_R else mc._spd(r, d)[0]
        row = None if act is None else act[m]
        for b in range(B):
            if (row is None or row[b] == 1) and not np.isnan(z[b]).any() and not np.isnan(fs[b].P).any():
                mah[m, b] = mahalanobis(fs[b], mtype, z[b], R[b] if per_filter_R else R)
        codes[m] = mc.apply_oracle(fs, "update", dict(mtype=mtype, z=z, R=R, slot=None, active=row))
        entries.append((mtype, z, R))
    untouched = [b for b in range(B) if all(codes[m, b] in (-1, orc.MEAS_GATED, orc.MEAS_NAN) for m in range(M))]
    return dict(N=N, partial=partial, drag=drag, params=sc["params"], x0=x0, P0=P0, len=ln, entries=entries, active=act,
                codes=codes, x_ref=np.stack([f.x.copy() for f in fs]), P_ref=np.stack([f.P.copy() for f in fs]), mahal=mah,
                untouched=untouched, lam=fs[0].lam.copy())


ALL5 = (orc.ACC, orc.ALT, orc.ATT, orc.POS, orc.VEL)
MIXED = (orc.ACC, orc.POS, orc.ATT, orc.POS, orc.VEL, orc.ALT)      # M = 6
MIXED_ACTIVE_ROW, MIXED_GATED, MIXED_NAN, MIXED_NAN_FILTER, MIXED_SKIPPED_FILTER = 1, 3, 4, 1, 2
FIX_TYPES = (orc.ACC, orc.ATT, orc.VEL, orc.ALT)
POISON_TYPES = (orc.ALT, orc.POS, orc.ATT)      # every one of them reads column 2 or 7 of P: row 7 / 2 of W is NaN


def _mixed_active():
    a = np.ones((len(MIXED), B), dtype=np.uint8)
    a[MIXED_ACTIVE_ROW] = [1, 0, 2, 1, 0]
    a[:, MIXED_SKIPPED_FILTER] = 2      # this filter sits the whole call out: bit for bit untouched
    return a


def _mixed_tweak(m, z):
    if m == MIXED_GATED:
        z += 50.0                       # POS 50 m off
    if m == MIXED_NAN:
        z[MIXED_NAN_FILTER, 2] = np.nan


def _fix_prepare(N):
    """rho < 0 and rho > 1e2 (the two branches tests/test_gpu_parity.py's fix_depth tests reach), written into x as
    set_state does: filter 0 meets them in an INACTIVE entry (fix_depth only), filters 1 and 4 after an accepted one"""
    def prepare(fs):
        fs[0].x[17 + 4] = -0.3
        if fs[0].len_features > 1:
            fs[0].x[17 + 5 + 4] = 250.0
        if fs[1].len_features > 1:
            fs[1].x[17 + 5 + 4] = 250.0
        if fs[4].len_features > 2:
            fs[4].x[17 + 5 * 2 + 4] = -0.3
    return prepare


def _fix_active():
    a = np.ones((len(FIX_TYPES), B), dtype=np.uint8)
    a[0, 0] = 0
    return a


def _poison(fs):
    fs[POISONED].P[2, 7] = fs[POISONED].P[7, 2] = np.nan


def case(name, N, variant=0):
    """name: all5 (variant 0: drag 1 / partial 1 and per-filter R, 1: drag 0 / partial 0 and a shared R, 2 / 3: the other two
    pairings), single (variant = the index into BODY), mixed, fix, poison, m2 (ACC and ATT: the IMU tick), m8 (eight entries)"""
    key = (name, N, variant)
    if key not in _CASES:
        seed = 9000 + 31 * N + variant
        if name == "all5":
            pd, perR = ((1, 1), (0, 0), (1, 1), (0, 0))[variant], (True, False, False, True)[variant]
            c = _build(N, pd[0], pd[1], ALL5, perR, seed)
        elif name == "single":
            c = _build(N, 1, 1, (BODY[variant],), True, seed + 100)
        elif name == "mixed":
            c = _build(N, 1, 1, MIXED, True, seed + 200, active=_mixed_active(), tweak=_mixed_tweak)
        elif name == "fix":
            c = _build(N, 1, 1, FIX_TYPES, True, seed + 300, active=_fix_active(), prepare=_fix_prepare(N))
        elif name == "poison":
            c = _build(N, 1, 1, POISON_TYPES, True, seed + 400, prepare=_poison)
        elif name == "m2":
            c = _build(N, 1, 1, (orc.ACC, orc.ATT), False, seed + 500)
        elif name == "m8":
            c = _build(N, 1, 1, ALL5 + (orc.ACC, orc.ATT, orc.ALT), True, seed + 600)
        else:
            raise ValueError(name)
        c["name"] = "%s N=%d v=%d" % (name, N, variant)
        _CASES[key] = c
    return _CASES[key]


def all_cases():
    """every case the GPU test runs at B = 5, for the CPU test"""
    out = []
    for N in SIZES:
        out += [("all5", N, 0), ("all5", N, 1), ("mixed", N, 0), ("m2", N, 0)]
    out += [("all5", 5, 2), ("all5", 5, 3), ("fix", 5, 0), ("fix", 17, 0), ("poison", 5, 0), ("poison", 50, 0), ("m8", 5, 0)]
    out += [("single", 5, v) for v in range(len(BODY))]
    return out


# ---- the run between two resident steps (GPU test 6) ------------------------------------------------------------------
def steps_case(N=50, nfeat=48):
    """init nfeat < N features, step, step, update_body([ACC, ATT]), step: the oracle's run and every input.  The rows and
    columns past 16 + 3 nfeat stay as the filter was created."""
    key = ("steps", N, nfeat)
    if key not in _CASES:
        sc = scene.make_scene(B, N, 3, 4700 + N)
        keep = [np.flatnonzero(sc["slot"][b] < nfeat) for b in range(B)]
        M = min(8, min(len(k) for k in keep))
        slot = np.stack([sc["slot"][b][keep[b][:M]] for b in range(B)]).astype(np.int32)
        z = np.stack([np.stack([sc["z"][s][b][keep[b][:M]] for b in range(B)]) for s in range(3)])
        prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
        fs = [orc.OracleFilter(N).init(**prm) for _ in range(B)]
        for b in range(B):
            for i in range(nfeat):
                fs[b].init_feature(sc["pix"][b, i], i)
        step_codes = []

        def step(s):
            step_codes.append(np.stack([fs[b].run_steps(sc["u"][s, b][None], sc["dt"][b], z[s, b][None], slot[b], sc["R"])[0]
                                        for b in range(B)]))
        step(0)
        step(1)
        r = np.random.default_rng(4800 + N)
        entries, codes, mah = [], np.zeros((2, B), dtype=np.int32), np.zeros((2, B))
        for m, mtype in enumerate((orc.ACC, orc.ATT)):
            zz = np.stack([predict(fs[b], mtype, 1, r) for b in range(B)])
            R = mc._spd(r, rdim(mtype, 1))[0]
            mah[m] = [mahalanobis(fs[b], mtype, zz[b], R) for b in range(B)]
            codes[m] = mc.apply_oracle(fs, "update", dict(mtype=mtype, z=zz, R=R, slot=None, active=None))
            entries.append((mtype, zz, R))
        step(2)
        _CASES[key] = dict(N=N, nfeat=nfeat, sc=sc, z=z, slot=slot, entries=entries, codes=codes, mahal=mah, step_codes=step_codes,
                           x_ref=np.stack([f.x.copy() for f in fs]), P_ref=np.stack([f.P.copy() for f in fs]))
    return _CASES[key]
