"""The cases of a frame's DEPTH updates in one launch (BatchVIEKF.update_depths, include/viekf_depth.h), shared by the CPU
check of their own conditions and of the identity the kernel rests on (tests/test_depth_cases_cpu.py) and by the GPU test
(tests/test_gpu_depth.py).  Plain numpy and the oracle: no GPU code, no pytest.

A case is ONE call: M entries (slot [B, M], z [B, M]) of one model (DEPTH or INV_DEPTH), R as a float (r_mode 0), [B] (1) or
[B, M] (2), active [B, M] or None, and the order (0 = entry 0 first, 1 = entry M - 1 first), on the ragged batch of
tests/meas_cases.py -- B = 5 filters with len = [N, N - 3, 1, 0, N - 1] clipped at 0 -- from the warm, dense-P start state of
tests/body_cases.py (x0, P0, len: the GPU test writes them with set_state, P as the mirrored lower triangle), plus the case's
own preparation (rho written into x, a NaN into P).  The entries are written while they run, in the call's order, on clones of
those filters: every z is the oracle's prediction at the state the entry will meet, plus noise drawn uniformly within
+- sqrt(R) / 2 -- so an honest entry's Mahalanobis distance r^2 / (H P H^T + R) stays below 0.25.  The reference for everything
-- x, P, result codes -- is OracleFilter.update applied entry by entry (meas_cases.apply_oracle).

case(name, N, variant) -> dict: N, params, partial, mtype, x0, P0, len, slot, z, R, r_mode, active, order, codes [B, M], x_ref,
P_ref, mahal [B, M] (the oracle's Mahalanobis distance of every entry that reached the gate, NaN elsewhere), untouched (filters
the call must leave bit for bit), lam."""
import numpy as np

from oracle import oracle as orc
from tests import body_cases as bc
from tests import meas_cases as mc

B = mc.B
SIZES = bc.SIZES                    # N = 5: n = 31, odd, one pad row; 16 / 17: nact 64 / 67, a wave boundary; 50: n = ld = 166
POISONED = mc.POISONED
NAN_BIT, NEG_DEPTH_BIT = 1, 4
_CASES = {}

fill = bc.fill


def start_P(c):
    """the case's start covariance as the device gets it: the oracle's lower triangle, mirrored"""
    low = np.tril(c["P0"])
    return low + np.tril(low, -1).transpose(0, 2, 1)


def rho_of(f, slot):
    return f.x[17 + 5 * slot + 4]


def predict(f, mtype, slot):
    rho = rho_of(f, slot)
    return 1.0 / rho if mtype == orc.DEPTH else rho


def mahalanobis(f, mtype, slot, z, R):
    """r^2 / (H P H^T + R) of the oracle filter f, before the update"""
    rho = rho_of(f, slot)
    H = -1.0 / (rho * rho) if mtype == orc.DEPTH else 1.0
    c = 18 + 3 * slot
    res = z - predict(f, mtype, slot)
    return float(res * res / (H * f.P[c, c] * H + R))


def r_at(R, b, m):
    R = np.asarray(R, dtype=np.float64)
    return float(R if R.ndim == 0 else (R[b] if R.ndim == 1 else R[b, m]))


def make_R(r, r_mode, M):
    """variances of 2 .. 6 cm (DEPTH) -- the same numbers serve INV_DEPTH"""
    if r_mode == 0:
        return float(r.uniform(0.02, 0.06) ** 2)
    return r.uniform(0.02, 0.06, (B,) if r_mode == 1 else (B, M)) ** 2


def _build(N, partial, mtype, slot, r_mode, seed, order=0, active=None, prepare=None, tweak=None, R=None):
    sc, fs = bc.warm(N, partial, 1)
    if prepare:
        prepare(fs)
    x0, P0, ln = np.stack([f.x.copy() for f in fs]), np.stack([f.P.copy() for f in fs]), mc.lens(fs)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    M = slot.shape[1]
    r = np.random.default_rng(seed)
    R = make_R(r, r_mode, M) if R is None else R
    act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    z = np.full((B, M), 3.0)
    codes, mah = np.zeros((B, M), dtype=np.int32), np.full((B, M), np.nan)
    for e in range(M):
        m = M - 1 - e if order else e
        Rm = np.array([[[r_at(R, b, m)]] for b in range(B)])
        for b in range(B):
            s = int(slot[b, m])
            if 0 <= s < fs[b].len_features:
                z[b, m] = predict(fs[b], mtype, s) + r.uniform(-0.5, 0.5) * np.sqrt(Rm[b, 0, 0])
        if tweak:
            tweak(m, z, fs)
        for b in range(B):
            s = int(slot[b, m])
            if (act is None or act[b, m] == 1) and 0 <= s < fs[b].len_features and not np.isnan(z[b, m]):
                d = mahalanobis(fs[b], mtype, s, z[b, m], Rm[b, 0, 0])
                if not np.isnan(d):
                    mah[b, m] = d
        codes[:, m] = mc.apply_oracle(fs, "update", dict(mtype=mtype, z=z[:, m:m + 1], R=Rm, slot=slot[:, m],
                                                         active=None if act is None else act[:, m]))
    untouched = [b for b in range(B) if all(codes[b, m] in (-1, orc.MEAS_GATED, orc.MEAS_NAN, orc.MEAS_INVALID) for m in range(M))]
    return dict(N=N, partial=partial, mtype=mtype, params=sc["params"], x0=x0, P0=P0, len=ln, slot=slot, z=z, R=R, r_mode=r_mode,
                active=act, order=order, codes=codes, x_ref=np.stack([f.x.copy() for f in fs]),
                P_ref=np.stack([f.P.copy() for f in fs]), mahal=mah, untouched=untouched, lam=fs[0].lam.copy())


# ---- every slot once ----------------------------------------------------------------------------------------------------
ONCE_VARIANTS = ((1, 0, 0), (1, 1, 1), (1, 2, 0), (0, 0, 1), (0, 1, 0), (0, 2, 1))      # (partial, r_mode, order)
ONCE_SKIP_FILTER = 1                # this filter's row holds a -1


def once_slots(N, seed):
    """M = N: every filter gets its own permutation of the slots (the ragged ones meet slots >= len: INVALID); one entry of
    filter 1's row is -1 (SKIPPED)"""
    r = np.random.default_rng(seed)
    slot = np.stack([r.permutation(N) for _ in range(B)]).astype(np.int32)
    slot[ONCE_SKIP_FILTER, int(r.integers(N))] = -1
    return slot


# ---- M past a wave and past N ----------------------------------------------------------------------------------------------
REPEAT_N, REPEAT_M, REPEAT_SLOT, REPEAT_AT = 17, 70, 2, (3, 20, 50)


def repeat_slots(seed):
    r = np.random.default_rng(seed)
    slot = r.integers(0, REPEAT_N, (B, REPEAT_M)).astype(np.int32)
    for b in range(B):
        row = slot[b]
        row[row == REPEAT_SLOT] = REPEAT_SLOT + 1                  # ... and nowhere else
        row[list(REPEAT_AT)] = REPEAT_SLOT
    return slot


# ---- mixed script ----------------------------------------------------------------------------------------------------------
MIXED_M, MIXED_GATED, MIXED_NAN, MIXED_NAN_FILTER, MIXED_SKIPPED_FILTER, MIXED_ACTIVE_FILTER = 8, 3, 5, 1, 2, 0
MIXED_SIZES = (5, 17, 50)


def mixed_slots(N):
    return np.array([[(3 * m + b) % (N - 1) for m in range(MIXED_M)] for b in range(B)], dtype=np.int32)


def _mixed_active():
    a = np.ones((B, MIXED_M), dtype=np.uint8)
    a[MIXED_ACTIVE_FILTER, :4] = [1, 0, 2, 1]       # 0, 1 and 2 within one filter's row
    a[4, 1] = 0
    a[MIXED_SKIPPED_FILTER, :] = 2                  # this filter sits the whole call out: bit for bit untouched
    return a


def _mixed_tweak(m, z, fs):
    if m == MIXED_GATED:
        z[:, m] += 40.0                             # 40 m off
    if m == MIXED_NAN:
        z[MIXED_NAN_FILTER, m] = np.nan


def all_gated(c):
    """a second call on the state case c leaves: every entry 1000 m off -> (z, codes, mahal) of that call; nothing moves, so
    every distance is taken at the one state"""
    sc, fs = bc.warm(c["N"], c["partial"], 1)
    z = np.full(c["slot"].shape, 3.0)
    codes, mah = np.zeros(c["slot"].shape, dtype=np.int32), np.full(c["slot"].shape, np.nan)
    for b in range(B):
        fs[b].x[:] = c["x_ref"][b]
        fs[b].P[:] = c["P_ref"][b]
        for m in range(c["slot"].shape[1]):
            s = int(c["slot"][b, m])
            if not 0 <= s < fs[b].len_features:
                codes[b, m] = -1 if s < 0 else orc.MEAS_INVALID
                continue
            z[b, m] = predict(fs[b], c["mtype"], s) + 1000.0
            mah[b, m] = mahalanobis(fs[b], c["mtype"], s, z[b, m], r_at(c["R"], b, m))
            codes[b, m] = orc.MEAS_GATED
    return z, codes, mah


# ---- fix_depth inside the chain --------------------------------------------------------------------------------------------
FIX_M = 5
FIX_NEG_FILTERS = (0, 4)            # the filters that meet a rho < 0


def _fix_prepare(fs):
    """rho < 0 and rho > 1e2 written into x as set_state does: filter 0 meets them in an INACTIVE entry (fix_depth only),
    filters 1 and 4 after an accepted one"""
    fs[0].x[17 + 4] = -0.3
    fs[0].x[17 + 5 + 4] = 250.0
    fs[1].x[17 + 5 + 4] = 250.0
    fs[4].x[17 + 5 * 2 + 4] = -0.3


def fix_slots():
    """slots 3 and 0 first (not the prepared ones), then the prepared features themselves: entries on the edited diagonals"""
    return np.tile(np.array([3, 0, 1, 2, 0], dtype=np.int32), (B, 1))


def _fix_active():
    a = np.ones((B, FIX_M), dtype=np.uint8)
    a[0, 0] = 0
    return a


# INV_DEPTH that drives rho negative (as in tests/meas_cases.py), then an entry elsewhere, then the same slot again
NEG_SLOT, NEG_FILTERS = 1, (0, 1, 4)


def _neg_prepare(fs):
    for b in NEG_FILTERS:
        fs[b].x[17 + 5 * NEG_SLOT + 4] = 0.004      # 250 m away: a step of a fraction of sigma crosses zero


def neg_slots():
    return np.tile(np.array([NEG_SLOT, 0, NEG_SLOT], dtype=np.int32), (B, 1))


def _neg_tweak(m, z, fs):
    if m == 0:
        for b in NEG_FILTERS:
            c = 18 + 3 * NEG_SLOT
            z[b, m] = rho_of(fs[b], NEG_SLOT) - 1.5 * np.sqrt(fs[b].P[c, c] + NEG_R)


NEG_R = 1e-4


# ---- a NaN in P that one entry's column meets ------------------------------------------------------------------------------
POISON_SLOT, POISON_ROW = 1, 7


def _poison(fs):
    c = 18 + 3 * POISON_SLOT
    fs[POISONED].P[POISON_ROW, c] = fs[POISONED].P[c, POISON_ROW] = np.nan


def poison_slots(N):
    """slot 1 in the middle, other columns before and after it"""
    nl = N - 1                                       # (the poisoned filter has N - 1 features)
    return np.tile(np.array([0, 2 % nl, POISON_SLOT, 3 % nl, 0], dtype=np.int32), (B, 1))


def case(name, N, variant=0):
    """name: once (variant: index into ONCE_VARIANTS), once_inv (INV_DEPTH; variant = order), repeat, mixed, fix, neg, poison"""
    key = (name, N, variant)
    if key not in _CASES:
        seed = 12000 + 37 * N + variant
        if name == "once":
            partial, r_mode, order = ONCE_VARIANTS[variant]
            c = _build(N, partial, orc.DEPTH, once_slots(N, seed), r_mode, seed + 1, order)
        elif name == "once_inv":
            c = _build(N, 1, orc.INV_DEPTH, once_slots(N, seed + 50), 2, seed + 51, variant, R=None)
        elif name == "repeat":
            c = _build(REPEAT_N, 1, orc.DEPTH, repeat_slots(seed + 100), 2, seed + 101, variant)
        elif name == "mixed":
            c = _build(N, 1, orc.DEPTH, mixed_slots(N), 1, seed + 200, variant, active=_mixed_active(), tweak=_mixed_tweak)
        elif name == "fix":
            c = _build(N, 1, orc.DEPTH, fix_slots(), 0, seed + 300, 0, active=_fix_active(), prepare=_fix_prepare)
        elif name == "neg":
            c = _build(N, 1, orc.INV_DEPTH, neg_slots(), 0, seed + 350, 0, prepare=_neg_prepare, tweak=_neg_tweak, R=NEG_R)
        elif name == "poison":
            c = _build(N, 1, orc.DEPTH, poison_slots(N), 2, seed + 400, 0, prepare=_poison)
        else:
            raise ValueError(name)
        c["name"] = "%s N=%d v=%d" % (name, N, variant)
        _CASES[key] = c
    return _CASES[key]


def all_cases():
    """every case the GPU test runs at B = 5 at sizes known without a device, for the CPU test"""
    out = [("once", N, v) for N in SIZES for v in range(len(ONCE_VARIANTS))]
    out += [("once_inv", N, v) for N in (5, 17) for v in (0, 1)]
    out += [("repeat", REPEAT_N, 0), ("repeat", REPEAT_N, 1)]
    out += [("mixed", N, N % 2) for N in MIXED_SIZES]
    out += [("fix", 5, 0), ("fix", 17, 0), ("neg", 5, 0), ("neg", 17, 0), ("poison", 5, 0), ("poison", 50, 0)]
    return out


# ---- behind a fused step (P packed) -------------------------------------------------------------------------------------------
def steps_case(N=50, nfeat=48):
    """init nfeat < N features, step, step, then ONE update_depths of M = nfeat entries, every slot once, reverse order, R per
    entry: the oracle's run and every input.  The rows and columns past 16 + 3 nfeat stay as the filter was created."""
    key = ("steps", N, nfeat)
    if key not in _CASES:
        st = bc.steps_case(N, nfeat)                               # (the scene, the frames' z and slot, and the steps' codes)
        sc = st["sc"]
        prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
        fs = [orc.OracleFilter(N).init(**prm) for _ in range(B)]
        for b in range(B):
            for i in range(nfeat):
                fs[b].init_feature(sc["pix"][b, i], i)
        for s in range(2):
            for b in range(B):
                fs[b].run_steps(sc["u"][s, b][None], sc["dt"][b], st["z"][s, b][None], st["slot"][b], sc["R"])
        r = np.random.default_rng(5100 + N)
        slot = np.stack([r.permutation(nfeat) for _ in range(B)]).astype(np.int32)
        R = make_R(r, 2, nfeat)
        z = np.zeros((B, nfeat))
        codes, mah = np.zeros((B, nfeat), dtype=np.int32), np.zeros((B, nfeat))
        for m in range(nfeat - 1, -1, -1):
            for b in range(B):
                z[b, m] = predict(fs[b], orc.DEPTH, int(slot[b, m])) + r.uniform(-0.5, 0.5) * np.sqrt(R[b, m])
                mah[b, m] = mahalanobis(fs[b], orc.DEPTH, int(slot[b, m]), z[b, m], R[b, m])
            codes[:, m] = mc.apply_oracle(fs, "update", dict(mtype=orc.DEPTH, z=z[:, m:m + 1], R=R[:, m].reshape(B, 1, 1),
                                                             slot=slot[:, m], active=None))
        _CASES[key] = dict(N=N, nfeat=nfeat, sc=sc, step_z=st["z"], step_slot=st["slot"], step_codes=st["step_codes"][:2], slot=slot,
                           z=z, R=R, codes=codes, mahal=mah, x_ref=np.stack([f.x.copy() for f in fs]),
                           P_ref=np.stack([f.P.copy() for f in fs]))
    return _CASES[key]


# ---- the identity, in numpy -------------------------------------------------------------------------------------------------
def _fix_depth(x, D, ln, reset, p0rr):
    """fix_depth_rule on the state x with P(rho, rho) in D -> status bits"""
    flag = 0
    for f in range(ln):
        k = 17 + 5 * f + 4
        if np.isnan(x[k]):
            x[k] = reset
            flag |= NAN_BIT
        if x[k] < 0.0:
            D[f] += (reset - x[k]) ** 2
            x[k] = reset
            flag |= NEG_DEPTH_BIT
        elif x[k] > 1e2:
            D[f] = p0rr
            x[k] = reset
    return flag


def chain(c, b, left_looking):
    """filter b of case c by k_update_generic's rules, in numpy, operation by operation.
    left_looking False: the M sequential launches -- every accepted entry updates the whole active block,
        P_ij -= L_ij (K[max(i,j)] W[min(i,j)]).
    left_looking True: the kernel's way -- the column an entry needs is taken from the START P's lower triangle and brought up to
        date with the W and S^-1 of the entries applied before it, the rho diagonals ride along in D, and ONE trailing pass
        applies every applied entry to the lower triangle.
    -> x, P (the active block mirrored from its lower triangle), codes, status bits, applied entries, fix_depth edits, the
    distances that reached the gate"""
    prm = c["params"]
    f = orc.OracleFilter(c["N"]).init(**{k: prm[k] for k in mc.ORACLE_KEYS})      # for boxplus() at a given x
    ln = int(c["len"][b])
    for i in range(ln):
        f.init_feature(np.array([300.0, 200.0]), i)
    x, P0 = c["x0"][b].copy(), c["P0"][b]
    n, nact, nxa = P0.shape[0], 16 + 3 * ln, 17 + 5 * ln
    lam = c["lam"] if c["partial"] else np.ones(n)
    L = (lam[:, None] + lam[None, :] - lam[:, None] * lam[None, :])[:nact, :nact]
    low = np.tril(P0[:nact, :nact])
    sym = low + np.tril(low, -1).T                                   # what the lower triangle says, read either way
    rho = 18 + 3 * np.arange(ln)
    D = sym[rho, rho].copy()
    P = sym.copy()                                                   # (sequential route only)
    rows = np.arange(nact)
    HI, LO = np.maximum.outer(rows, rows), np.minimum.outer(rows, rows)
    reset, p0rr = 1.0 / (2.0 * prm["min_depth"]), prm["P0_feat"][2]
    M = c["slot"].shape[1]
    codes, Ws, Sis, flag, fixes, mah = np.zeros(M, dtype=np.int32), [], [], 0, 0, []
    for e in range(M):
        m = M - 1 - e if c["order"] else e
        act = 1 if c["active"] is None else int(c["active"][b, m])
        s, z = int(c["slot"][b, m]), c["z"][b, m]
        if act == 2 or s < 0:
            codes[m] = -1
            continue
        if s >= ln:
            codes[m] = orc.MEAS_INVALID
            continue
        if np.isnan(z):
            codes[m] = orc.MEAS_NAN
            continue
        before = x.copy()
        if act == 0:
            Dd = D if left_looking else P[rho, rho].copy()
            flag |= _fix_depth(x, Dd, ln, reset, p0rr)
            if not left_looking:
                P[rho, rho] = Dd
            fixes += int((x != before).sum())
            continue
        r = x[17 + 5 * s + 4]
        zhat, H = (1.0 / r, -1.0 / (r * r)) if c["mtype"] == orc.DEPTH else (r, 1.0)
        col = 18 + 3 * s
        if left_looking:
            v = sym[:, col].copy()
            hi, lo = np.maximum(rows, col), np.minimum(rows, col)
            for Wk, Sk in zip(Ws, Sis):
                v = v - L[:, col] * ((Wk[hi] * Sk) * Wk[lo])
            v[col] = D[s]                                            # (the diagonal element is current in D, edits included)
        else:
            v = P[:, col].copy()
        W = v * H
        Si = 1.0 / (H * W[col] + r_at(c["R"], b, m))
        res = z - zhat
        mah.append((res * Si) * res)
        if (res * Si) * res > 9.0:
            codes[m] = orc.MEAS_GATED                                # no fix_depth
            continue
        K = W * Si
        Dd = D if left_looking else P[rho, rho].copy()
        if not (np.isnan(K).any() or np.isnan(H)):
            dx = np.zeros(n)
            dx[:nact] = (lam[:nact] * K) * res
            x[:nxa] = f.boxplus(x, dx)[:nxa]
            if left_looking:
                D -= L[rho, rho] * (K[rho] * W[rho])
                Ws.append(W)
                Sis.append(Si)
            else:
                P = P - L * (K[HI] * W[LO])
                Dd = P[rho, rho].copy()
                Ws.append(W)
        before = x.copy()
        flag |= _fix_depth(x, Dd, ln, reset, p0rr)
        if not left_looking:
            P[rho, rho] = Dd
        fixes += int((x != before).sum())
        if np.isnan(x[:nxa]).any():
            flag |= NAN_BIT
    if left_looking:                                                 # ONE trailing pass, the entries in order
        P = sym.copy()
        for Wk, Sk in zip(Ws, Sis):
            P = P - L * ((Wk[HI] * Sk) * Wk[LO])
        P[rho, rho] = D
    low = np.tril(P)
    Pn = c["P0"][b].copy()
    Pn[:nact, :nact] = low + np.tril(low, -1).T
    return x, Pn, codes, flag, len(Ws), fixes, mah
