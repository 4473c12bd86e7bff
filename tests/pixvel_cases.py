"""The cases of the PIXEL_VEL updates (BatchVIEKF.update_pixel_vels, include/viekf_pixvel.h), shared by the CPU check of their
own conditions (tests/test_pixvel_ref_cpu.py) and by the GPU test (tests/test_gpu_pixvel.py).  Plain numpy, the oracle's warm
filters of tests/body_cases.py and the numpy twin: no GPU code, no pytest.

A case is ONE call: M entries (slot [B, M], z [B, M, 2]), one gyro sample per filter, R as (2, 2) (r_mode 0), (B, 2, 2) (1) or
(B, M, 2, 2) (2), gyro_var, active [B, M] or None, and the order, on the ragged batch of tests/meas_cases.py -- B = 5 filters
with len = [N, N - 3, 1, 0, N - 1] clipped at 0 -- from the warm, dense-P start state of tests/body_cases.py, with a body
velocity of up to 1.5 m/s per axis and a gyro bias written into x (the warm filters hover: without them the flow would hang on
the gyro sample alone), plus the case's own preparation.  The entries are written while they run, in the call's order, on
numpy twins of those filters: every z is the model's prediction at the state the entry will meet (tests/pixvel_ref.py), plus
noise drawn uniformly within half the smaller standard deviation of R -- so an honest entry's Mahalanobis distance stays below
0.5, far from the gate at 9.  The reference for everything -- x, P, result codes -- is TwinFilter._correct applied entry by
entry through tests/pixvel_ref.py.

case(name, N, variant) -> dict: N, params, partial, drag, x0, P0, len, slot, z, gyro, R, r_mode, gyro_var, active, order, codes
[B, M], x_ref, P_ref, untouched (filters the call must leave bit for bit), poisoned (a filter the twin is no reference for)."""
import copy

import numpy as np

from oracle import np_twin
from tests import body_cases as bc
from tests import meas_cases as mc
from tests import pixvel_ref as pr

B = mc.B
SIZES = (1, 3, 12)                  # n = 19, 25, 52: odd and even, below and (with 256 threads) below one pass of the W loop
NAN_BIT, NEG_DEPTH_BIT = 1, 4
POISONED = mc.POISONED
_CASES = {}


def to_twin(sc, f, N):
    """a numpy twin at the oracle filter's state (P: the oracle's lower triangle, mirrored -- what the device gets)"""
    prm = {k: sc["params"][k] for k in mc.ORACLE_KEYS}
    t = np_twin.TwinFilter(N, **prm)
    t.x = f.x.copy()
    low = np.tril(f.P)
    t.P = low + np.tril(low, -1).T
    t.len = int(f.len_features)
    return t


def start(N, partial, drag, seed):
    """-> scene, B twins at the warm state with a velocity and a gyro bias written in"""
    sc, fs = bc.warm(N, partial, drag)
    r = np.random.default_rng(seed)
    ts = [to_twin(sc, f, N) for f in fs]
    for t in ts:
        t.x[3:6] = r.uniform(-1.5, 1.5, 3)
        t.x[13:16] = r.uniform(-0.02, 0.02, 3)
    return sc, ts


def make_R(r, r_mode, M):
    """SPD, not diagonal: standard deviations of 8 .. 20 px / s about a rotated axis"""
    def one():
        s = r.uniform(8.0, 20.0, 2)
        a = r.uniform(0.0, np.pi)
        Q = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
        return Q @ np.diag(s * s) @ Q.T
    if r_mode == 0:
        return one()
    if r_mode == 1:
        return np.stack([one() for _ in range(B)])
    return np.stack([np.stack([one() for _ in range(M)]) for _ in range(B)])


def r_at(R, b, m):
    R = np.asarray(R)
    return R if R.ndim == 2 else (R[b] if R.ndim == 3 else R[b, m])


def _build(N, partial, drag, slot, r_mode, seed, order=0, gyro_var=0.0, active=None, prepare=None, tweak=None, gyro_nan=(),
           poisoned=None):
    sc, ts = start(N, partial, drag, seed)
    if prepare:
        prepare(ts)
    x0, P0 = np.stack([t.x.copy() for t in ts]), np.stack([t.P.copy() for t in ts])
    ln = np.array([t.len for t in ts], dtype=np.int32)
    slot = np.ascontiguousarray(slot, dtype=np.int32)
    M = slot.shape[1]
    r = np.random.default_rng(seed + 1)
    R = make_R(r, r_mode, M)
    gyro = r.normal(0.0, 0.2, (B, 3))
    for b in gyro_nan:
        gyro[b, 1] = np.nan
    act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    z = np.full((B, M, 2), 7.0)
    codes = np.full((B, M), pr.SKIPPED, dtype=np.int32)
    for e in range(M):
        m = M - 1 - e if order else e
        for b, t in enumerate(ts):
            s = int(slot[b, m])
            if 0 <= s < t.len and not np.isnan(gyro[b]).any():
                zhat, _ = pr.h_pixel_vel(t, t.x, s, gyro[b])
                sd = np.sqrt(np.linalg.eigvalsh(r_at(R, b, m)).min())
                z[b, m] = zhat + r.uniform(-0.5, 0.5, 2) * sd
        if tweak:
            tweak(m, z)
        for b, t in enumerate(ts):
            a = 1 if act is None else int(act[b, m])
            s = int(slot[b, m])
            if a == 2 or s < 0:
                continue
            if s >= t.len:
                codes[b, m] = pr.INVALID
            elif np.isnan(z[b, m]).any() or np.isnan(gyro[b]).any():
                codes[b, m] = pr.NAN
            elif b == poisoned:
                codes[b, m] = pr.SUCCESS                       # (guarded: see case "poison")
            else:
                codes[b, m] = pr.update_pixel_vel(t, s, z[b, m], gyro[b], r_at(R, b, m), gyro_var, a != 0)
    untouched = [b for b in range(B) if all(codes[b, m] in (pr.SKIPPED, pr.GATED, pr.NAN, pr.INVALID) for m in range(M))]
    return dict(N=N, partial=partial, drag=drag, params=sc["params"], x0=x0, P0=P0, len=ln, slot=slot, z=z, gyro=gyro, R=R,
                r_mode=r_mode, gyro_var=gyro_var, active=act, order=order, codes=codes, x_ref=np.stack([t.x.copy() for t in ts]),
                P_ref=np.stack([t.P.copy() for t in ts]), untouched=untouched, poisoned=poisoned)


# ---- every slot once ----------------------------------------------------------------------------------------------------
ONCE_VARIANTS = ((1, 0, 0, 0.0), (1, 1, 1, 1e-4), (1, 2, 0, 0.0), (0, 0, 1, 1e-4), (0, 2, 1, 0.0))   # (partial, r_mode, order, gyro_var)
ONCE_SKIP_FILTER = 1                # this filter's row holds a -1


def once_slots(N, seed):
    """M = N: every filter gets its own permutation of the slots (the ragged ones meet slots >= len: INVALID); one entry of
    filter 1's row is -1 (SKIPPED)"""
    r = np.random.default_rng(seed)
    slot = np.stack([r.permutation(N) for _ in range(B)]).astype(np.int32)
    slot[ONCE_SKIP_FILTER, int(r.integers(N))] = -1
    return slot


# ---- M past a wave and past n -------------------------------------------------------------------------------------------
REPEAT_N, REPEAT_M = 2, 70          # n = 22 < 64 < M


# ---- mixed script -------------------------------------------------------------------------------------------------------
MIXED_N, MIXED_M, MIXED_GATED, MIXED_NAN, MIXED_NAN_FILTER, MIXED_SKIPPED_FILTER, MIXED_ACTIVE_FILTER, MIXED_GYRO_NAN_FILTER = 12, 8, 3, 5, 1, 2, 0, 4


def mixed_slots(N):
    return np.array([[(3 * m + b) % (N - 4) for m in range(MIXED_M)] for b in range(B)], dtype=np.int32)


def _mixed_active():
    a = np.ones((B, MIXED_M), dtype=np.uint8)
    a[MIXED_ACTIVE_FILTER, :4] = [1, 0, 2, 1]       # 0, 1 and 2 within one filter's row
    a[MIXED_NAN_FILTER, 1] = 0
    a[MIXED_SKIPPED_FILTER, :] = 2                  # this filter sits the whole call out: bit for bit untouched
    return a


def _mixed_tweak(m, z):
    if m == MIXED_GATED:
        z[:, m] += 5000.0                           # a flow far off
    if m == MIXED_NAN:
        z[MIXED_NAN_FILTER, m, 1] = np.nan


# ---- fix_depth inside the chain -----------------------------------------------------------------------------------------
FIX_NEG_FILTER, FIX_BIG_FILTER = 0, 4


def _fix_prepare(N):
    def prepare(ts):
        ts[FIX_NEG_FILTER].x[21 + 5 * (N - 1)] = -0.2       # rho < 0 on the last slot: P(rho, rho) += err^2, NEGATIVE_DEPTH
        ts[FIX_BIG_FILTER].x[21 + 5 * 1] = 150.0            # rho > 1e2 on slot 1: P(rho, rho) = P0_feat[2]
    return prepare


def fix_slots(N):
    """entry 0 on slot 0 (fix_depth fires behind it), then the repaired slots themselves, then slot 0 again"""
    row = [0, N - 1, 1, N - 1, 0]
    return np.array([row for _ in range(B)], dtype=np.int32)


# ---- a NaN in P ---------------------------------------------------------------------------------------------------------
POISON_SLOT = 1
POISON_AT = (7, 16 + 3 * POISON_SLOT)     # P(ATT_y, first bearing column of slot 1) and its mirror image: only an entry on slot 1
                                          # reads that column, and row 7 of its W and K is NaN


def _poison(ts):
    i, j = POISON_AT
    ts[POISONED].P[i, j] = ts[POISONED].P[j, i] = np.nan


def case(name, N, variant=0):
    key = (name, N, variant)
    if key in _CASES:
        return _CASES[key]
    if name == "once":
        partial, r_mode, order, gv = ONCE_VARIANTS[variant]
        c = _build(N, partial, variant % 2, once_slots(N, 40 + N), r_mode, 700 + 10 * N + variant, order, gv)
    elif name == "repeat":
        r = np.random.default_rng(91)
        c = _build(REPEAT_N, 1, 1, r.integers(0, REPEAT_N, (B, REPEAT_M)), 2, 800 + variant, variant, 1e-4)
    elif name == "mixed":
        c = _build(MIXED_N, 1, 1, mixed_slots(MIXED_N), 2, 810, variant, 0.0, _mixed_active(), None, _mixed_tweak, (MIXED_GYRO_NAN_FILTER,))
    elif name == "fix":
        act = np.ones((B, 5), dtype=np.uint8)
        act[:, 0] = variant                                    # variant 0: an inactive entry meets the bad rho; 1: an applied one
        c = _build(N, 1, 0, fix_slots(N), 1, 820 + N + variant, 0, 0.0, act, _fix_prepare(N))
    elif name == "poison":
        # the poisoned filter's entry on POISON_SLOT reads the column with the NaN: its gain has a NaN and the guard (:247) skips
        # the correction; its other entries are applied.  numpy would spread the NaN through its dense products (0 * NaN), so
        # the twin is no reference for that filter: the GPU test holds it to the two routes' agreement and to what is stated there.
        c = _build(N, 1, 1, once_slots(N, 45), 0, 830, 0, 0.0, None, _poison, poisoned=POISONED)
    else:
        raise ValueError(name)
    c["name"] = "%s N=%d v=%d" % (name, N, variant)
    _CASES[key] = c
    return c


def clone(c):
    return copy.deepcopy(c)
