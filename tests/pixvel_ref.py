"""Restatement of the PIXEL_VEL model and its entry points (include/viekf_pixvel.h) in numpy over oracle.np_twin.TwinFilter:
the model zhat = Hb f_zeta with its Jacobian, the update through TwinFilter._correct, the flow of a frame's features by id,
and the intake's pixel-velocity step over the oracle filters of tests/frame_ref.py.  Only tests/ import this."""
import numpy as np

from oracle import np_twin as tw
from oracle import oracle as orc

SKIPPED, SUCCESS, GATED, NAN, INVALID = -1, 0, 1, 2, 3
COLS_BODY = (3, 4, 5, 12, 13, 14)          # VEL, B_G: the body columns of H


def body_input(twin, gyro):
    """the u VIEKF::dynamics takes for a raw gyro sample: rotated by q_b_u as the propagate does; the accelerometer does
    not enter the feature rows"""
    return np.concatenate([np.zeros(3), tw.rota(twin.q_b_u, np.asarray(gyro, float))])


def h_pixel_vel(twin, x, i, gyro):
    """-> zhat [2] (px/s), H [2][n] at state x for the feature in slot i and a raw gyro sample.

    zhat = Hb f, Hb the 2x2 block of h_feat and f the first two outputs of the feature's dynamics.  With zeta the bearing,
    w = omega_c + rho zeta x v_c and T T^T = I - zeta zeta^T the bearing moves by zeta_dot = zeta x w, so
        zhat = Jpi(zeta) g(zeta),  g = zeta x omega_c + rho (zeta (zeta . v_c) - v_c),  Jpi = (1 / e_z) F (I - zeta e_z^T / e_z)
    depends on q_zeta through zeta alone, and d zeta / d delta = -skew(zeta) T_zeta (what h_feat's own H uses)."""
    n = twin.n
    ub = body_input(twin, gyro)
    xd, A, _ = twin.dynamics(x, ub)
    _, Hf = twin.h_feat(x, i)
    r0, rr = 16 + 3 * i, 18 + 3 * i
    Hb = Hf[:, r0:r0 + 2]
    zhat = Hb @ xd[r0:r0 + 2]
    H = np.zeros((2, n))
    H[:, 3:6] = Hb @ A[r0:r0 + 2, 3:6]
    H[:, 12:15] = Hb @ A[r0:r0 + 2, 12:15]
    H[:, rr] = Hb @ A[r0:r0 + 2, rr]
    # the bearing block, in zeta space
    qz, rho = x[17 + 5 * i:21 + 5 * i], x[21 + 5 * i]
    z = tw.rota(qz, tw.E_Z)
    Tz = tw.T_zeta(qz)
    v, om = x[3:6], ub[3:6] - x[13:16]
    Rbc = tw.Rmat(twin.q_b_c)
    vc, wc = Rbc @ (v + np.cross(om, twin.p_b_c)), Rbc @ om
    g = np.cross(z, wc) + rho * (z * (z @ vc) - vc)
    dg = -tw.skew(wc) + rho * ((z @ vc) * np.eye(3) + np.outer(z, vc))     # d g / d zeta
    ez = z[2]
    D = np.zeros((2, 3))
    for r in range(2):
        e_r = np.eye(3)[r]
        D[r] = twin.F[r, r] * (dg[r] / ez - g[r] * tw.E_Z / ez ** 2 - e_r * g[2] / ez ** 2 - z[r] * dg[2] / ez ** 2
                               + 2.0 * z[r] * g[2] * tw.E_Z / ez ** 3)
    H[:, r0:r0 + 2] = D @ (-tw.skew(z) @ Tz)
    return zhat, H


def update_pixel_vel(twin, i, z, gyro, R, gyro_var=0.0, active=True):
    """one PIXEL_VEL measurement on the twin: R_eff = R + gyro_var J J^T, J the B_G block of H -> result code"""
    zhat, H = h_pixel_vel(twin, twin.x, i, gyro)
    J = H[:, 12:15]
    R_eff = np.asarray(R, float) + gyro_var * (J @ J.T)
    return twin._correct(np.asarray(z, float) - zhat, H, R_eff, active)


def update_pixel_vels(twin, slot, z, gyro, R, gyro_var=0.0, active=None, order=0):
    """viekf_batch_update_pixel_vels for one filter: slot [M], z [M][2], R [M][2][2] (indexed [row, col]) -> result [M]"""
    M = len(slot)
    res = np.full(M, SKIPPED, dtype=np.int32)
    for e in range(M):
        m = M - 1 - e if order else e
        act = 1 if active is None else int(active[m])
        if act == 2 or slot[m] < 0:
            continue
        if slot[m] >= twin.len:
            res[m] = INVALID
            continue
        if np.isnan(z[m]).any() or np.isnan(gyro).any():
            res[m] = NAN
            continue
        res[m] = update_pixel_vel(twin, int(slot[m]), z[m], gyro, R[m], gyro_var, act != 0)
    return res


def pixel_flow(z_prev, ids_prev, z, ids, dt):
    """viekf_pixel_flow: z_prev [B][Mp][2], ids_prev [B][Mp], z [B][M][2], ids [B][M], dt [B] -> zdot [B][M][2]"""
    B, M = ids.shape
    out = np.full((B, M, 2), np.nan)
    for b in range(B):
        for m in range(M):
            if ids[b, m] < 0:
                continue
            hit = np.nonzero(ids_prev[b] == ids[b, m])[0]
            if hit.size == 0:
                continue
            k = hit[0]
            if np.isfinite(z[b, m]).all() and np.isfinite(z_prev[b, k]).all():
                out[b, m] = (z[b, m] - z_prev[b, k]) / dt[b]
    return out


def is_measurement(gid, feat_result, zdot):
    """an entry of a frame is a PIXEL_VEL measurement where its id is real, the FEAT was queued (SUCCESS or GATED) and the
    flow is finite"""
    return gid >= 0 and feat_result in (orc.MEAS_SUCCESS, orc.MEAS_GATED) and np.isfinite(zdot).all()


def intake_pixel_vel(twins, tables, ids, zdot, feat_result, gyro, R, gyro_var=0.0, use_pixel_vel=True, active=None, stale=()):
    """viekf_frame_intake_pixel_vel over one TwinFilter per filter.  tables[b]: the ids in slot order (what the intake tracks)
    just after its intake() of the same frame; ids [B][M], zdot [B][M][2], feat_result [B][M], gyro [B][3], R (2, 2), (B, 2, 2) or
    (B, M, 2, 2); stale: filters whose table is stale (left alone, ids >= 0 INVALID) -> result [B][M]"""
    B, M = ids.shape
    R = np.asarray(R, dtype=np.float64)
    result = np.full((B, M), SKIPPED, dtype=np.int32)
    for b, t in enumerate(twins):
        if active is not None and not active[b]:
            continue
        if b in stale:
            result[b][ids[b] >= 0] = INVALID
            continue
        tab = [int(v) for v in tables[b]]
        for i in reversed(range(M)):
            if not is_measurement(int(ids[b, i]), int(feat_result[b, i]), zdot[b, i]):
                continue
            if int(ids[b, i]) not in tab:
                result[b, i] = INVALID
                continue
            if np.isnan(gyro[b]).any():
                result[b, i] = NAN
                continue
            result[b, i] = update_pixel_vel(t, tab.index(int(ids[b, i])), zdot[b, i], gyro[b],
                                            R if R.ndim == 2 else (R[b] if R.ndim == 3 else R[b, i]), gyro_var, bool(use_pixel_vel))
    return result
