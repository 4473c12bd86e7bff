"""Restatement of the device-resident flight recorder (include/viekf_rec.h) in numpy, by another method than
the device's: poses become rotation matrices (oracle/np_twin.py's Rmat) and translations, the SE(3) alignment is Kabsch's
(an SVD with the determinant correction, not Horn's eigenvector), the yaw alignment the closed form, attitude errors the angle
of a rotation matrix.  Only tests/ and tools/rec_bench.py import this.  Also the flight of node_ref.LOOP_KFR through the
restated stack with every frame recorded, which fixes the bounds of the GPU test's closed loop."""
import functools
import math

import numpy as np

from oracle import np_twin as tw
from oracle import oracle as orc
from tests import frame_ref as F
from tests import node_ref as NR
from tests import sim_ref as R

ALIGN = ("none", "yaw", "se3")


def rot(q):
    """the ACTIVE rotation matrix of a pose's quaternion: q.rota(v) = rot(q) v"""
    return tw.Rmat(np.asarray(q, float)).T


def angle_of(Rm):
    """the rotation angle in [0, pi] of a rotation matrix = |q1 [-] q2| for Rm = rot(q2)^T rot(q1)"""
    w = 0.5 * np.array([Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    return math.atan2(np.linalg.norm(w), 0.5 * (np.trace(Rm) - 1.0))


def quat_of(Rm):
    """q with rot(q) = Rm and w >= 0 (Shepperd's choice of the largest pivot)"""
    t = np.trace(Rm)
    cand = np.array([t, Rm[0, 0], Rm[1, 1], Rm[2, 2]])
    i = int(np.argmax(cand))
    if i == 0:
        q = np.array([1.0 + t, Rm[2, 1] - Rm[1, 2], Rm[0, 2] - Rm[2, 0], Rm[1, 0] - Rm[0, 1]])
    elif i == 1:
        q = np.array([Rm[2, 1] - Rm[1, 2], 1.0 + 2.0 * Rm[0, 0] - t, Rm[0, 1] + Rm[1, 0], Rm[0, 2] + Rm[2, 0]])
    elif i == 2:
        q = np.array([Rm[0, 2] - Rm[2, 0], Rm[0, 1] + Rm[1, 0], 1.0 + 2.0 * Rm[1, 1] - t, Rm[1, 2] + Rm[2, 1]])
    else:
        q = np.array([Rm[1, 0] - Rm[0, 1], Rm[0, 2] + Rm[2, 0], Rm[1, 2] + Rm[2, 1], 1.0 + 2.0 * Rm[2, 2] - t])
    q = q / np.linalg.norm(q)
    return -q if q[0] < 0 else q


def rot_z(th):
    c, s = math.cos(th), math.sin(th)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def horn_matrix(A):
    """Horn's symmetric 4x4 matrix of A = sum t e^T (only its eigenvalues are used here: the gap)"""
    S = A.T
    return np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                     [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                     [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                     [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])


def centred(pt, pe):
    ct, ce = pt.mean(axis=0), pe.mean(axis=0)
    return ct, ce, (pt - ct).T @ (pe - ce)


def gaps(A):
    """(the relative gap between the two largest eigenvalues of Horn's matrix, |(A10 - A01, A00 + A11)| relative to |A|): where
    either is tiny the SE(3) rotation / the yaw is not unique (to rounding) and align_pose is not compared"""
    nrm = np.linalg.norm(A)
    if nrm == 0.0:
        return 0.0, 0.0
    lam = np.linalg.eigvalsh(horn_matrix(A))
    return float((lam[3] - lam[2]) / max(abs(lam[3]), abs(lam[0]))), float(math.hypot(A[1, 0] - A[0, 1], A[0, 0] + A[1, 1]) / nrm)


def alignment(pt, pe, align):
    """-> (R_a, t_a, A) for true / estimated positions [n][3], n >= 1"""
    ct, ce, A = centred(pt, pe)
    if align == "none":
        return np.eye(3), np.zeros(3), A
    if align == "yaw":
        s, c = A[1, 0] - A[0, 1], A[0, 0] + A[1, 1]
        Ra = rot_z(0.0 if s == 0.0 and c == 0.0 else math.atan2(s, c))
    elif align == "se3":                                     # Kabsch: argmax_R tr(R A^T) = U diag(1, 1, det(U V^T)) V^T
        U, _, Vt = np.linalg.svd(A)
        Ra = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt)) or 1.0]) @ Vt
    else:
        raise ValueError(align)
    return Ra, ct - Ra @ ce, A


def between(Ra, ta, Rb, tb):
    """T_a^-1 * T_b as (R, t)"""
    return Ra.T @ Rb, Ra.T @ (tb - ta)


def trajectory_error_one(est, tru, valid, align="yaw", delta=1):
    """one filter: est, tru [T][7], valid [T] -> dict of scalars, align_pose [7], n_used [2], gap, yaw_gap"""
    nan = float("nan")
    idx = np.nonzero(np.asarray(valid) != 0)[0]
    n = len(idx)
    out = dict(ate_pos=nan, ate_att=nan, rpe_pos=nan, rpe_att=nan, align_pose=np.full(7, nan), n_used=np.array([n, 0], np.int32),
               gap=0.0, yaw_gap=0.0)
    Re = {k: rot(est[k, 3:]) for k in idx}
    Rt = {k: rot(tru[k, 3:]) for k in idx}
    if n:
        pt, pe = tru[idx, :3], est[idx, :3]
        Ra, ta, A = alignment(pt, pe, align)
        out["gap"], out["yaw_gap"] = gaps(A)
        out["align_pose"] = np.concatenate([ta, quat_of(Ra)])
        assert np.abs(rot(out["align_pose"][3:]) - Ra).max() < 1e-12
        # (the residual from centred coordinates where there is an alignment: p_t - (R_a p_e + t_a) with t_a = c_t - R_a c_e)
        d = pt - (pe @ Ra.T + ta) if align == "none" else (pt - pt.mean(axis=0)) - (pe - pe.mean(axis=0)) @ Ra.T
        out["ate_pos"] = math.sqrt(np.mean(np.sum(d * d, axis=1)))
        out["ate_att"] = math.sqrt(np.mean([angle_of((Ra @ Re[k]).T @ Rt[k]) ** 2 for k in idx]))
    vs = set(int(k) for k in idx)
    dp, da = [], []
    for k in idx:
        k2 = int(k) + delta
        if k2 in vs:
            Er, Et_ = between(Re[k], est[k, :3], Re[k2], est[k2, :3])
            Tr, Tt_ = between(Rt[k], tru[k, :3], Rt[k2], tru[k2, :3])
            Dr, Dt = between(Tr, Tt_, Er, Et_)
            dp.append(Dt @ Dt)
            da.append(angle_of(Dr) ** 2)
    out["n_used"][1] = len(dp)
    if dp:
        out["rpe_pos"], out["rpe_att"] = math.sqrt(np.mean(dp)), math.sqrt(np.mean(da))
    return out


def trajectory_error(est, tru, valid, align="yaw", first=0, last=None, delta=1):
    """est, tru [B][T][7], valid [B][T] -> dict of [B] arrays (align_pose [B][7], n_used [B][2], gap [B], yaw_gap [B])"""
    last = est.shape[1] if last is None else last
    o = [trajectory_error_one(est[b, first:last], tru[b, first:last], valid[b, first:last], align, delta) for b in range(est.shape[0])]
    return {k: np.array([e[k] for e in o]) for k in o[0]}


def pose_ensemble(est, tru, valid, first=0, last=None):
    """-> [T'][4] = {n, rms |p_t - p_e|, rms angle, max |p_t - p_e|} over the filters valid on each frame"""
    last = est.shape[1] if last is None else last
    out = np.full((last - first, 4), np.nan)
    for i, k in enumerate(range(first, last)):
        bs = np.nonzero(valid[:, k] != 0)[0]
        out[i, 0] = len(bs)
        if len(bs):
            d = np.linalg.norm(tru[bs, k, :3] - est[bs, k, :3], axis=1)
            a = [angle_of(rot(est[b, k, 3:]).T @ rot(tru[b, k, 3:])) for b in bs]
            out[i, 1:] = math.sqrt(np.mean(d * d)), math.sqrt(np.mean(np.square(a))), d.max()
    return out


def _stats(v, lo, hi):
    v = v[np.isfinite(v)]
    if v.size == 0:
        return [0.0, float("nan"), float("nan"), 0.0, 0.0]
    return [float(v.size), float(math.fsum(v) / v.size), float(v.max()), 0.0 if lo is None else float((v < lo).sum()) / v.size,
            0.0 if hi is None else float((v > hi).sum()) / v.size]


def channels(chan, lo=None, hi=None, first=0, last=None):
    """chan [T][B][K] -> dict(per_frame [T'][K][5], per_filter [B][K][5])"""
    T, B, K = chan.shape
    last = T if last is None else last
    c = chan[first:last]
    bound = lambda a, j: None if a is None else a[j]        # noqa: E731
    return dict(per_frame=np.array([[_stats(c[i, :, j], bound(lo, j), bound(hi, j)) for j in range(K)] for i in range(last - first)]).reshape(last - first, K, 5),
                per_filter=np.array([[_stats(c[:, b, j], bound(lo, j), bound(hi, j)) for j in range(K)] for b in range(B)]).reshape(B, K, 5))


def pose_mul(T1, T2):
    """T1 * T2 of include/viekf.h, through matrices"""
    R1 = rot(T1[3:])
    return np.concatenate([T1[:3] + R1 @ T2[:3], quat_of(R1 @ rot(T2[3:]))])


# -- the closed loop, recorded ------------------------------------------------------------------------------------------------
# node_ref.LOOP_KFR through node_ref.fly_loop_kfr's stack (RefSimulator -> oracle propagate -> FrameRef -> NodeRef), four
# vehicles, 3 s at 250 / 25 Hz: on the tick before each of the 75 frames the global pose, the truth and the 6-dof node NEES
# are recorded, exactly where tests/test_gpu_node.py's and tests/test_gpu_rec.py's closed loops sample.  What
# tests/test_rec_ref_cpu.py::test_loop_kfr_recorded_through_the_restated_stack measures and prints on the CPU over all 75
# frames, worst over the four vehicles: yaw-aligned ATE 0.19261 m and 2.3176 degrees (0.1622 .. 0.1926 m), RPE over delta = 1
# 0.013009 m and 0.22279 degrees, the worst per-frame ANEES of the node NEES (the mean over the four vehicles) 4.4066.  Rounded
# up here.  The bounds are TWICE that, the margin of node_ref.LOOP_KFR_BOUNDS and for its reason: the device simulator draws the
# same Philox noise as sim_ref, so the GPU flight differs from this one by rounding only, and a factor of two covers one
# flipped gate decision.
LOOP_KFR_FRAMES = 75
LOOP_KFR_REC_MEASURED = dict(ate_m=0.193, ate_deg=2.32, rpe_m=0.0131, rpe_deg=0.223, anees=4.41)
LOOP_KFR_REC_BOUNDS = {k: 2.0 * v for k, v in LOOP_KFR_REC_MEASURED.items()}


def loop_kfr_figures(te, ch):
    """the five figures of LOOP_KFR_REC_MEASURED from trajectory_error(align = "yaw", delta = 1) and channels()["per_frame"],
    channel 0 the node NEES"""
    return dict(ate_m=float(np.max(te["ate_pos"])), ate_deg=float(np.degrees(np.max(te["ate_att"]))), rpe_m=float(np.max(te["rpe_pos"])),
                rpe_deg=float(np.degrees(np.max(te["rpe_att"]))), anees=float(np.max(ch[:, 0, 1])))


@functools.lru_cache(maxsize=1)
def fly_loop_kfr_recorded():
    """-> dict(est [4][75][7], tru [4][75][7], valid [4][75], chan [75][4][1] = the node NEES, stamps [75])"""
    N, p = NR.LOOP_KFR_N, NR.loop_kfr_params()
    lm = R.jittered_landmarks(77)
    est, tru, nees, stamps = [], [], [], []
    for sim in R.vehicles(NR.LOOP_KFR, p, N, lm, tmax=NR.LOOP_KFR_TMAX):
        ref = F.FrameRef(orc.OracleFilter(N).init(**{k: p[k] for k in NR.F_KEYS}), NR.LOOP_KFR_THRESH)
        nd = NR.NodeRef()
        st = dict(t=sim.t)

        def imu_cb(t, u, Rm, ref=ref, st=st):
            ref.f.propagate(u, t - st["t"])
            st["t"] = t

        def feat_cb(t, pix, ids, Rm, sim=sim, ref=ref, nd=nd):
            out = ref.intake(np.asarray(pix).reshape(-1, 2), list(ids), Rm)
            nd.update(out["did_reset"], out["edges"], sim.truth_state([]))

        sim.register_imu_cb(imu_cb)
        sim.register_feat_cb(feat_cb)
        e, r, c, s = [], [], [], []
        while sim.run():
            if sim.k % 10 != 9:                                        # the tick before each frame
                continue
            xt = sim.truth_state([])
            e.append(nd.global_pose(ref.f.x))
            r.append(np.concatenate([xt[0:3], xt[6:10]]))
            c.append(nd.global_error(ref.f.x, ref.f.P, xt)[1])
            s.append(sim.t)
        est.append(e); tru.append(r); nees.append(c); stamps = s      # noqa: E702
    est, tru = np.array(est), np.array(tru)
    return dict(est=est, tru=tru, valid=np.isfinite(est).all(axis=2).astype(np.uint8) & np.isfinite(tru).all(axis=2),
                chan=np.array(nees).T[:, :, None].copy(), stamps=np.array(stamps))
