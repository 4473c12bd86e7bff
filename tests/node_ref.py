"""Restatement of the device-resident node graph (include/viekf_node.h) over tests/frame_ref.py: the tail of
VIEKF::keyframe_reset (reference src/vi_ekf/vi_ekf_kfr.cpp:147-150), get_global_pose (:14-21), get_global_cov /
propagate_global_covariance (:23-53), the true node and the truth in the node frame.  The SE(3) algebra is
oracle.seq_oracle.xform_mul / xform_adj (rotation matrices, oracle/np_twin.py), not the product's quaternion code; only tests/
import this.  Also the scenario LOOP_KFR -- a closed loop in which the filters DO reset -- and its flight through the restated
stack, which fixes the bounds of the GPU test."""
import functools
import json
import math
import os

import numpy as np

from oracle import np_twin as tw
from oracle import oracle as orc
from oracle.seq_oracle import xform_adj, xform_mul
from tests import frame_ref as F
from tests import sim_ref as R

IDENTITY = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
POSE_IDX = [0, 1, 2, 6, 7, 8]          # the POS and ATT blocks of P (vi_ekf_kfr.cpp:28-31)


def yaw_of(q):                         # src/quat.cpp:221-224
    w, x, y, z = q
    return math.atan2(2.0 * (w * z + x * y), 1.0 - 2.0 * (y * y + z * z))


def euler_of(q):                       # src/quat.cpp:211-224
    w, x, y, z = q
    return (math.atan2(2.0 * (w * x + y * z), 1.0 - 2.0 * (x * x + y * y)), math.asin(2.0 * (w * y - z * x)), yaw_of(q))


def from_euler(roll, pitch, yaw):      # src/quat.cpp:150-165
    cp, sp, ct, st, cs, ss = (math.cos(roll / 2), math.sin(roll / 2), math.cos(pitch / 2), math.sin(pitch / 2),
                              math.cos(yaw / 2), math.sin(yaw / 2))
    return np.array([cp * ct * cs + sp * st * ss, sp * ct * cs - cp * st * ss, cp * st * cs + sp * ct * ss, cp * ct * ss - sp * st * cs])


def cholesky6(A, e):
    """6x6 lower Cholesky of A with e as one more row -> (info, nees): info = j + 1 of the first pivot that is not > 0
    (then nees is NaN), the rule of include/viekf_diag.h"""
    L = np.zeros((6, 6))
    y = np.zeros(6)
    for j in range(6):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return j + 1, float("nan")
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        y[j] = (e[j] - L[j, :j] @ y[:j]) / L[j, j]
    return 0, float(y @ y)


class NodeRef:
    """one filter's node graph: viekf_node_update / _global / _relative_truth / _global_error, step by step"""

    def __init__(self, trail_capacity=0):
        self.cap = int(trail_capacity)
        self.reset()

    def reset(self):
        self.node, self.node_cov, self.true_node, self.count = IDENTITY.copy(), np.zeros((6, 6)), IDENTITY.copy(), 0
        self.trail_nodes, self.trail_edges = np.zeros((self.cap, 7)), np.zeros((self.cap, 17))

    def update(self, did_reset, edge, x_true=None):
        if not did_reset:
            return
        edge = np.asarray(edge, dtype=np.float64)
        C = np.zeros((6, 6))
        C[:3, :3] = edge[7:16].reshape(3, 3, order="F")
        C[5, 5] = edge[16]
        A = xform_adj(self.node)
        self.node_cov = self.node_cov + A.T @ C @ A                     # :149, with the node before it moves
        if self.cap:
            self.trail_nodes[self.count % self.cap], self.trail_edges[self.count % self.cap] = self.node, edge
        self.node = xform_mul(self.node, edge[:7])                     # :150
        self.count += 1
        if x_true is not None:                                         # the reset's map (:120-125) applied to the truth
            self.true_node = np.concatenate([x_true[0:3], from_euler(0.0, 0.0, yaw_of(x_true[6:10]))])

    def global_pose(self, x):
        return xform_mul(self.node, np.concatenate([x[0:3], x[6:10]]))

    def global_cov(self, P):
        A = xform_adj(self.node)
        return self.node_cov + A.T @ P[np.ix_(POSE_IDX, POSE_IDX)] @ A

    def relative_truth(self, x_true):
        x = np.array(x_true, dtype=np.float64)
        t, q = self.true_node[:3], self.true_node[3:]
        x[0:3] = tw.rotp(q, x_true[0:3] - t)
        x[6:10] = tw.qmul(np.concatenate([[q[0]], -q[1:]]), x_true[6:10])
        return x

    def global_error(self, x, P, x_true):
        """-> (err [6], nees, info)"""
        pose = self.global_pose(x)
        err = np.concatenate([x_true[0:3] - pose[:3], tw.q_boxminus(x_true[6:10], pose[3:])])
        info, nees = cholesky6(self.global_cov(P), err)
        return err, nees, info


class BatchNodeRef:
    """B independent NodeRef behind the array shapes of vi_ekf_amd.NodeGraph"""

    def __init__(self, batch, trail_capacity=0):
        self.B = int(batch)
        self.r = [NodeRef(trail_capacity) for _ in range(self.B)]

    def update(self, did_reset, edges, x_true=None):
        for b, r in enumerate(self.r):
            r.update(did_reset[b], edges[b], None if x_true is None else x_true[b])

    def get(self):
        return dict(node=np.stack([r.node for r in self.r]), node_cov=np.stack([r.node_cov.ravel(order="F") for r in self.r]),
                    true_node=np.stack([r.true_node for r in self.r]), count=np.array([r.count for r in self.r], np.int32))

    def global_pose(self, x, P):
        """x [B][nx], P [B][n][n] -> pose [B][7], cov [B][6][6]"""
        return (np.stack([r.global_pose(x[b]) for b, r in enumerate(self.r)]),
                np.stack([r.global_cov(P[b]) for b, r in enumerate(self.r)]))

    def relative_truth(self, x_true):
        return np.stack([r.relative_truth(x_true[b]) for b, r in enumerate(self.r)])

    def global_error(self, x, P, x_true):
        o = [r.global_error(x[b], P[b], x_true[b]) for b, r in enumerate(self.r)]
        return dict(err=np.stack([e[0] for e in o]), nees=np.array([e[1] for e in o]), info=np.array([e[2] for e in o], np.int32))

    def trail(self):
        return np.stack([r.trail_nodes for r in self.r]), np.stack([r.trail_edges for r in self.r])


# -- the closed loop in which the filters reset ---------------------------------------------------------------------------
# sim_ref.LOOP on wider and quicker circles: the camera sweeps over the landmark field fast enough for the keyframe overlap to
# fall under 0.8 every few frames.  tmax = 3.0, N = 8, threshold 0.8, 250 / 25 Hz.
LOOP_KFR = dict(R.LOOP, radius=[1.2, 1.5, 1.0, 1.3], period=[5.0, 6.0, 4.0, 5.0])
LOOP_KFR_TMAX, LOOP_KFR_N, LOOP_KFR_THRESH = 3.0, 8, 0.8
# What tests/test_node_ref_cpu.py::test_loop_kfr_through_the_restated_stack measures and prints on the CPU, worst over the
# four vehicles on the tick before each frame: after t = 1 s the global error 0.5518 m and 2.009 degrees and the error relative
# to the true node 0.2158 m and 2.027 degrees (the largest component each), over the whole flight the global 6-dof NEES 5.814.
# Rounded up here.  The bounds are TWICE that: the device simulator draws the same Philox noise as sim_ref, so the GPU flight
# differs from this one by rounding only, and a factor of two covers one flipped gate decision.
LOOP_KFR_MEASURED = dict(global_m=0.552, global_deg=2.01, relative_m=0.216, relative_deg=2.03, nees=5.82)
LOOP_KFR_BOUNDS = {k: 2.0 * v for k, v in LOOP_KFR_MEASURED.items()}


def loop_kfr_recorded():
    """the frames on which each vehicle resets and the ids handed out, as fly_loop_kfr found them: tests/golden/
    loop_kfr_resets.json (tests/test_node_ref_cpu.py holds the file to the flight), so that the GPU test need not fly on the CPU"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loop_kfr_resets.json")) as fh:
        return json.load(fh)


def loop_kfr_params():
    p = dict(orc.EKF_YAML)
    p.update(use_keyframe_reset=True, keyframe_overlap_threshold=LOOP_KFR_THRESH)
    return p


def pose_errors(x_est_pos, x_est_q, x_true_pos, x_true_q):
    """(m, degrees): the largest component, as the closed-loop tests measure"""
    return np.array([np.abs(np.asarray(x_est_pos) - x_true_pos).max(), np.degrees(np.abs(orc.q_boxminus(x_est_q, x_true_q)).max())])


@functools.lru_cache(maxsize=1)
def fly_loop_kfr():
    """LOOP_KFR through the restated stack (RefSimulator -> oracle propagate -> FrameRef -> NodeRef), once per process
    -> list over the vehicles of dict(reset_frames, next_feat_id, worst [4] = global m / deg, relative m / deg after t = 1 s,
    nees (worst), chol_failures, nan), everything sampled on the tick before each frame"""
    N, p = LOOP_KFR_N, loop_kfr_params()
    lm = R.jittered_landmarks(77)
    res = []
    for sim in R.vehicles(LOOP_KFR, p, N, lm, tmax=LOOP_KFR_TMAX):
        ref = F.FrameRef(orc.OracleFilter(N).init(**{k: p[k] for k in F_KEYS}), LOOP_KFR_THRESH)
        nd = NodeRef()
        st = dict(t=sim.t, frame=0, reset_frames=[], nees=0.0, chol=0)

        def imu_cb(t, u, Rm, ref=ref, st=st):
            ref.f.propagate(u, t - st["t"])
            st["t"] = t

        def feat_cb(t, pix, ids, Rm, sim=sim, ref=ref, nd=nd, st=st):
            xt = sim.truth_state([])
            out = ref.intake(np.asarray(pix).reshape(-1, 2), list(ids), Rm)
            nd.update(out["did_reset"], out["edges"], xt)
            if out["did_reset"]:
                st["reset_frames"].append(st["frame"])
            st["frame"] += 1

        sim.register_imu_cb(imu_cb)
        sim.register_feat_cb(feat_cb)
        worst = np.zeros(4)
        while sim.run():
            if sim.k % 10 != 9:                                        # the tick before each frame
                continue
            xt, x, P = sim.truth_state([]), ref.f.x, ref.f.P
            err, nees, info = nd.global_error(x, P, xt)               # the factorisations the diagnostics run
            try:
                np.linalg.cholesky(P[np.ix_(POSE_IDX, POSE_IDX)])
            except np.linalg.LinAlgError:
                st["chol"] += 1
            st["chol"] += int(info != 0)
            if info == 0:
                st["nees"] = max(st["nees"], nees)
            if sim.t > 1.0:
                pose, xr = nd.global_pose(x), nd.relative_truth(xt)
                worst = np.maximum(worst, np.concatenate([pose_errors(pose[:3], pose[3:], xt[0:3], xt[6:10]),
                                                          pose_errors(x[0:3], x[6:10], xr[0:3], xr[6:10])]))
        res.append(dict(reset_frames=st["reset_frames"], next_feat_id=sim.next_feat_id, worst=worst, nees=st["nees"],
                        chol_failures=st["chol"], nan=bool(np.isnan(ref.f.x[:17 + 5 * ref.f.len_features]).any() or np.isnan(nd.node).any()
                                                           or np.isnan(nd.node_cov).any())))
    return res


F_KEYS = ("x0", "P0", "Qx", "lam", "Qu", "P0_feat", "Qx_feat", "lam_feat", "cam_center", "focal_len", "q_b_c", "p_b_c", "q_b_u",
          "min_depth", "use_drag_term", "use_partial_update", "use_keyframe_reset")
