"""Restatement of the device-resident frame intake (include/viekf_frame.h) over one oracle filter: what
VIEKF_ROS::color_image_callback does with a tracked frame (reference src/vi_ekf_ros.cpp:276-305) when the frame belongs to
the time the filter is at -- keep_only_features with the keyframe test (src/vi_ekf/vi_ekf_feat.cpp:81-142), the new
features of add_measurement (src/vi_ekf/vi_ekf_meas.cpp:136-147), and the frame's updates in the order the reference's queue
hands out measurements of one stamp (newest insertion first, :150-176).  Written with the oracle's clear_feature,
keyframe_reset_edge, init_feature(l, id, depth) and update(FEAT, ..., id); only tests/ import this."""
import numpy as np

from oracle import oracle as orc

SKIPPED = -1


class FrameRef:
    """one filter's intake: an oracle.OracleFilter, the keyframe list and steps 1-6 of viekf_frame_intake"""

    def __init__(self, filt, keyframe_overlap_threshold=0.8):
        self.f = filt
        self.thresh = float(keyframe_overlap_threshold)
        self.kf = []
        self.resets = 0

    def tracked(self):
        return list(self.f.feature_ids)

    def intake(self, z, ids, R, depth=None):
        """z [M][2], ids [M], R (2,2) or (M,2,2) indexed [row, col], depth [M] or None
        -> dict(result [M], gated [M] -1 padded, gated_count, did_reset, edges [17])"""
        f = self.f
        z = np.asarray(z, dtype=np.float64).reshape(-1, 2)
        ids = [int(v) for v in ids]
        M = len(ids)
        R = np.asarray(R, dtype=np.float64)
        result = np.full(M, SKIPPED, dtype=np.int32)
        # 1. padding and repeats
        seen, frame_ids, live = set(), [], []
        for i, gid in enumerate(ids):
            if gid < 0:
                continue
            if gid in seen:
                result[i] = orc.MEAS_INVALID
                continue
            seen.add(gid)
            frame_ids.append(gid)
            live.append(i)
        # 2. keep_only_features (vi_ekf_feat.cpp:81-117)
        overlap = 0
        for gid in self.tracked():
            if gid in seen:
                if gid in self.kf:
                    overlap += 1
            else:
                f.clear_feature(gid)
        # 3. the keyframe test (:119-139)
        did_reset, edges = 0, np.zeros(17)
        if f.use_keyframe_reset and len(self.kf) > 0 and overlap / float(len(self.kf)) < self.thresh:
            edges = f.keyframe_reset_edge()
            did_reset = 1
            self.resets += 1
            self.kf = list(frame_ids)
        elif f.use_keyframe_reset and len(self.kf) == 0:
            self.kf = list(frame_ids)
        # 4. NaN entries and new features, in frame order (vi_ekf_meas.cpp:136-147)
        queue = []
        for i in live:
            if np.isnan(z[i]).any():
                result[i] = orc.MEAS_NAN
            elif f.global_to_local_feature_id(ids[i]) < 0:
                if f.init_feature(z[i], ids[i], float("nan") if depth is None else float(depth[i])):
                    # (the reference numbers a new feature itself, vi_ekf_feat.cpp:29-30; the intake keeps the frame's id)
                    f._p.contents.feature_ids[f.len_features - 1] = ids[i]
                result[i] = orc.MEAS_NEW_FEATURE
            else:
                queue.append(i)
        # 5. the updates, last entry first
        for i in reversed(queue):
            result[i] = f.update(orc.FEAT, z[i], R if R.ndim == 2 else R[i], True, ids[i])
        # 6. what goes to the tracker's drop_feature
        g = [ids[i] for i in range(M) if i in queue and result[i] == orc.MEAS_GATED]
        gated = np.full(M, -1, dtype=np.int32)
        gated[:len(g)] = g
        return dict(result=result, gated=gated, gated_count=len(g), did_reset=did_reset, edges=edges)


class BatchFrameRef:
    """B independent FrameRef filters behind the array shapes of vi_ekf_amd.FrameIntake"""

    def __init__(self, batch, num_features, params, keyframe_overlap_threshold=0.8):
        keys = ("x0", "P0", "Qx", "lam", "Qu", "P0_feat", "Qx_feat", "lam_feat", "cam_center", "focal_len", "q_b_c", "p_b_c",
                "q_b_u", "min_depth", "use_drag_term", "use_partial_update", "use_keyframe_reset")
        self.B, self.N = int(batch), int(num_features)
        self.r = [FrameRef(orc.OracleFilter(self.N).init(**{k: params[k] for k in keys}), keyframe_overlap_threshold)
                  for _ in range(self.B)]

    def propagate(self, u, dt):
        """u [K][B][6], dt [K][B]"""
        for k in range(u.shape[0]):
            for b, r in enumerate(self.r):
                r.f.propagate(u[k, b], dt[k, b])

    def intake(self, z, ids, R, depth=None, active=None):
        B, M = self.B, ids.shape[1]
        out = dict(result=np.full((B, M), SKIPPED, np.int32), gated=np.full((B, M), -1, np.int32), gated_count=np.zeros(B, np.int32),
                   did_reset=np.zeros(B, np.uint8), edges=np.zeros((B, 17)))
        R = np.asarray(R, dtype=np.float64)
        for b, r in enumerate(self.r):
            if active is not None and not active[b]:
                continue
            Rb = R if R.ndim == 2 else R[b]
            o = r.intake(z[b], ids[b], Rb, None if depth is None else depth[b])
            for k in out:
                out[k][b] = o[k]
        return out

    def tracked(self):
        ids = np.full((self.B, self.N), -1, np.int32)
        ln = np.zeros(self.B, np.int32)
        for b, r in enumerate(self.r):
            t = r.tracked()
            ids[b, :len(t)], ln[b] = t, len(t)
        return ids, ln

    def state(self):
        """-> x [B][nx], P [B][n][n], len [B]"""
        return (np.stack([r.f.x.copy() for r in self.r]), np.stack([r.f.P.copy() for r in self.r]),
                np.array([r.f.len_features for r in self.r], np.int32))
