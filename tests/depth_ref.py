"""Restatement of the frame intake's depth step (viekf_frame_intake_depth, include/viekf_depth.h) over the oracle filters of
tests/frame_ref.py: the DEPTH measurement the reference's color_image_callback queues behind every FEAT it queued
(src/vi_ekf_ros.cpp:301-303), applied after the frame's FEAT updates (the kept deviation), last entry first, with
OracleFilter.update(DEPTH, ..., active = use_depth, id).  Only tests/ import this."""
import numpy as np

from oracle import oracle as orc

SKIPPED = -1


def is_measurement(gid, feat_result, depth):
    """an entry of a frame gets a DEPTH where its id is real, the FEAT was queued (SUCCESS or GATED) and the depth is finite"""
    return gid >= 0 and feat_result in (orc.MEAS_SUCCESS, orc.MEAS_GATED) and np.isfinite(depth)


def intake_depth(ref, ids, depth, feat_result, R, use_depth=True, active=None, stale=()):
    """ref: a frame_ref.BatchFrameRef just after its intake() of the same frame; ids [B][M], depth [B][M], feat_result [B][M]
    (that intake's result); R a float, [B] or [B][M]; stale: filters whose table is stale (left alone, ids >= 0 INVALID)
    -> result [B][M]"""
    B, M = ids.shape
    R = np.asarray(R, dtype=np.float64)
    result = np.full((B, M), SKIPPED, dtype=np.int32)
    for b, r in enumerate(ref.r):
        if active is not None and not active[b]:
            continue
        if b in stale:
            result[b][ids[b] >= 0] = orc.MEAS_INVALID
            continue
        f = r.f
        for i in reversed(range(M)):
            if not is_measurement(int(ids[b, i]), int(feat_result[b, i]), depth[b, i]):
                continue
            if f.global_to_local_feature_id(int(ids[b, i])) < 0:
                result[b, i] = orc.MEAS_INVALID
                continue
            Rbi = float(R if R.ndim == 0 else (R[b] if R.ndim == 1 else R[b, i]))
            result[b, i] = f.update(orc.DEPTH, np.array([depth[b, i]]), np.array([[Rbi]]), bool(use_depth), int(ids[b, i]))
    return result
