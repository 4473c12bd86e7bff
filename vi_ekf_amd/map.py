"""Python face of the device-resident landmark map (include/viekf_map.h): every feature slot of every filter of a BatchVIEKF
as a 3-D position in metres with a 3x3 covariance, in the node frame and in the global frame; a store of them keyed by the
frame intake's feature ids, which outlives feature loss and keyframe resets; and the metric error against the landmark the
simulator drew a feature from.  Plumbing only: the numbers come from libviekf_hip.so (csrc/viekf_kernels_map.hpp); there is
no CPU fallback.

Arguments are numpy arrays (host pointers, numpy results) or contiguous CUDA torch tensors on the batch's device (device
pointers, torch results), by the rules of BatchVIEKF._arg; one call takes one kind.  Calls without an input array take
`device=`.  With device tensors nothing crosses to the host.  Covariances are [..][6]: the lower triangle in the order
xx, yx, yy, zx, zy, zz.
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Companion

# every symbol include/viekf_map.h declares (tests check the library exports exactly these)
MAP_SYMBOLS = ["viekf_map_create", "viekf_map_destroy", "viekf_map_reset", "viekf_map_landmarks", "viekf_map_update",
               "viekf_map_get", "viekf_map_set", "viekf_map_error"]
MAX_CAPACITY = 4096     # VIEKF_MAP_MAX_CAPACITY


def _bind():
    L = capi.lib()
    if getattr(L, "_map_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.viekf_map_create.argtypes = [vp, vp, vp, i32, C.POINTER(vp)]
    L.viekf_map_destroy.argtypes = [vp]
    L.viekf_map_reset.argtypes = [vp]
    L.viekf_map_landmarks.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.viekf_map_update.argtypes = [vp]
    L.viekf_map_get.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_map_set.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_map_error.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp, vp, vp, vp, C.c_int]
    L._map_bound = True
    return L


class LandmarkMap(Companion):
    """
        lm = LandmarkMap(batch, frame=fi, node=ng, capacity=256)
        out = fi.intake(z, ids, R_pix)
        ng.update(out, x_true=truth)
        lm.update()                                   # after the node's move of the same frame
        live = lm.landmarks()                         # pos_node, cov_node, pos_global, cov_global of every slot
        cloud = lm.get()                              # ids, pos, cov, n_obs, node_count [B][capacity]
        err = lm.error(landmarks, frame_ids, landmark)
    """

    _destroy = "viekf_map_destroy"
    _STORE = (("ids", np.int32, ()), ("pos", np.float64, (3,)), ("cov", np.float64, (6,)), ("n_obs", np.int32, ()),
              ("node_count", np.int32, ()))

    def __init__(self, batch, frame=None, node=None, capacity=0):
        super().__init__(_bind(), batch)
        self.frame, self.node, self.capacity = frame, node, int(capacity)   # (both stay referenced: they must outlive the map)
        h = C.c_void_p()
        capi.check(self._L.viekf_map_create(batch._h, frame._handle() if frame is not None else None,
                                            node._handle() if node is not None else None, self.capacity, C.byref(h)))
        self._h = h

    def reset(self):
        """every entry of the store empty (pairs with BatchVIEKF.reset / FrameIntake.reset / NodeGraph.reset)"""
        capi.check(self._L.viekf_map_reset(self._handle()))

    def landmarks(self, device=False, sync=True, want=("pos_node", "cov_node", "pos_global", "cov_global")):
        """-> dict(pos_node [B][N][3], cov_node [B][N][6], pos_global, cov_global) of the live state: NaN for a slot past
        len_features or with a rho that is not finite and > 0.  Read-only on the batch."""
        g = self.batch
        h = self._handle()
        out, ptr = {}, []
        for k in ("pos_node", "cov_node", "pos_global", "cov_global"):
            if k in want:
                out[k], p = self._empty((g.B, g.N, 3 if k.startswith("pos") else 6), np.float64, device)
            else:
                p = None
            ptr.append(p)
        self._ready(device, sync)
        capi.check(self._L.viekf_map_landmarks(h, ptr[0], ptr[1], ptr[2], ptr[3], capi.DEVICE if device else capi.HOST))
        self._done(device, sync)
        return out

    def update(self, sync=False):
        """every valid tracked slot into the store, entry id % capacity (the larger id wins a shared residue).  Call it after
        NodeGraph.update of the same frame.  It takes no array, so it is only queued on the batch's stream, behind the
        intake's and the node graph's work; sync=True waits for it."""
        capi.check(self._L.viekf_map_update(self._handle()))
        if sync:
            self.batch.sync()

    def get(self, device=False):
        """-> dict(ids [B][cap] (-1: empty), pos [B][cap][3], cov [B][cap][6], n_obs [B][cap], node_count [B][cap]): the
        store as held, which is what set takes"""
        g = self.batch
        h = self._handle()
        out, ptr = {}, []
        for k, dt, tail in self._STORE:
            out[k], p = self._empty((g.B, self.capacity) + tail, dt, device)
            ptr.append(p)
        self._ready(device, True)
        capi.check(self._L.viekf_map_get(h, *ptr, capi.DEVICE if device else capi.HOST))
        self._done(device, True)
        return out

    def set(self, ids=None, pos=None, cov=None, n_obs=None, node_count=None):
        """write back what get returned (None skips an array)"""
        g = self.batch
        h = self._handle()
        g._keep = []
        given = dict(ids=ids, pos=pos, cov=cov, n_obs=n_obs, node_count=node_count)
        ptr, w = [], None
        for k, dt, tail in self._STORE:
            p, w = g._arg(given[k], dt, (g.B, self.capacity) + tail, w)
            ptr.append(p)
        if w is None:
            return
        dev = w == capi.DEVICE
        self._ready(dev, True)
        capi.check(self._L.viekf_map_set(h, *ptr, w))
        self._done(dev, True)

    def error(self, lm_true, frame_ids, landmark, sync=True):
        """lm_true [L][3] or [B][L][3]; frame_ids, landmark [B][M] as BatchSimulator.camera returns ids and landmark ->
        dict(err_node [B][N][3], nees [B][N], info [B][N], err_global [B][N][3]); NaN (info 0) for a slot that is not valid,
        whose id is not in the frame or whose landmark is outside the field"""
        g = self.batch
        h = self._handle()
        if len(lm_true.shape) not in (2, 3) or len(frame_ids.shape) != 2:
            raise ValueError("lm_true must be [L][3] or [B][L][3], frame_ids and landmark [B][M]")
        per = len(lm_true.shape) == 3
        Ln, M = int(lm_true.shape[-2]), int(frame_ids.shape[1])
        g._keep = []
        pl, w = g._arg(lm_true, np.float64, ((g.B, Ln, 3) if per else (Ln, 3)), None)
        pf, w = g._arg(frame_ids, np.int32, (g.B, M), w)
        pk, w = g._arg(landmark, np.int32, (g.B, M), w)
        dev = w == capi.DEVICE
        out = {}
        out["err_node"], p0 = self._empty((g.B, g.N, 3), np.float64, dev)
        out["nees"], p1 = self._empty((g.B, g.N), np.float64, dev)
        out["info"], p2 = self._empty((g.B, g.N), np.int32, dev)
        out["err_global"], p3 = self._empty((g.B, g.N, 3), np.float64, dev)
        self._ready(dev, sync)
        capi.check(self._L.viekf_map_error(h, pl, int(per), Ln, pf, pk, M, p0, p1, p2, p3, w))
        if dev and not sync:
            self._pending = (lm_true, frame_ids, landmark)
        self._done(dev, sync)
        return out
