"""Python face of the device-resident node graph (include/viekf_node.h): the global pose and covariance of every filter of a
BatchVIEKF across keyframe resets -- the node, its covariance, the true node, the reset count and the keyframe trail in device
memory, fed by what FrameIntake.intake / BatchVIEKF.keyframe_reset report.  Plumbing only: the numbers come from
libviekf_hip.so (csrc/viekf_kernels_node.hpp); there is no CPU fallback.

Arguments are numpy arrays (host pointers, numpy results) or contiguous CUDA torch tensors on the batch's device (device
pointers, torch results), by the rules of BatchVIEKF._arg; one call takes one kind.  Calls without an input array take
`device=`.  With device tensors nothing crosses to the host.
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Companion

# every symbol include/viekf_node.h declares (tests check the library exports exactly these)
NODE_SYMBOLS = ["viekf_node_create", "viekf_node_destroy", "viekf_node_reset", "viekf_node_update", "viekf_node_global",
                "viekf_node_relative_truth", "viekf_node_global_error", "viekf_node_get", "viekf_node_set", "viekf_node_trail"]
MAX_TRAIL = 4096     # VIEKF_NODE_MAX_TRAIL


def _bind():
    L = capi.lib()
    if getattr(L, "_node_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.viekf_node_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.viekf_node_destroy.argtypes = [vp]
    L.viekf_node_reset.argtypes = [vp]
    L.viekf_node_update.argtypes = [vp, vp, vp, vp, i32, C.c_int]
    L.viekf_node_global.argtypes = [vp, vp, vp, C.c_int]
    L.viekf_node_relative_truth.argtypes = [vp, vp, vp, i32, C.c_int]
    L.viekf_node_global_error.argtypes = [vp, vp, i32, vp, vp, vp, C.c_int]
    L.viekf_node_get.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.viekf_node_set.argtypes = [vp, vp, vp, vp, vp, C.c_int]
    L.viekf_node_trail.argtypes = [vp, vp, vp, C.c_int]
    L._node_bound = True
    return L


class NodeGraph(Companion):
    """
        ng = NodeGraph(batch, trail_capacity=0)
        out = fi.intake(z, ids, R_pix)
        ng.update(out, x_true=truth)            # or ng.update(did_reset, edges)
        pose, cov = ng.global_pose()            # [B][7] {t, q}, [B][6][6] indexed [row, col], ordered [pos; att]
        diag = consistency(batch, ng.relative_truth(x_true))
    """

    _destroy = "viekf_node_destroy"

    def __init__(self, batch, trail_capacity=0):
        super().__init__(_bind(), batch)
        self.trail_capacity = int(trail_capacity)
        h = C.c_void_p()
        capi.check(self._L.viekf_node_create(batch._h, self.trail_capacity, C.byref(h)))
        self._h = h

    def _ldx(self, x_true):
        if len(x_true.shape) != 2:
            raise ValueError("x_true must be [B][ldx]")
        return int(x_true.shape[1])

    def reset(self):
        """identity nodes, zero covariance, count 0 (pairs with BatchVIEKF.reset / FrameIntake.reset)"""
        capi.check(self._L.viekf_node_reset(self._handle()))

    def update(self, out_or_did_reset, edges=None, x_true=None, sync=True):
        """the node's move for every filter that reset: the dict FrameIntake.intake returns, or did_reset [B] uint8 and
        edges [B][17]; x_true [B][ldx >= 10] (BatchSimulator.truth_state) moves the true node as well"""
        g = self.batch
        h = self._handle()
        if isinstance(out_or_did_reset, dict):
            if edges is not None:
                raise ValueError("edges come with the intake's dict")
            did_reset, edges = out_or_did_reset["did_reset"], out_or_did_reset["edges"]
        else:
            did_reset = out_or_did_reset
        if did_reset is None or edges is None:
            raise ValueError("did_reset and edges are both needed")
        g._keep = []
        pd, w = g._arg(did_reset, np.uint8, (g.B,), None)
        pe, w = g._arg(edges, np.float64, (g.B, 17), w)
        ldx = 0
        px = None
        if x_true is not None:
            ldx = self._ldx(x_true)
            px, w = g._arg(x_true, np.float64, (g.B, ldx), w)
        dev = w == capi.DEVICE
        self._ready(dev, sync)
        capi.check(self._L.viekf_node_update(h, pd, pe, px, ldx, w))
        if dev and not sync:
            self._pending = (did_reset, edges, x_true)
        self._done(dev, sync)

    def global_pose(self, device=False, sync=True, cov=True):
        """-> (pose [B][7] = node * {x[POS], x[ATT]}, cov [B][6][6] indexed [row, col]) of the live state; read-only, and P
        is read in whatever form it is in"""
        g = self.batch
        h = self._handle()
        pose, pp = self._empty((g.B, 7), np.float64, device)
        cv, pc = self._empty((g.B, 6, 6), np.float64, device) if cov else (None, None)
        self._ready(device, sync)
        capi.check(self._L.viekf_node_global(h, pp, pc, capi.DEVICE if device else capi.HOST))
        self._done(device, sync)
        if cv is not None:   # the ABI hands out column-major
            cv = cv.transpose(1, 2) if device else np.swapaxes(cv, 1, 2)
        return pose, cv

    def relative_truth(self, x_true, sync=True):
        """x_true [B][ldx] in the inertial frame -> the same in the current (true) node frame, which is what the filter
        estimates: the x_true of vi_ekf_amd.consistency"""
        g = self.batch
        h = self._handle()
        ldx = self._ldx(x_true)
        g._keep = []
        px, w = g._arg(x_true, np.float64, (g.B, ldx), None)
        dev = w == capi.DEVICE
        xr, pr = self._empty((g.B, ldx), np.float64, dev)
        self._ready(dev, sync)
        capi.check(self._L.viekf_node_relative_truth(h, px, pr, ldx, w))
        if dev and not sync:
            self._pending = (x_true,)
        self._done(dev, sync)
        return xr

    def global_error(self, x_true, sync=True):
        """-> dict(err [B][6] = [x_true[POS] - t ; x_true[ATT] [-] q], nees [B], info [B]) against the global pose and
        covariance"""
        g = self.batch
        h = self._handle()
        ldx = self._ldx(x_true)
        g._keep = []
        px, w = g._arg(x_true, np.float64, (g.B, ldx), None)
        dev = w == capi.DEVICE
        out = {}
        out["err"], pe = self._empty((g.B, 6), np.float64, dev)
        out["nees"], pn = self._empty((g.B,), np.float64, dev)
        out["info"], pi = self._empty((g.B,), np.int32, dev)
        self._ready(dev, sync)
        capi.check(self._L.viekf_node_global_error(h, px, ldx, pe, pn, pi, w))
        if dev and not sync:
            self._pending = (x_true,)
        self._done(dev, sync)
        return out

    def get(self, device=False):
        """-> dict(node [B][7], node_cov [B][36] column-major, true_node [B][7], count [B]): what set takes"""
        g = self.batch
        h = self._handle()
        out = {}
        out["node"], p0 = self._empty((g.B, 7), np.float64, device)
        out["node_cov"], p1 = self._empty((g.B, 36), np.float64, device)
        out["true_node"], p2 = self._empty((g.B, 7), np.float64, device)
        out["count"], p3 = self._empty((g.B,), np.int32, device)
        self._ready(device, True)
        capi.check(self._L.viekf_node_get(h, p0, p1, p2, p3, capi.DEVICE if device else capi.HOST))
        self._done(device, True)
        return out

    def set(self, node=None, node_cov=None, true_node=None, count=None):
        """write back what get returned (None skips an array)"""
        g = self.batch
        h = self._handle()
        g._keep = []
        p0, w = g._arg(node, np.float64, (g.B, 7), None)
        p1, w = g._arg(node_cov, np.float64, (g.B, 36), w)
        p2, w = g._arg(true_node, np.float64, (g.B, 7), w)
        p3, w = g._arg(count, np.int32, (g.B,), w)
        if w is None:
            return
        dev = w == capi.DEVICE
        self._ready(dev, True)
        capi.check(self._L.viekf_node_set(h, p0, p1, p2, p3, w))
        self._done(dev, True)

    def trail(self, device=False):
        """-> (nodes [B][cap][7], edges [B][cap][17]) as stored: reset k of a filter sits at k % cap"""
        g = self.batch
        h = self._handle()
        nodes, pn = self._empty((g.B, self.trail_capacity, 7), np.float64, device)
        edges, pe = self._empty((g.B, self.trail_capacity, 17), np.float64, device)
        self._ready(device, True)
        capi.check(self._L.viekf_node_trail(h, pn, pe, capi.DEVICE if device else capi.HOST))
        self._done(device, True)
        return nodes, edges
