"""Python face of the device-resident flight recorder (include/viekf_rec.h): the estimated and the true pose of every filter
of a BatchVIEKF on every frame of a run, kept in device memory with up to eight scalar channels per filter and frame, and the
run judged there -- ATE after alignment in yaw and translation (or none, or SE(3)), RPE over a frame spacing, the ensemble's
pose error per frame, the channels' statistics (the ANEES when a channel holds a NEES).  Plumbing only: the numbers come from
libviekf_hip.so (csrc/viekf_kernels_rec.hpp); there is no CPU fallback.

Arguments are numpy arrays (host pointers, numpy results) or contiguous CUDA torch tensors on the batch's device (device
pointers, torch results), by the rules of BatchVIEKF._arg; one call takes one kind.  Calls without an input array take
`device=`.  With device tensors nothing crosses to the host.
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Companion

# every symbol include/viekf_rec.h declares (tests check the library exports exactly these)
REC_SYMBOLS = ["viekf_rec_create", "viekf_rec_destroy", "viekf_rec_reset", "viekf_rec_count", "viekf_rec_push", "viekf_rec_get",
               "viekf_rec_trajectory_error", "viekf_rec_pose_ensemble", "viekf_rec_channels"]
MAX_FRAMES = 4096       # VIEKF_REC_MAX_FRAMES
MAX_CHANNELS = 8        # VIEKF_REC_MAX_CHANNELS
ALIGN = {"none": 0, "yaw": 1, "se3": 2}


def _bind():
    L = capi.lib()
    if getattr(L, "_rec_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.viekf_rec_create.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.viekf_rec_destroy.argtypes = [vp]
    L.viekf_rec_reset.argtypes = [vp]
    L.viekf_rec_count.argtypes = [vp, C.POINTER(i32)]
    L.viekf_rec_push.argtypes = [vp, C.c_double, vp, vp, i32, vp, vp, C.c_int]
    L.viekf_rec_get.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_rec_trajectory_error.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_rec_pose_ensemble.argtypes = [vp, i32, i32, vp, C.c_int]
    L.viekf_rec_channels.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.c_int]
    L._rec_bound = True
    return L


class FlightRecorder(Companion):
    """
        fr = FlightRecorder(batch, capacity=256, channels=1)
        pose, _ = ng.global_pose(device=True, cov=False)
        err = ng.global_error(truth)
        fr.push(pose, truth, chan=err["nees"][:, None], stamp=t)       # every frame; nothing crosses to the host
        run = fr.trajectory_error(align="yaw", delta=1, device=True)  # ate_pos, ate_att, rpe_pos, rpe_att, align_pose, n_used
        ens = fr.pose_ensemble(device=True)                           # [T][4] = n, rms position, rms attitude, max position
        ch = fr.channels(lo, hi, device=True)                         # per_frame [T][K][5], per_filter [B][K][5]
    """

    _destroy = "viekf_rec_destroy"

    def __init__(self, batch, capacity, channels=0):
        super().__init__(_bind(), batch)
        self.capacity, self.n_channels = int(capacity), int(channels)   # (channels is the method)
        h = C.c_void_p()
        capi.check(self._L.viekf_rec_create(batch._h, self.capacity, self.n_channels, C.byref(h)))
        self._h = h

    @property
    def count(self):
        """frames held: the one frame index of the whole recorder, kept on the host"""
        n = C.c_int32()
        capi.check(self._L.viekf_rec_count(self._handle(), C.byref(n)))
        return n.value

    def reset(self):
        """count -> 0"""
        capi.check(self._L.viekf_rec_reset(self._handle()))

    def _range(self, first, last):
        first, last = int(first), self.count if last is None else int(last)
        if not 0 <= first <= last <= self.count:
            raise ValueError("need 0 <= first <= last <= count")
        return first, last

    def push(self, est_pose, x_true, chan=None, mask=None, stamp=0.0, sync=True):
        """appends one frame: est_pose [B][7] (NodeGraph.global_pose), x_true [B][ldx >= 10] (BatchSimulator.truth_state), chan
        [B][channels] (None exactly when the recorder has no channels), mask [B] uint8 or None.  A filter's frame is valid when
        its mask says so and its 14 pose numbers are finite: the device decides.  A full recorder raises and keeps every bit."""
        g = self.batch
        h = self._handle()
        if len(x_true.shape) != 2:
            raise ValueError("x_true must be [B][ldx]")
        ldx = int(x_true.shape[1])
        g._keep = []
        pe, w = g._arg(est_pose, np.float64, (g.B, 7), None)
        px, w = g._arg(x_true, np.float64, (g.B, ldx), w)
        # (the library refuses chan without channels and channels without chan)
        pc, w = g._arg(chan, np.float64, (g.B, self.n_channels) if self.n_channels or chan is None else tuple(chan.shape), w)
        pm, w = g._arg(mask, np.uint8, (g.B,), w)
        dev = w == capi.DEVICE
        self._ready(dev, sync)
        capi.check(self._L.viekf_rec_push(h, float(stamp), pe, px, ldx, pc, pm, w))
        if dev and not sync:
            self._pending = (est_pose, x_true, chan, mask)
        self._done(dev, sync)

    def get(self, device=False):
        """-> dict(est [B][T][7], tru [B][T][7], valid [B][T] uint8, chan [T][B][channels], stamps [T]) with T = count: what was
        pushed, bit for bit"""
        g = self.batch
        h = self._handle()
        T = self.count
        out = {}
        out["est"], p0 = self._empty((g.B, T, 7), np.float64, device)
        out["tru"], p1 = self._empty((g.B, T, 7), np.float64, device)
        out["valid"], p2 = self._empty((g.B, T), np.uint8, device)
        out["chan"], p3 = self._empty((T, g.B, self.n_channels), np.float64, device)
        out["stamps"], p4 = self._empty((T,), np.float64, device)
        self._ready(device, True)
        capi.check(self._L.viekf_rec_get(h, p0, p1, p2, p3, p4, capi.DEVICE if device else capi.HOST))
        self._done(device, True)
        return out

    def trajectory_error(self, align="yaw", first=0, last=None, delta=1, device=False, sync=True):
        """-> dict(ate_pos [B], ate_att [B] (radians), rpe_pos [B], rpe_att [B], align_pose [B][7], n_used [B][2] = frames and
        pairs) of every filter over its valid frames first <= k < last, aligned by "none", "yaw" (yaw and translation, the four
        directions a visual-inertial filter cannot observe) or "se3"; RPE over the pairs (k, k + delta).  NaN where there is
        no frame / no pair."""
        g = self.batch
        h = self._handle()
        if align not in ALIGN:
            raise ValueError("align must be one of %s" % sorted(ALIGN))
        first, last = self._range(first, last)
        out, ptr = {}, []
        for k, dt, tail in (("ate_pos", np.float64, ()), ("ate_att", np.float64, ()), ("rpe_pos", np.float64, ()),
                            ("rpe_att", np.float64, ()), ("align_pose", np.float64, (7,)), ("n_used", np.int32, (2,))):
            out[k], p = self._empty((g.B,) + tail, dt, device)
            ptr.append(p)
        self._ready(device, sync)
        capi.check(self._L.viekf_rec_trajectory_error(h, ALIGN[align], first, last, int(delta), *ptr, capi.DEVICE if device else capi.HOST))
        self._done(device, sync)
        return out

    def pose_ensemble(self, first=0, last=None, device=False, sync=True):
        """-> [T'][4] = {n, rms |p_t - p_e|, rms |q_t [-] q_e|, max |p_t - p_e|} per frame over the filters valid on it,
        unaligned; NaN where n = 0"""
        h = self._handle()
        first, last = self._range(first, last)
        out, p = self._empty((last - first, 4), np.float64, device)
        self._ready(device, sync)
        capi.check(self._L.viekf_rec_pose_ensemble(h, first, last, p, capi.DEVICE if device else capi.HOST))
        self._done(device, sync)
        return out

    def channels(self, lo=None, hi=None, first=0, last=None, device=False, sync=True):
        """-> dict(per_frame [T'][K][5], per_filter [B][K][5]), each {n finite, mean, max, fraction < lo[j], fraction > hi[j]}:
        per_frame over the batch (its mean is the ANEES of a NEES channel), per_filter over the frames.  lo / hi [K] (the
        caller's chi-square bounds) or None: fraction 0.  They decide whether the call takes host or device arrays; without
        them `device=` does."""
        g = self.batch
        h = self._handle()
        first, last = self._range(first, last)
        K = self.n_channels
        g._keep = []
        pl, w = g._arg(lo, np.float64, (K,), None)
        ph, w = g._arg(hi, np.float64, (K,), w)
        dev = bool(device) if w is None else w == capi.DEVICE
        out = {}
        out["per_frame"], p0 = self._empty((last - first, K, 5), np.float64, dev)
        out["per_filter"], p1 = self._empty((g.B, K, 5), np.float64, dev)
        self._ready(dev, sync)
        capi.check(self._L.viekf_rec_channels(h, first, last, pl, ph, p0, p1, capi.DEVICE if dev else capi.HOST))
        if dev and not sync:
            self._pending = (lo, hi)
        self._done(dev, sync)
        return out
