"""Python face of the device-resident frame intake (include/viekf_frame.h): what VIEKF_ROS::color_image_callback does with
a tracked frame -- keep_only_features and its keyframe test, the id -> slot lookup, init_feature for new ids, the frame's
FEAT updates in the reference's order -- for every filter of a BatchVIEKF, with the feature-id tables in device memory.
Plumbing only: the numbers come from libviekf_hip.so (csrc/viekf_kernels_frame.hpp); there is no CPU fallback.

Arguments are numpy arrays (host pointers, numpy results) or contiguous CUDA torch tensors on the batch's device (device
pointers, torch results), by the rules of BatchVIEKF._arg; one call takes one kind.  With device tensors nothing crosses to
the host: z, ids and depth are exactly what BatchSimulator.camera(device=True) and KLTTracker hand out.
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Companion, is_torch, r_colmajor

# every symbol include/viekf_frame.h declares (tests check the library exports exactly these)
FRAME_SYMBOLS = ["viekf_frame_create", "viekf_frame_destroy", "viekf_frame_reset", "viekf_frame_set_tracked",
                 "viekf_frame_tracked", "viekf_frame_intake"]
MAX_M = 4096     # VIEKF_FRAME_MAX_M


class FrameIntake(Companion):
    """
        fi = FrameIntake(batch)
        out = fi.intake(z, ids, R_pix)         # dict(result [B][M], gated [B][M], gated_count [B], did_reset [B], edges [B][17])
        ids, ln = fi.tracked()                  # [B][N] -1 padded in slot order (BatchSimulator.truth_state takes it), [B]
    """

    _destroy = "viekf_frame_destroy"

    def __init__(self, batch):
        super().__init__(capi.lib(), batch)
        h = C.c_void_p()
        capi.check(self._L.viekf_frame_create(batch._h, C.byref(h)))
        self._h = h

    def reset(self):
        """no ids tracked, no keyframe list (pairs with BatchVIEKF.reset)"""
        capi.check(self._L.viekf_frame_reset(self._handle()))

    def set_tracked(self, ids):
        """adopt a state written with BatchVIEKF.set_state / init_feature: ids [B][N], row b = len_features[b] distinct
        ids >= 0, then -1 (host arrays are checked)"""
        g = self.batch
        h = self._handle()
        g._keep = []
        p, w = g._arg(ids, np.int32, (g.B, g.N), None)
        self._ready(w == capi.DEVICE, True)
        capi.check(self._L.viekf_frame_set_tracked(h, p, w))
        self._done(w == capi.DEVICE, True)

    def tracked(self, device=False):
        """-> (ids [B][N] -1 padded in slot order, len [B])"""
        g = self.batch
        h = self._handle()
        ids, pi = self._empty((g.B, g.N), np.int32, device)
        ln, pl = self._empty((g.B,), np.int32, device)
        self._ready(device, True)
        capi.check(self._L.viekf_frame_tracked(h, pi, pl, capi.DEVICE if device else capi.HOST))
        self._done(device, True)
        return ids, ln

    def intake(self, z, ids, R, depth=None, active=None, sync=True):
        """one frame per filter: z [B][M][2] NaN padded, ids [B][M] -1 padded, R (2,2), (B,2,2) or (B,M,2,2) indexed
        [row, col], depth [B][M] or None, active [B] uint8 or None
        -> dict(result [B][M], gated [B][M], gated_count [B], did_reset [B], edges [B][17]), where the inputs live.
        With device tensors and sync=False the call returns once its work is queued on the batch's stream: inputs and
        outputs are then the caller's to order (batch.sync(), or a stream shared with torch)."""
        g = self.batch
        h = self._handle()
        g._keep = []
        B = g.B
        if len(ids.shape) != 2:
            raise ValueError("ids must be [B][M]")
        M = int(ids.shape[1])
        pz, w = g._arg(z, np.float64, (B, M, 2), None)
        pi, w = g._arg(ids, np.int32, (B, M), w)
        Rc, r_mode = r_colmajor(R, B, M)
        pR, w = g._arg(Rc, np.float64, tuple(Rc.shape), w)
        pd, w = g._arg(depth, np.float64, (B, M), w)
        pa, w = g._arg(active, np.uint8, (B,), w)
        dev = w == capi.DEVICE
        out = {}
        out["result"], pres = self._empty((B, M), np.int32, dev)
        out["gated"], pg = self._empty((B, M), np.int32, dev)
        out["gated_count"], pgc = self._empty((B,), np.int32, dev)
        out["did_reset"], pdr = self._empty((B,), np.uint8, dev)
        out["edges"], pe = self._empty((B, 17), np.float64, dev)
        self._ready(dev, sync)
        capi.check(self._L.viekf_frame_intake(h, M, pz, pi, pd, pR, r_mode, pa, pres, pg, pgc, pdr, pe, w))
        if dev and not sync:
            self._pending = (z, ids, Rc, depth, active)   # (re-laid-out R must outlive the queued work)
        self._done(dev, sync)
        return out

    def intake_depth(self, out_or_result, ids, depth, R, use_depth=True, active=None):
        """the frame's DEPTH measurements, behind intake() of the same frame (viekf_frame_intake_depth, include/viekf_depth.h):
        out_or_result = what intake() returned, or its "result" [B][M]; ids [B][M] and depth [B][M] as given to intake();
        R the DEPTH variance: a float, [B] or [B][M]; use_depth False = inactive measurements (fix_depth only); active [B]
        uint8 or None -> result [B][M], where the inputs live"""
        g = self.batch
        h = self._handle()
        g._keep = []
        B = g.B
        fres = out_or_result["result"] if isinstance(out_or_result, dict) else out_or_result
        if len(ids.shape) != 2:
            raise ValueError("ids must be [B][M]")
        M = int(ids.shape[1])
        if not is_torch(R):
            R = np.asarray(R, dtype=np.float64)
            if is_torch(depth):                                # (a plain number beside device tensors)
                import torch
                R = torch.as_tensor(R, dtype=torch.float64, device=depth.device).contiguous()
        r_mode = {(): 0, (1,): 0, (B,): 1, (B, M): 2}.get(tuple(R.shape))
        if r_mode is None:
            raise ValueError("R must be a scalar, [B] or [B][M]")
        if r_mode == 0:
            R = R.reshape(1)
        pi, w = g._arg(ids, np.int32, (B, M), None)
        pd, w = g._arg(depth, np.float64, (B, M), w)
        pf, w = g._arg(fres, np.int32, (B, M), w)
        pR, w = g._arg(R, np.float64, tuple(R.shape), w)
        pa, w = g._arg(active, np.uint8, (B,), w)
        dev = w == capi.DEVICE
        result, pres = self._empty((B, M), np.int32, dev)
        self._ready(dev, True)
        capi.check(self._L.viekf_frame_intake_depth(h, M, pi, pd, pf, pR, r_mode, 1 if use_depth else 0, pa, pres, w))
        self._done(dev, True)
        return result

    def intake_pixel_vel(self, out_or_result, ids, zdot, gyro, R, gyro_var=0.0, use_pixel_vel=True, active=None):
        """the frame's PIXEL_VEL measurements, behind intake() (and intake_depth()) of the same frame
        (viekf_frame_intake_pixel_vel, include/viekf_pixvel.h): out_or_result = what intake() returned, or its "result" [B][M];
        ids [B][M] as given to intake(); zdot [B][M][2] the flow (pixel_flow), NaN where there is none; gyro [B][3] the raw gyro
        sample; R (2,2), (B,2,2) or (B,M,2,2) indexed [row, col]; use_pixel_vel False = inactive measurements (fix_depth only);
        active [B] uint8 or None -> result [B][M], where the inputs live"""
        g = self.batch
        h = self._handle()
        g._keep = []
        B = g.B
        fres = out_or_result["result"] if isinstance(out_or_result, dict) else out_or_result
        if len(ids.shape) != 2:
            raise ValueError("ids must be [B][M]")
        M = int(ids.shape[1])
        pi, w = g._arg(ids, np.int32, (B, M), None)
        pd, w = g._arg(zdot, np.float64, (B, M, 2), w)
        pf, w = g._arg(fres, np.int32, (B, M), w)
        pg, w = g._arg(gyro, np.float64, (B, 3), w)
        Rc, r_mode = r_colmajor(R, B, M)
        pR, w = g._arg(Rc, np.float64, tuple(Rc.shape), w)
        pa, w = g._arg(active, np.uint8, (B,), w)
        dev = w == capi.DEVICE
        result, pres = self._empty((B, M), np.int32, dev)
        self._ready(dev, True)
        capi.check(self._L.viekf_frame_intake_pixel_vel(h, M, pi, pd, pf, pg, pR, r_mode, float(gyro_var), 1 if use_pixel_vel else 0,
                                                        pa, pres, w))
        self._done(dev, True)
        return result
