"""Python face of the device-resident camera model (include/viekf_cam.h): radial-tangential lens distortion (k1, k2, p1, p2,
the `distortion:` key of a camera's parameter file) for `batch` cameras -- points and their measurement noise from raw to
ideal pixels, the mask that keeps a tracker inside the model, whole images warped either way.  Plumbing only: every number
comes from libviekf_hip.so (csrc/viekf_cam.hip); there is no CPU fallback, and the header is the specification.

Arguments are numpy arrays (host pointers, numpy results) or contiguous CUDA torch tensors on the model's device (device
pointers, torch results, nothing crossing to the host); one call takes one kind.  With tensors and sync=False a call
returns once its work is queued on the model's stream: inputs and outputs are then the caller's to order (sync(), or
set_stream with a stream shared with torch).

The real-camera route -- the tracker reports raw pixels, the filter wants the pinhole's:

    cam = CameraModel(B)
    cam.load_yaml("ocam.yaml", "ekf.yaml")             # raw camera + distortion; the filter's focal_len / cam_center
    trk.set_mask(cam.valid_mask(640, 480))             # keep the tracker inside the model
    feats, ids, cnt = trk.load_image(frames)          # raw pixels
    depth = trk.sample_depth(depth_mm, min_depth)      # read at the RAW pixels, before undistorting
    z, R_out, st = cam.undistort_points(feats, R_pix)
    out = intake.intake(z, ids, R_out, depth=depth)

and the simulator's ideal frames as a real lens would give them: cam.warp(img, "distort", depth=depth_mm).
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Handle, empty, is_torch, r_colmajor

# every symbol include/viekf_cam.h declares (tests check the library exports exactly these)
CAM_SYMBOLS = [
    "viekf_cam_intrinsics_default", "viekf_cam_load_yaml", "viekf_cam_create", "viekf_cam_destroy", "viekf_cam_dims",
    "viekf_cam_set_stream", "viekf_cam_sync", "viekf_cam_set_intrinsics", "viekf_cam_get_intrinsics",
    "viekf_cam_distort_points", "viekf_cam_undistort_points", "viekf_cam_valid_mask", "viekf_cam_warp",
]
MAX_M = 4096                                   # VIEKF_CAM_MAX_M
OK, PADDING, OUT_OF_MODEL = 0, 1, 2            # VIEKF_CAM_OK ...
RECTIFY, DISTORT = 0, 1                        # VIEKF_CAM_RECTIFY, VIEKF_CAM_DISTORT
_DIRECTIONS = {"rectify": RECTIFY, "distort": DISTORT, RECTIFY: RECTIFY, DISTORT: DISTORT}


class Intrinsics(C.Structure):
    """struct viekf_cam_intrinsics (include/viekf_cam.h)"""
    _fields_ = [("focal", C.c_double * 2), ("center", C.c_double * 2), ("dist", C.c_double * 4),
                ("out_focal", C.c_double * 2), ("out_center", C.c_double * 2), ("min_det", C.c_double)]

    def to_dict(self):
        return dict(focal=list(self.focal), center=list(self.center), dist=list(self.dist), out_focal=list(self.out_focal),
                    out_center=list(self.out_center), min_det=self.min_det)


def _bind():
    L = capi.lib()
    if getattr(L, "_cam_bound", False):
        return L
    vp, i32, KP = C.c_void_p, C.c_int32, C.POINTER(Intrinsics)
    L.viekf_cam_intrinsics_default.argtypes = [KP]
    L.viekf_cam_load_yaml.argtypes = [C.c_char_p, C.c_char_p, KP]
    L.viekf_cam_create.argtypes = [i32, i32, C.POINTER(vp)]
    L.viekf_cam_destroy.argtypes = [vp]
    L.viekf_cam_dims.argtypes = [vp, C.POINTER(i32), C.POINTER(i32)]
    L.viekf_cam_set_stream.argtypes = [vp, vp]
    L.viekf_cam_sync.argtypes = [vp]
    L.viekf_cam_set_intrinsics.argtypes = [vp, vp, i32]
    L.viekf_cam_get_intrinsics.argtypes = [vp, vp, vp]
    L.viekf_cam_distort_points.argtypes = [vp, i32, vp, vp, vp, C.c_int]
    L.viekf_cam_undistort_points.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, C.c_int]
    L.viekf_cam_valid_mask.argtypes = [vp, i32, i32, vp, C.c_int]
    L.viekf_cam_warp.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, i32, C.c_int]
    L._cam_bound = True
    return L


def load_yaml(path, params_path=None):
    """viekf_cam_load_yaml -> Intrinsics: cam_center, focal_len and distortion (absent: zeros) of `path`; out_focal /
    out_center from `params_path`, or from `path` itself.  Needs no device."""
    k = Intrinsics()
    capi.check(_bind().viekf_cam_load_yaml(str(path).encode(), None if params_path is None else str(params_path).encode(), C.byref(k)))
    return k


class CameraModel(Handle):
    """`batch` cameras on one device, all with one intrinsics set or each with its own (the module docstring has the route).

        cam = CameraModel(B)
        cam.set_intrinsics(focal=[533.0, 533.5], center=[316.7, 230.7], dist=[-0.2834, 0.074, 1.9e-4, 1.8e-5])
        z_raw, J = cam.distort_points(z, jacobian=True)
        z, R_out, status = cam.undistort_points(z_raw, R)
    """

    _destroy = "viekf_cam_destroy"

    def __init__(self, batch, device=0):
        super().__init__(_bind())
        self.B, self.device = int(batch), int(device)
        h = C.c_void_p()
        capi.check(self._L.viekf_cam_create(self.B, self.device, C.byref(h)))
        self._h = h
        self._pending = None

    # -- handle ---------------------------------------------------------------------------------------------------------
    def set_stream(self, stream):
        """a hipStream_t handle (int, e.g. torch.cuda.current_stream().cuda_stream) or None for the null stream"""
        capi.check(self._L.viekf_cam_set_stream(self._handle(), None if stream is None else C.c_void_p(int(stream))))

    def sync(self):
        capi.check(self._L.viekf_cam_sync(self._handle()))
        self._pending = None

    @property
    def sets(self):
        """1 while one intrinsics set is shared, batch otherwise"""
        n = C.c_int32()
        capi.check(self._L.viekf_cam_dims(self._handle(), None, C.byref(n)))
        return n.value

    def set_intrinsics(self, focal, center, dist=(0.0, 0.0, 0.0, 0.0), out_focal=None, out_center=None, min_det=0.0):
        """focal, center (of the raw image), dist = (k1, k2, p1, p2), out_focal / out_center (the pinhole the filter uses; None:
        the raw camera's own) and min_det: each one value for every camera, or one row per camera ([B][2], [B][4], [B]) --
        any per-camera argument makes the whole table per camera.  Host values only: the library derives r_valid on the host."""
        vals = dict(focal=focal, center=center, dist=dist, out_focal=focal if out_focal is None else out_focal,
                    out_center=center if out_center is None else out_center, min_det=min_det)
        cols = dict(focal=2, center=2, dist=4, out_focal=2, out_center=2, min_det=1)
        per = False
        for name, a in vals.items():
            if is_torch(a):
                if a.is_cuda:
                    raise ValueError("intrinsics are host memory: r_valid is derived on the host (got a CUDA tensor for %s)" % name)
                a = a.numpy()
            a = np.asarray(a, dtype=np.float64)
            vals[name] = a
            per |= a.ndim > (0 if cols[name] == 1 else 1)
        n = self.B if per else 1
        ks = (Intrinsics * n)()
        for name, a in vals.items():
            a = np.broadcast_to(a, (n,) if cols[name] == 1 else (n, cols[name]))
            for s in range(n):
                if cols[name] == 1:
                    setattr(ks[s], name, float(a[s]))
                else:
                    getattr(ks[s], name)[:] = [float(v) for v in a[s]]
        capi.check(self._L.viekf_cam_set_intrinsics(self._handle(), C.cast(ks, C.c_void_p), int(per)))

    def load_yaml(self, path, params_path=None, min_det=0.0):
        """one set for every camera from a parameter file (module-level load_yaml) -> the Intrinsics that were set"""
        k = load_yaml(path, params_path)
        k.min_det = float(min_det)
        capi.check(self._L.viekf_cam_set_intrinsics(self._handle(), C.cast(C.pointer(k), C.c_void_p), 0))
        return k

    def intrinsics(self):
        """-> (list of the sets as dicts, r_valid [sets]) as the library holds them"""
        n = self.sets
        ks, rv = (Intrinsics * n)(), np.empty(n)
        capi.check(self._L.viekf_cam_get_intrinsics(self._handle(), C.cast(ks, C.c_void_p), C.c_void_p(rv.ctypes.data)))
        return [k.to_dict() for k in ks], rv

    # -- arguments ------------------------------------------------------------------------------------------------------
    def _arg(self, a, dtype, shape, where, keep):
        """-> (pointer, where); BatchVIEKF._arg's rules: all arrays of one call live on the same side"""
        if a is None:
            return None, where
        if is_torch(a):
            import torch
            want = getattr(torch, np.dtype(dtype).name)
            if not a.is_cuda or a.dtype != want or not a.is_contiguous():
                raise ValueError("device arguments must be contiguous CUDA tensors of dtype %s" % want)
            if a.device.index != self.device:
                raise ValueError("device arguments must live on cuda:%d" % self.device)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("expected shape %s, got %s" % (tuple(shape), tuple(a.shape)))
            if where not in (None, capi.DEVICE):
                raise ValueError("cannot mix host and device arguments in one call")
            keep.append(a)
            return C.c_void_p(a.data_ptr()), capi.DEVICE
        arr = np.ascontiguousarray(a, dtype=dtype)
        if arr.shape != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (tuple(shape), arr.shape))
        if where not in (None, capi.HOST):
            raise ValueError("cannot mix host and device arguments in one call")
        keep.append(arr)
        return C.c_void_p(arr.ctypes.data), capi.HOST

    def _empty(self, shape, dtype, dev):
        return empty(shape, dtype, self.device if dev else None)

    def _ready(self, dev, sync):
        """device outputs come from torch's caching allocator and the inputs may still be in torch's queue, while the work
        runs on the model's stream (as BatchSimulator does)"""
        if dev and sync:
            import torch
            torch.cuda.synchronize(self.device)

    def _done(self, dev, sync, keep):
        if dev and sync:
            self.sync()
        elif dev:
            self._pending = keep                     # (re-laid-out inputs must outlive the queued work)

    @staticmethod
    def _points_shape(z):
        if len(z.shape) != 3 or int(z.shape[2]) != 2:
            raise ValueError("points must be [B][M][2]")
        return int(z.shape[1])

    # -- points ---------------------------------------------------------------------------------------------------------
    def distort_points(self, z, jacobian=False, sync=True):
        """ideal pixels z [B][M][2] (NaN padding stays NaN) -> raw pixels [B][M][2]; with jacobian=True also
        J = d z_raw / d z_ideal as [B][M][2][2] indexed [row, col]"""
        h, keep = self._handle(), []
        M = self._points_shape(z)
        pz, w = self._arg(z, np.float64, (self.B, M, 2), None, keep)
        dev = w == capi.DEVICE
        out, po = self._empty((self.B, M, 2), np.float64, dev)
        J, pj = self._empty((self.B, M, 2, 2), np.float64, dev) if jacobian else (None, None)
        self._ready(dev, sync)
        capi.check(self._L.viekf_cam_distort_points(h, M, pz, po, pj, w))
        self._done(dev, sync, keep)
        if not jacobian:
            return out
        return out, (J.transpose(-1, -2) if dev else np.swapaxes(J, -1, -2))     # (stored column-major)

    def undistort_points(self, z_raw, R=None, sync=True):
        """raw pixels z_raw [B][M][2] with NaN padding, R (2,2), (B,2,2) or (B,M,2,2) indexed [row, col] or None
        -> (z [B][M][2], R_out [B][M][2][2] indexed [row, col] or None, status [B][M] of OK / PADDING / OUT_OF_MODEL).
        R_out is a transposed view of the column-major array the library wrote, which is the array FrameIntake.intake and
        BatchVIEKF's updates pass on as it is: J_u R J_u^T per entry; the entry's input R where the status is not OK."""
        h, keep = self._handle(), []
        M = self._points_shape(z_raw)
        pz, w = self._arg(z_raw, np.float64, (self.B, M, 2), None, keep)
        pR, r_mode = None, 0
        if R is not None:
            Rc, r_mode = r_colmajor(R, self.B, M)
            pR, w = self._arg(Rc, np.float64, tuple(Rc.shape), w, keep)
        dev = w == capi.DEVICE
        z, po = self._empty((self.B, M, 2), np.float64, dev)
        st, ps = self._empty((self.B, M), np.int32, dev)
        Ro, pRo = self._empty((self.B, M, 2, 2), np.float64, dev) if R is not None else (None, None)
        self._ready(dev, sync)
        capi.check(self._L.viekf_cam_undistort_points(h, M, pz, pR, r_mode, po, pRo, ps, w))
        self._done(dev, sync, keep)
        if Ro is not None:
            Ro = Ro.transpose(-1, -2) if dev else np.swapaxes(Ro, -1, -2)
        return z, Ro, st

    # -- pixels ---------------------------------------------------------------------------------------------------------
    def valid_mask(self, width, height, device=False, sync=True):
        """255 where the raw pixel centre is inside the model, 0 elsewhere: [height][width] while one set is shared,
        [B][height][width] otherwise -- what KLTTracker.set_mask takes"""
        h = self._handle()
        W, H = int(width), int(height)
        shape = (H, W) if self.sets == 1 else (self.B, H, W)
        m, pm = self._empty(shape, np.uint8, device)
        self._ready(device, sync)
        capi.check(self._L.viekf_cam_valid_mask(h, W, H, pm, capi.DEVICE if device else capi.HOST))
        self._done(device, sync, [])
        return m

    def warp(self, src, direction, depth=None, fill=0, sync=True):
        """src [B][H][W] uint8 and, optionally, its depth image [B][H][W] float32 (mm, +inf = none).  direction "rectify": src is
        the raw image, the result the ideal one; "distort": src is ideal (BatchSimulator.render's), the result what a real lens
        would give.  Grey is bilinear, depth nearest neighbour; `fill` and +inf outside the source or the model.
        -> dst, or (dst, dst_depth) with depth."""
        h, keep = self._handle(), []
        if direction not in _DIRECTIONS:
            raise ValueError("direction must be 'rectify' or 'distort'")
        if len(src.shape) != 3 or int(src.shape[0]) != self.B:
            raise ValueError("src must be [B][H][W]")
        H, W = int(src.shape[1]), int(src.shape[2])
        ps, w = self._arg(src, np.uint8, (self.B, H, W), None, keep)
        pd, w = self._arg(depth, np.float32, (self.B, H, W), w, keep)
        dev = w == capi.DEVICE
        dst, po = self._empty((self.B, H, W), np.uint8, dev)
        dd, pdd = self._empty((self.B, H, W), np.float32, dev) if depth is not None else (None, None)
        self._ready(dev, sync)
        capi.check(self._L.viekf_cam_warp(h, _DIRECTIONS[direction], W, H, ps, po, pd, pdd, int(fill), w))
        self._done(dev, sync, keep)
        return dst if depth is None else (dst, dd)
