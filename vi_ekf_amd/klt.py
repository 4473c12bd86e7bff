"""Python face of the batched KLT feature tracker (include/viekf_klt.h): the reference's KLT_Tracker for `batch`
cameras, plus `track_frame`, the glue of VIEKF_ROS::color_image_callback (reference src/vi_ekf_ros.cpp:254-314).
Plumbing only -- every pixel is processed in libviekf_hip.so (csrc/viekf_klt.hip); there is no CPU fallback.

Frames and masks may be numpy arrays (host) or torch tensors on the tracker's device (no copy through the host).
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Handle, is_torch

# every symbol include/viekf_klt.h declares (tests check the library exports exactly these)
KLT_SYMBOLS = [
    "viekf_klt_create", "viekf_klt_destroy", "viekf_klt_dims", "viekf_klt_reset", "viekf_klt_set_stream", "viekf_klt_sync",
    "viekf_klt_set_mask", "viekf_klt_load_image", "viekf_klt_drop_features", "viekf_klt_sample_depth",
    "viekf_klt_get_points", "viekf_klt_get_level",
]
MAX_FEATURES = 1024
FEAT, DEPTH = 6, 8          # viekf_meas_type (include/viekf.h)


def _bind():
    L = capi.lib()
    if getattr(L, "_klt_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.viekf_klt_create.argtypes = [i32, i32, i32, i32, i32, i32, i32, C.POINTER(vp)]
    L.viekf_klt_destroy.argtypes = [vp]
    L.viekf_klt_dims.argtypes = [vp] + [C.POINTER(i32)] * 6
    L.viekf_klt_reset.argtypes = [vp]
    L.viekf_klt_set_stream.argtypes = [vp, vp]
    L.viekf_klt_sync.argtypes = [vp]
    L.viekf_klt_set_mask.argtypes = [vp, vp, i32, C.c_int]
    L.viekf_klt_load_image.argtypes = [vp, vp, i32, vp, vp, vp, vp, C.c_int]
    L.viekf_klt_drop_features.argtypes = [vp, vp, i32, vp]
    L.viekf_klt_sample_depth.argtypes = [vp, vp, C.c_double, vp, C.c_int]
    L.viekf_klt_get_points.argtypes = [vp, vp, vp, vp, vp]
    L.viekf_klt_get_level.argtypes = [vp, i32, vp]
    L._klt_bound = True
    return L


def _p(a):
    return C.c_void_p(a.ctypes.data)


class KLTTracker(Handle):
    """`batch` KLT_Tracker instances (reference include/klt_tracker.h) of one image size, on one device.

        trk = KLTTracker(B, 640, 480, max_features=50, radius=30)
        feats, ids, count = trk.load_image(frames)      # frames [B][H][W] (GRAY8) or [B][H][W][3] (BGR8)
    """

    _destroy = "viekf_klt_destroy"

    def __init__(self, batch, width, height, max_features=12, radius=30, invert_image=False, device=0):
        super().__init__(_bind())
        self.B, self.W, self.H = int(batch), int(width), int(height)
        self.MF, self.radius, self.invert = int(max_features), int(radius), bool(invert_image)
        self.device = int(device)
        h = C.c_void_p()
        capi.check(self._L.viekf_klt_create(self.B, self.W, self.H, self.MF, self.radius, int(self.invert), self.device,
                                            C.byref(h)))
        self._h = h
        lv = C.c_int32()
        capi.check(self._L.viekf_klt_dims(self._handle(), None, None, None, None, None, C.byref(lv)))
        self.levels = lv.value

    def reset(self):
        capi.check(self._L.viekf_klt_reset(self._handle()))

    def set_stream(self, stream):
        """a hipStream_t handle (int, e.g. torch.cuda.current_stream().cuda_stream) or None for the null stream"""
        capi.check(self._L.viekf_klt_set_stream(self._handle(), None if stream is None else C.c_void_p(int(stream))))

    def sync(self):
        capi.check(self._L.viekf_klt_sync(self._handle()))

    def _frame_arg(self, a, dtype):
        """-> (pointer, keep-alive, where) of a host array or a device tensor"""
        if is_torch(a):
            import torch
            if a.is_cuda:
                t = a.contiguous()
                assert t.dtype == getattr(torch, np.dtype(dtype).name), t.dtype
                torch.cuda.synchronize(t.device)
                return C.c_void_p(t.data_ptr()), t, capi.DEVICE
            a = a.numpy()
        a = np.ascontiguousarray(a, dtype=dtype)
        return _p(a), a, capi.HOST

    def set_mask(self, mask):
        """KLT_Tracker::set_feature_mask: mask [H][W] (every camera) or [B][H][W] (one per camera); > 1 means usable"""
        per = len(mask.shape) == 3
        assert tuple(mask.shape[-2:]) == (self.H, self.W) and (not per or mask.shape[0] == self.B)
        p, keep, where = self._frame_arg(mask, np.uint8)
        capi.check(self._L.viekf_klt_set_mask(self._handle(), p, int(per), where))
        del keep

    def load_image(self, frames, active=None):
        """KLT_Tracker::load_image on every camera (or those with active[b] != 0) -> (features [B][MF][2] float64 clamped to
        the image, NaN padded; ids [B][MF] int32, -1 padded; count [B]).  Host frames give numpy results; device frames give
        torch tensors on that device (left on the device: no copy through the host)."""
        shp = tuple(frames.shape)
        assert shp[:3] == (self.B, self.H, self.W) and (len(shp) == 3 or (len(shp) == 4 and shp[3] in (1, 3))), shp
        ch = 1 if len(shp) == 3 else shp[3]
        p, keep, where = self._frame_arg(frames, np.uint8)
        if where == capi.DEVICE:
            import torch
            dev = keep.device
            feats = torch.empty((self.B, self.MF, 2), dtype=torch.float64, device=dev)
            ids = torch.empty((self.B, self.MF), dtype=torch.int32, device=dev)
            cnt = torch.empty(self.B, dtype=torch.int32, device=dev)
            act = None
            if active is not None:
                act = torch.as_tensor(np.asarray(active, np.uint8) if not is_torch(active) else active).to(dev, torch.uint8).contiguous()
            capi.check(self._L.viekf_klt_load_image(self._handle(), p, ch, None if act is None else C.c_void_p(act.data_ptr()),
                                                    C.c_void_p(feats.data_ptr()), C.c_void_p(ids.data_ptr()),
                                                    C.c_void_p(cnt.data_ptr()), capi.DEVICE))
            self.sync()
            return feats, ids, cnt
        feats = np.empty((self.B, self.MF, 2))
        ids = np.empty((self.B, self.MF), np.int32)
        cnt = np.empty(self.B, np.int32)
        act = None if active is None else np.ascontiguousarray(active, dtype=np.uint8).reshape(self.B)
        capi.check(self._L.viekf_klt_load_image(self._handle(), p, ch, None if act is None else _p(act), _p(feats), _p(ids), _p(cnt),
                                                capi.HOST))
        return feats, ids, cnt

    def drop_features(self, ids):
        """KLT_Tracker::drop_feature for ids [B][k] (-1 = none) -> found [B][k] bool"""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(self.B, -1)
        found = np.zeros(ids.shape, np.uint8)
        capi.check(self._L.viekf_klt_drop_features(self._handle(), _p(ids), ids.shape[1], _p(found)))
        return found.astype(bool)

    def sample_depth(self, depth_mm, min_depth):
        """the depth read of color_image_callback (vi_ekf_ros.cpp:284-297) at the last frame's features -> [B][MF] metres
        (NaN: padding, > 1e3 or < min_depth)"""
        assert tuple(depth_mm.shape) == (self.B, self.H, self.W)
        p, keep, where = self._frame_arg(depth_mm, np.float32)
        if where == capi.DEVICE:
            import torch
            out = torch.empty((self.B, self.MF), dtype=torch.float64, device=keep.device)
            capi.check(self._L.viekf_klt_sample_depth(self._handle(), p, float(min_depth), C.c_void_p(out.data_ptr()), capi.DEVICE))
            self.sync()
            return out
        out = np.empty((self.B, self.MF))
        capi.check(self._L.viekf_klt_sample_depth(self._handle(), p, float(min_depth), _p(out), capi.HOST))
        return out

    def get_points(self):
        """the tracked state, unclamped -> (list of float32 [n][2], list of int32 ids [n], next_id [B])"""
        pts = np.zeros((self.B, self.MF, 2), np.float32)
        ids = np.zeros((self.B, self.MF), np.int32)
        cnt = np.zeros(self.B, np.int32)
        nid = np.zeros(self.B, np.int32)
        capi.check(self._L.viekf_klt_get_points(self._handle(), _p(pts), _p(ids), _p(cnt), _p(nid)))
        return [pts[b, :cnt[b]].copy() for b in range(self.B)], [ids[b, :cnt[b]].copy() for b in range(self.B)], nid

    def level_shape(self, level):
        w, h = self.W, self.H
        for _ in range(level):
            w, h = (w + 1) // 2, (h + 1) // 2
        return h, w

    def get_level(self, level):
        """pyramid level `level` of the last frame -> [B][h_l][w_l] u8"""
        out = np.zeros((self.B,) + self.level_shape(level), np.uint8)
        capi.check(self._L.viekf_klt_get_level(self._handle(), int(level), _p(out)))
        return out


def track_frame(seq, tracker, t, frames, feat_R, depth_mm=None, depth_R=None, min_depth=None, use_depth=True, active=None):
    """One camera frame of VIEKF_ROS::color_image_callback (reference src/vi_ekf_ros.cpp:276-313) for every filter of `seq`
    (a SeqVIEKF whose batch has one filter per tracker camera):

        features, ids = tracker.load_image(frame)
        keep_only_features(ids)
        add_measurement(FEAT, depth)   for every feature, in order (one add_frame call)
        add_measurement(DEPTH)         where that returned MEAS_SUCCESS and the depth is finite (depth images given)
        handle_measurements -> drop_feature(gated)

    -> dict(features, ids, count, result [B][MF], gated (list per filter), depth [B][MF] or None)."""
    B, MF = tracker.B, tracker.MF
    assert seq.B == B, "one filter per camera"
    feats, ids, cnt = tracker.load_image(frames, active=active)
    if is_torch(feats):
        feats, ids, cnt = feats.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().numpy()
    depth = None
    if depth_mm is not None:
        depth = tracker.sample_depth(depth_mm, seq.core.params.min_depth if min_depth is None else min_depth)
        if is_torch(depth):
            depth = depth.cpu().numpy()
    seq.keep_only_features(ids)
    zdepth = depth if (depth is not None and use_depth) else np.full((B, MF), np.nan)
    # NaN padding: add_frame answers VIEKF_MEAS_NAN for a padded slot before its id is read
    mask = None if active is None or not seq.independent else np.asarray(active, np.uint8)
    res = seq.add_frame(t, feats, feat_R, ids, active=True, depth=zdepth, mask=mask)
    if depth is not None and depth_R is not None:
        # DEPTH only where FEAT succeeded and the depth is finite: a NaN z answers MEAS_NAN without an update
        ok = (res == capi.MEAS_SUCCESS) & np.isfinite(depth)
        for j in range(MF):
            if ok[:, j].any():
                z = np.where(ok[:, j], depth[:, j], np.nan)[:, None]
                seq.add_measurement(t, z, DEPTH, depth_R, active=use_depth, id=ids[:, j])
    gated = seq.handle_measurements()
    cap = max(1, max(len(g) for g in gated))
    drop = np.full((B, cap), -1, np.int32)
    for b, g in enumerate(gated):
        drop[b, :len(g)] = g
    if any(gated):
        tracker.drop_features(drop)
    return dict(features=feats, ids=ids, count=cnt, result=res, gated=gated, depth=depth)
