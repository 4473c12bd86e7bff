"""BatchVIEKF: a batch of independent filters on one MI355X, driven through the C ABI.

Method names follow the reference class vi_ekf::VIEKF (reference include/vi_ekf.h:82-338):
propagate_state -> propagate, update(FEAT) -> update_feat, init_feature, get_state,
get_covariance.  numpy arrays are passed as host pointers, torch CUDA tensors as device
pointers; nothing is computed in Python.
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import is_torch, r_colmajor


class BatchVIEKF:
    def __init__(self, batch, num_features, params, device=0):
        """params: one parameter set (dict or capi.Params) for every filter, or a list of `batch` of them, one per filter: the
        batch is then created with entry 0, given the list (set_params) and reset, so that filter b starts at ITS x0 / P0."""
        L = capi.lib()
        per_filter = None
        if isinstance(params, (list, tuple)):
            if len(params) != int(batch):
                raise ValueError("a list of parameter sets needs one entry per filter: %d, got %d" % (int(batch), len(params)))
            per_filter, params = params, params[0]
        if isinstance(params, dict):
            params = capi.Params.from_dict(params)
        self.params = params
        self._h = C.c_void_p()
        capi.check(L.viekf_batch_create(int(batch), int(num_features), C.byref(params), int(device), C.byref(self._h)))
        self.B, self.N = int(batch), int(num_features)
        self.nx, self.n = 17 + 5 * self.N, 16 + 3 * self.N
        self.device = int(device)
        self._keep = []
        if per_filter is not None:
            try:
                self.set_params(per_filter)
                self.reset()
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            capi.lib().viekf_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- argument marshalling -------------------------------------------------------------
    def _arg(self, a, dtype, shape, where):
        """-> (pointer, where).  All array arguments of one call must live on the same side."""
        if a is None:
            return None, where
        if is_torch(a):
            import torch
            want = {np.float64: torch.float64, np.int32: torch.int32, np.uint8: torch.uint8, np.uint32: torch.int32}[dtype]
            if not a.is_cuda or a.dtype != want or not a.is_contiguous():
                raise ValueError("device arguments must be contiguous CUDA tensors of dtype %s" % want)
            if tuple(a.shape) != tuple(shape):
                raise ValueError("expected shape %s, got %s" % (shape, tuple(a.shape)))
            if where not in (None, capi.DEVICE):
                raise ValueError("cannot mix host and device arguments in one call")
            return C.c_void_p(a.data_ptr()), capi.DEVICE
        arr = np.ascontiguousarray(a, dtype=dtype)
        if arr.shape != tuple(shape):
            raise ValueError("expected shape %s, got %s" % (shape, arr.shape))
        if where not in (None, capi.HOST):
            raise ValueError("cannot mix host and device arguments in one call")
        self._keep.append(arr)
        return C.c_void_p(arr.ctypes.data), capi.HOST

    def _out(self, a, dtype, shape, where):
        if is_torch(a):
            return self._arg(a, dtype, shape, where)
        if a.dtype != dtype or not a.flags.c_contiguous or a.shape != tuple(shape):
            raise ValueError("output array must be C-contiguous %s of shape %s" % (dtype, shape))
        if where not in (None, capi.HOST):
            raise ValueError("cannot mix host and device arguments in one call")
        return C.c_void_p(a.ctypes.data), capi.HOST

    # ---- C ABI calls -----------------------------------------------------------------------
    def set_stream(self, hip_stream_ptr):
        capi.check(capi.lib().viekf_batch_set_stream(self._h, C.c_void_p(hip_stream_ptr or 0)))

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def sync(self):
        capi.check(capi.lib().viekf_batch_sync(self._h))

    def set_kernel(self, family):
        capi.check(capi.lib().viekf_batch_set_kernel(self._h, int(family)))

    def set_tuning(self, key, value):
        """kernel selection knobs for tests and experiments (viekf_batch_set_tuning; capi.TUNE_*)"""
        capi.check(capi.lib().viekf_batch_set_tuning(self._h, int(key), int(value)))

    def describe(self):
        """which kernels a step of this batch launches (viekf_batch_describe)"""
        buf = C.create_string_buffer(256)
        capi.check(capi.lib().viekf_batch_describe(self._h, buf, 256))
        return buf.value.decode()

    def reset(self):
        capi.check(capi.lib().viekf_batch_reset(self._h))

    def set_drag_term(self, use_drag_term):
        """the run-time drag switch (viekf_batch_set_drag_term): every filter's parameter set follows it"""
        capi.check(capi.lib().viekf_batch_set_drag_term(self._h, int(bool(use_drag_term))))

    def get_drag_term(self):
        out = C.c_int32(0)
        capi.check(capi.lib().viekf_batch_get_drag_term(self._h, C.byref(out)))
        return bool(out.value)

    def set_params(self, params):
        """one parameter set per filter (viekf_batch_set_params_filters): a list of `batch` dicts or capi.Params; None = back to the
        set the batch was created with.  Holds for every launch after the call; x0 / P0 are seen by the next reset()."""
        if params is None:
            capi.check(capi.lib().viekf_batch_set_params_filters(self._h, None))
            return
        if len(params) != self.B:
            raise ValueError("a list of parameter sets needs one entry per filter: %d, got %d" % (self.B, len(params)))
        arr = (capi.Params * self.B)()
        for b, p in enumerate(params):
            arr[b] = capi.Params.from_dict(p) if isinstance(p, dict) else p
        capi.check(capi.lib().viekf_batch_set_params_filters(self._h, arr))

    def params_of(self, b):
        """-> capi.Params: filter b's current parameter set (viekf_batch_get_params_filter)"""
        p = capi.Params()
        capi.check(capi.lib().viekf_batch_get_params_filter(self._h, int(b), C.byref(p)))
        return p

    def get_state(self):
        """-> x [B][nx] (reference get_state(), include/vi_ekf.h:277)"""
        x = np.empty((self.B, self.nx))
        capi.check(capi.lib().viekf_batch_get_state(self._h, C.c_void_p(x.ctypes.data), None, None, capi.HOST))
        return x

    def get_covariance(self):
        """-> P [B][n][n] as numpy [b, i, j] (reference get_covariance(), include/vi_ekf.h:278)"""
        P = np.empty((self.B, self.n, self.n))
        capi.check(capi.lib().viekf_batch_get_state(self._h, None, C.c_void_p(P.ctypes.data), None, capi.HOST))
        return np.ascontiguousarray(P.transpose(0, 2, 1))  # column-major per filter -> [b, row, col]

    def get_len_features(self):
        ln = np.empty(self.B, dtype=np.int32)
        capi.check(capi.lib().viekf_batch_get_state(self._h, None, None, C.c_void_p(ln.ctypes.data), capi.HOST))
        return ln

    def set_state(self, x=None, P=None, len_features=None):
        """x [B][nx]; P [B][n][n] indexed [b, row, col]; len_features [B]"""
        self._keep = []
        px = pP = pl = None
        if x is not None:
            px, _ = self._arg(x, np.float64, (self.B, self.nx), None)
        if P is not None:
            Pc = np.ascontiguousarray(np.asarray(P, dtype=np.float64).transpose(0, 2, 1))
            pP, _ = self._arg(Pc, np.float64, (self.B, self.n, self.n), None)
        if len_features is not None:
            pl, _ = self._arg(len_features, np.int32, (self.B,), None)
        capi.check(capi.lib().viekf_batch_set_state(self._h, px, pP, pl, capi.HOST))
        self._keep = []

    def get_status(self):
        f = np.empty(self.B, dtype=np.uint32)
        capi.check(capi.lib().viekf_batch_get_status(self._h, C.c_void_p(f.ctypes.data), capi.HOST))
        return f

    def propagate(self, u, dt):
        """numeric core of propagate_state (reference vi_ekf.cpp:262-318); u [B][6] raw IMU, dt [B]"""
        self._keep = []
        pu, w = self._arg(u, np.float64, (self.B, 6), None)
        pdt, w = self._arg(dt, np.float64, (self.B,), w)
        capi.check(capi.lib().viekf_batch_propagate(self._h, pu, pdt, w))
        self._keep = []

    def init_feature(self, pix, depth=None, mask=None):
        """reference vi_ekf_feat.cpp:6-47 for every filter (or those with mask != 0) -> ok [B]"""
        self._keep = []
        ppix, w = self._arg(pix, np.float64, (self.B, 2), None)
        pdep, w = self._arg(depth, np.float64, (self.B,), w)
        pm, w = self._arg(mask, np.uint8, (self.B,), w)
        if w == capi.DEVICE:
            import torch
            ok = torch.empty(self.B, dtype=torch.int32, device=pix.device)
        else:
            ok = np.empty(self.B, dtype=np.int32)
        pok, w = self._out(ok, np.int32, (self.B,), w)
        capi.check(capi.lib().viekf_batch_init_feature(self._h, ppix, pdep, pm, pok, w))
        self._keep = []
        return ok

    def _meas_args(self, z, slot, R, result):
        M = int(slot.shape[1])
        pz, w = self._arg(z, np.float64, (self.B, M, 2), None)
        ps, w = self._arg(slot, np.int32, (self.B, M), w)
        R, r_mode = r_colmajor(R, self.B, M)
        pR, w = self._arg(R, np.float64, tuple(R.shape), w)
        if is_torch(R):
            self._keep.append(R)
        if result is None:
            if w == capi.DEVICE:
                import torch
                result = torch.empty((self.B, M), dtype=torch.int32, device=z.device)
            else:
                result = np.empty((self.B, M), dtype=np.int32)
        pres, w = self._out(result, np.int32, (self.B, M), w)
        return M, pz, ps, pR, r_mode, pres, result, w

    def update_feat(self, z, slot, R, result=None):
        """M sequential active FEAT updates (reference vi_ekf_meas.cpp:196-278) -> result [B][M]"""
        self._keep = []
        M, pz, ps, pR, r_mode, pres, result, w = self._meas_args(z, slot, R, result)
        capi.check(capi.lib().viekf_batch_update_feat(self._h, pz, ps, M, pR, r_mode, pres, w))
        self._keep = []
        return result

    def update(self, mtype, z, R, slot=None, active=None):
        """ONE measurement of any reference model per filter (reference vi_ekf_meas.cpp:196-386); host arrays.
        z [B][zdim]; R (rdim,rdim) shared or (B,rdim,rdim); slot [B] for feature models -> result [B]"""
        self._keep = []
        z = np.ascontiguousarray(z, dtype=np.float64)
        zdim = z.shape[1]
        R = np.asarray(R, dtype=np.float64)
        rdim = R.shape[-1]
        if R.ndim == 2:
            r_mode, Rc = 0, np.ascontiguousarray(R.T)
        else:
            r_mode, Rc = 1, np.ascontiguousarray(R.transpose(0, 2, 1))
        pz, w = self._arg(z, np.float64, (self.B, zdim), None)
        pR, w = self._arg(Rc, np.float64, Rc.shape, w)
        ps, w = self._arg(slot, np.int32, (self.B,), w)
        pa, w = self._arg(active, np.uint8, (self.B,), w)
        res = np.empty(self.B, dtype=np.int32)
        capi.check(capi.lib().viekf_batch_update(self._h, int(mtype), pz, zdim, pR, rdim, r_mode, ps, pa,
                                                 C.c_void_p(res.ctypes.data), capi.HOST))
        self._keep = []
        return res

    def update_body(self, entries, active=None, result=None):
        """The body-sensor updates of one tick, in order, in one pass over P (viekf_batch_update_body, include/viekf_body.h).
        entries: a list of (mtype, z, R) with mtype ACC / ALT / ATT / POS / VEL, z [B][zdim] and R (rdim, rdim) shared by the
        filters or (B, rdim, rdim) -- all entries the same way -- as numpy arrays; or, for device memory, the tuple
        (types, zdim, rdim, z, R) with types / zdim / rdim as sequences of M ints and z [M][B][4], R [M][9] or [M][B][9]
        (each R column-major in its cell) as CUDA tensors.  active [M][B] (0 / 1 / 2 as update()) or None.
        -> (result [M][B], route): route 1 = the fused launch, 0 = M launches of update()'s kernel"""
        self._keep = []
        if isinstance(entries, tuple):
            types, zdim, rdim, z, R = entries
            M = len(types)
        else:
            M = len(entries)
            types, zdim, rdim = [], [], []
            z = np.zeros((M, self.B, 4))
            per_filter = [np.asarray(e[2]).ndim == 3 for e in entries]
            if any(per_filter) != all(per_filter):
                raise ValueError("R must be shared in every entry or per filter in every entry")
            R = np.zeros((M, self.B, 9) if M and per_filter[0] else (M, 9))
            for m, (mtype, zm, Rm) in enumerate(entries):
                zm = np.asarray(zm, dtype=np.float64)
                Rm = np.asarray(Rm, dtype=np.float64)
                if zm.ndim != 2 or zm.shape[0] != self.B or not 1 <= zm.shape[1] <= 4:
                    raise ValueError("z of entry %d must be [B][zdim], zdim 1..4" % m)
                if Rm.shape[-1] != Rm.shape[-2] or not 1 <= Rm.shape[-1] <= 3 or (Rm.ndim == 3 and Rm.shape[0] != self.B):
                    raise ValueError("R of entry %d must be (rdim, rdim) or (B, rdim, rdim), rdim 1..3" % m)
                r = Rm.shape[-1]
                types.append(int(mtype)); zdim.append(zm.shape[1]); rdim.append(r)
                z[m, :, :zm.shape[1]] = zm
                R[m, ..., :r * r] = np.swapaxes(Rm, -1, -2).reshape(Rm.shape[:-2] + (r * r,))
        if not (len(types) == len(zdim) == len(rdim) == M):
            raise ValueError("types, zdim and rdim must have one value per entry")
        r_mode = 1 if len(R.shape) == 3 else 0
        ty, zd, rd = (np.ascontiguousarray(v, dtype=np.int32) for v in (types, zdim, rdim))
        pz, w = self._arg(z, np.float64, (M, self.B, 4), None)
        pR, w = self._arg(R, np.float64, (M, self.B, 9) if r_mode else (M, 9), w)
        pa, w = self._arg(active, np.uint8, (M, self.B), w)
        if result is None:
            if w == capi.DEVICE:
                import torch
                result = torch.empty((M, self.B), dtype=torch.int32, device=z.device)
            else:
                result = np.empty((M, self.B), dtype=np.int32)
        pres, w = self._out(result, np.int32, (M, self.B), w)
        route = C.c_int32(-1)
        capi.check(capi.lib().viekf_batch_update_body(self._h, M, C.c_void_p(ty.ctypes.data), C.c_void_p(zd.ctypes.data),
                                                      C.c_void_p(rd.ctypes.data), pz, pR, r_mode, pa, pres, C.byref(route), w))
        self._keep = []
        return result, route.value

    def update_depths(self, mtype, z, slot, R, active=None, order=0, result=None):
        """M DEPTH (or INV_DEPTH) updates per filter in one pass over P (viekf_batch_update_depths, include/viekf_depth.h).
        mtype DEPTH or INV_DEPTH; z [B][M], slot [B][M] (a slot may repeat; -1 = no entry); R the variance: a float, [B] or
        [B][M]; active [B][M] (0 / 1 / 2 as update()) or None; order 0 = entry 0 first, 1 = entry M-1 first (the
        reference's queue order within a stamp).  numpy arrays, or contiguous CUDA tensors (R then a tensor of shape (1,),
        (B,) or (B, M)) -- one call takes one kind.
        -> (result [B][M], route): route 1 = the fused launch, 0 = M launches of update()'s kernel"""
        self._keep = []
        if len(slot.shape) != 2:
            raise ValueError("slot must be [B][M]")
        M = int(slot.shape[1])
        if not is_torch(R):
            R = np.asarray(R, dtype=np.float64)
            if is_torch(z):                                    # (a plain number beside device tensors)
                import torch
                R = torch.as_tensor(R, dtype=torch.float64, device=z.device).contiguous()
                self._depths_R = R                             # (must outlive the queued work: kept until the next call)
        r_mode = {(): 0, (1,): 0, (self.B,): 1, (self.B, M): 2}.get(tuple(R.shape))
        if r_mode is None:
            raise ValueError("R must be a scalar, [B] or [B][M]")
        if r_mode == 0:
            R = R.reshape(1)
        ps, w = self._arg(slot, np.int32, (self.B, M), None)
        pz, w = self._arg(z, np.float64, (self.B, M), w)
        pR, w = self._arg(R, np.float64, tuple(R.shape), w)
        pa, w = self._arg(active, np.uint8, (self.B, M), w)
        if result is None:
            if w == capi.DEVICE:
                import torch
                result = torch.empty((self.B, M), dtype=torch.int32, device=z.device)
            else:
                result = np.empty((self.B, M), dtype=np.int32)
        pres, w = self._out(result, np.int32, (self.B, M), w)
        route = C.c_int32(-1)
        capi.check(capi.lib().viekf_batch_update_depths(self._h, int(mtype), M, ps, pz, pR, r_mode, pa, int(order), pres,
                                                        C.byref(route), w))
        self._keep = []
        return result, route.value

    def update_pixel_vels(self, z, slot, gyro, R, gyro_var=0.0, active=None, order=0, result=None):
        """M PIXEL_VEL (image velocity) updates per filter (viekf_batch_update_pixel_vels, include/viekf_pixvel.h).
        z [B][M][2] px / s (pixel_flow), slot [B][M] (a slot may repeat; -1 = no entry), gyro [B][3] the raw gyro sample,
        R (2,2), (B,2,2) or (B,M,2,2) indexed [row, col]; gyro_var the variance of one gyro axis; active [B][M] (0 / 1 / 2 as
        update()) or None; order 0 = entry 0 first, 1 = entry M-1 first.  numpy arrays or contiguous CUDA tensors -- one call
        takes one kind.
        -> (result [B][M], route): route 1 = the fused launch, 0 = M launches of the single-entry kernel"""
        self._keep = []
        if len(slot.shape) != 2:
            raise ValueError("slot must be [B][M]")
        M = int(slot.shape[1])
        ps, w = self._arg(slot, np.int32, (self.B, M), None)
        pz, w = self._arg(z, np.float64, (self.B, M, 2), w)
        pg, w = self._arg(gyro, np.float64, (self.B, 3), w)
        Rc, r_mode = r_colmajor(R, self.B, M)
        pR, w = self._arg(Rc, np.float64, tuple(Rc.shape), w)
        if is_torch(Rc):
            self._pixvels_R = Rc                               # (must outlive the queued work: kept until the next call)
        pa, w = self._arg(active, np.uint8, (self.B, M), w)
        if result is None:
            if w == capi.DEVICE:
                import torch
                result = torch.empty((self.B, M), dtype=torch.int32, device=z.device)
            else:
                result = np.empty((self.B, M), dtype=np.int32)
        pres, w = self._out(result, np.int32, (self.B, M), w)
        route = C.c_int32(-1)
        capi.check(capi.lib().viekf_batch_update_pixel_vels(self._h, M, ps, pz, pg, pR, r_mode, float(gyro_var), pa, int(order), pres,
                                                            C.byref(route), w))
        self._keep = []
        return result, route.value

    def pixel_vels_route(self, route):
        """hold update_pixel_vels / FrameIntake.intake_pixel_vel of this batch to a route: -1 automatic, 0 the M launches, 1 fused"""
        capi.check(capi.lib().viekf_batch_pixel_vels_route(self._h, int(route)))

    def eval_pixel_vel(self, slot, gyro, jacobian=True):
        """zhat = h_pixel_vel(x) [B][2] (px / s) at the current state for the feature in slot [B] and the raw gyro sample
        gyro [B][3], and H [B][2][n] (None with jacobian=False): viekf_batch_eval_pixel_vel.  numpy arrays or contiguous CUDA
        tensors; the filter is left untouched.  A slot outside [0, len): NaN."""
        self._keep = []
        ps, w = self._arg(slot, np.int32, (self.B,), None)
        pg, w = self._arg(gyro, np.float64, (self.B, 3), w)
        if w == capi.DEVICE:
            import torch
            zhat = torch.empty((self.B, 2), dtype=torch.float64, device=gyro.device)
            H = torch.empty((self.B, 2, self.n), dtype=torch.float64, device=gyro.device) if jacobian else None
        else:
            zhat = np.empty((self.B, 2))
            H = np.empty((self.B, 2, self.n)) if jacobian else None
        pz, w = self._out(zhat, np.float64, (self.B, 2), w)
        pH = None
        if jacobian:
            pH, w = self._out(H, np.float64, (self.B, 2, self.n), w)
        capi.check(capi.lib().viekf_batch_eval_pixel_vel(self._h, ps, pg, pz, pH, w))
        self._keep = []
        return zhat, H

    def pixel_flow(self, z_prev, ids_prev, z, ids, dt):
        """the image velocity of a frame's features from the frame before, by id (viekf_pixel_flow): z_prev [B][Mp][2],
        ids_prev [B][Mp], z [B][M][2], ids [B][M], dt [B] -> zdot [B][M][2], NaN where an id has no finite partner"""
        self._keep = []
        if len(ids.shape) != 2 or len(ids_prev.shape) != 2:
            raise ValueError("ids and ids_prev must be [B][M]")
        Mp, M = int(ids_prev.shape[1]), int(ids.shape[1])
        pzp, w = self._arg(z_prev, np.float64, (self.B, Mp, 2), None)
        pip, w = self._arg(ids_prev, np.int32, (self.B, Mp), w)
        pz, w = self._arg(z, np.float64, (self.B, M, 2), w)
        pi, w = self._arg(ids, np.int32, (self.B, M), w)
        pdt, w = self._arg(dt, np.float64, (self.B,), w)
        if w == capi.DEVICE:
            import torch
            zdot = torch.empty((self.B, M, 2), dtype=torch.float64, device=z.device)
        else:
            zdot = np.empty((self.B, M, 2))
        po, w = self._out(zdot, np.float64, (self.B, M, 2), w)
        capi.check(capi.lib().viekf_pixel_flow(self._h, Mp, pzp, pip, M, pz, pi, pdt, po, w))
        self._keep = []
        return zdot

    def keep_features(self, keep):
        """drop the features with keep[b, f] == 0 and compact (reference vi_ekf_feat.cpp:50-117) -> new len [B]"""
        self._keep = []
        pk, w = self._arg(keep, np.uint8, (self.B, self.N), None)
        nl = np.empty(self.B, dtype=np.int32)
        capi.check(capi.lib().viekf_batch_keep_features(self._h, pk, C.c_void_p(nl.ctypes.data), capi.HOST))
        self._keep = []
        return nl

    def keyframe_reset(self, mask=None):
        """keyframe reset of the filters with mask[b] != 0 (None = all), reference vi_ekf_kfr.cpp:56-157.
        Returns the edges [B][17] = {t(3), q_yaw(4), cov_pos(9, column-major), cov_yaw} (zeros outside the mask)."""
        self._keep = []
        pm = None
        if mask is not None:
            pm, _ = self._arg(mask, np.uint8, (self.B,), None)
        edge = np.zeros((self.B, 17), dtype=np.float64)
        capi.check(capi.lib().viekf_batch_keyframe_reset(self._h, pm, C.c_void_p(edge.ctypes.data), capi.HOST))
        self._keep = []
        return edge

    def eval_xdot(self, u):
        """dx_ of VIEKF::dynamics at the current state for the input u [B][6] (reference vi_ekf_dyn.cpp:6-134): [B][n]"""
        self._keep = []
        pu, _ = self._arg(u, np.float64, (self.B, 6), None)
        out = np.zeros((self.B, self.n), dtype=np.float64)
        capi.check(capi.lib().viekf_batch_eval_xdot(self._h, pu, C.c_void_p(out.ctypes.data), capi.HOST))
        self._keep = []
        return out

    def eval_h(self, mtype, slot=None):
        """zhat = h(x) of a measurement model at the current state (reference vi_ekf_meas.cpp:281-386): [B][4], NaN padded"""
        self._keep = []
        ps = None
        if slot is not None:
            ps, _ = self._arg(slot, np.int32, (self.B,), None)
        out = np.zeros((self.B, 4), dtype=np.float64)
        capi.check(capi.lib().viekf_batch_eval_h(self._h, int(mtype), ps, C.c_void_p(out.ctypes.data), capi.HOST))
        self._keep = []
        return out

    def get_cov_diag(self):
        out = np.zeros((self.B, self.n), dtype=np.float64)
        capi.check(capi.lib().viekf_batch_get_cov_diag(self._h, C.c_void_p(out.ctypes.data), capi.HOST))
        return out

    def history_resize(self, depth):
        capi.check(capi.lib().viekf_batch_history_resize(self._h, int(depth)))

    def snapshot(self, slot):
        capi.check(capi.lib().viekf_batch_snapshot(self._h, int(slot)))

    def restore(self, slot):
        capi.check(capi.lib().viekf_batch_restore(self._h, int(slot)))

    def select_filters(self, slot):
        """per-filter live ring slots (viekf_batch_select_filters); slot [B] int32 on the host, < 0 = unchanged"""
        sl = np.ascontiguousarray(slot, dtype=np.int32)
        if sl.shape != (self.B,):
            raise ValueError("expected shape %s, got %s" % ((self.B,), sl.shape))
        capi.check(capi.lib().viekf_batch_select_filters(self._h, C.c_void_p(sl.ctypes.data)))

    def propagate_n_filters_to(self, u, dt, k_count, dst_slot):
        """filter b: k_count[b] propagates (u [K,B,6], dt [K,B]; rows k >= k_count[b] are not read) from its live ring slot into
        dst_slot[b] (viekf_batch_propagate_n_filters_to) -> intermediates_written"""
        self._keep = []
        K = int(u.shape[0])
        pu, w = self._arg(u, np.float64, (K, self.B, 6), None)
        pdt, w = self._arg(dt, np.float64, (K, self.B), w)
        pk, _ = self._arg(np.asarray(k_count), np.int32, (self.B,), None)
        pd, _ = self._arg(np.asarray(dst_slot), np.int32, (self.B,), None)
        iw = C.c_int32(-1)
        capi.check(capi.lib().viekf_batch_propagate_n_filters_to(self._h, K, pu, pdt, pk, pd, C.byref(iw), w))
        self._keep = []
        return iw.value

    def step_n(self, u, dt, z, slot, R, result=None):
        """K propagates (u [K,B,6], dt [K,B]: the IMU samples since the last frame) + M feature updates in one launch"""
        self._keep = []
        K = int(u.shape[0])
        pu, w0 = self._arg(u, np.float64, (K, self.B, 6), None)
        pdt, w0 = self._arg(dt, np.float64, (K, self.B), w0)
        if z is None:     # K propagates, no measurements
            M, pz, ps, pR, r_mode, pres, result, w = 0, None, None, None, 0, None, None, w0
        else:
            M, pz, ps, pR, r_mode, pres, result, w = self._meas_args(z, slot, R, result)
        if w != w0:
            raise ValueError("cannot mix host and device arguments in one call")
        capi.check(capi.lib().viekf_batch_step_n(self._h, K, pu, pdt, pz, ps, M, pR, r_mode, pres, w))
        self._keep = []
        return result

    def step(self, u, dt, z, slot, R, result=None):
        """one hot-path step: propagate + M feature updates"""
        self._keep = []
        pu, w0 = self._arg(u, np.float64, (self.B, 6), None)
        pdt, w0 = self._arg(dt, np.float64, (self.B,), w0)
        M, pz, ps, pR, r_mode, pres, result, w = self._meas_args(z, slot, R, result)
        if w != w0:
            raise ValueError("cannot mix host and device arguments in one call")
        capi.check(capi.lib().viekf_batch_step(self._h, pu, pdt, pz, ps, M, pR, r_mode, pres, w))
        self._keep = []
        return result
