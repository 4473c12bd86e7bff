"""Python face of the batched flight simulator (include/viekf_sim.h): `batch` vehicles of sim.Simulator on the device --
truth, IMU stream, feature lists, GRAY8 frames and depth images in the layouts BatchVIEKF, SeqVIEKF and KLTTracker take.
Plumbing only -- every number comes from libviekf_hip.so (csrc/viekf_sim.hip); there is no CPU fallback, and sim.py stays
the specification.

With `device=True` a method returns torch tensors on the simulator's device (no copy through the host; the call waits
for its work, so the tensors can be used from any stream); otherwise numpy arrays.
"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import Handle, empty, is_torch

# every symbol include/viekf_sim.h declares (tests check the library exports exactly these)
SIM_SYMBOLS = [
    "viekf_sim_config_default", "viekf_sim_create", "viekf_sim_destroy", "viekf_sim_dims", "viekf_sim_reset",
    "viekf_sim_set_stream", "viekf_sim_sync", "viekf_sim_set_vehicles", "viekf_sim_set_landmarks", "viekf_sim_imu",
    "viekf_sim_step", "viekf_sim_camera", "viekf_sim_render", "viekf_sim_get_truth", "viekf_sim_truth_state",
]
MAX_LANDMARKS = 1024


class SimConfig(C.Structure):
    """struct viekf_sim_config (include/viekf_sim.h)"""
    _fields_ = [
        ("imu_rate", C.c_double), ("accel_sigma", C.c_double), ("gyro_sigma", C.c_double), ("pix_sigma", C.c_double),
        ("grid_origin", C.c_double), ("grid_pitch", C.c_double), ("grid_n", C.c_int32), ("max_features", C.c_int32),
        ("win_u_min", C.c_double), ("win_u_max", C.c_double), ("win_v_min", C.c_double), ("win_v_max", C.c_double),
        ("win_min_depth", C.c_double),
    ]


def _bind():
    L = capi.lib()
    if getattr(L, "_sim_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.viekf_sim_config_default.argtypes = [C.POINTER(SimConfig)]
    L.viekf_sim_create.argtypes = [i32, C.POINTER(capi.Params), C.POINTER(SimConfig), i32, C.POINTER(vp)]
    L.viekf_sim_destroy.argtypes = [vp]
    L.viekf_sim_dims.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32), C.POINTER(C.c_int64)]
    L.viekf_sim_reset.argtypes = [vp]
    L.viekf_sim_set_stream.argtypes = [vp, vp]
    L.viekf_sim_sync.argtypes = [vp]
    L.viekf_sim_set_vehicles.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_sim_set_landmarks.argtypes = [vp, vp, i32, C.c_int]
    L.viekf_sim_imu.argtypes = [vp, vp, C.c_int]
    L.viekf_sim_step.argtypes = [vp, i32, vp, C.c_int]
    L.viekf_sim_camera.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_sim_render.argtypes = [vp, i32, i32, vp, vp, C.c_int]
    L.viekf_sim_get_truth.argtypes = [vp, vp, vp, C.c_int]
    L.viekf_sim_truth_state.argtypes = [vp, vp, i32, vp, C.c_int]
    L._sim_bound = True
    return L


def landmarks_like(simulator):
    """the landmark field [L][3] of a sim.Simulator (its jitter comes from numpy's generator, which the device does not
    reproduce), for BatchSimulator.set_landmarks"""
    return np.ascontiguousarray(simulator.landmarks, dtype=np.float64)


class BatchSimulator(Handle):
    """`batch` sim.Simulator vehicles on one device.

        bs = BatchSimulator(B, params, max_features=8, seed=seeds, radius=radii)
        bs.set_landmarks(landmarks_like(sim.Simulator(params)))
        u0 = bs.imu()                       # [B][6], sim.imu() before the first run()
        u = bs.step(10)                     # [10][B][6], ten IMU periods in one launch
        z, ids, count, depth, lm = bs.camera(8)
        img, depth_mm = bs.render(640, 480, depth=True)
    """

    def __init__(self, batch, params, max_features=12, device=0, imu_rate=250.0, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5,
                 grid=(-3.0, 0.22, 28), window=(15.0, 625.0, 15.0, 465.0, 0.2), seed=None, radius=None, period=None,
                 accel_bias=None, gyro_bias=None):
        super().__init__(_bind())
        self.B, self.MF, self.device = int(batch), int(max_features), int(device)
        self.params = params if isinstance(params, capi.Params) else capi.Params.from_dict(params)
        cfg = SimConfig()
        capi.check(self._L.viekf_sim_config_default(C.byref(cfg)))
        cfg.imu_rate, cfg.accel_sigma, cfg.gyro_sigma, cfg.pix_sigma = imu_rate, accel_sigma, gyro_sigma, pix_sigma
        cfg.grid_origin, cfg.grid_pitch, cfg.grid_n = float(grid[0]), float(grid[1]), int(grid[2])
        cfg.max_features = self.MF
        cfg.win_u_min, cfg.win_u_max, cfg.win_v_min, cfg.win_v_max, cfg.win_min_depth = [float(w) for w in window]
        self.config = cfg
        self.L = cfg.grid_n * cfg.grid_n
        self.dt = 1.0 / float(imu_rate)
        h = C.c_void_p()
        capi.check(self._L.viekf_sim_create(self.B, C.byref(self.params), C.byref(cfg), self.device, C.byref(h)))
        self._h = h
        if any(a is not None for a in (seed, radius, period, accel_bias, gyro_bias)):
            self.set_vehicles(seed, radius, period, accel_bias, gyro_bias)

    _destroy = "viekf_sim_destroy"

    # -- handle ---------------------------------------------------------------------------------------------------------
    def reset(self):
        capi.check(self._L.viekf_sim_reset(self._handle()))

    def set_stream(self, stream):
        """a hipStream_t handle (int, e.g. torch.cuda.current_stream().cuda_stream) or None for the null stream"""
        capi.check(self._L.viekf_sim_set_stream(self._handle(), None if stream is None else C.c_void_p(int(stream))))

    def sync(self):
        capi.check(self._L.viekf_sim_sync(self._handle()))

    @property
    def tick(self):
        k = C.c_int64()
        capi.check(self._L.viekf_sim_dims(self._handle(), None, None, None, C.byref(k)))
        return k.value

    @property
    def t(self):
        return self.tick * self.dt

    def _per_vehicle(self, a, dtype, cols):
        if a is None:
            return None
        a = np.asarray(a, dtype=dtype)
        shape = (self.B,) if cols == 1 else (self.B, cols)
        return np.ascontiguousarray(np.broadcast_to(a, shape))

    def set_vehicles(self, seed=None, radius=None, period=None, accel_bias=None, gyro_bias=None):
        """per-vehicle values, each a scalar / one row (every vehicle) or one per vehicle; None keeps what is set.  Starts
        the simulation again (viekf_sim_reset)."""
        arrs = [self._per_vehicle(seed, np.uint64, 1), self._per_vehicle(radius, np.float64, 1), self._per_vehicle(period, np.float64, 1),
                self._per_vehicle(accel_bias, np.float64, 3), self._per_vehicle(gyro_bias, np.float64, 3)]
        ptrs = [None if a is None else C.c_void_p(a.ctypes.data) for a in arrs]
        capi.check(self._L.viekf_sim_set_vehicles(self._handle(), *ptrs, capi.HOST))

    def set_landmarks(self, lm):
        """[L][3] for every vehicle or [B][L][3]; numpy or a device tensor.  Starts the simulation again."""
        per = len(lm.shape) == 3
        assert tuple(lm.shape[-2:]) == (self.L, 3) and (not per or lm.shape[0] == self.B), tuple(lm.shape)
        if is_torch(lm) and lm.is_cuda:
            import torch
            t = lm.to(torch.float64).contiguous()
            torch.cuda.synchronize(t.device)
            capi.check(self._L.viekf_sim_set_landmarks(self._handle(), C.c_void_p(t.data_ptr()), int(per), capi.DEVICE))
            self.sync()
            return
        a = np.ascontiguousarray(lm.numpy() if is_torch(lm) else lm, dtype=np.float64)
        capi.check(self._L.viekf_sim_set_landmarks(self._handle(), C.c_void_p(a.ctypes.data), int(per), capi.HOST))

    # -- outputs --------------------------------------------------------------------------------------------------------
    def _empty(self, shape, dtype, device):
        """-> (array, pointer, where)"""
        return empty(shape, dtype, self.device if device else None) + (capi.DEVICE if device else capi.HOST,)

    def _ready(self, device):
        """device outputs come from torch's caching allocator and are written on the simulator's stream: whatever torch still
        has queued on a recycled block must be over first (as KLTTracker does for its inputs)"""
        if device:
            import torch
            torch.cuda.synchronize(self.device)

    def _done(self, device):
        if device:
            self.sync()

    def imu(self, device=False):
        """Simulator.imu() at the current tick, without stepping -> [B][6]"""
        u, p, where = self._empty((self.B, 6), np.float64, device)
        self._ready(device)
        capi.check(self._L.viekf_sim_imu(self._handle(), p, where))
        self._done(device)
        return u

    def step(self, K=1, device=False):
        """K IMU periods (each _control, _step_truth, imu()) in one launch -> u [K][B][6], the `u` of BatchVIEKF.step_n"""
        u, p, where = self._empty((int(K), self.B, 6), np.float64, device)
        self._ready(device)
        capi.check(self._L.viekf_sim_step(self._handle(), int(K), p, where))
        self._done(device)
        return u

    def camera(self, num_features=None, device=False):
        """Simulator._camera() -> (z [B][N][2] NaN padded, ids [B][N] -1 padded, count [B], depth [B][N] NaN padded,
        landmark [B][N] -1 padded)"""
        N = self.MF if num_features is None else int(num_features)
        z, pz, where = self._empty((self.B, max(N, 0), 2), np.float64, device)
        ids, pi, _ = self._empty((self.B, max(N, 0)), np.int32, device)
        cnt, pc, _ = self._empty((self.B,), np.int32, device)
        dep, pd, _ = self._empty((self.B, max(N, 0)), np.float64, device)
        lm, pl, _ = self._empty((self.B, max(N, 0)), np.int32, device)
        self._ready(device)
        capi.check(self._L.viekf_sim_camera(self._handle(), N, pz, pi, pc, pd, pl, where))
        self._done(device)
        return z, ids, cnt, dep, lm

    def render(self, width=640, height=480, depth=False, device=False):
        """Simulator.render() -> img [B][height][width] u8 (and, with depth=True, the range in mm as float32, +inf where a
        ray misses the ground)"""
        img, pi, where = self._empty((self.B, int(height), int(width)), np.uint8, device)
        dmm, pd = None, None
        if depth:
            dmm, pd, _ = self._empty((self.B, int(height), int(width)), np.float32, device)
        self._ready(device)
        capi.check(self._L.viekf_sim_render(self._handle(), int(width), int(height), pi, pd, where))
        self._done(device)
        return (img, dmm) if depth else img

    def truth(self, device=False):
        """-> (state [B][13] = pos, att, vel_body, omega like Simulator.state(), t [B])"""
        st, ps, where = self._empty((self.B, 13), np.float64, device)
        t, pt, _ = self._empty((self.B,), np.float64, device)
        self._ready(device)
        capi.check(self._L.viekf_sim_get_truth(self._handle(), ps, pt, where))
        self._done(device)
        return st, t

    def truth_state(self, ids, device=None):
        """the true state in the filter's layout [B][17 + 5 N] for the feature slots ids [B][N] (-1 or an id that is no
        longer tracked: five NaNs), for diag.consistency(batch, x_true).  A device tensor of ids gives a device tensor."""
        if is_torch(ids) and ids.is_cuda:
            import torch
            t = ids.to(torch.int32).contiguous()
            torch.cuda.synchronize(t.device)
            N = int(t.shape[1])
            x, px, _ = self._empty((self.B, 17 + 5 * N), np.float64, True)
            self._ready(True)
            capi.check(self._L.viekf_sim_truth_state(self._handle(), C.c_void_p(t.data_ptr()), N, px, capi.DEVICE))
            self.sync()
            return x
        a = np.ascontiguousarray(ids.numpy() if is_torch(ids) else ids, dtype=np.int32).reshape(self.B, -1)
        N = a.shape[1]
        if device:
            import torch
            return self.truth_state(torch.as_tensor(a).to("cuda:%d" % self.device))
        x = np.empty((self.B, 17 + 5 * N))
        capi.check(self._L.viekf_sim_truth_state(self._handle(), C.c_void_p(a.ctypes.data) if N else None, N, C.c_void_p(x.ctypes.data), capi.HOST))
        return x
