"""numpy restatement of what the batched simulator (include/viekf_sim.h) adds to vi_ekf_amd/sim.py: the
counter-based noise (Philox4x32-10 -> two 53-bit uniforms -> Box-Muller), a Simulator whose imu() and _camera() draw
from it and which takes its landmarks and per-vehicle values from the caller, the renderer's value before rint / clip
with the depth in double, and the true state in the filter's layout.  Test infrastructure only: the simulator itself is
the HIP code in csrc/viekf_sim.hip; truth and control are sim.Simulator's own code, inherited, and project() is its loop
over landmarks written as array operations (held to the inherited one bit for bit by tests/test_sim_ref_cpu.py).
"""
import math

import numpy as np

from vi_ekf_amd import sim as S

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
U32 = 0xFFFFFFFF
STREAM_IMU, STREAM_PIX = 0, 1


def philox4x32_10(key, ctr):
    """key (k0, k1), ctr (c0, c1, c2, c3): python ints or uint arrays (broadcast) -> four uint32 arrays"""
    k0, k1 = (np.asarray(k, dtype=np.uint64) & U32 for k in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & U32 for c in ctr])
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & U32, (p0 >> 32) ^ c3 ^ k1, p0 & U32
        k0, k1 = (k0 + W0) & U32, (k1 + W1) & U32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def uniform53(hi, lo):
    """two words -> a uniform in (0, 1) with 53 random bits"""
    return ((hi >> np.uint32(5)).astype(np.float64) * 67108864.0 + (lo >> np.uint32(6)).astype(np.float64) + 0.5) * 2.0 ** -53


def normal_pair(seed, tick, stream, block):
    """two standard normals per (seed, tick, stream, block): sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2)"""
    seed = np.asarray(seed, dtype=np.uint64)
    w = philox4x32_10((seed & np.uint64(U32), seed >> np.uint64(32)), (tick, stream, block, 0))
    u1, u2 = uniform53(w[0], w[1]), uniform53(w[2], w[3])
    r, a = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
    return r * np.cos(a), r * np.sin(a)


def imu_normals(seed, tick):
    """the six normals of the IMU sample at `tick`: acc x y z, gyr x y z -> [..., 6]"""
    n = [normal_pair(seed, tick, STREAM_IMU, blk) for blk in range(3)]
    return np.stack([n[0][0], n[0][1], n[1][0], n[1][1], n[2][0], n[2][1]], axis=-1)


def _rotp_rows(q, V):
    """sim.q_rotp for every row of V [n][3]"""
    w, qv = q[0], q[1:4]
    t = -2.0 * np.cross(qv, V)
    return V + w * t - np.cross(qv, t)


class RefSimulator(S.Simulator):
    """sim.Simulator with the counter-based noise and caller-supplied landmarks.  With landmarks=None it keeps the field
    sim.Simulator draws from numpy's generator for `seed`."""

    def __init__(self, params, num_features=8, seed=1, landmarks=None, **kw):
        super().__init__(params, num_features=num_features, seed=seed, **kw)
        self.seed = int(seed)
        if landmarks is not None:
            self.landmarks = np.array(landmarks, dtype=np.float64)
        self.last_landmarks = []

    def project(self, ids=None):
        """Simulator.project with the loop over landmarks written as array operations (the same operations in the same
        order on every row: tests/test_sim_ref_cpu.py holds it to the inherited one bit for bit)"""
        L = self.landmarks if ids is None else self.landmarks[np.asarray(ids, int)]
        pc = _rotp_rows(self.q_b_c, _rotp_rows(self.q, L - self.pos) - self.p_b_c).reshape(-1, 3)
        z = pc[:, 2]
        ok = z > 0.2
        zs = np.where(ok, z, 1.0)
        pix = np.stack([self.f[0] * pc[:, 0] / zs + self.c[0], self.f[1] * pc[:, 1] / zs + self.c[1]], axis=1)
        vis = ok & (pix[:, 0] > 15) & (pix[:, 0] < 625) & (pix[:, 1] > 15) & (pix[:, 1] < 465)
        return pix, np.linalg.norm(pc, axis=1), vis

    def copy_truth_from(self, other):
        """take another simulator's vehicle state and clock, keeping this one's camera bookkeeping"""
        self.pos, self.vel, self.q, self.w, self.az = other.pos.copy(), other.vel.copy(), other.q.copy(), other.w.copy(), other.az
        self.k, self.t = other.k, other.t

    def imu(self, noise=True):
        acc_b = np.array([-self.mu * self.vel[0], -self.mu * self.vel[1], self.az]) + self.accel_bias_
        gyr_b = self.w + self.gyro_bias_
        if noise:
            n = imu_normals(self.seed, self.k)
            acc_b = acc_b + self.accel_sigma * n[0:3]
            gyr_b = gyr_b + self.gyro_sigma * n[3:6]
        return np.concatenate([S.q_rotp(self.q_b_u, acc_b), S.q_rotp(self.q_b_u, gyr_b)])

    def _camera(self):
        pix, depth, vis = self.project()
        for i in self.tracked:
            if not vis[i]:
                del self.feat_id[i]
        self.tracked = [i for i in self.tracked if vis[i]]
        if len(self.tracked) < self.N:
            dist = np.linalg.norm(pix - self.c, axis=1)
            cand = [i for i in np.argsort(dist, kind="stable") if vis[i] and i not in self.tracked]    # (ties by index)
            order = cand[::3] + cand[1::3] + cand[2::3]
            for i in order[: self.N - len(self.tracked)]:
                self.tracked.append(int(i))
                self.feat_id[int(i)] = self.next_feat_id
                self.next_feat_id += 1
        lm = list(self.tracked)
        self.last_landmarks = lm
        nx, ny = normal_pair(self.seed, self.k, STREAM_PIX, np.asarray(lm, dtype=np.uint64))
        z = pix[lm] + self.pix_sigma * np.stack([nx, ny], axis=1).reshape(len(lm), 2)
        return z, [self.feat_id[i] for i in lm], depth[lm]

    def advance(self, K=1):
        """K IMU periods without callbacks -> u [K][6] (what viekf_sim_step writes for this vehicle)"""
        out = np.empty((K, 6))
        for i in range(K):
            self._control()
            self._step_truth()
            self.k += 1
            self.t = self.k * self.dt
            out[i] = self.imu()
        return out

    def camera_padded(self, N=None):
        """_camera() in the padded shape of viekf_sim_camera -> (z [N][2], ids [N], count, depth [N], landmark [N])"""
        N = self.N if N is None else N
        z, ids, depth = self._camera()
        n = len(ids)
        zp, ip, dp, lp = np.full((N, 2), np.nan), np.full(N, -1, np.int32), np.full(N, np.nan), np.full(N, -1, np.int32)
        zp[:n], ip[:n], dp[:n], lp[:n] = z, ids, depth, self.last_landmarks
        return zp, ip, n, dp, lp

    def render_values(self, width=640, height=480):
        """render()'s arithmetic, restated -> (value before rint / clip [H][W] double, range in mm [H][W] double with inf
        where the ray misses, hit [H][W])"""
        v, u = np.mgrid[0:height, 0:width].astype(np.float64)
        dc = np.stack([(u - self.c[0]) / self.f[0], (v - self.c[1]) / self.f[1], np.ones_like(u)], -1).reshape(-1, 3)
        Rbc = np.stack([S.q_rota(self.q_b_c, e) for e in np.eye(3)], 1)
        Rib = np.stack([S.q_rota(self.q, e) for e in np.eye(3)], 1)
        d = dc @ (Rib @ Rbc).T
        C = self.pos + S.q_rota(self.q, self.p_b_c)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = -C[2] / d[:, 2]
        hit = np.isfinite(t) & (t > 0)
        t = np.where(hit, t, 0.0)
        X, Y = C[0] + t * d[:, 0], C[1] + t * d[:, 1]
        g = np.arange(-3.0, 3.0001, 0.22)
        ng = len(g)
        fi, fj = np.floor((X - g[0]) / 0.22).astype(int), np.floor((Y - g[0]) / 0.22).astype(int)
        blobs = np.zeros_like(X)
        for di in (0, 1):
            for dj in (0, 1):
                i, j = fi + di, fj + dj
                ok = (i >= 0) & (i < ng) & (j >= 0) & (j < ng)
                k = np.where(ok, i * ng + j, 0)
                amp = 0.55 + 0.45 * np.sin(12.9898 * k + 4.1414)
                r2 = (X - self.landmarks[k, 0]) ** 2 + (Y - self.landmarks[k, 1]) ** 2
                blobs += np.where(ok, amp * np.exp(-r2 * (1.0 / (2 * 0.045 ** 2))), 0.0)
        shade = 0.5 + 0.25 * np.sin(1.3 * X + 0.4) * np.cos(0.9 * Y - 0.2)
        val = np.where(hit, 50.0 + 60.0 * shade + 140.0 * np.minimum(blobs, 1.0), 30.0)
        rng_mm = np.where(hit, t * np.linalg.norm(d, axis=1) * 1e3, np.inf)
        return val.reshape(height, width), rng_mm.reshape(height, width), hit.reshape(height, width)

    def truth_state(self, ids):
        """the true state in the filter's layout [17 + 5 N] for the feature slots `ids` (viekf_sim_truth_state)"""
        ids = list(ids)
        x = np.full(17 + 5 * len(ids), np.nan)
        x[0:3], x[3:6], x[6:10], x[10:13], x[13:16], x[16] = self.pos, self.vel, self.q, self.accel_bias_, self.gyro_bias_, self.mu
        by_id = {fid: l for l, fid in self.feat_id.items()}
        for j, fid in enumerate(ids):
            if fid in by_id:
                pc = S.q_rotp(self.q_b_c, S.q_rotp(self.q, self.landmarks[by_id[fid]] - self.pos) - self.p_b_c)
                r = np.linalg.norm(pc)
                zt = pc / r
                # from_two_unit_vectors(e_z, zeta), reference src/quat.cpp:167-185
                if zt[2] < 1.0:
                    invs = 1.0 / math.sqrt(2.0 * (1.0 + zt[2]))
                    q = np.array([0.5 / invs, -zt[1] * invs, zt[0] * invs, 0.0])
                    q = q / np.linalg.norm(q)
                else:
                    q = np.array([1.0, 0.0, 0.0, 0.0])
                x[17 + 5 * j: 21 + 5 * j], x[21 + 5 * j] = q, 1.0 / r
        return x


def jittered_landmarks(seed, origin=-3.0, pitch=0.22, ng=28, jitter=0.08):
    """a landmark field [ng^2][3] like sim.Simulator's, with its own generator (a regular grid has exact distance ties)"""
    rng = np.random.default_rng(seed)
    g = origin + pitch * np.arange(ng)
    gx, gy = np.meshgrid(g, g, indexing="ij")
    jit = rng.uniform(-jitter, jitter, (gx.size, 2))
    return np.stack([gx.ravel() + jit[:, 0], gy.ravel() + jit[:, 1], np.zeros(gx.size)], axis=1)


# -- the scenarios the CPU and the GPU tests share ------------------------------------------------------------------------
# five vehicles with different seed, radius (0.35 ... 1.5), period and biases (tests of step and camera)
FIVE = dict(
    seed=[11, 2 ** 40 + 7, 3, 2 ** 63 + 12345, 99],
    radius=[0.35, 0.6, 0.9, 1.2, 1.5],
    period=[8.0, 7.0, 6.0, 9.0, 8.0],
    accel_bias=[[0.05, -0.04, 0.03], [0.0, 0.0, 0.0], [-0.02, 0.03, 0.01], [0.04, 0.04, -0.05], [0.01, -0.02, 0.02]],
    gyro_bias=[[0.004, -0.003, 0.002], [0.0, 0.0, 0.0], [0.001, 0.002, -0.003], [-0.004, 0.001, 0.001], [0.002, 0.002, 0.002]],
)
# four vehicles on different trajectories and seeds for the closed loop through the sequencer, N = 8, 2 s at 250 / 25 Hz
LOOP = dict(
    seed=[1, 2, 3, 4],
    radius=[0.35, 0.45, 0.3, 0.4],
    period=[8.0, 7.0, 9.0, 8.0],
    accel_bias=[[0.05, -0.04, 0.03]] * 4,
    gyro_bias=[[0.004, -0.003, 0.002]] * 4,
)
LOOP_BOUNDS = (0.6, 0.4, 2.5)      # m, m/s, degrees: those of tests/test_sim_end_to_end.py::test_hip_sequencer_on_the_simulator


def vehicles(cfg, params, num_features, landmarks, **kw):
    """one RefSimulator per vehicle of a scenario"""
    return [RefSimulator(params, num_features=num_features, seed=cfg["seed"][b], landmarks=landmarks, radius=cfg["radius"][b],
                         period=cfg["period"][b], accel_bias=cfg["accel_bias"][b], gyro_bias=cfg["gyro_bias"][b], **kw)
            for b in range(len(cfg["seed"]))]
