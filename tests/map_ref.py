"""Restatement of the device-resident landmark map (include/viekf_map.h) over oracle/np_twin.py's functions
(rotation matrices, not the product's quaternion code): a feature's 3-D position in the node frame and in the global frame,
the analytic Jacobian J of l(x [+] d) and Sigma = J P9 J^T, the store with its rules, and the error against a true landmark.
Only tests/ and tools/map_bench.py import this.  Also the flight of sim_ref.LOOP with keyframe resets on through the
restated stack, which fixes the bound of the GPU test's closed loop."""
import functools
import math

import numpy as np

from oracle import np_twin as tw
from oracle import oracle as orc
from tests import frame_ref as F
from tests import node_ref as NR
from tests import sim_ref as R

TRI = ((0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2))      # the order of a covariance's six numbers: xx, yx, yy, zx, zy, zz


def idx9(j):
    """rows and columns of P that l depends on: POS, ATT, feature j"""
    return [0, 1, 2, 6, 7, 8, 16 + 3 * j, 17 + 3 * j, 18 + 3 * j]


def tri(S):
    return np.array([S[i, j] for i, j in TRI])


def valid(x, j, ln):
    rho = x[21 + 5 * j]
    return bool(j < ln and np.isfinite(rho) and rho > 0.0)


def landmark(x, j, q_b_c, p_b_c):
    """l = pos + rota(att, p_b_c + rota(q_b_c, zeta / rho)) of feature slot j"""
    zeta = tw.rota(x[17 + 5 * j:21 + 5 * j], tw.E_Z)
    b = p_b_c + tw.rota(q_b_c, zeta / x[21 + 5 * j])
    return x[0:3] + tw.rota(x[6:10], b)


def jacobian(x, j, q_b_c, p_b_c):
    """J [3][9] = d l(x [+] d) / d d at d = 0 over the columns idx9(j), for the boxplus of vi_ekf_helper.cpp:88-98"""
    qz, rho = x[17 + 5 * j:21 + 5 * j], x[21 + 5 * j]
    zeta = tw.rota(qz, tw.E_Z)
    b = p_b_c + tw.rota(q_b_c, zeta / rho)
    RaT, RcT = tw.Rmat(x[6:10]).T, tw.Rmat(q_b_c).T
    J = np.zeros((3, 9))
    J[:, 0:3] = np.eye(3)
    J[:, 3:6] = -RaT @ tw.skew(b)
    J[:, 6:8] = -RaT @ RcT @ tw.skew(zeta) @ tw.T_zeta(qz) / rho
    J[:, 8] = -RaT @ RcT @ zeta / rho ** 2
    return J


def sigma(x, P, j, q_b_c, p_b_c):
    J = jacobian(x, j, q_b_c, p_b_c)
    i9 = idx9(j)
    L = np.tril(P[np.ix_(i9, i9)])                           # the lower triangle only, as the kernels read it
    return J @ (L + np.tril(L, -1).T) @ J.T


def to_global(node, l, S):
    """l_G = node.t + rota(node.q, l), Sigma_G = R(node.q)^T Sigma R(node.q)"""
    Rn = tw.Rmat(node[3:])
    return node[:3] + Rn.T @ l, Rn.T @ S @ Rn


def cholesky3(A, e):
    """3x3 lower Cholesky of A with e as one more row -> (info, nees) by the rule of include/viekf_diag.h"""
    L = np.zeros((3, 3))
    y = np.zeros(3)
    for j in range(3):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0.0:
            return j + 1, float("nan")
        L[j, j] = math.sqrt(d)
        for i in range(j + 1, 3):
            L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
        y[j] = (e[j] - L[j, :j] @ y[:j]) / L[j, j]
    return 0, float(y @ y)


class MapRef:
    """one filter's map: viekf_map_landmarks / _update / _error, slot by slot"""

    def __init__(self, N, q_b_c, p_b_c, capacity=0):
        self.N, self.cap = int(N), int(capacity)
        self.q_b_c, self.p_b_c = np.asarray(q_b_c, float), np.asarray(p_b_c, float)
        self.reset()

    def reset(self):
        c = self.cap
        self.ids, self.pos, self.cov = np.full(c, -1, np.int32), np.zeros((c, 3)), np.zeros((c, 6))
        self.n_obs, self.node_count = np.zeros(c, np.int32), np.zeros(c, np.int32)

    def slot(self, x, P, ln, j, node):
        """-> (l, Sigma, l_G, Sigma_G) or None for a slot that is not valid"""
        if not valid(x, j, ln):
            return None
        l, S = landmark(x, j, self.q_b_c, self.p_b_c), sigma(x, P, j, self.q_b_c, self.p_b_c)
        return (l, S) + to_global(node, l, S)

    def landmarks(self, x, P, ln, node=NR.IDENTITY):
        out = dict(pos_node=np.full((self.N, 3), np.nan), cov_node=np.full((self.N, 6), np.nan),
                   pos_global=np.full((self.N, 3), np.nan), cov_global=np.full((self.N, 6), np.nan))
        for j in range(self.N):
            s = self.slot(x, P, ln, j, node)
            if s is not None:
                out["pos_node"][j], out["cov_node"][j], out["pos_global"][j], out["cov_global"][j] = s[0], tri(s[1]), s[2], tri(s[3])
        return out

    def update(self, x, P, ln, table, table_len, node=NR.IDENTITY, count=0):
        """table [N] the intake's ids (-1 padded), table_len its length"""
        if self.cap == 0 or ln != table_len:                 # no store; a stale table: nothing moves
            return
        want = {}                                            # entry -> (id, slot): the larger id of a residue, then the later slot
        for j in range(self.N):
            g = int(table[j])
            if valid(x, j, ln) and g >= 0:
                e = g % self.cap
                if e not in want or (g, j) > want[e]:
                    want[e] = (g, j)
        for e, (g, j) in want.items():
            _, _, lg, Sg = self.slot(x, P, ln, j, node)
            self.n_obs[e] = self.n_obs[e] + 1 if self.ids[e] == g else 1
            self.ids[e], self.pos[e], self.cov[e], self.node_count[e] = g, lg, tri(Sg), count

    def error(self, x, P, ln, table, table_len, lm_true, frame_ids, lm_index, node=NR.IDENTITY, true_node=NR.IDENTITY):
        """lm_true [L][3]; frame_ids, lm_index [M] as the simulator's camera writes them"""
        out = dict(err_node=np.full((self.N, 3), np.nan), nees=np.full(self.N, np.nan), info=np.zeros(self.N, np.int32),
                   err_global=np.full((self.N, 3), np.nan))
        if ln != table_len:
            return out
        fids = [int(v) for v in frame_ids]
        for j in range(self.N):
            s, g = self.slot(x, P, ln, j, node), int(table[j])
            if s is None or g < 0 or g not in fids:
                continue
            k = int(lm_index[fids.index(g)])
            if k < 0 or k >= len(lm_true):
                continue
            e = tw.rotp(true_node[3:], lm_true[k] - true_node[:3]) - s[0]
            out["err_node"][j], out["err_global"][j] = e, lm_true[k] - s[2]
            out["info"][j], out["nees"][j] = cholesky3(s[1], e)
        return out


class BatchMapRef:
    """B independent MapRef behind the array shapes of vi_ekf_amd.LandmarkMap; nodes / true nodes [B][7] and counts [B] as
    NodeGraph.get hands them out, or None for the identity"""

    def __init__(self, batch, N, q_b_c, p_b_c, capacity=0):
        self.B = int(batch)
        self.r = [MapRef(N, q_b_c, p_b_c, capacity) for _ in range(self.B)]

    @staticmethod
    def _row(a, b, default):
        return default if a is None else a[b]

    def landmarks(self, x, P, ln, node=None):
        o = [r.landmarks(x[b], P[b], ln[b], self._row(node, b, NR.IDENTITY)) for b, r in enumerate(self.r)]
        return {k: np.stack([e[k] for e in o]) for k in o[0]}

    def update(self, x, P, ln, table, table_len, node=None, count=None):
        for b, r in enumerate(self.r):
            r.update(x[b], P[b], ln[b], table[b], table_len[b], self._row(node, b, NR.IDENTITY), self._row(count, b, 0))

    def get(self):
        return dict(ids=np.stack([r.ids for r in self.r]), pos=np.stack([r.pos for r in self.r]), cov=np.stack([r.cov for r in self.r]),
                    n_obs=np.stack([r.n_obs for r in self.r]), node_count=np.stack([r.node_count for r in self.r]))

    def error(self, x, P, ln, table, table_len, lm_true, frame_ids, lm_index, node=None, true_node=None):
        per = np.ndim(lm_true) == 3
        o = [r.error(x[b], P[b], ln[b], table[b], table_len[b], lm_true[b] if per else lm_true, frame_ids[b], lm_index[b],
                     self._row(node, b, NR.IDENTITY), self._row(true_node, b, NR.IDENTITY)) for b, r in enumerate(self.r)]
        return {k: np.stack([e[k] for e in o]) for k in o[0]}


# -- the closed loop --------------------------------------------------------------------------------------------------------
# sim_ref.LOOP, four vehicles, N = 8, 2 s at 250 / 25 Hz with use_keyframe_reset ON (threshold 0.8), landmarks
# jittered_landmarks(77), a store of LOOP_MAP_CAPACITY entries: simulator -> propagate -> intake -> node update -> map update ->
# map error on every frame.  What tests/test_map_ref_cpu.py::test_loop_through_the_restated_stack measures and prints on the
# CPU: the worst |err_node| component after t = 1 s over the features whose store entry has n_obs >= 5 is 1.3747 m (1.2072 ..
# 1.3747 over the four vehicles; the worst landmark NEES of the flight is 0.875, so Sigma covers it), LOOP_MAP_MEASURED
# rounded up.  The GPU test's bound is TWICE
# that: the device simulator draws the same Philox noise as sim_ref, so the GPU flight differs from this one through
# parity-level differences only.  The vehicles keep their first eight features and do not reset in these 2 s (that is why
# node_ref.LOOP_KFR exists); the resets with a map are tests/test_gpu_map.py's scripted frames.
LOOP_MAP_TMAX, LOOP_MAP_N, LOOP_MAP_THRESH, LOOP_MAP_CAPACITY, LOOP_MAP_MIN_OBS = 2.0, 8, 0.8, 32, 5
LOOP_MAP_MEASURED = 1.375
LOOP_MAP_BOUND = 2.0 * LOOP_MAP_MEASURED


def loop_map_params():
    p = dict(orc.EKF_YAML)
    p.update(use_keyframe_reset=True, keyframe_overlap_threshold=LOOP_MAP_THRESH)
    return p


@functools.lru_cache(maxsize=1)
def fly_loop_map():
    """-> list over the vehicles of dict(worst = the largest |err_node| component after t = 1 s over features with
    n_obs >= LOOP_MAP_MIN_OBS, counted = how many slot-frames that covers, resets, entries = filled store entries, nees_worst,
    bad = slots whose factorisation failed or whose error was NaN although tracked and in the frame)"""
    N, p = LOOP_MAP_N, loop_map_params()
    lm = R.jittered_landmarks(77)
    res = []
    for sim in R.vehicles(R.LOOP, p, N, lm, tmax=LOOP_MAP_TMAX):
        ref = F.FrameRef(orc.OracleFilter(N).init(**{k: p[k] for k in NR.F_KEYS}), LOOP_MAP_THRESH)
        nd = NR.NodeRef()
        mp = MapRef(N, p["q_b_c"], p["p_b_c"], LOOP_MAP_CAPACITY)
        st = dict(t=sim.t, worst=0.0, counted=0, nees=0.0, bad=0)

        def imu_cb(t, u, Rm, ref=ref, st=st):
            ref.f.propagate(u, t - st["t"])
            st["t"] = t

        def feat_cb(t, pix, ids, Rm, sim=sim, ref=ref, nd=nd, mp=mp, st=st):
            xt = sim.truth_state([])
            out = ref.intake(np.asarray(pix).reshape(-1, 2), list(ids), Rm)
            nd.update(out["did_reset"], out["edges"], xt)
            table = np.full(N, -1, np.int32)
            tr = ref.tracked()
            table[:len(tr)] = tr
            x, P, ln = ref.f.x, ref.f.P, ref.f.len_features
            mp.update(x, P, ln, table, len(tr), nd.node, nd.count)
            err = mp.error(x, P, ln, table, len(tr), lm, list(ids), list(sim.last_landmarks), nd.node, nd.true_node)
            for j in range(ln):
                if np.isnan(err["err_node"][j]).any() or err["info"][j] != 0:
                    st["bad"] += 1
                    continue
                st["nees"] = max(st["nees"], err["nees"][j])
                e = table[j] % mp.cap
                if t > 1.0 and mp.ids[e] == table[j] and mp.n_obs[e] >= LOOP_MAP_MIN_OBS:
                    st["worst"] = max(st["worst"], float(np.abs(err["err_node"][j]).max()))
                    st["counted"] += 1

        sim.register_imu_cb(imu_cb)
        sim.register_feat_cb(feat_cb)
        while sim.run():
            pass
        res.append(dict(worst=st["worst"], counted=st["counted"], resets=nd.count, entries=int((mp.ids >= 0).sum()),
                        nees_worst=st["nees"], bad=st["bad"]))
    return res
