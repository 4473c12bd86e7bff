"""The cases of the PER-FILTER PARAMETER SETS (viekf_batch_set_params_filters, BatchVIEKF.set_params), shared by the CPU check of
their own conditions (tests/test_perfilter_cases_cpu.py) and by the GPU test (tests/test_gpu_perfilter.py).  Plain numpy, the
oracle and -- for PIXEL_VEL, which the oracle does not state -- the numpy twin at the oracle filter's state: no GPU code, no pytest.

case(N, B, nonunit=None) is ONE script on B filters, every filter with a parameter set of its own and inputs of its own:

  0. reset (filter b at ITS x0 / P0), init_feature of slots 0 .. N - 2 from the scene's pixels (NaN depth: min_depth, camera, P0_feat)
  1. step_n(K = 2, M)      2. step_n(K = 2, M)      3. update_body([ACC, ATT])      4. update_depths(DEPTH, Md entries)
  5. update_pixel_vels(Mp entries)      6. init_feature into the free slot N - 1      7. keep_features (slot 1 goes everywhere,
  slot 0 too in the odd filters)      8. keyframe_reset (all)      9. propagate

The sets are drawn around the set of vi_ekf_amd/scene.py::make_scene (with X0_AWAY of tests/hetero_cases.py as x0 and a process
noise Qx, Qx_feat that is not zero, so that a factor on it is a change): filter b has every VARYING field at least 12 % away from
filter 0's (FACTOR_STEP per step of b mod 5), Qu a factor of 3, 1 / 3, 9 or 1 / 9 away, q_b_c and q_b_u turned by 0.1 rad per step and
renormalised, the attitude of x0 likewise; lambda stays within (0, 1].  lam_feat keeps [1, 1, x] (every filter unit-Lambda) unless
`nonunit` names a filter, which gets lam_feat[0] = 0.7.  Beyond five filters the sets repeat with b mod 5 and Qu carries a factor
1 + 1e-6 b, so that all B sets are distinct (tiled(), for the large batch: the GPU test compares it with batches of one only).

The body, depth and image-velocity measurements are the reference filter's own prediction at the state the entry meets, plus noise
well inside R; they are part of the case and stay as they are when run_filter is given another set (the sensitivity check).

case(...) -> dict: N, B, nf, params (list of B dicts), pix, u [5, B, 6], dtA, dtB [2, B], dt [B], R, zA, slotA, zB, slotB [B, M ..],
body (list of (mtype, z [B, zdim], R)), dslot, dz [B, Md], dR, pslot, pz [B, Mp, 2], gyro [B, 3], pR, keep [B, N], x0_ref, P0_ref
(after the reset), codes (dict of int arrays), x_ref, P_ref, len_ref."""
import numpy as np

from oracle import np_twin
from oracle import oracle as orc
from tests import hetero_cases as hc
from tests import meas_cases as mc
from tests import pixvel_ref as pr
from vi_ekf_amd import scene

VARYING = ("x0", "P0", "Qx", "lam", "Qu", "P0_feat", "Qx_feat", "lam_feat", "cam_center", "focal_len", "q_b_c", "p_b_c", "q_b_u",
           "min_depth")
FACTOR_STEP = 0.12
QU_FACTORS = (1.0, 3.0, 1.0 / 3.0, 9.0, 1.0 / 9.0)
TURN = 0.1                       # rad per step of b mod 5
BASE = dict(x0=hc.X0_AWAY.tolist(), Qx=[2e-3] * 16, Qx_feat=[1e-3, 1e-3, 2e-3])
ACC_NOISE, ATT_NOISE, DEPTH_NOISE = 0.02, 0.005, 0.02
R_ACC = np.array([[0.09, 0.01], [0.01, 0.16]])
R_ATT = np.array([[0.02, 0.002, 0.0], [0.002, 0.03, 0.001], [0.0, 0.001, 0.025]])
R_DEPTH = 0.1
R_PIXVEL = np.array([[225.0, 20.0], [20.0, 144.0]])
_CASES = {}


def _turned(q, angle, axis):
    q = np.asarray(q, dtype=np.float64)
    a = np.asarray(axis, dtype=np.float64)
    d = np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * a / np.linalg.norm(a)])
    out = np_twin.qmul(q, d)
    return out / np.linalg.norm(out)


def draw(base, b, nonunit=False):
    """filter b's set around `base`"""
    k = b % 5
    up, down = 1.0 + FACTOR_STEP * k, 1.0 - FACTOR_STEP * k
    p = dict(base)
    x0 = np.asarray(base["x0"], dtype=np.float64).copy()
    x0[0:6] *= up; x0[10:17] *= down
    x0[6:10] = _turned(x0[6:10], TURN * k, (1.0, -2.0, 0.5))
    p["x0"] = x0
    p["P0"] = np.asarray(base["P0"], dtype=np.float64) * up
    p["Qx"] = np.asarray(base["Qx"], dtype=np.float64) * down
    p["lam"] = np.asarray(base["lam"], dtype=np.float64) * down            # (base <= 1: stays within (0, 1])
    p["Qu"] = np.asarray(base["Qu"], dtype=np.float64) * QU_FACTORS[k] * (1.0 + 1e-6 * b)
    p["P0_feat"] = np.asarray(base["P0_feat"], dtype=np.float64) * up
    p["Qx_feat"] = np.asarray(base["Qx_feat"], dtype=np.float64) * up
    lf = np.asarray(base["lam_feat"], dtype=np.float64).copy()
    lf[2] *= down
    if nonunit:
        lf[0] = 0.7
    p["lam_feat"] = lf
    p["cam_center"] = np.asarray(base["cam_center"], dtype=np.float64) * down
    p["focal_len"] = np.asarray(base["focal_len"], dtype=np.float64) * up
    p["q_b_c"] = _turned(base["q_b_c"], TURN * k, (0.3, 1.0, -0.7))
    p["p_b_c"] = np.asarray(base["p_b_c"], dtype=np.float64) * up
    p["q_b_u"] = _turned(base["q_b_u"], TURN * k, (-1.0, 0.4, 0.8))
    p["min_depth"] = float(base["min_depth"]) * up
    assert (p["lam"] > 0).all() and (p["lam"] <= 1).all() and (lf > 0).all() and (lf <= 1).all()
    return p


def oracle_kw(p):
    return {k: p[k] for k in mc.ORACLE_KEYS}


def _twin_at(f, N, p):
    t = np_twin.TwinFilter(N, **oracle_kw(p))
    t.x = f.x.copy()
    low = np.tril(f.P)
    t.P = low + np.tril(low, -1).T
    t.len = int(f.len_features)
    return t


def run_filter(c, b, p=None, write=None, rng=None):
    """filter b of case c through the script on the oracle with the set p (default: its own) -> dict x0, P0, x, P, len, codes.
    write: the case under construction -- the predicted measurements of steps 3 .. 5 are drawn (rng) and stored in it."""
    N, nf = c["N"], c["nf"]
    p = c["params"][b] if p is None else p
    f = orc.OracleFilter(N).init(**oracle_kw(p))
    out = dict(x0=f.x.copy(), P0=f.P.copy())
    codes = {}
    for i in range(nf):
        assert f.init_feature(c["pix"][b, i], i)
    for tag, u, dts in (("A", c["u"][0:2], c["dtA"]), ("B", c["u"][2:4], c["dtB"])):
        for k in range(2):
            f.propagate(u[k, b], float(dts[k, b]))
        sl = c["slot" + tag][b]
        codes[tag] = np.array([f.update(orc.FEAT, c["z" + tag][b, m], c["R"], True, int(sl[m])) for m in range(len(sl))], dtype=np.int32)
    if write is not None:
        write["body"][0][1][b] = f.x[10:12] - f.x[16] * f.x[3:5] + rng.normal(0, ACC_NOISE, 2)
    cb = [f.update(orc.ACC, c["body"][0][1][b], R_ACC, True, -1)]
    if write is not None:
        write["body"][1][1][b] = orc.q_boxplus(f.x[6:10], rng.normal(0, ATT_NOISE, 3))
    cb.append(f.update(orc.ATT, c["body"][1][1][b], R_ATT, True, -1))
    codes["body"] = np.array(cb, dtype=np.int32)
    cd = []
    for m, s in enumerate(c["dslot"][b]):
        if write is not None:
            write["dz"][b, m] = 1.0 / f.x[17 + 5 * s + 4] + rng.normal(0, DEPTH_NOISE)
        cd.append(f.update(orc.DEPTH, [c["dz"][b, m]], [[R_DEPTH]], True, int(s)))
    codes["depth"] = np.array(cd, dtype=np.int32)
    t = _twin_at(f, N, p)
    cp = []
    for m, s in enumerate(c["pslot"][b]):
        if write is not None:
            zhat, _ = pr.h_pixel_vel(t, t.x, int(s), c["gyro"][b])
            write["pz"][b, m] = zhat + rng.uniform(-2.0, 2.0, 2)
        cp.append(pr.update_pixel_vel(t, int(s), c["pz"][b, m], c["gyro"][b], R_PIXVEL, 0.0, True))
    codes["pixvel"] = np.array(cp, dtype=np.int32)
    f.x[:] = t.x
    f.P[:, :] = t.P
    codes["init"] = np.array([int(f.init_feature(c["pix"][b, N - 1], -1))], dtype=np.int32)
    ids = f.feature_ids
    for s in range(len(ids)):
        if not c["keep"][b, s]:
            f.clear_feature(ids[s])
    out["len_kept"] = int(f.len_features)
    out["edge"] = f.keyframe_reset_edge()
    f.propagate(c["u"][4, b], float(c["dt"][b]))
    out.update(x=f.x.copy(), P=f.P.copy(), len=int(f.len_features), codes=codes)
    return out


def inputs(N, B, nonunit=None):
    """the sets and every input that does not depend on a filter's state"""
    nf = N - 1
    M, Md, Mp = min(nf, 20), min(nf, 4), min(nf, 3)
    sc = scene.make_scene(B, N, 5, 7300 + 11 * N + B, params=BASE)
    r = np.random.default_rng(7400 + 13 * N + B)
    params = [draw(sc["params"], b, nonunit == b) for b in range(B)]
    dt = scene.DT * (0.5 + 0.25 * (np.arange(B) % 5))
    c = dict(N=N, B=B, nf=nf, params=params, pix=sc["pix"], u=sc["u"], R=np.asarray(sc["R"], dtype=np.float64).reshape(2, 2), dt=dt,
             dtA=np.ascontiguousarray(dt[None, :] * np.array([1.0, 1.1])[:, None]),
             dtB=np.ascontiguousarray(dt[None, :] * np.array([0.9, 1.2])[:, None]))
    for tag in "AB":
        slot = np.stack([r.permutation(nf)[:M] for _ in range(B)]).astype(np.int32)
        c["slot" + tag] = slot
        c["z" + tag] = np.stack([sc["pix"][b, slot[b]] for b in range(B)]) + r.normal(0.0, 0.5, (B, M, 2))
    c["body"] = [(orc.ACC, np.zeros((B, 2)), R_ACC), (orc.ATT, np.zeros((B, 4)), R_ATT)]
    c["dslot"] = np.stack([r.permutation(nf)[:Md] for _ in range(B)]).astype(np.int32)
    c["dz"] = np.zeros((B, Md))
    c["dR"] = R_DEPTH
    c["pslot"] = np.stack([r.permutation(nf)[:Mp] for _ in range(B)]).astype(np.int32)
    c["pz"] = np.zeros((B, Mp, 2))
    c["gyro"] = r.normal(0.0, 0.2, (B, 3))
    c["pR"] = R_PIXVEL
    keep = np.ones((B, N), dtype=np.uint8)
    keep[:, 1] = 0
    keep[1::2, 0] = 0
    c["keep"] = keep
    return c, r


def case(N, B, nonunit=None):
    key = (N, B, nonunit)
    if key not in _CASES:
        c, r = inputs(N, B, nonunit)
        runs = [run_filter(c, b, write=c, rng=r) for b in range(B)]
        c["x0_ref"], c["P0_ref"] = np.stack([o["x0"] for o in runs]), np.stack([o["P0"] for o in runs])
        c["x_ref"], c["P_ref"] = np.stack([o["x"] for o in runs]), np.stack([o["P"] for o in runs])
        c["len_ref"] = np.array([o["len"] for o in runs], dtype=np.int32)
        c["len_kept"] = np.array([o["len_kept"] for o in runs], dtype=np.int32)
        c["edge_ref"] = np.stack([o["edge"] for o in runs])
        c["codes"] = {k: np.stack([o["codes"][k] for o in runs]) for k in runs[0]["codes"]}
        for a in [c["x_ref"], c["P_ref"], c["zA"], c["zB"], c["dz"], c["pz"], c["body"][0][1], c["body"][1][1]]:
            a.setflags(write=False)
        _CASES[key] = c
    return _CASES[key]


def tiled(c, B):
    """case c repeated to B filters (inputs of filter b: those of b mod c.B); the sets drawn anew, so that all B differ"""
    src = np.arange(B) % c["B"]
    t = dict(N=c["N"], B=B, nf=c["nf"], R=c["R"], dR=c["dR"], pR=c["pR"])
    base = scene.make_scene(1, c["N"], 1, 1, params=BASE)["params"]
    t["params"] = [draw(base, b) for b in range(B)]
    for k in ("pix", "dt", "zA", "slotA", "zB", "slotB", "dslot", "dz", "pslot", "pz", "gyro", "keep"):
        t[k] = np.ascontiguousarray(c[k][src])
    for k in ("u", "dtA", "dtB"):
        t[k] = np.ascontiguousarray(c[k][:, src])
    t["body"] = [(m, np.ascontiguousarray(z[src]), R) for m, z, R in c["body"]]
    return t


def one(c, b):
    """filter b of case c as a case of one filter (what a batch of one is given)"""
    return tiled_rows(c, [b])


def tiled_rows(c, rows):
    rows = np.asarray(rows)
    t = dict(N=c["N"], B=len(rows), nf=c["nf"], R=c["R"], dR=c["dR"], pR=c["pR"], params=[c["params"][int(b)] for b in rows])
    for k in ("pix", "dt", "zA", "slotA", "zB", "slotB", "dslot", "dz", "pslot", "pz", "gyro", "keep"):
        t[k] = np.ascontiguousarray(c[k][rows])
    for k in ("u", "dtA", "dtB"):
        t[k] = np.ascontiguousarray(c[k][:, rows])
    t["body"] = [(m, np.ascontiguousarray(z[rows]), R) for m, z, R in c["body"]]
    return t


# (N, B, nonunit) of the cases the GPU test holds against the oracle
ORACLE_CASES = [(3, 3, None), (12, 5, None), (50, 4, None), (50, 4, 2), (90, 3, None)]
