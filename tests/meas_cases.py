"""One script of generic measurement updates and feature-lifecycle calls on a RAGGED batch, shared by the CPU check of its
own conditions (tests/test_meas_cases_cpu.py) and the GPU parity test (tests/test_gpu_generic_update.py).  Plain numpy and the
oracle: no GPU code, no pytest.

build(N, partial, drag, seed) warms B = 5 oracle filters up (all N features, two steps of M = min(N, 8) FEAT updates, so that
P is dense), and writes the script while running it on CLONES of them: every z is the oracle's own prediction at the state
the call will meet, plus seeded noise.  It returns the scene, the warm filters (the state the script starts from) and the
script, a list of (kind, args):

  update          args: mtype, z [B, zdim], R ([r, r] shared or [B, r, r] per filter), slot [B] or None (LOCAL slots),
                  active [B] or None (0 = fix_depth only, 2 = the filter skips the call)
  init_feature    args: pix [B, 2], depth [B], mask [B] or None
  keep_features   args: keep [B, N]
  keyframe_reset  args: mask [B]
  propagate       args: u [B, 6], dt [B]        (between two generic updates: it leaves P packed or, above N = 77, current in
                                                 the lower triangle only; the next update enters from there, provided the
                                                 caller does not read P in between)
  poison_P        args: b, i, j                 (P[b, i, j] = P[b, j, i] = NaN, through set_state on the device)

Every args also carries `label`, `expect` ({filter: result code} of the results that are NOT 0, or {filter: ok} / the new
lengths for the lifecycle calls) and `untouched` (the filters whose x and P the call must leave bit for bit).

The ragged fill is len = [N, N - 3, 1, 0, N - 1], made by keep_features from the middle outwards.  The oracle addresses
features by GLOBAL id, numbers them itself and ignores the id passed to init_feature, so after a drop local slot s is no
longer id s: apply_oracle maps slots to ids through the filter's own table.  (A wrong id does not raise, it measures slot -1.)
"""
import numpy as np

from oracle import oracle as orc
from vi_ekf_amd import scene

B = 5
NEEDS_SLOT = (orc.QZETA, orc.FEAT, orc.DEPTH, orc.INV_DEPTH)
NEG_DEPTH_FILTERS = (1, 2, 3)     # filters whose newest feature is fresh when the negative-depth INV_DEPTH arrives
POISONED = 4                      # filter that gets a NaN into P
ORACLE_KEYS = ("x0", "P0", "Qx", "lam", "Qu", "P0_feat", "Qx_feat", "lam_feat", "cam_center", "focal_len", "q_b_c", "p_b_c",
               "q_b_u", "min_depth", "use_drag_term", "use_partial_update", "use_keyframe_reset")


# (N, partial, drag) of the GPU test: the smallest sizes that reach each regime -- N = 5: n = 31, ld = 32 (odd n, one pad row);
# 50: n = ld = 166, the headline size (fused launches leave P packed); 77: n = 247, ld = 248, the last on-chip size; 83: n = 265,
# ld = 272 (seven pad rows, matrix-core propagate)
CASES = [(5, 1, 1), (50, 1, 1), (77, 1, 1), (83, 1, 1), (5, 0, 0), (83, 0, 0)]
_BUILT = {}


def cached(N, partial, drag):
    """build() once per case; the filters are the shared reference and stay as they are: run clones of them"""
    key = (N, partial, drag)
    if key not in _BUILT:
        _BUILT[key] = build(N, partial, drag, 300 + N)
    sc, fs, script = _BUILT[key]
    return sc, [f.clone() for f in fs], script


def nan_split(got, ref):
    """two arrays that must have their NaNs in the same places -> both with the NaNs replaced by 0, for a comparison of the rest"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    bad = np.isnan(ref)
    assert np.array_equal(np.isnan(got), bad), "NaNs in different places"
    return np.where(bad, 0.0, got), np.where(bad, 0.0, ref)


def fill(N):
    """the ragged feature counts after the first keep_features"""
    return [N, N - 3, 1, 0, N - 1]


def warm_m(N):
    return min(N, 8)


def _drop_order(N):
    """slots ordered from the middle outwards"""
    mid = (N - 1) / 2.0
    return sorted(range(N), key=lambda s: (abs(s - mid), s))


def first_keep(N):
    keep = np.ones((B, N), dtype=np.uint8)
    order = _drop_order(N)
    for b, ln in enumerate(fill(N)):
        keep[b, order[:N - ln]] = 0
    return keep


def lens(fs):
    return np.array([f.len_features for f in fs], dtype=np.int32)


def apply_oracle(fs, kind, a):
    """run one script entry on the oracle filters -> what the device call returns (result codes, ok, new lengths, edges)"""
    if kind == "update":
        mtype, z, R = a["mtype"], a["z"], np.asarray(a["R"])
        res = np.zeros(B, dtype=np.int32)
        for b, f in enumerate(fs):
            act = 1 if a["active"] is None else int(a["active"][b])
            sl = int(a["slot"][b]) if a["slot"] is not None else 0
            # -1 (the filter skips the call, slot < 0), 3 (slot not tracked) and 2 (NaN in z) are the C ABI's own answers,
            # decided before the filter is looked at: the oracle has no such call, so they are stated here, in the kernel's
            # order, and the filter is left alone.  (A check of them against `expect` on the CPU checks the script, not the oracle.)
            if act == 2:                                       # the filter skips the call
                res[b] = -1
            elif mtype in NEEDS_SLOT and not 0 <= sl < f.len_features:
                res[b] = -1 if sl < 0 else orc.MEAS_INVALID
            elif np.isnan(z[b]).any():
                res[b] = orc.MEAS_NAN
            else:
                gid = f.feature_ids[sl] if mtype in NEEDS_SLOT else -1
                res[b] = f.update(mtype, z[b], R[b] if R.ndim == 3 else R, bool(act), gid)
        return res
    if kind == "init_feature":
        ok = np.zeros(B, dtype=np.int32)
        for b, f in enumerate(fs):
            if a["mask"] is None or a["mask"][b]:
                ok[b] = int(f.init_feature(a["pix"][b], -1, float(a["depth"][b])))
        return ok
    if kind == "keep_features":
        for b, f in enumerate(fs):
            ids = f.feature_ids
            for s in range(len(ids)):
                if not a["keep"][b, s]:
                    f.clear_feature(ids[s])
        return lens(fs)
    if kind == "keyframe_reset":
        edge = np.zeros((B, 17))
        for b, f in enumerate(fs):
            if a["mask"][b]:
                edge[b] = f.keyframe_reset_edge()
        return edge
    if kind == "propagate":
        for b, f in enumerate(fs):
            f.propagate(a["u"][b], float(a["dt"][b]))
        return None
    if kind == "poison_P":
        fs[a["b"]].P[a["i"], a["j"]] = np.nan
        fs[a["b"]].P[a["j"], a["i"]] = np.nan
        return None
    raise ValueError(kind)


def make_filters(sc, N):
    prm = {k: sc["params"][k] for k in ORACLE_KEYS}
    fs = [orc.OracleFilter(N).init(**prm) for _ in range(B)]
    for i in range(N):
        for b in range(B):
            fs[b].init_feature(sc["pix"][b, i], i)
    return fs


def warm_inputs(sc, N, s):
    """z, slot of warm step s: the first M measurements of the scene's frame"""
    M = warm_m(N)
    return np.ascontiguousarray(sc["z"][s][:, :M, :]), np.ascontiguousarray(sc["slot"][:, :M])


def _spd(r, d):
    """per-filter R, SPD and not diagonal: 0.05 (A A^T + d I)"""
    A = r.normal(0.0, 1.0, (B, d, d))
    return 0.05 * (A @ A.transpose(0, 2, 1) + d * np.eye(d))


def build(N, partial, drag, seed):
    sc = scene.make_scene(B, N, 2, seed, params=dict(use_partial_update=partial, use_drag_term=drag))
    fs = make_filters(sc, N)
    for s in range(2):
        z, slot = warm_inputs(sc, N, s)
        for b in range(B):
            fs[b].run_steps(sc["u"][s, b][None], sc["dt"][b], z[b][None], slot[b], sc["R"])
    run = [f.clone() for f in fs]      # the script is written against these; fs stays at the warm state
    r = np.random.default_rng(seed + 1000)
    script = []
    rho0 = 1.0 / (2.0 * sc["params"]["min_depth"])

    def emit(kind, label, expect=None, untouched=(), **a):
        a.update(label=label, expect=dict(expect or {}), untouched=tuple(untouched))
        script.append((kind, a))
        return apply_oracle(run, kind, a)

    def update(label, mtype, z, R, slot=None, active=None, expect=None, untouched=()):
        return emit("update", label, expect, untouched, mtype=mtype, z=np.ascontiguousarray(z, dtype=np.float64),
                    R=np.asarray(R, dtype=np.float64), slot=None if slot is None else np.asarray(slot, dtype=np.int32),
                    active=None if active is None else np.asarray(active, dtype=np.uint8))

    X = lambda: np.stack([f.x.copy() for f in run])
    last = lambda: np.maximum(lens(run) - 1, 0).astype(np.int32)        # slot[b] = len[b] - 1; the empty filter passes 0
    feat = lambda b, k: run[b].x[17 + 5 * last()[b] + k]
    empty = lambda: {b: orc.MEAS_INVALID for b in range(B) if run[b].len_features == 0}

    emit("keep_features", "ragged fill", expect=dict(enumerate(fill(N))), untouched=(0,), keep=first_keep(N))
    assert list(lens(run)) == fill(N)

    # ---- one measurement per model, R per filter and not diagonal (r_mode 1) ----
    x = X()
    if drag:
        update("ACC (drag)", orc.ACC, x[:, 10:12] - x[:, 16:17] * x[:, 3:5] + r.normal(0, 0.1, (B, 2)), _spd(r, 2))
    else:
        update("ACC (gravity)", orc.ACC, np.stack([run[b].h(orc.ACC)[0][:3] for b in range(B)]) + r.normal(0, 0.1, (B, 3)),
               _spd(r, 3))
    update("ALT", orc.ALT, -X()[:, 2:3] + r.normal(0, 0.05, (B, 1)), _spd(r, 1))
    update("ATT", orc.ATT, np.stack([orc.q_boxplus(run[b].x[6:10], r.normal(0, 0.02, 3)) for b in range(B)]), _spd(r, 3))
    update("POS", orc.POS, X()[:, 0:3] + r.normal(0, 0.05, (B, 3)), _spd(r, 3))
    update("VEL", orc.VEL, X()[:, 3:6] + r.normal(0, 0.05, (B, 3)), _spd(r, 3))
    # The propagate, and straight after it an update of the LAST feature: its column of P lies almost wholly above the diagonal,
    # which is what a propagate that keeps only the lower triangle current leaves stale.  That update lists no untouched filter
    # (the empty filter's invalid slot is pinned bit for bit by the three feature models after it), so that a caller has no
    # reason to read P between the two calls.
    emit("propagate", "propagate between two generic updates", u=sc["u"][1].copy(), dt=sc["dt"].copy())
    e = empty()
    assert list(e) == [3]
    sl = last()
    qf = np.stack([orc.q_feat_boxplus(run[b].x[17 + 5 * sl[b]:21 + 5 * sl[b]] if b not in e else [1.0, 0, 0, 0],
                                      r.normal(0, 0.01, 2)) for b in range(B)])
    update("QZETA", orc.QZETA, qf, _spd(r, 2), slot=sl, expect=e)
    dep = np.stack([[(1.0 / feat(b, 4) if b not in e else 3.0) + r.normal(0, 0.05)] for b in range(B)])
    update("DEPTH", orc.DEPTH, dep, _spd(r, 1), slot=sl, expect=e, untouched=e)
    rho = np.stack([[(feat(b, 4) if b not in e else rho0) + r.normal(0, 0.01)] for b in range(B)])
    update("INV_DEPTH", orc.INV_DEPTH, rho, _spd(r, 1), slot=sl, expect=e, untouched=e)
    zf = np.stack([(run[b].h(orc.FEAT, None, run[b].feature_ids[sl[b]])[0][:2] if b not in e else np.array([300.0, 200.0]))
                   + r.normal(0, 0.5, 2) for b in range(B)])
    update("FEAT", orc.FEAT, zf, sc["R"], slot=sl, expect=e, untouched=e)

    # ---- edge calls ----
    # 0 runs fix_depth only, 2 returns -1 and leaves the filter alone
    update("POS, mixed active", orc.POS, X()[:, 0:3] + r.normal(0, 0.05, (B, 3)), _spd(r, 3), active=[1, 0, 2, 1, 0],
           expect={2: -1}, untouched=(2,))
    update("POS 50 m off (gated)", orc.POS, X()[:, 0:3] + 50.0, _spd(r, 3), expect={b: orc.MEAS_GATED for b in range(B)},
           untouched=range(B))
    z = X()[:, 3:6] + r.normal(0, 0.05, (B, 3))
    z[1, 2] = np.nan
    update("VEL with a NaN in z of filter 1", orc.VEL, z, _spd(r, 3), expect={1: orc.MEAS_NAN}, untouched=(1,))
    # init_feature on the ragged batch: the full filter and the masked one answer ok == 0
    mask = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    full = [b for b in range(B) if run[b].len_features == N]
    assert full == [0]
    ok = {b: int(bool(mask[b]) and b not in full) for b in range(B)}
    emit("init_feature", "init_feature with a depth, under a mask", expect=ok, untouched=[b for b in ok if not ok[b]],
         pix=sc["pix"][:, 0, :] + 3.0, depth=np.full(B, 4.0), mask=mask)
    full = [b for b in range(B) if run[b].len_features == N]
    ok = {b: int(b not in full) for b in range(B)}
    emit("init_feature", "init_feature with depth NaN", expect=ok, untouched=full, pix=sc["pix"][:, 1 % N, :] - 2.0,
         depth=np.full(B, np.nan), mask=None)
    # fix_depth after an ACCEPTED update: the fresh feature (rho0, P_rr = P0_feat[2]) is driven to rho < 0 by z = -2 rho0;
    # the two full filters, whose newest feature is an old one, get an ordinary measurement
    fresh = [b for b in range(B) if b not in full]
    assert tuple(fresh) == NEG_DEPTH_FILTERS
    sl = last()
    z = np.stack([[-2.0 * rho0] if b in fresh else [feat(b, 4) + r.normal(0, 0.01)] for b in range(B)])
    for b in fresh:
        assert run[b].x[21 + 5 * sl[b]] == rho0
    update("INV_DEPTH that drives rho negative", orc.INV_DEPTH, z, np.array([[0.01]]), slot=sl)
    # keep_features on the ragged batch again: the first of filter 0, the last of filter 1, nothing of the others
    keep = np.ones((B, N), dtype=np.uint8)
    keep[0, 0] = 0
    keep[1, run[1].len_features - 1] = 0
    nl = lens(run) - [1, 1, 0, 0, 0]
    emit("keep_features", "keep_features again", expect=dict(enumerate(int(v) for v in nl)), untouched=(2, 3, 4), keep=keep)
    # a NaN in a body row of P: K has a NaN, the update is skipped (vi_ekf_meas.cpp:247), fix_depth runs, the code is 0
    emit("poison_P", "NaN into P", b=POISONED, i=2, j=7)
    update("ALT on a P with a NaN", orc.ALT, -X()[:, 2:3] + r.normal(0, 0.05, (B, 1)), _spd(r, 1), untouched=(POISONED,))
    # keyframe reset under a mask (the dense N P N^T of the oracle would smear the NaN: the poisoned filter stays out)
    mask = np.array([1, 0, 1, 1, 0], dtype=np.uint8)
    emit("keyframe_reset", "keyframe_reset under a mask", untouched=(1, 4), mask=mask)
    update("POS after the reset", orc.POS, X()[:, 0:3] + r.normal(0, 0.05, (B, 3)), _spd(r, 3), untouched=(POISONED,))
    return sc, fs, script
