"""The device-resident frame intake (include/viekf_frame.h, vi_ekf_amd.FrameIntake) against its restatement
tests/frame_ref.py, by the project's parity rule: integers exact, floats max|d| <= 1e-9 max|ref| per array on
the active block -- and against itself where the claim is bit for bit: several features per launch against one per launch,
device pointers against host pointers, a batch against batches of one, ring slots against the batch's own buffers."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import frame_ref as F
from tests import sim_ref as R
from tests.test_frame_ref_cpu import CLOSED_LOOP_BOUNDS

pytestmark = pytest.mark.gpu

STREAMING, RESIDENT = 1, 2
DT = 0.004
OUT_KEYS = ("result", "gated", "gated_count", "did_reset", "edges")


def _params(**kw):
    p = dict(orc.EKF_YAML)
    p.update(kw)
    return p


def _batch(B, N, p, family=0):
    import vi_ekf_amd as v
    g = v.BatchVIEKF(B, N, dict(p, keyframe_overlap_threshold=0.8, name="frame"))
    if family:
        g.set_kernel(family)
    return g


def close(a, ref, rel=1e-9):
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape
    return np.abs(a - ref).max() <= rel * np.abs(ref).max() if a.size else True


def active_block(x, P, ln):
    """x and P with everything past each filter's features zeroed"""
    x, P = x.copy(), P.copy()
    for b in range(x.shape[0]):
        x[b, 17 + 5 * ln[b]:] = 0.0
        m = 16 + 3 * ln[b]
        P[b, m:, :] = 0.0
        P[b, :, m:] = 0.0
    return x, P


def state(g):
    return g.get_state(), g.get_covariance(), g.get_len_features()


def same_bits(sa, sb):
    return all(np.array_equal(a, b, equal_nan=True) for a, b in zip(sa, sb))


def against_ref(out, fi, g, rout, ref, what=""):
    """every output of an intake, the table and the filter against the restatement"""
    for k in ("result", "gated", "gated_count", "did_reset"):
        assert np.array_equal(np.asarray(out[k]), rout[k]), (what, k, out[k], rout[k])
    assert close(out["edges"], rout["edges"]), (what, "edges")
    ids, ln = fi.tracked()
    rids, rln = ref.tracked()
    assert np.array_equal(ids, rids) and np.array_equal(ln, rln), (what, ids, rids)
    x, P, glen = state(g)
    rx, rP, rlen = ref.state()
    assert np.array_equal(glen, rlen) and np.array_equal(glen, ln), (what, glen, rlen)
    x, P = active_block(x, P, glen)
    rx, rP = active_block(rx, rP, rlen)
    assert close(x, rx) and close(P, rP), (what, np.abs(x - rx).max(), np.abs(P - rP).max())


def hover(K, B, seed):
    rng = np.random.default_rng(seed)
    u = np.zeros((K, B, 6))
    u[:, :, 2] = -9.80665
    u += rng.normal(0.0, 0.01, u.shape)
    return u, np.full((K, B), DT)


def pix(gid, cols=11, px=40.0, py=35.0):
    return np.array([120.0 + px * (gid % cols), 90.0 + py * (gid // cols % 9)])


def frame(rng, B, M, rows, far=(), nan=(), spread=100):
    """rows: the id row (shorter than M: -1 padded) every filter gets, offset by `spread` * b so that the tables differ;
    far / nan: indices of entries whose pixel is moved by 300 px / is NaN"""
    ids = np.full((B, M), -1, np.int32)
    z = np.full((B, M, 2), np.nan)
    depth = np.full((B, M), np.nan)
    for b in range(B):
        for i, gid in enumerate(rows):
            if gid < 0:
                continue
            ids[b, i] = gid + spread * b
            z[b, i] = pix(gid) + 3.0 * b + rng.normal(0.0, 0.5, 2)
            if i % 2 == 0:
                depth[b, i] = 2.0 + 0.1 * i + 0.05 * b
            if i in far:
                z[b, i] += 300.0
            if i in nan:
                z[b, i, i % 2] = np.nan
    return z, ids, depth


def noise(B, M, r_mode):
    if r_mode == 0:
        return np.array([[10.0, 0.5], [0.5, 12.0]])
    Rm = np.zeros((B, M, 2, 2))
    for b in range(B):
        for i in range(M):
            Rm[b, i] = [[10.0 + i, 0.3 * b], [0.3 * b, 12.0 + 0.5 * i]]
    return Rm


# ---- several features per launch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [12, 50])
def test_multi_init_equals_sequential_init(N):
    """k_init_features against the same number of k_init_feature launches, bit for bit: x, all of P, len.  B = 3 with 0, 1
    and more new features than free slots, NaN and finite depth mixed, P packed on entry (a step_n ran before)."""
    import vi_ekf_amd as v
    B, k0, extra = 3, N - 3, 6
    p = _params(use_keyframe_reset=False)
    rng = np.random.default_rng(5)
    ga, gb = _batch(B, N, p), _batch(B, N, p)
    z0, ids0, _ = frame(rng, B, k0, list(range(k0)), spread=0)
    u, dt = hover(2, B, 1)
    for g in (ga, gb):
        for j in range(k0):
            g.init_feature(z0[:, j].copy(), np.full(B, np.nan))
        g.step_n(u, dt, None, None, None)
    fi = v.FrameIntake(ga)
    tr = np.full((B, N), -1, np.int32)
    tr[:, :k0] = ids0
    fi.set_tracked(tr)
    M = k0 + extra
    zn, idn, dn = frame(rng, B, M, list(range(M)), spread=0)
    zn[:, :k0] = np.nan                                     # the tracked ids are present, without an update
    count = [0, 1, extra]
    for b in range(B):
        idn[b, k0 + count[b]:] = -1
    out = fi.intake(zn, idn, noise(B, M, 0), depth=dn)
    for j in range(extra):
        mask = np.array([j < c for c in count], np.uint8)
        gb.init_feature(zn[:, k0 + j].copy(), dn[:, k0 + j].copy(), mask)
    assert np.array_equal(ga.get_len_features(), [k0, k0 + 1, N])
    assert same_bits(state(ga), state(gb))
    assert (out["result"][2, k0:] == 4).all() and (out["result"][:, :k0] == 2).all() and (out["result"][0, k0:] == -1).all()
    assert np.array_equal(fi.tracked()[0][2], list(range(N)))            # (the overflow found no slot and is not in the table)


# ---- scripted frames ----------------------------------------------------------------------------------------------------
#          ids of a frame (filter b sees them + 100 b)          far     nan    inactive filters
SCRIPT = [
    ([0, 1, 2, 3, 4, 5, 6, 7],                                   (),     (),    ()),       # fills the filter
    ([1, 2, 3, 4, 5, 6, 7],                                      (),     (),    ()),       # first slot dropped
    ([1, 2, 3, 5, 6, 7],                                         (),     (),    ()),       # a middle slot
    ([1, 2, 3, 5, 6, 8, 9],                                      (),     (),    ()),       # the last slot; two new
    ([20, 21, 22, 23, 24, 25],                                   (),     (),    (3,)),     # all new: overlap 0
    ([20, 21, 22, 23, 24, 25, 26, 27, 28, 29],                   (),     (),    (3,)),     # overfull: two of four fit
    ([20, 21, 22, 23, 24, 25, 26, 27, 40],                       (),     (1, 8), ()),      # NaN on a tracked and an untracked id
    ([20, 21, 20, 22, 23, 24, 25, 26, 27, 22],                   (),     (),    ()),       # repeats
    ([20, -1, 21, 22, -1, 23, 24, 25, 26, 27],                   (),     (),    ()),       # padding in the middle
    ([20, 21, 22, 23, 24, 25, 26, 27],                           (3, 6), (),    ()),       # two gated
    ([],                                                         (),     (),    ()),       # an empty frame
    ([50, 51, 52],                                               (),     (),    (1,)),
    ([52, 51, 50, 53],                                           (),     (),    ()),
]


@pytest.mark.parametrize("r_mode", [0, 2])
@pytest.mark.parametrize("family", [STREAMING, RESIDENT])
@pytest.mark.parametrize("use_kfr", [0, 1])
def test_scripted_frames_against_the_restatement(use_kfr, family, r_mode):
    import vi_ekf_amd as v
    B, N, M, K = 5, 8, 10, 3
    p = _params(use_keyframe_reset=bool(use_kfr))
    g, ref = _batch(B, N, p, family), F.BatchFrameRef(B, N, p, 0.8)
    fi = v.FrameIntake(g)
    rng = np.random.default_rng(7)
    Rm = noise(B, M, r_mode)
    seen = set()
    resets = 0
    for k, (rows, far, nan, off) in enumerate(SCRIPT):
        u, dt = hover(K, B, 100 + k)
        g.step_n(u, dt, None, None, None)
        ref.propagate(u, dt)
        z, ids, depth = frame(rng, B, M, rows, far, nan)
        active = None
        if off:
            active = np.ones(B, np.uint8)
            active[list(off)] = 0
        out = fi.intake(z, ids, Rm, depth=depth, active=active)
        rout = ref.intake(z, ids, Rm, depth=depth, active=active)
        against_ref(out, fi, g, rout, ref, "frame %d" % k)
        seen |= set(np.unique(out["result"]).tolist())
        resets += int(out["did_reset"].sum())
        for b in off:
            assert (out["result"][b] == -1).all() and out["gated_count"][b] == 0 and not out["did_reset"][b]
    assert seen == {-1, 0, 1, 2, 3, 4}                       # every answer occurred
    assert (resets > 0) == bool(use_kfr)
    assert g.get_status().max() < 8


# ---- tables wider than a wave -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,family", [(77, RESIDENT), (150, STREAMING)])
def test_tables_wider_than_a_wave(N, family):
    """N and M past 64: the chunked ballots, with drops on both sides of index 64.  Only a dozen entries a frame carry a
    pixel (the others are present with NaN z), which keeps the dense reference quick."""
    import vi_ekf_amd as v
    B, M = 2, N + 3
    p = _params(use_keyframe_reset=True)
    g, ref = _batch(B, N, p, family), F.BatchFrameRef(B, N, p, 0.8)
    fi = v.FrameIntake(g)
    rng = np.random.default_rng(11)
    Rm = noise(B, M, 0)

    def wide(rows, live):
        ids = np.full((B, M), -1, np.int32)
        z = np.full((B, M, 2), np.nan)
        for b in range(B):
            for i, gid in enumerate(rows):
                ids[b, i] = gid + 1000 * b
                if live is None or gid in live:
                    z[b, i] = np.array([40.0 + 37.0 * (gid % 16), 40.0 + 43.0 * (gid // 16 % 10)]) + 2.0 * b + rng.normal(0.0, 0.5, 2)
        return z, ids

    first = list(range(M))                                   # three more than fit
    drop1 = {3, 60, 63, 64, 70, N - 1}
    second = [i for i in range(N) if i not in drop1] + [500, 501, 502, 503, 504, 505, 506, 507]
    drop2 = {0, 10, 65, 66, 500}
    third = [i for i in second if i not in drop2][::-1]
    live = {1, 2, 61, 62, 67, 68, 71, N - 2, 501, 502, 503, 505}
    for k, (rows, lv) in enumerate(((first, None), (second, live | set(range(500, 508))), (third, live))):
        u, dt = hover(2, B, 200 + k)
        g.step_n(u, dt, None, None, None)
        ref.propagate(u, dt)
        z, ids = wide(rows, lv)
        out = fi.intake(z, ids, Rm)
        rout = ref.intake(z, ids, Rm)
        against_ref(out, fi, g, rout, ref, "frame %d" % k)
    assert (g.get_len_features() == N - len(drop2)).all() and (out["result"] == 0).sum() >= 2 * 10


# ---- bit for bit ----------------------------------------------------------------------------------------------------------
def fly(g, fi, frames, conv=None, steps=True):
    """the frames of SCRIPT-like tuples through one intake -> list of outputs (numpy)"""
    outs = []
    for k, (z, ids, depth, active, Rm) in enumerate(frames):
        if steps:
            u, dt = hover(2, g.B, 300 + k)
            g.step_n(u, dt, None, None, None)
        if conv:
            o = fi.intake(conv(z), conv(ids), conv(Rm), depth=conv(depth), active=None if active is None else conv(active))
            assert all(o[k].is_cuda for k in OUT_KEYS)
            o = {k: o[k].cpu().numpy() for k in OUT_KEYS}
        else:
            o = fi.intake(z, ids, Rm, depth=depth, active=active)
        outs.append(o)
    return outs


def script_frames(B, N, M, seed, r_mode=0, count=None):
    rng = np.random.default_rng(seed)
    fr = []
    for rows, far, nan, off in SCRIPT[:count]:
        rows = [r for r in rows][:M]
        z, ids, depth = frame(rng, B, M, rows, far, nan)
        active = None
        if off:
            active = np.ones(B, np.uint8)
            active[[o % B for o in off]] = 0
        fr.append((z, ids, depth, active, noise(B, M, r_mode)))
    return fr


def test_device_pointers_equal_host_pointers():
    import torch
    import vi_ekf_amd as v
    B, N, M = 4, 8, 10
    p = _params(use_keyframe_reset=True)
    frames = script_frames(B, N, M, 13, r_mode=2)
    gh, gd = _batch(B, N, p), _batch(B, N, p)
    fh, fd = v.FrameIntake(gh), v.FrameIntake(gd)
    oh = fly(gh, fh, frames)
    od = fly(gd, fd, frames, conv=lambda a: None if a is None else torch.as_tensor(a).cuda().contiguous())
    for a, b in zip(oh, od):
        for k in OUT_KEYS:
            assert np.array_equal(a[k], b[k]), k
    assert same_bits(state(gh), state(gd))
    th, td = fh.tracked(), fd.tracked(device=True)
    assert td[0].is_cuda and np.array_equal(th[0], td[0].cpu().numpy()) and np.array_equal(th[1], td[1].cpu().numpy())


def test_a_filter_does_not_depend_on_its_batch():
    """B = 300 at N = 12 against batches of one (one handle, reset between filters), bit for bit.  Both run the streaming
    family: which resident instance a batch gets depends on its size, and that is not what this test is about."""
    import vi_ekf_amd as v
    B, N, M, nf = 300, 12, 14, 4
    p = _params(use_keyframe_reset=True)
    rng = np.random.default_rng(17)
    frames = []
    for k in range(nf):
        z = np.full((B, M, 2), np.nan)
        ids = np.full((B, M), -1, np.int32)
        for b in range(B):
            rows = rng.permutation(20)[:rng.integers(0, M + 1)] if k else np.arange(12)      # a random subset of 20 ids
            for i, gid in enumerate(rows):
                ids[b, i] = gid
                z[b, i] = pix(int(gid), cols=5, px=90.0, py=80.0) + rng.normal(0.0, 0.5, 2)
        frames.append((z, ids, None, None, noise(B, M, 0)))
    g = _batch(B, N, p, STREAMING)
    outs = fly(g, v.FrameIntake(g), frames)
    x, P, ln = state(g)
    g1 = _batch(1, N, p, STREAMING)
    f1 = v.FrameIntake(g1)
    hv = [hover(2, B, 300 + k) for k in range(nf)]
    for b in range(B):
        g1.reset()
        f1.reset()
        for k, (z, ids, _, _, Rm) in enumerate(frames):
            u, dt = hv[k]
            g1.step_n(u[:, b:b + 1].copy(), dt[:, b:b + 1].copy(), None, None, None)
            o = f1.intake(z[b:b + 1], ids[b:b + 1], Rm)
            for key in OUT_KEYS:
                assert np.array_equal(o[key][0], outs[k][key][b]), (b, k, key)
        x1, P1, l1 = state(g1)
        assert l1[0] == ln[b] and np.array_equal(x1[0], x[b]) and np.array_equal(P1[0], P[b]), b
    assert len(set(ln.tolist())) > 3


def test_per_filter_live_slots_are_followed():
    """B = 3 with a history ring and select_filters: the same frames as on a batch that works in its own buffers"""
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, N, M = 3, 8, 10
    p = _params(use_keyframe_reset=True)
    frames = script_frames(B, N, M, 19, count=6)
    ga, gb = _batch(B, N, p), _batch(B, N, p)
    gb.history_resize(4)
    live = np.array([2, 0, 3], np.int32)
    capi.check(capi.lib().viekf_batch_snapshot_filters(gb._h, C.c_void_p(live.ctypes.data), capi.HOST))
    gb.select_filters(live)
    oa = fly(ga, v.FrameIntake(ga), frames, steps=False)
    ob = fly(gb, v.FrameIntake(gb), frames, steps=False)
    for a, b in zip(oa, ob):
        for k in OUT_KEYS:
            assert np.array_equal(a[k], b[k]), k
    assert same_bits(state(ga), state(gb)) and ga.get_len_features().max() > 0


def test_stale_table():
    """a feature started behind the intake's back: INVALID, nothing moves; set_tracked adopts the state"""
    import vi_ekf_amd as v
    B, N, M = 2, 8, 10
    p = _params(use_keyframe_reset=True)
    g, ref = _batch(B, N, p), F.BatchFrameRef(B, N, p, 0.8)
    fi = v.FrameIntake(g)
    rng = np.random.default_rng(23)
    Rm = noise(B, M, 0)
    z, ids, _ = frame(rng, B, M, [0, 1, 2, 3], spread=0)
    against_ref(fi.intake(z, ids, Rm), fi, g, ref.intake(z, ids, Rm), ref, "first")
    px = np.tile(pix(9), (B, 1))
    assert g.init_feature(px, np.full(B, np.nan)).all()
    for r in ref.r:
        assert r.f.init_feature(px[0], 9)
        r.f._p.contents.feature_ids[r.f.len_features - 1] = 9
    before, tab = state(g), fi.tracked()
    z, ids, _ = frame(rng, B, M, [0, 1, -1, 3, 9], spread=0)
    out = fi.intake(z, ids, Rm)
    assert np.array_equal(out["result"][0], [3, 3, -1, 3, 3, -1, -1, -1, -1, -1]) and np.array_equal(out["result"][0], out["result"][1])
    assert not out["did_reset"].any() and not out["gated_count"].any() and not out["edges"].any()
    assert same_bits(before, state(g)) and np.array_equal(tab[0], fi.tracked()[0]) and np.array_equal(tab[1], fi.tracked()[1])
    fi.set_tracked(np.array([[0, 1, 2, 3, 9, -1, -1, -1]] * B, np.int32))
    against_ref(fi.intake(z, ids, Rm), fi, g, ref.intake(z, ids, Rm), ref, "adopted")
    assert (g.get_len_features() == 4).all()


# ---- closed loop ----------------------------------------------------------------------------------------------------------
def test_closed_loop_with_nothing_crossing_to_the_host():
    """four vehicles of sim_ref.LOOP drive four filters for 2 s (250 Hz IMU, 25 Hz frames, N = 8): BatchSimulator.step ->
    step_n -> camera -> intake, every array between the calls a CUDA tensor.  After t = 1 s the errors stay inside the bounds
    tests/test_frame_ref_cpu.py fixed by flying the restated stack; the true state in the intake's slot order makes the
    consistency diagnostics finite."""
    import torch
    import vi_ekf_amd as v
    B, N = 4, 8
    p = _params(use_keyframe_reset=False)
    per = {k: R.LOOP[k] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    bs = v.BatchSimulator(B, p, max_features=N, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5, **per)
    bs.set_landmarks(R.jittered_landmarks(77))
    g = _batch(B, N, p)
    fi = v.FrameIntake(g)
    R_pix = torch.diag(torch.tensor([10.0, 10.0], dtype=torch.float64)).cuda()
    dt = torch.full((10, B), bs.dt, dtype=torch.float64, device="cuda")
    worst = np.zeros((B, 3))
    for f in range(50):
        u = bs.step(10, device=True)
        g.step_n(u, dt, None, None, None)
        z, ids, cnt, dep, _ = bs.camera(N, device=True)
        out = fi.intake(z, ids, R_pix)
        assert u.is_cuda and z.is_cuda and ids.is_cuda and all(out[k].is_cuda for k in OUT_KEYS)
        if bs.t > 1.0:                                        # (the test's own look at the state, not part of the loop)
            x, (st, _) = g.get_state(), bs.truth()
            assert not np.isnan(x[:, :17]).any()
            for b in range(B):
                e = [np.abs(x[b, 0:3] - st[b, 0:3]).max(), np.abs(x[b, 3:6] - st[b, 7:10]).max(),
                     np.degrees(np.abs(orc.q_boxminus(x[b, 6:10], st[b, 3:7])).max())]
                worst[b] = np.maximum(worst[b], e)
    print("closed loop on the device, worst errors (m, m/s, deg):", worst.max(axis=0))
    assert (worst < np.array(CLOSED_LOOP_BOUNDS)).all(), worst
    assert (worst > 0).all() and (cnt.cpu().numpy() == N).all()
    tracked, ln = fi.tracked(device=True)
    assert tracked.is_cuda and np.array_equal(ln.cpu().numpy(), g.get_len_features())
    diag = v.consistency(g, bs.truth_state(tracked))
    g.sync()
    assert (diag["info"].cpu().numpy() == 0).all() and np.isfinite(diag["nees"].cpu().numpy()).all()
    assert np.isfinite(diag["logdet"].cpu().numpy()).all()


# ---- argument rules -------------------------------------------------------------------------------------------------------
def test_argument_rules():
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, N, M = 2, 4, 5
    p = _params()
    g = _batch(B, N, p)
    fi = v.FrameIntake(g)
    rng = np.random.default_rng(29)
    z, ids, depth = frame(rng, B, M, [0, 1, 2], spread=0)
    Rm = noise(B, M, 0)
    with pytest.raises(ValueError, match="mix"):
        fi.intake(torch.as_tensor(z).cuda(), ids, Rm)
    with pytest.raises(ValueError, match="mix"):
        fi.intake(z, ids, Rm, active=torch.ones(B, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="shape"):
        fi.intake(z[:, :4], ids, Rm)
    with pytest.raises(ValueError, match="shape"):
        fi.intake(z, ids, Rm, depth=depth[:1])
    with pytest.raises(ValueError, match="R must"):
        fi.intake(z, ids, np.zeros((3, 2, 2)))
    with pytest.raises(ValueError, match="shape"):
        fi.set_tracked(np.zeros((B, N + 1), np.int32))
    for bad in (0, 4097):
        with pytest.raises(v.ViekfError) as e:
            fi.intake(np.zeros((B, bad, 2)), np.full((B, bad), -1, np.int32), Rm)
        assert e.value.code == capi.ERR_INVALID and "4096" in str(e.value)
    L, h = capi.lib(), fi._h
    ptr = C.c_void_p(z.ctypes.data)
    assert L.viekf_frame_intake(h, M, None, ptr, None, ptr, 0, None, None, None, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_frame_intake(h, M, ptr, ptr, None, ptr, 3, None, None, None, None, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_frame_intake(h, M, ptr, ptr, None, ptr, 0, None, None, None, None, None, None, 7) == capi.ERR_INVALID
    g.init_feature(np.tile(pix(0), (B, 1)), np.full(B, np.nan))
    g.init_feature(np.tile(pix(1), (B, 1)), np.full(B, np.nan))
    for rows in ([[5, 5, -1, -1]] * B, [[5, -1, -1, -1]] * B, [[5, 6, 7, -1]] * B, [[5, -1, 6, -1]] * B):      # repeat, short, long, gap
        with pytest.raises(v.ViekfError) as e:
            fi.set_tracked(np.array(rows, np.int32))
        assert e.value.code == capi.ERR_INVALID and "set_tracked" in str(e.value)
    fi.set_tracked(np.array([[5, 6, -1, -1]] * B, np.int32))
    assert np.array_equal(fi.tracked()[1], [2, 2])
    capi.check(L.viekf_batch_set_active(g._h, C.c_void_p(np.ones(B, np.uint8).ctypes.data), capi.HOST))
    with pytest.raises(v.ViekfError, match="participation"):
        fi.intake(z, ids, Rm)
    capi.check(L.viekf_batch_set_active(g._h, None, capi.HOST))
    out = fi.intake(z, ids, Rm)                               # every output optional: the call with none of them
    assert L.viekf_frame_intake(h, M, ptr, C.c_void_p(ids.ctypes.data), None, C.c_void_p(np.ascontiguousarray(Rm.T).ctypes.data), 0,
                                None, None, None, None, None, None, capi.HOST) == capi.OK
    assert out["result"].shape == (B, M)
    # a destroyed batch: the intake refuses to go on, and its own tables can still be released
    g.close()
    with pytest.raises(ValueError, match="closed"):
        fi.intake(z, ids, Rm)
    with pytest.raises(ValueError, match="closed"):
        v.FrameIntake(g)
    fi.close()
    with pytest.raises(ValueError, match="closed"):
        fi.tracked()
