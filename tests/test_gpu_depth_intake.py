"""FrameIntake.intake_depth (viekf_frame_intake_depth, include/viekf_depth.h) behind FrameIntake.intake of the same frame, on
device pointers, against tests/depth_ref.py driving the oracle in the same order: which entries get a DEPTH, their codes, and
x and P by the parity rule of tests/test_gpu_frame.py.  The frames hold a new id, a NaN pixel, a NaN depth, a repeated id, a
gated FEAT and an inactive filter at once."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import depth_ref as D
from tests import frame_ref as F
from tests.test_gpu_frame import _batch, _params, against_ref, frame, noise, same_bits, state

pytestmark = pytest.mark.gpu

B = 3
INACTIVE = 1
# (N, M, first frame's id row, second frame's id row, far, nan pixel, nan depth): the second frame holds the ids of the first
# (tracked: FEAT + DEPTH), a NEW id, a REPEATED id, an entry 300 px off (FEAT gated: it still gets its DEPTH), a NaN pixel and
# a NaN depth
FRAMES = {
    5: (5, 8, [0, 1, 2, 3], [0, 1, 2, 3, 7, 1, -1, -1], (2,), (1,), (3,)),
    17: (17, 17, list(range(12)), list(range(12)) + [40, 5, 41, -1, -1], (2, 9), (1,), (3, 6)),
}


def second_frame(rng, N):
    n_, M, rows1, rows2, far, nanpix, nandepth = FRAMES[N]
    z, ids, depth = frame(rng, B, M, rows2, far, nanpix)
    for b in range(B):
        for i, gid in enumerate(rows2):
            if gid >= 0:
                depth[b, i] = 2.0 + 0.1 * i + 0.05 * b          # every entry has a depth ...
    depth[:, list(nandepth)] = np.nan                          # ... but these
    return z, ids, depth


def to_dev(torch, *arrays):
    return [None if a is None else torch.tensor(a, device="cuda:0") for a in arrays]


def fly(N, use_depth=True, r_mode=2):
    """frame 1 (every id new), propagates, frame 2 with intake and intake_depth on device pointers; the same on the oracle
    -> everything the tests compare"""
    import torch
    import vi_ekf_amd as v
    n_, M, rows1, rows2, far, nanpix, nandepth = FRAMES[N]
    p = _params(use_keyframe_reset=False)
    g, ref = _batch(B, N, p), F.BatchFrameRef(B, N, p, 0.8)
    fi = v.FrameIntake(g)
    rng = np.random.default_rng(300 + N)
    Rm = noise(B, M, 0)
    z, ids, depth = frame(rng, B, M, rows1)
    against_ref(fi.intake(z, ids, Rm, depth=depth), fi, g, ref.intake(z, ids, Rm, depth=depth), ref, "first frame")
    u = np.zeros((2, B, 6))
    u[:, :, 2] = -9.80665
    dt = np.full((2, B), 0.004)
    g.step_n(u, dt, None, None, None)
    ref.propagate(u, dt)
    z, ids, depth = second_frame(rng, N)
    active = np.ones(B, np.uint8)
    active[INACTIVE] = 0
    Rd = (0.04, np.array([0.03, 0.04, 0.05]), 0.02 + 0.01 * np.arange(B * M, dtype=np.float64).reshape(B, M) / (B * M))[r_mode]
    dz, dids, ddepth, dRm, dact = to_dev(torch, z, ids, depth, Rm, active)
    out = fi.intake(dz, dids, dRm, depth=ddepth, active=dact)
    rout = ref.intake(z, ids, Rm, depth=depth, active=active)
    fres = out["result"].cpu().numpy()
    against_ref({k: out[k].cpu().numpy() for k in out}, fi, g, rout, ref, "second frame")
    return dict(g=g, fi=fi, ref=ref, out=out, fres=fres, z=z, ids=ids, depth=depth, active=active, Rd=Rd, dev=(dids, ddepth, dact),
                torch=torch, M=M)


@pytest.mark.parametrize("N,r_mode", [(5, 2), (17, 0), (17, 1)])
def test_intake_then_intake_depth(N, r_mode):
    s = fly(N, r_mode=r_mode)
    torch, g, fi, ref = s["torch"], s["g"], s["fi"], s["ref"]
    n_, M, rows1, rows2, far, nanpix, nandepth = FRAMES[N]
    dids, ddepth, dact = s["dev"]
    dR = s["Rd"] if r_mode == 0 else torch.tensor(s["Rd"], device="cuda:0")
    res = fi.intake_depth(s["out"], dids, ddepth, dR, True, dact).cpu().numpy()
    want = D.intake_depth(ref, s["ids"], s["depth"], s["fres"], s["Rd"], True, s["active"])
    assert np.array_equal(res, want), (res, want)
    # which entries got a DEPTH: the tracked ids with a depth, the FEAT-gated one among them; not the new id (NEW_FEATURE), the
    # NaN pixel (MEAS_NAN), the NaN depth, the repeat (INVALID), the padding, the inactive filter
    fres = s["fres"]
    for b in range(B):
        for i in range(M):
            got_depth = res[b, i] != -1
            assert got_depth == (b != INACTIVE and D.is_measurement(int(s["ids"][b, i]), int(fres[b, i]), s["depth"][b, i])), (b, i)
    live = [b for b in range(B) if b != INACTIVE]
    assert (fres[live][:, list(far)] == orc.MEAS_GATED).all() and (res[live][:, list(far)] == 0).all()
    assert (fres[live][:, list(nanpix)] == orc.MEAS_NAN).all() and (fres[live] == orc.MEAS_NEW_FEATURE).any() and (fres[live] == orc.MEAS_INVALID).any()
    assert (res[live][:, list(nandepth)] == -1).all() and (res[INACTIVE] == -1).all() and (res[live] == 0).sum() >= 2 * (len(rows1) - 3)
    o = {k: s["out"][k].cpu().numpy() for k in s["out"]}
    against_ref(o, fi, g, o, ref, "after intake_depth")      # (the intake's outputs were compared in fly(): here the table, x and P)
    P = g.get_covariance()
    assert np.array_equal(P, P.transpose(0, 2, 1))
    assert g.get_status().max() < 8


def test_use_depth_off_runs_fix_depth_only():
    """use_depth = 0: the measurements are inactive -- SUCCESS, x and P as the oracle's inactive updates leave them (fix_depth
    only: here nothing to fix, so the filters are bit for bit as the intake left them)"""
    s = fly(5)
    g, fi, ref = s["g"], s["fi"], s["ref"]
    dids, ddepth, dact = s["dev"]
    before = state(g)
    res = fi.intake_depth(s["out"]["result"], dids, ddepth, 0.04, False, dact).cpu().numpy()
    want = D.intake_depth(ref, s["ids"], s["depth"], s["fres"], 0.04, False, s["active"])
    assert np.array_equal(res, want) and (res == 0).any() and set(np.unique(res)) == {-1, 0}
    assert same_bits(before, state(g))
    assert np.array_equal(state(g)[2], ref.state()[2])


def test_stale_table_and_an_id_that_left_the_table():
    """a feature started behind the intake's back: every id >= 0 answers INVALID and nothing moves.  After set_tracked adopts
    the state, an id that is not in the table answers INVALID on its own and the others are applied"""
    s = fly(17)                                                        # (14 of 17 slots taken: room for one more feature)
    g, fi, ref, torch = s["g"], s["fi"], s["ref"], s["torch"]
    dids, ddepth, dact = s["dev"]
    M = s["M"]
    px = np.tile(np.array([500.0, 300.0]), (B, 1))
    mask = np.array([1, 0, 0], np.uint8)
    assert g.init_feature(px, np.full(B, np.nan), mask)[0] == 1          # filter 0 only: its table is stale now
    before = state(g)
    res = fi.intake_depth(s["out"], dids, ddepth, 0.04, True, dact).cpu().numpy()
    assert (res[0][s["ids"][0] >= 0] == orc.MEAS_INVALID).all() and (res[0][s["ids"][0] < 0] == -1).all() and (res[INACTIVE] == -1).all()
    ref.r[0].f.init_feature(px[0], 99)
    ref.r[0].f._p.contents.feature_ids[ref.r[0].f.len_features - 1] = 99
    want = D.intake_depth(ref, s["ids"], s["depth"], s["fres"], 0.04, True, s["active"], stale=(0,))
    assert np.array_equal(res, want)
    x, P, ln = state(g)
    assert np.array_equal(x[0], before[0][0]) and np.array_equal(P[0], before[1][0])
    # adopt; then claim a FEAT success for an id the table does not hold
    tab, tl = ref.tracked()
    fi.set_tracked(tab)
    ids2 = s["ids"].copy()
    ids2[:, 0] = 77 + 100 * np.arange(B)
    fres2 = s["fres"].copy()
    res = fi.intake_depth(torch.tensor(fres2, device="cuda:0"), torch.tensor(ids2, device="cuda:0"), ddepth, 0.04, True, None).cpu().numpy()
    want = D.intake_depth(ref, ids2, s["depth"], fres2, 0.04, True, None)
    assert np.array_equal(res, want) and (res[[0, 2], 0] == orc.MEAS_INVALID).all() and (res == 0).any()      # (filter 1 had no frame)


def test_argument_rules():
    import ctypes as C
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    g = _batch(2, 5, _params())
    fi = v.FrameIntake(g)
    L, h = capi.lib(), fi._h
    ids, dep, fr, R = np.zeros((2, 4), np.int32), np.full((2, 4), 3.0), np.zeros((2, 4), np.int32), np.array([0.04])
    p = lambda a: C.c_void_p(a.ctypes.data)
    before = state(g)
    assert L.viekf_frame_intake_depth(h, 0, p(ids), p(dep), p(fr), p(R), 0, 1, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_frame_intake_depth(h, capi.DEPTHS_MAX_M + 1, p(ids), p(dep), p(fr), p(R), 0, 1, None, None, capi.HOST) == capi.ERR_INVALID
    for k in range(4):
        a = [p(ids), p(dep), p(fr), p(R)]
        a[k] = None
        assert L.viekf_frame_intake_depth(h, 4, a[0], a[1], a[2], a[3], 0, 1, None, None, capi.HOST) == capi.ERR_INVALID, k
    assert L.viekf_frame_intake_depth(h, 4, p(ids), p(dep), p(fr), p(R), 3, 1, None, None, capi.HOST) == capi.ERR_INVALID
    assert L.viekf_frame_intake_depth(h, 4, p(ids), p(dep), p(fr), p(R), 0, 1, None, None, 7) == capi.ERR_INVALID
    assert same_bits(before, state(g))
    res = fi.intake_depth(fr, ids, dep, 0.04)                            # host arrays; no id is tracked: INVALID
    assert res.shape == (2, 4) and (res == orc.MEAS_INVALID).all() and same_bits(before, state(g))
