"""The device-resident flight recorder (include/viekf_rec.h, vi_ekf_amd.FlightRecorder) against its restatement
tests/rec_ref.py (Kabsch by SVD, rotation matrices) fed the arrays `get` returns, by the tolerance of tests/test_gpu_parity.py
(max|d| <= 1e-9 max|ref| per array and 1e-6 element-wise); the NaN pattern and the integer outputs exact -- and against itself
where the claim is bit for bit: two calls, device pointers against host pointers, `get` against what was pushed.

align_pose, and ate_att which depends on it, are compared only where the alignment is unique: under "se3" where the relative
gap between the two largest eigenvalues of Horn's matrix (rec_ref's) is > 1e-3, under "yaw" where the two arguments of the
atan2 are not both tiny (or there is one frame at most: both sides take theta = 0).  With the inputs here that leaves out the
"se3" cases of T <= 2 only, where every rotation about the line through the two points is a maximiser.  ate_pos does not
depend on which maximiser is taken and is always compared."""
import numpy as np
import pytest

from tests import node_ref as NR
from tests import rec_ref as RR
from tests import sim_ref as R
from tests.test_gpu_node import cuda, host
from tests.test_gpu_parity import assert_close
from tests.test_rec_ref_cpu import circle, moved, random_pose, yaw_pose

pytestmark = pytest.mark.gpu

TE_KEYS = ("ate_pos", "ate_att", "rpe_pos", "rpe_att", "align_pose", "n_used")


def bits(a):
    return np.ascontiguousarray(host(a)).view(np.uint8)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def batch(B):
    import vi_ekf_amd as v
    from oracle import oracle as orc
    return v.BatchVIEKF(B, 1, dict(orc.EKF_YAML, name="rec"))


def flights(rng, B, T, shift=0.0):
    """-> (est, tru [B][T][7]): B noisy circles (2 cm, radii 1 .. 1.5 m), every estimate moved by a pose of its own so that the
    alignments have something to find"""
    est, tru = np.zeros((B, T, 7)), np.zeros((B, T, 7))
    for b in range(B):
        e, tru[b] = circle(rng, T, shift=shift, radius=1.0 + 0.5 * rng.uniform())
        est[b] = moved(np.concatenate([rng.normal(0.0, 0.3, 3), yaw_pose(rng)[3:]]), e) if b % 2 else e
        if shift:                                            # (moved() rotates about the origin: bring the estimate back beside the truth)
            est[b, :, :3] += tru[b, :, :3].mean(axis=0) - est[b, :, :3].mean(axis=0) + rng.normal(0.0, 0.2, 3)
    return est, tru


def truth_rows(tru_k, ldx, fill=0.25):
    """[B][7] -> x_true [B][ldx] in the layout of viekf_sim_truth_state: position 0:3, attitude 6:10"""
    x = np.full((tru_k.shape[0], ldx), fill)
    x[:, 0:3], x[:, 6:10] = tru_k[:, :3], tru_k[:, 3:]
    return x


def record(fr, est, tru, chan=None, mask=None, device=False, ldx=11, t0=0.5):
    dev = cuda if device else (lambda a: a)
    for k in range(est.shape[1]):
        fr.push(dev(np.ascontiguousarray(est[:, k])), dev(truth_rows(tru[:, k], ldx)), chan=None if chan is None else dev(np.ascontiguousarray(chan[k])),
                mask=None if mask is None else dev(np.ascontiguousarray(mask[:, k])), stamp=t0 + 0.04 * k)


def held(got, ref, what, rows=None):
    """the NaN pattern exact, the rest by assert_close; rows: the filters to compare"""
    got, ref = host(got), np.asarray(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if rows is not None:
        got, ref = got[rows], ref[rows]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (what, got, ref)
    if (~nan).any():
        assert_close(got[~nan], ref[~nan], what)


def trajectory_against_ref(fr, rec, align, delta, first=0, last=None, what="", device=False):
    out = fr.trajectory_error(align, first, last, delta, device=device)
    ref = RR.trajectory_error(rec["est"], rec["tru"], rec["valid"], align, first, last, delta)
    assert np.array_equal(host(out["n_used"]), ref["n_used"]), (what, host(out["n_used"]), ref["n_used"])
    n = ref["n_used"][:, 0]
    unique = {"none": n >= 0, "yaw": (ref["yaw_gap"] > 1e-3) | (n <= 1), "se3": ref["gap"] > 1e-3}[align]
    for k in ("ate_pos", "rpe_pos", "rpe_att"):
        held(out[k], ref[k], "%s %s %s delta %d" % (what, align, k, delta))
    # where the alignment is not unique the outputs still carry the NaN pattern
    assert np.array_equal(np.isnan(host(out["ate_att"])), n == 0) and np.array_equal(np.isnan(host(out["align_pose"])).all(axis=1), n == 0)
    if unique.any():
        held(out["ate_att"], ref["ate_att"], "%s %s ate_att" % (what, align), unique)
        held(out["align_pose"], ref["align_pose"], "%s %s align_pose" % (what, align), unique)
    q = host(out["align_pose"])[n > 0, 3:]
    assert (np.abs(np.linalg.norm(q, axis=1) - 1.0) <= 1e-12).all() and (q[:, 0] >= 0).all()
    return out, ref, unique


def batch_reductions_against_ref(fr, rec, lo=None, hi=None, first=0, last=None, what="", device=False):
    ens = fr.pose_ensemble(first, last, device=device)
    rens = RR.pose_ensemble(rec["est"], rec["tru"], rec["valid"], first, last)
    assert np.array_equal(host(ens)[:, 0], rens[:, 0]), what
    held(ens, rens, what + " pose_ensemble")
    if rec["chan"].shape[2] == 0:
        return ens, None
    ch = fr.channels(None if lo is None else (cuda(lo) if device else lo), None if hi is None else (cuda(hi) if device else hi), first, last,
                     device=device)
    rch = RR.channels(rec["chan"], lo, hi, first, last)
    for k in ("per_frame", "per_filter"):
        g, r = host(ch[k]), rch[k]
        assert np.array_equal(g[..., 0], r[..., 0]) and np.array_equal(g[..., 3:], r[..., 3:]), (what, k)   # counts and fractions: exact
        assert np.array_equal(g[..., 2], r[..., 2], equal_nan=True), (what, k, "max")
        held(g[..., 1], r[..., 1], "%s %s mean" % (what, k))
    return ens, ch


# ---- frame counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 64, 65, 257])
def test_frame_counts(T):
    """B = 3, a recorder of capacity T filled to the last frame (T = capacity exactly): one frame, a pair, the smallest count
    with a unique SE(3) alignment, one wave of lanes, one more, one past the 256-lane stride.  All three alignments with
    delta = 1, 5 and T (no pair: NaN)."""
    import vi_ekf_amd as v
    B = 3
    rng = np.random.default_rng(100 + T)
    est, tru = flights(rng, B, T)
    fr = v.FlightRecorder(batch(B), T, 0)
    record(fr, est, tru)
    assert fr.count == T
    rec = fr.get()
    assert same(rec["est"], est) and same(rec["tru"], tru) and rec["valid"].all() and rec["chan"].shape == (T, B, 0)
    compared = 0
    for align in RR.ALIGN:
        for delta in (1, 5, T):
            out, ref, unique = trajectory_against_ref(fr, rec, align, delta, what="T = %d" % T)
            assert (ref["n_used"] == [T, max(T - delta, 0)]).all()
            assert np.isnan(host(out["rpe_pos"])).all() == (delta >= T)
            compared += int(unique.sum())
        assert unique.all() or (align == "se3" and T <= 2), (align, T, ref["gap"])
    assert compared >= 6 * B
    batch_reductions_against_ref(fr, rec, what="T = %d" % T)


# ---- batch sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 65, 300])
def test_batch_sizes(B):
    """T = 8, K = 3: one lane, one wave plus a lane, more than one workgroup's worth of filters for the two reductions over the
    batch; every tenth filter sits a frame out, and the chi-square bounds are the caller's"""
    import vi_ekf_amd as v
    T, K = 8, 3
    rng = np.random.default_rng(200 + B)
    est, tru = flights(rng, B, T)
    chan = rng.chisquare(6, (T, B, K))
    mask = np.ones((B, T), np.uint8)
    mask[::10, 3] = 0
    fr = v.FlightRecorder(batch(B), T + 2, K)
    record(fr, est, tru, chan, mask, ldx=10)
    rec = fr.get()
    assert np.array_equal(rec["valid"], mask) and same(rec["chan"], chan)
    lo, hi = np.array([1.64, 2.0, 0.5]), np.array([12.59, 9.0, 20.0])
    ens, ch = batch_reductions_against_ref(fr, rec, lo, hi, what="B = %d" % B)
    assert ens[3, 0] == B - len(range(0, B, 10)) and (host(ch["per_frame"])[:, :, 0] == B).all()
    batch_reductions_against_ref(fr, rec, None, hi, what="B = %d, no lower bound" % B)
    trajectory_against_ref(fr, rec, "yaw", 1, what="B = %d" % B)


# ---- masks with holes -------------------------------------------------------------------------------------------------------
def test_masks_with_holes():
    """B = 5, T = 70: filter 0 is never valid, filter 1 once, filter 2 has a NaN (and an infinite) pose entry on some frames --
    the device finds those itself, the mask says valid --, filter 3 is masked out of every third frame, filter 4 flies whole.
    Channels carry NaN and infinities that are left out one by one; a channel with nothing finite gives n = 0, NaN, NaN, 0, 0."""
    import vi_ekf_amd as v
    B, T, K = 5, 70, 2
    rng = np.random.default_rng(300)
    est, tru = flights(rng, B, T)
    mask = np.ones((B, T), np.uint8)
    mask[0] = 0
    mask[1] = 0
    mask[1, 33] = 1
    mask[3, ::3] = 0
    est[2, 10, 5] = np.nan
    tru[2, 11, 0] = np.inf
    est[2, 40, 1] = -np.inf
    tru[2, 41, 6] = np.nan
    chan = rng.chisquare(6, (T, B, K))
    chan[5, 4, 0] = np.nan
    chan[6, :, 1] = np.nan
    chan[:, 3, 1] = np.inf
    chan[7, 2, 0] = -np.inf
    fr = v.FlightRecorder(batch(B), 128, K)
    record(fr, est, tru, chan, mask, ldx=17)
    rec = fr.get()
    want = mask.copy()
    want[2, [10, 11, 40, 41]] = 0
    assert np.array_equal(rec["valid"], want)
    assert same(rec["est"], est) and same(rec["tru"], tru) and same(rec["chan"], chan)       # stored as given, NaN and all
    for align in RR.ALIGN:
        for delta in (1, 3):
            out, ref, _ = trajectory_against_ref(fr, rec, align, delta, what="holes")
            assert ref["n_used"][:2].tolist() == [[0, 0], [1, 0]] and ref["n_used"][2, 0] == T - 4
            o = {k: host(out[k]) for k in TE_KEYS}
            assert np.isnan(o["ate_pos"][0]) and np.isnan(o["align_pose"][0]).all() and np.isnan(o["rpe_pos"][:2]).all()
            assert o["ate_pos"][1] == 0.0 or align == "none"
    ens, ch = batch_reductions_against_ref(fr, rec, np.array([1.0, 1.0]), np.array([12.0, 12.0]), what="holes")
    pf, pb = host(ch["per_frame"]), host(ch["per_filter"])
    assert pf[5, 0, 0] == B - 1 and pf[7, 0, 0] == B - 1 and pf[6, 1].tolist()[0] == 0 and np.isnan(pf[6, 1, 1:3]).all() and (pf[6, 1, 3:] == 0).all()
    assert pb[3, 1, 0] == 0 and np.isnan(pb[3, 1, 1]) and pb[4, 0, 0] == T - 1
    assert host(ens)[33, 0] == 3 + 0 and host(ens)[10, 0] == 2      # frame 33: filters 1, 2, 4 (3 is masked: 33 % 3 == 0); frame 10: 3 and 4


# ---- far from the origin ----------------------------------------------------------------------------------------------------
def test_shifted_trajectories():
    """the circles 1e4 m from the origin in x and y, T = 75, B = 3: align_pose and the ATE inside the tolerance for all three
    alignments.  A kernel that formed A as sum p_t p_e^T - n c_t c_e^T would lose nine digits here and put the translation of
    align_pose centimetres out (tests/test_rec_ref_cpu.py measures 1e-7 relative in A): 1e-9 of 1e4 m is 10 micrometres."""
    import vi_ekf_amd as v
    B, T = 3, 75
    rng = np.random.default_rng(400)
    est, tru = flights(rng, B, T, shift=1e4)
    assert np.abs(tru[:, :, :2]).min() > 9e3
    fr = v.FlightRecorder(batch(B), T, 0)
    record(fr, est, tru)
    rec = fr.get()
    for align in RR.ALIGN:
        out, ref, unique = trajectory_against_ref(fr, rec, align, 1, what="shifted")
        assert unique.all()
        if align != "none":
            assert (host(out["ate_pos"]) < 0.1).all() and (host(out["ate_pos"]) > 0.01).all()
            # the aligned estimate lands on the truth: align_pose * T_est against T_true, frame by frame, to the ATE's order
            ap = host(out["align_pose"])
            for b in range(B):
                d = tru[b, :, :3] - np.array([RR.pose_mul(ap[b], est[b, k])[:3] for k in range(T)])
                assert abs(np.sqrt((d * d).sum(axis=1).mean()) - host(out["ate_pos"])[b]) <= 1e-9 * 1e4


# ---- an exact transform -----------------------------------------------------------------------------------------------------
def test_exact_transform_comes_back():
    """the truth is G * estimate exactly, G a yaw and a translation (for "yaw" and "se3") and a general rigid motion ("se3"):
    align_pose is G, ate_pos <= 1e-9 max|p|, and the attitude and relative errors vanish to rounding"""
    import vi_ekf_amd as v
    B, T = 3, 66
    rng = np.random.default_rng(500)
    est, _ = flights(rng, B, T)
    for align, make in (("yaw", yaw_pose), ("se3", yaw_pose), ("se3", random_pose)):
        G = np.array([make(rng) for _ in range(B)])
        tru = np.array([moved(G[b], est[b]) for b in range(B)])
        fr = v.FlightRecorder(batch(B), T, 0)
        record(fr, est, tru)
        out = fr.trajectory_error(align, delta=2)
        assert_close(out["align_pose"], G, "exact %s align_pose" % align)
        assert (out["ate_pos"] <= 1e-9 * np.abs(tru[:, :, :3]).max()).all(), out["ate_pos"]
        assert (out["ate_att"] <= 1e-12).all() and (out["rpe_pos"] <= 1e-12).all() and (out["rpe_att"] <= 1e-12).all()
        assert (out["n_used"] == [T, T - 2]).all()
        fr.close()


# ---- sub-ranges -------------------------------------------------------------------------------------------------------------
def test_sub_ranges_equal_a_recorder_of_those_frames():
    """[first, last) of a 40-frame recorder against a recorder that holds only those frames (by the tolerance: the lanes take
    other elements, so the sums run in another order), and against the restatement; last = None is count; an empty range gives
    n = 0 and NaN"""
    import vi_ekf_amd as v
    B, T, K = 4, 40, 2
    rng = np.random.default_rng(600)
    est, tru = flights(rng, B, T)
    chan = rng.chisquare(6, (T, B, K))
    mask = np.ones((B, T), np.uint8)
    mask[1, 8:12] = 0
    g = batch(B)
    whole = v.FlightRecorder(g, T, K)
    record(whole, est, tru, chan, mask)
    rec = whole.get()
    lo, hi = np.array([1.0, 2.0]), np.array([12.0, 10.0])
    for first, last in ((7, 29), (0, 1), (38, None), (11, 12)):
        sl = slice(first, last)
        part = v.FlightRecorder(g, T, K)
        record(part, est[:, sl], tru[:, sl], chan[sl], mask[:, sl])
        for align in RR.ALIGN:
            a, _, unique = trajectory_against_ref(whole, rec, align, 2, first, last, what="sub-range")
            b = part.trajectory_error(align, delta=2)
            assert np.array_equal(a["n_used"], b["n_used"])
            for k in ("ate_pos", "rpe_pos", "rpe_att"):
                held(a[k], b[k], "sub-range against a recorder of its own, " + k)
            if unique.any():
                held(a["ate_att"], b["ate_att"], "sub-range ate_att", unique)
                held(a["align_pose"], b["align_pose"], "sub-range align_pose", unique)
        ea, ca = batch_reductions_against_ref(whole, rec, lo, hi, first, last, what="sub-range")
        held(ea, part.pose_ensemble(), "sub-range pose_ensemble")
        cb = part.channels(lo, hi)
        for k in ("per_frame", "per_filter"):
            held(ca[k], cb[k], "sub-range " + k)
        part.close()
    empty = whole.trajectory_error("yaw", 5, 5)
    assert (empty["n_used"] == 0).all() and all(np.isnan(empty[k]).all() for k in TE_KEYS[:5])
    assert whole.pose_ensemble(5, 5).shape == (0, 4)


# ---- bit for bit ------------------------------------------------------------------------------------------------------------
def test_two_calls_and_both_kinds_of_pointer_agree_bit_for_bit():
    """B = 65, T = 70, K = 2 with holes: every evaluation twice gives the same bits (fixed-order sums, no atomics), and a
    recorder pushed and read through device tensors gives the bits of one pushed and read through numpy arrays"""
    import torch
    import vi_ekf_amd as v
    B, T, K = 65, 70, 2
    rng = np.random.default_rng(700)
    est, tru = flights(rng, B, T)
    chan = rng.chisquare(6, (T, B, K))
    chan[3, 5, 1] = np.nan
    mask = (rng.uniform(size=(B, T)) > 0.1).astype(np.uint8)
    g = batch(B)
    fh, fd = v.FlightRecorder(g, T, K), v.FlightRecorder(g, T + 7, K)
    record(fh, est, tru, chan, mask)
    record(fd, est, tru, chan, mask, device=True)
    rh, rd = fh.get(), fd.get(device=True)
    assert all(rd[k].is_cuda for k in rd) and all(same(rh[k], rd[k]) for k in rh)
    assert np.array_equal(rh["stamps"], 0.5 + 0.04 * np.arange(T))
    lo, hi = np.array([1.0, 2.0]), np.array([12.0, 10.0])
    for align in RR.ALIGN:
        a, b = fh.trajectory_error(align, 3, 66, 2), fh.trajectory_error(align, 3, 66, 2)
        c = fd.trajectory_error(align, 3, 66, 2, device=True)
        assert all(torch.is_tensor(c[k]) and c[k].is_cuda for k in c)
        for k in TE_KEYS:
            assert same(a[k], b[k]) and same(a[k], c[k]), (align, k)
    e = [fh.pose_ensemble(), fh.pose_ensemble(), fd.pose_ensemble(device=True)]
    assert same(e[0], e[1]) and same(e[0], e[2])
    c = [fh.channels(lo, hi), fh.channels(lo, hi), fd.channels(cuda(lo), cuda(hi))]
    for k in ("per_frame", "per_filter"):
        assert same(c[0][k], c[1][k]) and same(c[0][k], c[2][k]) and c[2][k].is_cuda, k
    trajectory_against_ref(fd, rh, "se3", 2, 3, 66, what="device pointers", device=True)
    batch_reductions_against_ref(fd, rh, lo, hi, what="device pointers", device=True)


# ---- state handling ---------------------------------------------------------------------------------------------------------
def test_full_reset_and_argument_rules():
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B, T, K = 2, 4, 1
    rng = np.random.default_rng(800)
    est, tru = flights(rng, B, T + 1)
    chan = rng.chisquare(6, (T + 1, B, K))
    g = batch(B)
    for cap, ch in ((0, 0), (4097, 0), (4, -1), (4, 9)):
        with pytest.raises(v.ViekfError) as e:
            v.FlightRecorder(g, cap, ch)
        assert e.value.code == capi.ERR_INVALID
    v.FlightRecorder(g, 4096, 8).close()
    fr = v.FlightRecorder(g, T, K)
    assert fr.count == 0 and fr.get()["est"].shape == (B, 0, 7)
    record(fr, est[:, :T], tru[:, :T], chan[:T])
    before = fr.get()
    figures = fr.trajectory_error("se3")
    # a full recorder refuses and keeps every bit
    with pytest.raises(v.ViekfError) as e:
        fr.push(est[:, T], truth_rows(tru[:, T], 11), chan=chan[T])
    assert e.value.code == capi.ERR_INVALID and "full" in str(e.value) and fr.count == T
    after = fr.get()
    assert all(same(before[k], after[k]) for k in before) and all(same(figures[k], fr.trajectory_error("se3")[k]) for k in figures)
    # the argument rules; each refusal leaves the count alone
    x = truth_rows(tru[:, 0], 11)
    fr.reset()
    assert fr.count == 0
    for bad in (lambda: fr.push(est[:, 0], x),                                               # channels without chan
                lambda: fr.push(est[:, 0], np.zeros((B, 9)), chan=chan[0]),                 # ldx < 10
                lambda: fr.trajectory_error("yaw", delta=0), lambda: fr.trajectory_error("yaw", 0, 1),
                lambda: fr.pose_ensemble(1, 0), lambda: fr.channels(first=0, last=2)):
        with pytest.raises((v.ViekfError, ValueError)):
            bad()
    L = fr._L
    assert L.viekf_rec_trajectory_error(fr._h, 3, 0, -1, 1, None, None, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_rec_trajectory_error(fr._h, 1, 0, -1, 1, None, None, None, None, None, None, 0) == capi.ERR_INVALID and b"output" in L.viekf_last_error()
    assert L.viekf_rec_trajectory_error(fr._h, 1, 0, 1, 1, None, None, None, None, None, None, 0) == capi.ERR_INVALID   # last > count
    assert L.viekf_rec_channels(fr._h, 0, -1, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_rec_pose_ensemble(fr._h, 0, -1, None, 0) == capi.ERR_INVALID
    assert L.viekf_rec_push(fr._h, 0.0, None, None, 11, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_rec_push(fr._h, 0.0, est[:, 0].ctypes.data, x.ctypes.data, 11, chan[0].ctypes.data, None, 7) == capi.ERR_INVALID
    assert fr.count == 0
    nochan = v.FlightRecorder(g, T, 0)
    with pytest.raises(v.ViekfError) as e:
        nochan.push(est[:, 0], x, chan=chan[0])                                             # chan without channels
    assert e.value.code == capi.ERR_INVALID and nochan.count == 0
    with pytest.raises(v.ViekfError):
        nochan.channels()
    # reset, then other frames: what is held is the new run
    record(fr, est[:, 1:3], tru[:, 1:3], chan[1:3], t0=9.0)
    again = fr.get()
    assert fr.count == 2 and same(again["est"], est[:, 1:3]) and same(again["chan"], chan[1:3]) and again["stamps"].tolist() == [9.0, 9.04]
    trajectory_against_ref(fr, again, "yaw", 1, what="after reset")
    fr.close()
    with pytest.raises(ValueError):
        fr.count


# ---- closed loop ------------------------------------------------------------------------------------------------------------
def test_closed_loop_recorded_on_the_device():
    """node_ref.LOOP_KFR, B = 4, N = 8, 3 s at 250 / 25 Hz with keyframe resets on, flown as tests/test_gpu_node.py flies it:
    BatchSimulator.step -> step_n -> camera -> FrameIntake.intake -> NodeGraph.update, every array a CUDA tensor.  On the tick
    before each of the 75 frames the global pose, the truth and five channels {node NEES, nees[0..3] of consistency} go into the
    recorder.  The three evaluations equal rec_ref on the recorded arrays, and the yaw-aligned ATE, the RPE over one frame and the
    worst per-frame ANEES of the node NEES lie inside rec_ref.LOOP_KFR_REC_BOUNDS (twice what the restated flight measures on
    the CPU: 0.193 m, 2.32 deg; 0.0131 m, 0.223 deg; 4.41)."""
    import torch
    import vi_ekf_amd as v
    B, N = 4, NR.LOOP_KFR_N
    p = NR.loop_kfr_params()
    per = {k: NR.LOOP_KFR[k] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    bs = v.BatchSimulator(B, p, max_features=N, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5, **per)
    bs.set_landmarks(R.jittered_landmarks(77))
    g = v.BatchVIEKF(B, N, dict(p, name="rec"))
    fi, ng = v.FrameIntake(g), v.NodeGraph(g, 8)
    fr = v.FlightRecorder(g, RR.LOOP_KFR_FRAMES, 5)
    R_pix = torch.diag(torch.tensor([10.0, 10.0], dtype=torch.float64)).cuda()
    dt9 = torch.full((9, B), bs.dt, dtype=torch.float64, device="cuda")
    dt1 = torch.full((1, B), bs.dt, dtype=torch.float64, device="cuda")
    for f in range(RR.LOOP_KFR_FRAMES):
        u = bs.step(9, device=True)
        g.step_n(u, dt9, None, None, None)
        # the tick before the frame
        tracked, _ = fi.tracked(device=True)
        xt = bs.truth_state(tracked)
        ge = ng.global_error(xt)
        pose, _ = ng.global_pose(device=True, cov=False)
        diag = v.consistency(g, ng.relative_truth(xt))
        chan = torch.cat([ge["nees"][:, None], diag["nees"]], dim=1).contiguous()
        assert pose.is_cuda and xt.is_cuda and chan.is_cuda and chan.shape == (B, 5)
        fr.push(pose, xt, chan=chan, stamp=bs.t)
        u = bs.step(1, device=True)
        g.step_n(u, dt1, None, None, None)
        z, ids, cnt, dep, _ = bs.camera(N, device=True)
        out = fi.intake(z, ids, R_pix)
        tracked, _ = fi.tracked(device=True)
        ng.update(out, x_true=bs.truth_state(tracked))
    assert fr.count == RR.LOOP_KFR_FRAMES and min(ng.get()["count"]) >= 5
    rec = fr.get()
    # (the node NEES always factors here, as tests/test_gpu_node.py holds; a consistency block that does not is a NaN the
    #  statistics leave out)
    assert rec["valid"].all() and np.isfinite(rec["chan"][:, :, 0]).all() and np.all(np.diff(rec["stamps"]) > 0)
    te, ref, unique = trajectory_against_ref(fr, rec, "yaw", 1, what="closed loop", device=True)
    assert unique.all() and all(te[k].is_cuda for k in te)
    for align in ("none", "se3"):
        trajectory_against_ref(fr, rec, align, 5, what="closed loop", device=True)
    lo, hi = np.array([1.64, 0.35, 4.17, 9.39, 1.0]), np.array([12.59, 7.81, 16.92, 28.87, 100.0])   # (chi-square 5 % / 95 % of 6, 3, 9, 16 dof)
    ens, ch = batch_reductions_against_ref(fr, rec, lo, hi, what="closed loop", device=True)
    fig = RR.loop_kfr_figures({k: host(te[k]) for k in te}, host(ch["per_frame"]))
    print("closed loop recorded on the device, yaw-aligned, worst over the vehicles: %s" % {k: float("%.5g" % x) for k, x in fig.items()})
    print("restated flight on the CPU: %s" % RR.LOOP_KFR_REC_MEASURED)
    for k, bound in RR.LOOP_KFR_REC_BOUNDS.items():
        assert 0.0 < fig[k] < bound, (k, fig[k], bound)
