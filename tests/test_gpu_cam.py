"""The device-resident camera model (include/viekf_cam.h, vi_ekf_amd.CameraModel) against the numpy restatement
tests/cam_ref.py, by the project's parity rule: max|d| <= 1e-9 max|ref| per array, integers and NaN patterns
exact -- points, Jacobians, the measurement noise and the status, the valid mask, both image warps -- its arrays as the
arrays FrameIntake takes, and the handle's rules."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import cam_ref as CR
from tests import sim_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MARGIN = 1e-3                                    # every point of the point tests is classified at least this clearly


def _cam(B):
    import vi_ekf_amd as v
    return v.CameraModel(B)


def close(a, ref, rel=1e-9):
    """the parity rule, NaN in the same places"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape and np.array_equal(np.isnan(a), np.isnan(ref))
    if not np.isfinite(ref).any():
        return True
    return np.nanmax(np.abs(a - ref)) <= rel * np.nanmax(np.abs(ref))


def scaled(W, H, dist, min_det=0.0, off=(0.3, -0.2)):
    """a camera for a W x H image with the corners at radius 1.08, as 70 x 50 at f = 40: both folding sets fold inside it"""
    return dict(focal=[W * 4.0 / 7.0, W * 4.0 / 7.0], center=[W * 0.5 + off[0], H * 0.5 + off[1]], dist=list(dist), min_det=min_det)


@functools.lru_cache(maxsize=None)
def three(W, H):
    """three cameras with different coefficients for a W x H image: ocam's lens, and the two sets that fold"""
    specs = [scaled(W, H, CR.DIST_SETS[0], off=(0.3, -0.2)), scaled(W, H, CR.DIST_SETS[1], off=(-0.4, -0.5)), scaled(W, H, CR.DIST_SETS[2], off=(0.2, 0.35))]
    return specs, [CR.make(**s) for s in specs]


def set_per_camera(cam, specs):
    cam.set_intrinsics(focal=np.array([s["focal"] for s in specs]), center=np.array([s["center"] for s in specs]),
                       dist=np.array([s["dist"] for s in specs]), min_det=np.array([s["min_det"] for s in specs]))


def check_r_valid(cam, ks):
    got, rv = cam.intrinsics()
    assert len(got) == len(ks) and np.array_equal(rv, [k["r_valid"] for k in ks])
    for g, k in zip(got, ks):
        assert g["focal"] == list(k["f"]) and g["dist"] == list(k["k"]) and g["out_center"] == list(k["C"]) and g["min_det"] == k["min_det"]


def clear(r):
    """restated undistort results -> which points are classified with margin"""
    m = r["margin"]
    return (r["status"] == CR.PADDING) | (~np.isnan(m) & (m >= MARGIN))


def points_for(k, W, H, M, fill, rng):
    """one camera's row: the principal point, the image's border, then random raw points over the image and a little beyond
    it that the restatement classifies with margin; NaN padding from `fill` on"""
    c = k["c"]
    special = [[c[0], c[1]], [0.0, 0.0], [W - 1.0, 0.0], [0.0, H - 1.0], [W - 1.0, H - 1.0], [W * 0.5, 0.0], [0.0, H * 0.5], [W - 1.0, c[1]]]
    pool = rng.uniform([-0.1 * W, -0.1 * H], [1.1 * W, 1.1 * H], (4 * M + 16, 2))
    pool = pool[clear(CR.undistort(k, pool))]
    row = np.concatenate([np.array(special), pool])[:M]
    row[fill:] = np.nan
    return row


def r_inputs(B, M, rng):
    A = rng.normal(0.0, 1.0, (B, M, 2, 2))
    Rm = A @ np.swapaxes(A, -1, -2) + 0.5 * np.eye(2)
    return [Rm[0, 0], Rm[:, 0], Rm]             # r_mode 0, 1, 2, indexed [row, col]


def run_points(cam, ks, z, Rs, device):
    """every point entry of the handle on one input, numpy or tensors -> a flat list of numpy arrays"""
    import torch
    conv = (lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()) if device else (lambda a: a)
    back = (lambda a: a.cpu().numpy()) if device else (lambda a: np.asarray(a))
    out = []
    raw, J = cam.distort_points(conv(z), jacobian=True)
    assert (raw.is_cuda and J.is_cuda) if device else isinstance(raw, np.ndarray)
    out += [back(raw), back(J), back(cam.distort_points(conv(z)))]
    zi, Ro, st = cam.undistort_points(conv(z))
    assert Ro is None
    out += [back(zi), back(st)]
    for Rm in Rs:
        zi, Ro, st = cam.undistort_points(conv(z), conv(Rm))
        assert (zi.is_cuda and Ro.is_cuda and st.is_cuda) if device else isinstance(Ro, np.ndarray)
        out += [back(zi), back(Ro), back(st)]
    return out


def check_points(ks, z, Rs, got):
    """`got` of run_points against the restatement, camera by camera; every point classified with margin"""
    B, M = z.shape[:2]
    n_ok = n_out = 0
    for b in range(B):
        k = ks[b if len(ks) > 1 else 0]
        raw, J = CR.distort(k, z[b])
        assert close(got[0][b], raw) and close(got[1][b], np.swapaxes(J.reshape(M, 2, 2), -1, -2)) and np.array_equal(got[2][b], got[0][b], equal_nan=True)
        r = CR.undistort(k, z[b])
        assert clear(r).all(), (b, r["margin"], r["status"])       # a status mismatch is never excused
        assert np.array_equal(got[4][b], r["status"]) and got[4].dtype == np.int32 and close(got[3][b], r["z"])
        n_ok += (r["status"] == CR.OK).sum()
        n_out += (r["status"] == CR.OUT_OF_MODEL).sum()
        for mode, Rm in enumerate(Rs):
            Rb = Rm if mode == 0 else Rm[b]
            Rc = np.swapaxes(Rb, -1, -2).reshape(Rb.shape[:-2] + (4,))
            if mode == 1:
                Rc = Rc[None]
            rr = CR.undistort(k, z[b], Rc)
            zi, Ro, st = got[5 + 3 * mode:8 + 3 * mode]
            ref_Ro = np.swapaxes(rr["R_out"].reshape(M, 2, 2), -1, -2)
            assert np.array_equal(zi[b], got[3][b], equal_nan=True) and np.array_equal(st[b], r["status"])
            assert close(Ro[b], ref_Ro) and np.array_equal(Ro[b, :, 0, 1], Ro[b, :, 1, 0])
            notok = r["status"] != CR.OK
            assert np.array_equal(Ro[b][notok], np.broadcast_to(Rb, (M, 2, 2))[notok])     # the entry's input R, bit for bit
    return n_ok, n_out


# ---- points -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 7, 65])
@pytest.mark.parametrize("per_camera", [True, False], ids=["per_camera", "shared"])
def test_points_against_the_restatement(M, per_camera):
    """B = 3, one lane / a ragged wave / two waves; per-camera intrinsics with three different lenses on a 70 x 50 image whose
    corners lie beyond the fold of two of them, or the second folding set shared; ragged rows with NaN padding, the principal
    point, the border; z, J, R_out and status for the three r_modes; host and device pointers give the same bits"""
    B, W, H = 3, 70, 50
    specs, ks = three(W, H)
    if not per_camera:
        specs, ks = specs[2:], ks[2:]
    cam = _cam(B)
    if per_camera:
        set_per_camera(cam, specs)
    else:
        cam.set_intrinsics(**specs[0])
    assert cam.sets == (B if per_camera else 1)
    check_r_valid(cam, ks)
    rng = np.random.default_rng(100 + M)
    fills = [M, max(M - 2, 1), max(M // 2, 1)] if M > 1 else [1, 1, 0]
    z = np.stack([points_for(ks[b if per_camera else 0], W, H, M, fills[b], rng) for b in range(B)])
    if M == 1:                                   # one point per camera: the principal point, a corner beyond the fold, padding
        z[1, 0] = [0.0, 0.0]
    Rs = r_inputs(B, M, rng)
    host = run_points(cam, ks, z, Rs, False)
    n_ok, n_out = check_points(ks, z, Rs, host)
    assert n_ok > 0 and (M == 1 or n_out > 0) and np.isnan(z).any()
    dev = run_points(cam, ks, z, Rs, True)
    assert all(np.array_equal(a, b, equal_nan=True) and a.dtype == b.dtype for a, b in zip(host, dev))


def test_points_min_det_puts_the_corners_outside():
    """ocam's lens on 640 x 480 with min_det = 0.5: det J_d falls to 0.43 towards the corners, so they are OUT_OF_MODEL while
    the same points are OK with min_det = 0; and the two pinholes differ (the filter's own focal length and centre)"""
    B, M = 2, 9
    out = dict(out_focal=[611.1864013671875, 611.5557861328125], out_center=[315.83184814453125, 242.1165771484375])
    z = np.array([[0.0, 0.0], [639.0, 0.0], [0.0, 479.0], [639.0, 479.0], [316.680559, 230.660661], [320.0, 0.0], [0.0, 240.0], [100.0, 100.0], [500.0, 400.0]])
    z = np.stack([z, z[::-1]])
    Rs = r_inputs(B, M, np.random.default_rng(9))
    for min_det, corners in ((0.5, CR.OUT_OF_MODEL), (0.0, CR.OK)):
        k = CR.make(min_det=min_det, **CR.OCAM, **out)
        cam = _cam(B)
        if min_det:                              # the same camera from its parameter files
            k_set = cam.load_yaml(os.path.join(ROOT, "tests", "golden", "cam_settings.yaml"), os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml"), min_det=min_det)
            assert k_set.to_dict() == dict(min_det=min_det, **CR.OCAM, **out)
        else:
            cam.set_intrinsics(min_det=min_det, **CR.OCAM, **out)
        check_r_valid(cam, [k])
        got = run_points(cam, [k], z, Rs, False)
        check_points([k], z, Rs, got)
        assert (got[4][0, :4] == corners).all() and (got[4][0, 4:] == CR.OK).all()
    assert k["r_valid"] == CR.SCAN_CAP


# ---- mask -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(70, 50), (8, 6), (640, 480)])
def test_valid_mask(W, H):
    """70 x 50 is no multiple of four pixels nor of the 64 x 16 tile (pairs are stored, ragged tiles), 8 x 6 is smaller than
    one tile, 640 x 480 is the real size; three lenses per camera, then one of them shared.  The restatement classifies every
    pixel of these cameras with a margin above 1e-9, so every pixel is compared."""
    specs, ks = three(W, H)
    refs = [CR.valid_mask(k, W, H) for k in ks]
    for m, mg in refs:
        assert not np.isnan(mg).any() and (mg >= 1e-9).all()      # no pixel to leave out
    assert (refs[1][0] == 0).any() and (refs[1][0] == 255).any() and (refs[0][0] == 255).all()
    cam = _cam(3)
    set_per_camera(cam, specs)
    got = cam.valid_mask(W, H)
    assert got.shape == (3, H, W) and got.dtype == np.uint8
    for b in range(3):
        assert np.array_equal(got[b], refs[b][0]), (b, (got[b] != refs[b][0]).sum())
    dev = cam.valid_mask(W, H, device=True)
    assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), got)
    cam.set_intrinsics(**specs[2])
    one = cam.valid_mask(W, H)
    assert one.shape == (H, W) and np.array_equal(one, refs[2][0])
    assert np.array_equal(cam.valid_mask(W, H, device=True).cpu().numpy(), one)


def test_valid_mask_feeds_the_tracker():
    """the mask is what KLTTracker.set_mask takes, shared or per camera, on the device"""
    import vi_ekf_amd as v
    W, H = 64, 48
    specs, ks = three(W, H)
    cam = _cam(2)
    trk = v.KLTTracker(2, W, H, max_features=16, radius=3)
    cam.set_intrinsics(**specs[1])
    trk.set_mask(cam.valid_mask(W, H, device=True))
    set_per_camera(cam, specs[1:])
    trk.set_mask(cam.valid_mask(W, H, device=True))
    trk.set_mask(cam.valid_mask(W, H))
    trk.sync()


# ---- warp -------------------------------------------------------------------------------------------------------------------
def _render(W, H, pitched):
    """two textured frames with depth from the simulator; pitched: the horizon crosses the image, +inf depth above it"""
    import vi_ekf_amd as v
    p = dict(orc.EKF_YAML)
    p["use_keyframe_reset"] = False
    p["cam_center"] = [W * 0.5 - 4.2, H * 0.5 + 1.1]
    if pitched:
        p["x0"] = [0, 0, -2, 0, 0, 0, np.cos(0.815), 0, np.sin(0.815), 0, 0, 0, 0, 0, 0, 0, 0.1]
    bs = v.BatchSimulator(2, p, seed=[1, 2], radius=[0.35, 1.2], period=[8.0, 6.0])
    bs.set_landmarks(R.jittered_landmarks(77))
    if not pitched:                              # (mid-flight; the pitched camera looks at the horizon from where it starts)
        bs.step(300)
    return bs.render(W, H, depth=True)


def check_warp(cam, ks, direction, img, dmm, fill):
    """one warp, with and without depth, host and device, against the restatement"""
    import torch
    B, H, W = img.shape
    dst, dd = cam.warp(img, direction, depth=dmm, fill=fill)
    assert dst.dtype == np.uint8 and dd.dtype == np.float32 and np.array_equal(cam.warp(img, direction, fill=fill), dst)
    tdst, tdd = cam.warp(torch.as_tensor(img).cuda(), direction, depth=torch.as_tensor(dmm).cuda(), fill=fill)
    assert tdst.is_cuda and tdd.is_cuda and np.array_equal(tdst.cpu().numpy(), dst) and np.array_equal(tdd.cpu().numpy().view(np.uint32), dd.view(np.uint32))
    seen = dict(sampled=0, filled=0, inf_in=0)
    for b in range(B):
        w = CR.warp(ks[b], {"rectify": CR.RECTIFY, "distort": CR.DISTORT}[direction], img[b], dmm[b], fill)
        unclear = CR.warp_unclear(w, W, H)
        assert unclear.mean() <= 1e-3                           # the restatement alone stays within 0.1 %
        keep = ~unclear
        err = np.abs(dst[b].astype(np.float64) - w["val"])
        assert err[keep].max() <= 0.5 + 1e-6, (direction, b, err[keep].max())
        assert np.array_equal(dd[b][keep].view(np.uint32), w["depth"][keep].view(np.uint32))      # bit-equal, unblended
        nothing = keep & ~w["sampled"]
        assert (dst[b][nothing] == fill).all() and np.isposinf(dd[b][nothing]).all()
        seen["sampled"] += int(w["sampled"].sum())
        seen["filled"] += int((~w["sampled"]).sum())
        seen["inf_in"] += int((np.isposinf(w["depth"]) & w["sampled"]).sum())
    return seen


@pytest.mark.parametrize("W,H", [(70, 50), (160, 120)])
@pytest.mark.parametrize("direction", ["rectify", "distort"])
def test_warp_against_the_restatement(direction, W, H):
    """B = 2, a folding barrel lens and a pincushion lens (so both directions meet the source's border and the model's), a
    textured simulator frame with depth: grey within half a level of the restatement's unrounded value, depth bit-equal,
    `fill` = 77 and +inf exactly where the restatement puts them"""
    specs = [scaled(W, H, CR.DIST_SETS[2], off=(0.2, 0.35)), scaled(W, H, CR.DIST_SETS[3], off=(-0.4, 0.1))]
    ks = [CR.make(**s) for s in specs]
    img, dmm = _render(W, H, False)
    assert img.std() > 5.0 and np.isfinite(dmm).all()
    cam = _cam(2)
    set_per_camera(cam, specs)
    seen = check_warp(cam, ks, direction, img, dmm, 77)
    assert seen["sampled"] > 0.5 * W * H and seen["filled"] > 0.01 * W * H, seen


def test_warp_with_rays_that_miss():
    """a pitched camera: +inf depth is in the source and goes through nearest neighbour as it is, both directions, fill 0"""
    W, H = 70, 50
    specs = [scaled(W, H, CR.DIST_SETS[0]), scaled(W, H, CR.DIST_SETS[2])]
    ks = [CR.make(**s) for s in specs]
    img, dmm = _render(W, H, True)
    assert np.isposinf(dmm).any() and np.isfinite(dmm).any()
    cam = _cam(2)
    set_per_camera(cam, specs)
    for direction in ("rectify", "distort"):
        seen = check_warp(cam, ks, direction, img, dmm, 0)
        assert seen["inf_in"] > 0 and seen["sampled"] > 0


# ---- through the intake -----------------------------------------------------------------------------------------------------
def test_round_trip_through_the_intake():
    """B = 4, N = 12, ten frames of BatchSimulator.step / camera -> step_n -> FrameIntake, twice from the same seed: once fed z
    and R_pix (r_mode 0), once fed undistort(distort(z)) through ocam's lens with the per-entry noise that undistort hands out
    for the raw noise J R_pix J^T -- which is R_pix again (r_mode 2).  The round trip moves z by less than 1e-12 px; results,
    ids and resets are equal, state and covariance within the parity rule; and the tensors CameraModel hands out are the
    tensors the intake passes to the library, with no copy in between."""
    import torch
    import vi_ekf_amd as v
    B, N = 4, 12
    p = dict(orc.EKF_YAML)
    per = {k: R.LOOP[k] for k in ("seed", "radius", "period", "accel_bias", "gyro_bias")}
    R_pix = torch.diag(torch.tensor([10.0, 10.0], dtype=torch.float64)).cuda()
    cam = _cam(B)
    cam.set_intrinsics(focal=p["focal_len"], center=p["cam_center"], dist=CR.OCAM["dist"])

    def fly(through_the_lens):
        bs = v.BatchSimulator(B, p, max_features=N, accel_sigma=0.3, gyro_sigma=0.01, pix_sigma=0.5, **per)
        bs.set_landmarks(R.jittered_landmarks(77))
        g = v.BatchVIEKF(B, N, dict(p, name="cam"))
        fi = v.FrameIntake(g)
        dt = torch.full((10, B), bs.dt, dtype=torch.float64, device="cuda")
        outs, moved = [], 0.0
        for f in range(10):
            u = bs.step(10, device=True)
            g.step_n(u, dt, None, None, None)
            z, ids, cnt, dep, _ = bs.camera(N, device=True)
            if not through_the_lens:
                out = fi.intake(z, ids, R_pix)
            else:
                z_raw, J = cam.distort_points(z, jacobian=True)
                R_raw = J @ R_pix @ J.transpose(-1, -2)
                R_raw = torch.where(torch.isnan(R_raw), R_pix.expand(B, N, 2, 2), R_raw).contiguous()
                z2, R_out, st = cam.undistort_points(z_raw, R_raw)
                assert z2.is_cuda and R_out.is_cuda and st.is_cuda and tuple(R_out.shape) == (B, N, 2, 2)
                pad = torch.isnan(z[..., 0])
                assert torch.equal(st, torch.where(pad, CR.PADDING, CR.OK).to(torch.int32)) and torch.equal(torch.isnan(z2[..., 0]), pad)
                moved = max(moved, float((z2 - z)[~pad].abs().max()))
                assert float((R_out - R_pix).abs().max()) <= 1e-9 * 10.0
                seen = []
                arg = g._arg
                g._arg = lambda a, *rest: (seen.append(a), arg(a, *rest))[1]
                out = fi.intake(z2, ids, R_out)
                g._arg = arg
                # z as handed out; R_out's column-major storage as the library wrote it, not a re-laid-out copy
                assert seen[0] is z2 and seen[2].data_ptr() == R_out.data_ptr() and tuple(seen[2].shape) == (B, N, 2, 2) and seen[2].is_contiguous()
            outs.append({k: out[k].cpu().numpy() for k in ("result", "gated", "gated_count", "did_reset")})
            outs[-1]["ids"] = ids.cpu().numpy()
        return outs, g.get_state(), g.get_covariance(), g.get_len_features(), moved

    a, xa, Pa, la, _ = fly(False)
    b, xb, Pb, lb, moved = fly(True)
    print("undistort(distort(z)) moved z by at most %.3e px over ten frames" % moved)
    assert 0.0 <= moved < 1e-12
    for fa, fb in zip(a, b):
        assert all(np.array_equal(fa[k], fb[k]) for k in fa)
    assert sum(int((f["result"] == 0).sum()) for f in a) > 0
    assert np.array_equal(la, lb) and close(xb, xa) and close(Pb, Pa)


# ---- handles ----------------------------------------------------------------------------------------------------------------
def test_streams_and_a_ragged_block():
    """300 cameras x 3 points is no multiple of the block of 256 lanes; the same numbers on the handle's own stream, on
    torch's current stream without waiting (sync=False), and on the null stream"""
    import torch
    B, M, W, H = 300, 3, 70, 50
    specs, ks = three(W, H)
    cam = _cam(B)
    set_per_camera(cam, [specs[b % 3] for b in range(B)])
    rng = np.random.default_rng(12)
    rows = [points_for(k, W, H, 8, 8, rng)[[0, 1, 7]] for k in ks]
    z = np.stack([rows[b % 3] for b in range(B)])
    z[7, 1] = np.nan
    Rm = r_inputs(B, M, rng)[2]
    zi, Ro, st = cam.undistort_points(z, Rm)
    for b in (0, 1, 2, 7, 255, 256, 299):
        r = CR.undistort(ks[b % 3], z[b], np.swapaxes(Rm[b], -1, -2).reshape(M, 4))
        assert clear(r).all() and np.array_equal(st[b], r["status"]) and close(zi[b], r["z"])
        assert close(Ro[b], np.swapaxes(r["R_out"].reshape(M, 2, 2), -1, -2))
    assert set(np.unique(st)) == {CR.OK, CR.PADDING, CR.OUT_OF_MODEL}
    tz, tR = torch.as_tensor(z).cuda(), torch.as_tensor(Rm).cuda()
    for stream in (torch.cuda.current_stream().cuda_stream, None):
        cam.set_stream(stream)
        torch.cuda.synchronize()
        dz, dR, ds = cam.undistort_points(tz, tR, sync=False)
        cam.sync()
        torch.cuda.synchronize()
        assert np.array_equal(dz.cpu().numpy(), zi, equal_nan=True) and np.array_equal(dR.cpu().numpy(), Ro) and np.array_equal(ds.cpu().numpy(), st)
    cam.close()
    with pytest.raises(ValueError):
        cam.sync()


def test_refusals():
    import torch
    import vi_ekf_amd as v
    from vi_ekf_amd import capi
    B = 2
    cam = _cam(B)
    L, h = cam._L, cam._h
    D, Hh = capi.DEVICE, capi.HOST

    def refused(rc, word):
        assert rc == capi.ERR_INVALID and word in L.viekf_last_error().decode(), (rc, L.viekf_last_error())

    z = np.zeros((B, 4, 2))
    out = np.zeros((B, 4, 4))
    pz, po = C.c_void_p(z.ctypes.data), C.c_void_p(out.ctypes.data)
    # M < 1, and past the limit
    refused(L.viekf_cam_distort_points(h, 0, pz, po, None, Hh), "M must be")
    refused(L.viekf_cam_undistort_points(h, -1, pz, None, 0, po, None, None, Hh), "M must be")
    refused(L.viekf_cam_undistort_points(h, 4097, pz, None, 0, po, None, None, Hh), "M must be")
    with pytest.raises(v.ViekfError):
        cam.undistort_points(np.zeros((B, 0, 2)))
    refused(L.viekf_cam_undistort_points(h, 4, pz, None, 0, po, po, None, Hh), "R_out needs R")
    refused(L.viekf_cam_undistort_points(h, 4, pz, pz, 3, po, po, None, Hh), "r_mode")
    refused(L.viekf_cam_distort_points(h, 4, pz, po, None, 2), "where")
    # odd width, sizes
    m = np.zeros((B, 16, 16), np.uint8)
    pm = C.c_void_p(m.ctypes.data)
    refused(L.viekf_cam_valid_mask(h, 7, 6, pm, Hh), "even")
    refused(L.viekf_cam_valid_mask(h, 2, 6, pm, Hh), "[4, 16384]")
    refused(L.viekf_cam_warp(h, 0, 9, 8, pm, pm, None, None, 0, Hh), "even")
    refused(L.viekf_cam_warp(h, 2, 8, 8, pm, pm, None, None, 0, Hh), "direction")
    refused(L.viekf_cam_warp(h, 0, 8, 8, pm, pm, None, None, 256, Hh), "fill")
    refused(L.viekf_cam_warp(h, 0, 8, 8, pm, pm, pm, None, 0, Hh), "together")
    with pytest.raises(v.ViekfError):
        cam.valid_mask(7, 6)
    with pytest.raises(ValueError):
        cam.warp(np.zeros((B + 1, 8, 8), np.uint8), "rectify")
    with pytest.raises(ValueError):
        cam.warp(np.zeros((B, 8, 8), np.uint8), "sideways")
    # misaligned device pointers
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p0 = buf.data_ptr()
    assert p0 % 16 == 0
    refused(L.viekf_cam_distort_points(h, 4, C.c_void_p(p0 + 4), C.c_void_p(p0 + 1024), None, D), "aligned")
    refused(L.viekf_cam_undistort_points(h, 4, C.c_void_p(p0), None, 0, C.c_void_p(p0 + 1024), None, C.c_void_p(p0 + 2050), D), "aligned")
    refused(L.viekf_cam_valid_mask(h, 8, 6, C.c_void_p(p0 + 2), D), "aligned")
    refused(L.viekf_cam_warp(h, 0, 8, 8, C.c_void_p(p0 + 1), C.c_void_p(p0 + 1026), None, None, 0, D), "aligned")
    refused(L.viekf_cam_warp(h, 0, 8, 8, C.c_void_p(p0 + 1), C.c_void_p(p0 + 1024), C.c_void_p(p0 + 2048), C.c_void_p(p0 + 3080), 0, D), "aligned")
    # a source at an odd address is fine: it is read in bytes
    capi.check(L.viekf_cam_warp(h, 0, 8, 8, C.c_void_p(p0 + 1), C.c_void_p(p0 + 1024), None, None, 0, D))
    cam.sync()
    # mixed sides, wrong dtype, another shape
    with pytest.raises(ValueError):
        cam.undistort_points(torch.zeros(B, 4, 2, dtype=torch.float64, device="cuda"), np.eye(2))
    with pytest.raises(ValueError):
        cam.distort_points(torch.zeros(B, 4, 2, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        cam.distort_points(np.zeros((B + 1, 4, 2)))
    with pytest.raises(ValueError):
        cam.undistort_points(np.zeros((B, 4, 2)), np.zeros((3, 3)))
    # per-camera intrinsics are host memory: a device pointer is refused by the library, a CUDA tensor by the wrapper
    dk = torch.zeros(B * 13, dtype=torch.float64, device="cuda")
    refused(L.viekf_cam_set_intrinsics(h, C.c_void_p(dk.data_ptr()), 1), "host memory")
    with pytest.raises(ValueError):
        cam.set_intrinsics(focal=torch.ones(B, 2, dtype=torch.float64, device="cuda"), center=[0.0, 0.0])
    # values that are no camera
    for bad in (dict(focal=[0.0, 1.0]), dict(focal=[1.0, np.nan]), dict(dist=[np.inf, 0, 0, 0]), dict(out_focal=[-1.0, 1.0])):
        kw = dict(dict(focal=[1.0, 1.0], center=[0.0, 0.0]), **bad)
        with pytest.raises(v.ViekfError):
            cam.set_intrinsics(**kw)
    # nothing above changed the table: still the default identity
    ks, rv = cam.intrinsics()
    assert len(ks) == 1 and ks[0]["focal"] == [1.0, 1.0] and ks[0]["dist"] == [0.0] * 4 and rv[0] == CR.SCAN_CAP
    zi, _, st = cam.undistort_points(np.array([[[0.5, -0.25]], [[3.0, 3.0]]]))
    assert np.array_equal(zi[0], [[0.5, -0.25]]) and st[0, 0] == CR.OK and st[1, 0] == CR.OUT_OF_MODEL and np.isnan(zi[1]).all()
