"""tests/cam_ref.py, the restatement the device-resident camera model (include/viekf_cam.h) is tested against, on its own: its
Jacobian is the derivative of its forward map, undistort inverts distort, returns no wrong preimage and is complete inside the
model, zero coefficients are the identity.  And the C ABI without a device: the exports, the header as C11, the YAML reader."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import cam_ref as CR
from vi_ekf_amd import cam as vcam
from vi_ekf_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
# the two cameras of the tests: ocam.yaml's 640 x 480, and a 70 x 50 image at f = 40 whose corners lie at radius 1.08
BIG = dict(focal=CR.OCAM["focal"], center=CR.OCAM["center"], size=(640, 480))
SMALL = dict(focal=[40.0, 40.0], center=[35.0, 25.0], size=(70, 50))


def disc(rng, n, radius):
    r, th = radius * np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * np.pi, n)
    return np.stack([r * np.cos(th), r * np.sin(th)], -1)


@pytest.mark.parametrize("dist", CR.DIST_SETS)
def test_jacobian_is_the_derivative_of_the_forward_map(dist):
    """unit focal length, so pixels are normalised units: the analytic J against central differences of distort with h = 1e-5,
    within 1e-7 of the largest entry of J (truncation ~ h^2 |f'''| / 6 ~ 1e-10, rounding ~ eps / h ~ 1e-11: two decades)"""
    k = CR.make([1.0, 1.0], [0.0, 0.0], dist)
    p = disc(np.random.default_rng(3), 400, min(k["r_valid"], 1.2))
    h = 1e-5
    _, J = CR.distort(k, p)
    Jfd = np.empty_like(J)
    for col, d in enumerate((np.array([h, 0.0]), np.array([0.0, h]))):
        Jfd[:, 2 * col:2 * col + 2] = (CR.distort(k, p + d)[0] - CR.distort(k, p - d)[0]) / (2 * h)
    rel = np.abs(J - Jfd).max(-1) / np.abs(J).max(-1)
    print("analytic J_d against central differences, worst relative to max|J|: %.3e" % rel.max())
    assert rel.max() <= 1e-7
    assert np.array_equal(J[:, 1], J[:, 2])                  # J_d is symmetric


def test_jacobian_carries_both_pinholes():
    """d raw / d ideal = diag(f) J_d diag(1 / F), column-major; and J_u of undistort is its inverse at the solution"""
    k = CR.make([500.0, 510.0], [300.0, 200.0], CR.DIST_SETS[2], out_focal=[400.0, 420.0], out_center=[310.0, 190.0])
    z = np.array([[100.0, 50.0], [310.0, 190.0], [600.0, 400.0]])
    raw, J = CR.distort(k, z)
    h = 1e-4
    for col, d in enumerate((np.array([h, 0.0]), np.array([0.0, h]))):
        fd = (CR.distort(k, z + d)[0] - CR.distort(k, z - d)[0]) / (2 * h)
        assert np.abs(fd - J[:, 2 * col:2 * col + 2]).max() <= 1e-7 * np.abs(J).max()
    r = CR.undistort(k, raw)
    assert (r["status"] == CR.OK).all() and np.abs(r["z"] - z).max() <= 1e-10
    for i in range(3):
        Jm, Ju = J[i].reshape(2, 2).T, r["Ju"][i].reshape(2, 2)
        assert np.abs(Ju @ Jm - np.eye(2)).max() <= 1e-12


@pytest.mark.parametrize("dist", CR.DIST_SETS)
@pytest.mark.parametrize("camera", [BIG, SMALL], ids=["640x480", "70x50"])
def test_round_trip_no_wrong_preimage(dist, camera):
    """every pixel centre of the image and a cloud of random raw points: distort(undistort(p)) = p to 1e-12 px wherever the
    status is OK, every OK result lies within r_valid, Newton needs at most 13 of its 20 iterations and never runs out"""
    k = CR.make(camera["focal"], camera["center"], dist)
    W, H = camera["size"]
    rng = np.random.default_rng(4)
    raw = np.concatenate([CR.pixel_grid(W, H).reshape(-1, 2), rng.uniform([-0.2 * W, -0.2 * H], [1.2 * W, 1.2 * H], (4000, 2))])
    r = CR.undistort(k, raw)
    ok = r["status"] == CR.OK
    assert ok.mean() > 0.5 and set(np.unique(r["status"])) <= {CR.OK, CR.OUT_OF_MODEL}
    back, _ = CR.distort(k, r["z"])
    err = np.abs(back - raw)[ok].max()
    rad = np.hypot((r["z"][:, 0] - k["C"][0]) / k["F"][0], (r["z"][:, 1] - k["C"][1]) / k["F"][1])
    print("dist %s %dx%d: r_valid %.6f, OK %.4f, iterations <= %d, round trip %.3e px" % (dist, W, H, k["r_valid"], ok.mean(), r["iters"].max(), err))
    assert err <= 1e-12
    assert (rad[ok] <= k["r_valid"]).all() and np.isnan(r["z"][~ok]).all()
    assert r["iters"].max() <= 13 and not np.isnan(r["margin"]).any()


@pytest.mark.parametrize("dist", CR.DIST_SETS)
def test_complete_inside_the_model_and_the_fold_is_refused(dist):
    """points p forward-mapped from inside 0.98 r_valid (whose image also lies within r_valid, which the rule asks of the
    start: that matters for the pincushion set alone, whose r_valid is the scan's cap) all invert to themselves; 1e-12 in
    normalised units -- the last Newton step leaves step^2 ~ 1e-28, the rest is the rounding of the residual through J^-1,
    eps |x| / sigma_min(J) ~ 1e-14 with sigma_min >= 0.03 inside 0.98 r_valid: two decades.  Points forward-mapped from
    beyond r_valid are never answered with a point beyond r_valid: what comes back, if anything, is the inner preimage."""
    k = CR.make([1.0, 1.0], [0.0, 0.0], dist)
    rng = np.random.default_rng(5)
    p = disc(rng, 20000, 0.98 * k["r_valid"])
    raw, _ = CR.distort(k, p)
    start_inside = np.hypot(raw[:, 0], raw[:, 1]) <= k["r_valid"]
    r = CR.undistort(k, raw)
    assert (r["status"][start_inside] == CR.OK).all()
    err = np.abs(r["z"] - p)[start_inside].max()
    print("dist %s: r_valid %.6f, %d of %d starts inside, worst |undistort(distort(p)) - p| %.3e" % (dist, k["r_valid"], start_inside.sum(), p.shape[0], err))
    assert err <= 1e-12
    if k["r_valid"] < CR.SCAN_CAP:                           # the folding sets
        assert start_inside.all()
        far = disc(rng, 20000, 1.6 * k["r_valid"])
        far = far[np.hypot(far[:, 0], far[:, 1]) > 1.02 * k["r_valid"]]
        raw, _ = CR.distort(k, far)
        r = CR.undistort(k, raw)
        ok = r["status"] == CR.OK
        assert ok.any()                                      # (beyond the fold the lens maps back inside its image)
        assert (np.hypot(r["z"][ok, 0], r["z"][ok, 1]) <= k["r_valid"]).all()
        assert np.abs(CR.distort(k, r["z"][ok])[0] - raw[ok]).max() <= 1e-12
    else:                                                    # covers the images of the tests entirely
        assert start_inside.mean() > 0.01 and np.hypot(p[start_inside, 0], p[start_inside, 1]).max() > 1.2


def test_bare_determinant_test_is_not_enough():
    """the reason for r_valid: with the cap as r_valid (det > 0 alone), the folding set on the 70 x 50 image returns points
    beyond the fold -- wrong preimages -- which the derived r_valid refuses"""
    k = CR.make(SMALL["focal"], SMALL["center"], CR.DIST_SETS[2])
    loose = dict(k, r_valid=CR.SCAN_CAP, rv2=CR.SCAN_CAP ** 2)
    raw = CR.pixel_grid(70, 50)
    a, b = CR.undistort(loose, raw), CR.undistort(k, raw)
    rad = np.hypot((a["z"][..., 0] - 35.0) / 40.0, (a["z"][..., 1] - 25.0) / 40.0)
    wrong = (a["status"] == CR.OK) & (rad > k["r_valid"])
    assert wrong.any() and (b["status"][wrong] == CR.OUT_OF_MODEL).all()
    xd = CR.forward(k, np.array([k["r_valid"]]), np.array([0.0]))[0][0]
    assert 0.70 < xd < 0.76 < 1.08                           # the fold's distorted radius; the corners lie at 1.08


def test_ocam_figures():
    """the camera of ocam.yaml on 640 x 480: det J_d falls to 0.43 and never to 0 (r_valid is the cap), raw and ideal pixels
    differ by up to 99 px; with min_det = 0.5 the corners leave the model"""
    k = CR.make(**CR.OCAM)
    r = CR.undistort(k, CR.pixel_grid(640, 480))
    assert k["r_valid"] == CR.SCAN_CAP and (r["status"] == CR.OK).all()
    assert 0.42 < r["margin"].min() < 0.44
    shift = np.hypot(*(r["z"] - CR.pixel_grid(640, 480)).transpose(2, 0, 1))
    assert 95.0 < shift.max() < 103.0 and 10.0 < np.median(shift) < 14.0
    k5 = CR.make(min_det=0.5, **CR.OCAM)
    m, _ = CR.valid_mask(k5, 640, 480)
    assert k5["r_valid"] < 1.0 and m[0, 0] == 0 and m[479, 639] == 0 and m[240, 320] == 255 and 0.95 < (m == 255).mean() < 1.0


def test_zero_coefficients_are_the_identity():
    """no distortion and the same pinhole on both sides: the status is OK after one iteration and R_out = R exactly, for every
    R layout.  z comes back as F ((u - c) / f) + C: exactly u where that arithmetic is exact (a power-of-two focal length and
    dyadic pixels), within two roundings of u -- 2 eps max|u| -- for ocam's focal length."""
    rng = np.random.default_rng(6)
    R = rng.normal(0.0, 1.0, (5, 7, 2, 2))
    R = R @ np.swapaxes(R, -1, -2)
    Rc = np.swapaxes(R, -1, -2).reshape(5, 7, 4)
    exact = CR.make([512.0, 256.0], [320.0, 240.5], [0.0] * 4)
    u = np.round(rng.uniform(0.0, 640.0, (5, 7, 2)) * 64.0) / 64.0
    u[1, 3] = np.nan
    for Rin in (Rc, Rc[:, :1], Rc[:1, :1]):
        r = CR.undistort(exact, u, Rin)
        assert np.array_equal(r["z"], u, equal_nan=True) and r["iters"].max() == 1
        assert np.array_equal(r["R_out"], np.broadcast_to(Rin, Rc.shape)) and r["status"][1, 3] == CR.PADDING
        assert (np.delete(r["status"].ravel(), 10) == CR.OK).all()
    assert np.array_equal(CR.distort(exact, u)[0], u, equal_nan=True)
    k = CR.make(CR.OCAM["focal"], CR.OCAM["center"], [0.0] * 4)
    u = rng.uniform(0.0, 640.0, (5, 7, 2))
    r = CR.undistort(k, u, Rc)
    assert np.abs(r["z"] - u).max() <= 2 * np.finfo(float).eps * 640.0 and np.array_equal(r["R_out"], Rc)


def test_r_out_is_the_congruence():
    """R_out = J_u R J_u^T against numpy's matrix product, symmetric bit for bit"""
    k = CR.make(out_focal=[611.2, 611.6], out_center=[315.8, 242.1], **CR.OCAM)
    rng = np.random.default_rng(7)
    raw = rng.uniform([0.0, 0.0], [640.0, 480.0], (50, 2))
    A = rng.normal(0.0, 1.0, (50, 2, 2))
    R = A @ np.swapaxes(A, -1, -2)
    r = CR.undistort(k, raw, np.swapaxes(R, -1, -2).reshape(50, 4))
    Ju = r["Ju"].reshape(50, 2, 2)
    want = Ju @ R @ np.swapaxes(Ju, -1, -2)
    got = np.swapaxes(r["R_out"].reshape(50, 2, 2), -1, -2)
    assert np.abs(got - want).max() <= 1e-13 * np.abs(want).max() and np.array_equal(r["R_out"][:, 1], r["R_out"][:, 2])
    assert (np.linalg.eigvalsh(got) > 0).all()


def test_warp_restatement_round_trip():
    """an image distorted and rectified again comes back, away from the border, to within the two bilinear blurs: a smooth ramp
    is reproduced to 1 grey level; depth goes through nearest neighbour unblended (every output value is an input value)"""
    k = CR.make(SMALL["focal"], SMALL["center"], [-0.1, 0.01, 1e-3, -1e-3])
    xs, ys = np.meshgrid(np.arange(70.0), np.arange(50.0))
    img = np.floor(40.0 + 2.0 * xs + 1.5 * ys).astype(np.uint8)
    depth = (1000.0 + 10.0 * xs * ys).astype(np.float32)
    depth[:5] = np.inf
    d = CR.warp(k, CR.DISTORT, img, depth, fill=7)
    raw = np.floor(d["val"] + 0.5).astype(np.uint8)
    back = CR.warp(k, CR.RECTIFY, raw, d["depth"], fill=9)
    inner = back["sampled"] & (xs > 8) & (xs < 61) & (ys > 8) & (ys < 41)
    assert inner.sum() > 1000 and np.abs(back["val"] - img)[inner].max() <= 1.5
    assert np.isin(d["depth"][d["sampled"]], depth).all() and np.isposinf(d["depth"][~d["sampled"]]).all()
    assert (d["val"][~d["sampled"]] == 7).all() and (~d["sampled"]).any() and np.isposinf(d["depth"]).sum() > (~d["sampled"]).sum()


# -- C ABI without a device -----------------------------------------------------------------------------------------------
def test_header_and_library_agree():
    txt = open(os.path.join(ROOT, "include", "viekf_cam.h")).read()
    nocom = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    syms = sorted(set(re.findall(r"\b(viekf_cam_[a-z_0-9]+)\s*\(", nocom)))
    assert sorted(vcam.CAM_SYMBOLS) == syms and len(syms) == 13
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "vi_ekf_amd", "libviekf_hip.so")], capture_output=True, text=True, check=True)
    exported = sorted(ln.split()[-1] for ln in out.stdout.splitlines() if re.search(r"\bviekf_cam_", ln))
    assert exported == syms, exported                        # exactly the declared ones
    for name, val in (("MAX_ITER", CR.MAX_ITER), ("SCAN_DIRS", CR.SCAN_DIRS), ("MAX_M", vcam.MAX_M)):
        assert int(re.search(r"#define\s+VIEKF_CAM_%s\s+(\d+)" % name, txt).group(1)) == val
    for name, val in (("STEP_TOL", CR.STEP_TOL), ("SCAN_STEP", CR.SCAN_STEP), ("SCAN_CAP", CR.SCAN_CAP)):
        assert float(re.search(r"#define\s+VIEKF_CAM_%s\s+([0-9.e+-]+)" % name, txt).group(1)) == val
    for name, val in (("OK", CR.OK), ("PADDING", CR.PADDING), ("OUT_OF_MODEL", CR.OUT_OF_MODEL), ("RECTIFY", CR.RECTIFY), ("DISTORT", CR.DISTORT)):
        assert int(re.search(r"#define\s+VIEKF_CAM_%s\s+(\d+)" % name, txt).group(1)) == val == getattr(vcam, name)
    assert C.sizeof(vcam.Intrinsics) == 13 * 8
    assert L.viekf_abi_version() == 1
    # no header of the other modules got a new symbol
    for h in os.listdir(os.path.join(ROOT, "include")):
        if h != "viekf_cam.h":
            assert "viekf_cam" not in open(os.path.join(ROOT, "include", h)).read(), h
    import vi_ekf_amd
    assert vi_ekf_amd.CameraModel is vcam.CameraModel


def test_header_is_plain_c11(tmp_path):
    """tests/c/cam_header.c: C11, -Wall -Wextra -Werror -pedantic, links and runs without a GPU"""
    import subprocess
    from vi_ekf_amd import _build
    _build.build()
    libdir = os.path.join(ROOT, "vi_ekf_amd")
    exe = os.path.join(str(tmp_path), "cam_header")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "c", "cam_header.c"), "-L" + libdir, "-lviekf_hip", "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "cam header ok" in out.stdout, out.stderr


def test_load_yaml(tmp_path):
    """the block-style fixture with a distortion key, one without it, the filter's pinhole from a second file, and the errors"""
    k = vcam.load_yaml(os.path.join(GOLDEN, "cam_settings.yaml")).to_dict()
    assert k["focal"] == CR.OCAM["focal"] and k["center"] == CR.OCAM["center"] and k["dist"] == CR.OCAM["dist"]
    assert k["out_focal"] == k["focal"] and k["out_center"] == k["center"] and k["min_det"] == 0.0
    k = vcam.load_yaml(os.path.join(GOLDEN, "cam_settings_pinhole.yaml")).to_dict()
    assert k["dist"] == [0.0] * 4 and k["focal"] == [611.1864013671875, 611.5557861328125] and k["out_center"] == k["center"]
    ekf = os.path.join(ROOT, "vi_ekf_amd", "params", "ekf.yaml")
    k = vcam.load_yaml(os.path.join(GOLDEN, "cam_settings.yaml"), ekf).to_dict()
    p = capi.load_yaml(ekf).to_dict()
    assert k["focal"] == CR.OCAM["focal"] and k["out_focal"] == list(p["focal_len"]) and k["out_center"] == list(p["cam_center"])
    assert vcam.load_yaml(ekf).to_dict()["dist"] == [0.0] * 4   # the filter's own file has no distortion key
    L = vcam._bind()
    out = vcam.Intrinsics()
    assert L.viekf_cam_load_yaml(str(tmp_path / "absent.yaml").encode(), None, C.byref(out)) == capi.ERR_YAML
    bad = tmp_path / "bad.yaml"
    bad.write_text("cam_center: [1, 2]\nfocal_len: [3, 4]\ndistortion: [0.1, 0.2, 0.3]\n")
    assert L.viekf_cam_load_yaml(str(bad).encode(), None, C.byref(out)) == capi.ERR_YAML and b"distortion" in L.viekf_last_error()
    nofocal = tmp_path / "nofocal.yaml"
    nofocal.write_text("cam_center: [1, 2]\n")
    assert L.viekf_cam_load_yaml(str(nofocal).encode(), None, C.byref(out)) == capi.ERR_YAML and b"focal_len" in L.viekf_last_error()


def test_null_handles_are_refused():
    L = vcam._bind()
    assert L.viekf_cam_create(1, 0, None) == capi.ERR_INVALID
    assert L.viekf_cam_create(0, 0, C.byref(C.c_void_p())) == capi.ERR_INVALID
    assert L.viekf_cam_destroy(None) == capi.ERR_INVALID
    assert L.viekf_cam_dims(None, None, None) == capi.ERR_INVALID
    assert L.viekf_cam_set_stream(None, None) == capi.ERR_INVALID
    assert L.viekf_cam_sync(None) == capi.ERR_INVALID
    assert L.viekf_cam_set_intrinsics(None, None, 0) == capi.ERR_INVALID
    assert L.viekf_cam_get_intrinsics(None, None, None) == capi.ERR_INVALID
    assert L.viekf_cam_distort_points(None, 1, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_cam_undistort_points(None, 1, None, None, 0, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_cam_valid_mask(None, 8, 8, None, 0) == capi.ERR_INVALID
    assert L.viekf_cam_warp(None, 0, 8, 8, None, None, None, None, 0, 0) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()
    assert L.viekf_cam_intrinsics_default(None) == capi.ERR_INVALID
