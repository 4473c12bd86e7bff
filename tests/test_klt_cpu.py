"""No-GPU checks of the KLT tracker: properties of the numpy restatement tests/klt_ref.py (the spec of DESIGN.md §9), each
listed deviation on a small sequence, and the C ABI of include/viekf_klt.h without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vi_ekf_amd as v
from tests import klt_ref as K
from vi_ekf_amd import capi
from vi_ekf_amd import klt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def smooth(W, H, dx=0.0, dy=0.0):
    """analytic texture: a sum of sines with enough structure at every pyramid level"""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    X, Y = xx - dx, yy - dy
    img = (128 + 45 * np.sin(X / 9.0 + 0.5 * np.sin(Y / 23.0)) * np.cos(Y / 11.0) + 35 * np.sin((X + 2 * Y) / 31.0)
           + 25 * np.cos((3 * X - Y) / 53.0))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


# -- restatement properties --------------------------------------------------------------------------------------------
def test_bgr2gray_integer_formula():
    rng = np.random.default_rng(1)
    img = rng.integers(0, 256, (17, 23, 3)).astype(np.uint8)
    g = K.bgr2gray(img)
    for y, x in [(0, 0), (5, 7), (16, 22)]:
        b, gg, r = (int(c) for c in img[y, x])
        assert g[y, x] == (1868 * b + 9617 * gg + 4899 * r + 8192) >> 14
    assert K.bgr2gray(np.full((1, 1, 3), 255, np.uint8))[0, 0] == 255
    assert K.bgr2gray(np.array([[[0, 0, 255]]], np.uint8))[0, 0] == 76      # pure red
    np.testing.assert_array_equal(K.prepare(img, invert=True), g[::-1, ::-1])


def test_pyr_down_matches_direct_convolution():
    rng = np.random.default_rng(2)
    for h, w in [(9, 13), (10, 12), (31, 24)]:
        img = rng.integers(0, 256, (h, w)).astype(np.uint8)
        out = K.pyr_down(img)
        assert out.shape == ((h + 1) // 2, (w + 1) // 2)
        k = [1, 4, 6, 4, 1]
        for y in range(out.shape[0]):
            for x in range(out.shape[1]):
                s = sum(k[j] * k[i] * int(img[K.reflect101(2 * y - 2 + j, h), K.reflect101(2 * x - 2 + i, w)])
                        for j in range(5) for i in range(5))
                assert out[y, x] == (s + 128) >> 8


def test_pyramid_levels_stop_above_the_window():
    assert [l.shape for l in K.pyramid(np.zeros((480, 640), np.uint8))] == [(480, 640), (240, 320), (120, 160), (60, 80)]
    assert [l.shape for l in K.pyramid(np.zeros((60, 100), np.uint8))] == [(60, 100), (30, 50)]
    assert len(K.pyramid(np.zeros((40, 40), np.uint8))) == 1


def test_detect_finds_square_corners():
    W, H, r = 200, 150, 8
    img = np.full((H, W), 30, np.uint8)
    corners = []
    for x0, y0, s in [(20, 20, 30), (110, 30, 40), (40, 90, 35), (140, 95, 30)]:
        img[y0:y0 + s, x0:x0 + s] = 220
        corners += [(x0, y0), (x0 + s - 1, y0), (x0, y0 + s - 1), (x0 + s - 1, y0 + s - 1)]
    pts = K.detect(img, np.full((H, W), 255, np.uint8), 40, r)
    assert len(pts) == 16
    c = np.array(corners, float)
    d = np.sqrt(((pts[:, None, :] - c[None]) ** 2).sum(-1))
    # every detection at a corner and every corner detected: the 7x7 score peaks two pixels inside, on the diagonal
    np.testing.assert_allclose(d.min(1), np.sqrt(8.0))
    np.testing.assert_allclose(d.min(0), np.sqrt(8.0))
    pd = np.sqrt(((pts[:, None] - pts[None]) ** 2).sum(-1)) + np.eye(len(pts)) * 1e9
    assert pd.min() >= r
    # a mask hides a square; k limits the count; the first pick is the strongest
    m = np.full((H, W), 255, np.uint8)
    m[15:60, 15:60] = 0
    pm = K.detect(img, m, 40, r)
    assert len(pm) == 12 and not ((pm[:, 0] < 60) & (pm[:, 1] < 60)).any()
    assert len(K.detect(img, m, 5, r)) == 5


def test_detect_ties_break_by_raster_order():
    img = np.full((60, 90), 20, np.uint8)
    for x0 in (10, 50):
        img[20:36, x0:x0 + 16] = 200          # two identical squares: their corner scores tie exactly
    xs, ys, lam = K.candidates(img, np.full(img.shape, 255, np.uint8))
    top = lam == lam[0]
    assert top.sum() >= 2
    idx = ys[top] * 90 + xs[top]
    assert (np.diff(idx) > 0).all()


@pytest.mark.parametrize("shift", [(0.3, -0.7), (2.25, 1.5), (-7.6, 11.3), (18.4, -22.7), (-33.1, 29.6), (40.0, -38.5)])
def test_lk_recovers_subpixel_translation(shift):
    W, H = 320, 240
    f0, f1 = smooth(W, H), smooth(W, H, *shift)
    pts = K.detect(f0, np.full((H, W), 255, np.uint8), 80, 10)
    # points whose shifted window stays clear of the image border
    q = pts + np.array(shift, np.float32)
    keep = (q[:, 0] > 25) & (q[:, 0] < W - 25) & (q[:, 1] > 25) & (q[:, 1] < H - 25)
    nxt, st = K.lk(K.pyramid(f0), K.pyramid(f1), pts[keep])
    assert st.mean() > 0.9
    err = np.abs(nxt - q[keep])[st].max(1)
    assert np.median(err) <= 0.05, np.median(err)


# -- deviations ---------------------------------------------------------------------------------------------------------
def test_drop_feature_keeps_points_and_ids_aligned():
    W, H = 200, 150
    t = K.Tracker(W, H, 10, 12)
    t.load_image(smooth(W, H))
    ids0, pts0 = t.ids.copy(), t.pts.copy()
    assert t.drop_feature(int(ids0[2])) and not t.drop_feature(10 ** 6)
    np.testing.assert_array_equal(t.ids, np.delete(ids0, 2))
    np.testing.assert_array_equal(t.pts, np.delete(pts0, 2, 0))
    f, ids = t.load_image(smooth(W, H, 1.5, -0.5))
    # every surviving old id sits at its own point, moved by the shift
    for i, fid in enumerate(ids):
        j = list(ids0).index(fid) if fid < len(ids0) else -1
        if j >= 0 and 25 < pts0[j][0] < W - 25 and 25 < pts0[j][1] < H - 25:
            assert np.abs(f[i] - (pts0[j] + [1.5, -0.5])).max() < 0.1
    assert ids0[2] not in ids[: (ids < len(ids0)).sum()]


def test_prune_uses_the_intended_neighbour_test():
    """two points that converge: the later one (visited first) is kept, the earlier one is dropped, whatever was erased"""
    W, H = 120, 90
    t = K.Tracker(W, H, 3, 10)
    t.initialised = True
    g = smooth(W, H)
    t.prev_pyr = K.pyramid(g)
    t.set_points(np.array([[30.0, 30.0], [60.0, 40.0], [64.0, 43.0]], np.float32), np.array([7, 8, 9], np.int32))
    t.next_id = 10
    t.mask[:, :] = 255
    t.mask[:, :40] = 0                              # the first point's position is masked
    f, ids = t.load_image(g)
    # id 7 dropped by the mask, id 8 dropped as too close to id 9 (kept, higher index); replenished with new ids
    assert list(ids[:1]) == [9] and 7 not in ids and 8 not in ids
    assert (ids[1:] >= 10).all()


def test_replenish_mask_is_a_disc():
    t = K.Tracker(60, 50, 5, 4)
    t.set_points(np.array([[20.5, 30.4]], np.float32), np.array([0], np.int32))
    m = t._replenish_mask()
    cx, cy = 20, 30                                  # cvRound: 20.5 -> 20 (half to even)
    yy, xx = np.nonzero(m == 0)
    assert ((xx - cx) ** 2 + (yy - cy) ** 2 <= 16).all() and len(xx) == sum(
        1 for x in range(60) for y in range(50) if (x - cx) ** 2 + (y - cy) ** 2 <= 16)


def test_depth_read_is_clamped_and_fully_flipped():
    W, H = 30, 20
    t = K.Tracker(W, H, 4, 2)
    d = np.arange(W * H, dtype=np.float32).reshape(H, W) * 10 + 2000
    t.features = np.array([[W, H], [0.0, 0.0], [12.5, 7.5], [3.2, 4.7]])
    z = t.sample_depth(d, 1.5)
    mm = lambda v: float(np.float32(float(v) * 1e-3))    # noqa: E731  (float * 1e-3 in double, stored as float)
    assert z[0] == mm(d[H - 1, W - 1])                   # the saturated coordinate reads the last pixel
    assert z[2] == mm(d[8, 13])                          # round half away from zero
    ti = K.Tracker(W, H, 4, 2, invert_image=True)
    ti.features = t.features
    np.testing.assert_array_equal(ti.sample_depth(d, 1.5), t.sample_depth(np.ascontiguousarray(d[::-1, ::-1]), 1.5))
    d2 = d.copy()
    d2[:] = 1.2e6
    assert np.isnan(t.sample_depth(d2, 1.5)).all()       # > 1e3 m
    assert np.isnan(t.sample_depth(d, 8.5)).all()        # < min_depth (every depth here is under 8 m)


# -- C ABI without a device -----------------------------------------------------------------------------------------------
def declared_klt_symbols():
    txt = open(os.path.join(ROOT, "include", "viekf_klt.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(viekf_klt_[a-z_0-9]+)\s*\(", txt)))


def test_header_and_library_agree():
    syms = declared_klt_symbols()
    assert sorted(klt.KLT_SYMBOLS) == syms and len(syms) >= 10
    L = capi.lib()
    for s in syms:
        assert hasattr(L, s), "libviekf_hip.so does not export %s" % s
    assert L.viekf_abi_version() == 1


def test_argument_validation_without_device():
    L = klt._bind()
    out = C.c_void_p()
    assert L.viekf_klt_create(4, 640, 480, 12, 30, 0, 0, None) == capi.ERR_INVALID
    for args in [(0, 640, 480, 12, 30), (4, 4, 480, 12, 30), (4, 640, 480, 0, 30), (4, 640, 480, 2000, 30), (4, 640, 480, 12, -1)]:
        assert L.viekf_klt_create(*args, 0, 0, C.byref(out)) == capi.ERR_INVALID, args
        assert not out.value
    assert L.viekf_klt_destroy(None) == capi.ERR_INVALID
    assert L.viekf_klt_reset(None) == capi.ERR_INVALID
    assert L.viekf_klt_sync(None) == capi.ERR_INVALID
    assert L.viekf_klt_load_image(None, None, 1, None, None, None, None, 0) == capi.ERR_INVALID
    assert L.viekf_klt_set_mask(None, None, 0, 0) == capi.ERR_INVALID
    assert L.viekf_klt_drop_features(None, None, 0, None) == capi.ERR_INVALID
    assert L.viekf_klt_sample_depth(None, None, 1.5, None, 0) == capi.ERR_INVALID
    assert L.viekf_klt_get_points(None, None, None, None, None) == capi.ERR_INVALID
    assert L.viekf_klt_get_level(None, 0, None) == capi.ERR_INVALID
    assert b"null" in L.viekf_last_error()


@pytest.mark.skipif(v.device_count() > 0, reason="needs a machine WITHOUT a GPU")
def test_no_cpu_fallback():
    with pytest.raises(v.ViekfError) as e:
        v.KLTTracker(2, 640, 480, max_features=12, radius=30)
    assert e.value.code == capi.ERR_NO_DEVICE
