"""The HIP KLT tracker (include/viekf_klt.h) against the numpy restatement tests/klt_ref.py: the corner detector and the
pyramid bit for bit, LK to 0.02 px, the tracker's lifecycle frame by frame, and the batch / input invariances."""
import numpy as np
import pytest

from tests import klt_ref as K

pytestmark = pytest.mark.gpu


def _tracker(*a, **kw):
    from vi_ekf_amd.klt import KLTTracker
    return KLTTracker(*a, **kw)


def texture(W, H, dx=0.0, dy=0.0, seed=0):
    """smooth analytic texture shifted by (dx, dy) px: Gaussian blobs at random places plus low-frequency shading"""
    rng = np.random.default_rng(seed)
    xs = np.arange(W) - dx
    ys = np.arange(H) - dy
    img = 90.0 + 30.0 * np.outer(np.cos(ys / 29.0 - 0.2), np.ones(W)) * np.sin(xs / 37.0 + 0.3)[None, :]
    cx = rng.uniform(-60, W + 60, 120)
    cy = rng.uniform(-60, H + 60, 120)
    amp = rng.uniform(-80, 110, 120)
    sg = rng.uniform(3.0, 7.0, 120)
    for i in range(120):          # separable blobs, each on its own +-5 sigma box
        x0, x1 = np.searchsorted(xs, cx[i] - 5 * sg[i]), np.searchsorted(xs, cx[i] + 5 * sg[i])
        y0, y1 = np.searchsorted(ys, cy[i] - 5 * sg[i]), np.searchsorted(ys, cy[i] + 5 * sg[i])
        if x1 > x0 and y1 > y0:
            gx = np.exp(-(xs[x0:x1] - cx[i]) ** 2 / (2 * sg[i] ** 2))
            gy = np.exp(-(ys[y0:y1] - cy[i]) ** 2 / (2 * sg[i] ** 2))
            img[y0:y1, x0:x1] += amp[i] * np.outer(gy, gx)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def squares(W, H, n, seed, size=12):
    """identical squares: their corners tie exactly, so the raster tie-break decides the order"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 40, np.uint8)
    for _ in range(n):
        x, y = int(rng.integers(12, W - 12 - size)), int(rng.integers(12, H - 12 - size))
        img[y:y + size, x:x + size] = 200
    return img


def plateau(W, H):
    """period-7 pattern: every interior 7x7 block sees the same structure sums, so the score is one plateau and every
    interior pixel is a candidate (far more than the LDS sort holds)"""
    f = np.array([0, 40, 90, 130, 90, 40, 10])
    g = np.array([0, 60, 20, 100, 30, 70, 5])
    yy, xx = np.mgrid[0:H, 0:W]
    return (f[xx % 7] + g[yy % 7]).astype(np.uint8)


def _first_frame(W, H, frames, MF, r, masks=None, per_camera=False):
    B = len(frames)
    trk = _tracker(B, W, H, max_features=MF, radius=r)
    if masks is not None:
        trk.set_mask(masks if per_camera else masks[0])
    f, ids, cnt = trk.load_image(np.stack(frames))
    for b in range(B):
        m = np.full((H, W), 255, np.uint8) if masks is None else np.where((masks[b] if per_camera else masks[0]) > 1, 255, 0)
        ref = K.detect(frames[b], m, MF, r)
        assert cnt[b] == len(ref), (b, cnt[b], len(ref))
        np.testing.assert_array_equal(f[b, :cnt[b]], ref.astype(np.float64), err_msg="camera %d" % b)
        np.testing.assert_array_equal(ids[b, :cnt[b]], np.arange(cnt[b]))
        assert np.isnan(f[b, cnt[b]:]).all() and (ids[b, cnt[b]:] == -1).all()
    return trk


@pytest.mark.parametrize("W,H", [(640, 480), (333, 251)])
def test_detector_bit_for_bit(W, H):
    B = 8
    frames = [texture(W, H, seed=s) for s in range(5)] + [squares(W, H, 30, 1), squares(W, H, 30, 2), plateau(W, H)]
    _first_frame(W, H, frames, 200, 9)
    rng = np.random.default_rng(3)
    masks = rng.integers(0, 4, (B, H, W)).astype(np.uint8) * 85        # 0 / 85 / 170 / 255, then > 1
    masks[:, : H // 3] = 255
    masks[:, H // 2:, W // 2:] = 1                                       # 1 is "not usable"
    _first_frame(W, H, frames, 120, 5, masks=masks, per_camera=True)
    _first_frame(W, H, frames, 60, 12, masks=masks[:1], per_camera=False)


def test_plateau_overflows_lds_and_ties_break_by_raster():
    W, H = 333, 251
    img = plateau(W, H)
    xs, ys, _ = K.candidates(img, np.full((H, W), 255, np.uint8))
    assert len(xs) > 8192                                                # (the global-memory sort path)
    _first_frame(W, H, [img, squares(W, H, 40, 5)], 300, 3)


def test_pyramid_bit_for_bit():
    for W, H in [(640, 480), (333, 251), (100, 47)]:
        frames = np.stack([texture(W, H, seed=s) for s in range(3)])
        trk = _tracker(3, W, H, max_features=10, radius=10)
        trk.load_image(frames)
        for b in range(3):
            ref = K.pyramid(frames[b])
            assert trk.levels == len(ref)
            for l in range(len(ref)):
                np.testing.assert_array_equal(trk.get_level(l)[b], ref[l], err_msg="level %d of %dx%d" % (l, W, H))


def test_lk_against_restatement_and_truth():
    W, H, MF = 640, 480, 200
    shifts = [(0.37, -0.61), (3.3, 2.7), (-12.4, 7.9), (25.25, -18.5), (-38.2, 33.3), (40.0, -39.6)]
    B = len(shifts)
    f0 = np.stack([texture(W, H, seed=11)] * B)
    f1 = np.stack([texture(W, H, dx, dy, seed=11) for dx, dy in shifts])
    trk = _tracker(B, W, H, max_features=MF, radius=8)
    trk.load_image(f0)
    p0, i0, _ = trk.get_points()
    trk.load_image(f1)
    p1, i1, _ = trk.get_points()
    errs = []
    pyr0 = K.pyramid(f0[0])
    for b, (dx, dy) in enumerate(shifts):
        nxt, st = K.lk(pyr0, K.pyramid(f1[b]), p0[b])
        tracked = np.isin(i0[b], i1[b])                # LK status 0 drops; so do the border, mask and neighbour tests
        sel = i1[b] < len(i0[b])
        g = p1[b][sel]
        r = nxt[i1[b][sel]]
        assert st[i1[b][sel]].all()
        np.testing.assert_allclose(g, r, atol=0.02, rtol=0)
        # truth: points whose window stays inside the image and that the restatement tracked
        inside = (g[:, 0] > 12) & (g[:, 0] < W - 12) & (g[:, 1] > 12) & (g[:, 1] < H - 12)
        errs.append(np.abs(g - (p0[b][i1[b][sel]] + np.array([dx, dy], np.float32)))[inside].max(1))
        assert tracked.sum() >= 0.5 * len(i0[b]) * (1 if abs(dx) < 30 else 0.5)
    e = np.concatenate(errs)
    assert np.median(e) <= 0.05 and np.percentile(e, 99) <= 0.2, (np.median(e), np.percentile(e, 99))


def _pan(W, H, k):
    return texture(W, H, 6.5 * k + 0.3 * np.sin(k), -2.25 * k, seed=21)


def test_lifecycle_30_frames_against_restatement():
    W, H, MF, r = 640, 480, 50, 25
    B = 2
    trk = _tracker(B, W, H, max_features=MF, radius=r)
    mask = np.full((H, W), 255, np.uint8)
    mask[300:420, 40:200] = 0                                       # a masked region
    trk.set_mask(mask)
    refs = [K.Tracker(W, H, MF, r) for _ in range(B)]
    for rf in refs:
        rf.set_mask(mask)
    replenished = 0
    for k in range(30):
        frames = np.stack([_pan(W, H, k), _pan(W, H, -k)])
        if k > 0:
            pts, ids, nid = trk.get_points()
            for b in range(B):
                refs[b].set_points(pts[b], ids[b])
                refs[b].next_id = int(nid[b])
        f, ids, cnt = trk.load_image(frames)
        for b in range(B):
            rf_f, rf_i = refs[b].load_image(frames[b])
            assert cnt[b] == len(rf_i), (k, b)
            np.testing.assert_array_equal(ids[b, :cnt[b]], rf_i, err_msg="frame %d camera %d" % (k, b))
            np.testing.assert_allclose(f[b, :cnt[b]], rf_f, atol=0.02, rtol=0)
        if k % 5 == 4:                                              # drop_features between frames
            drop = np.stack([ids[b, [0, 3]] for b in range(B)])
            found = trk.drop_features(drop)
            assert found.all()
            assert not trk.drop_features(np.full((B, 1), 10 ** 6)).any()
        replenished = max(replenished, int(trk.get_points()[2].min()))
    assert replenished > MF                                         # points left the image and were replenished


def test_batch_invariance_inactive_and_inputs():
    import torch
    W, H, MF, r = 333, 251, 40, 10
    B = 4
    seq = [np.stack([texture(W, H, 2.0 * k * (b + 1) - 3, -1.5 * k, seed=30 + b) for b in range(B)]) for k in range(6)]
    big = _tracker(B, W, H, max_features=MF, radius=r)
    one = _tracker(1, W, H, max_features=MF, radius=r)
    for fr in seq:
        fb, ib, cb = big.load_image(fr)
        f1, i1, c1 = one.load_image(fr[2:3])
        np.testing.assert_array_equal(fb[2:3], f1)
        np.testing.assert_array_equal(ib[2:3], i1)
    np.testing.assert_array_equal(big.get_points()[0][2], one.get_points()[0][0])
    # inactive cameras are untouched; the skipped frame then never happened for them
    act = np.array([1, 0, 1, 0], np.uint8)
    before = big.get_points()
    skip = _tracker(B, W, H, max_features=MF, radius=r)
    for fr in seq:
        skip.load_image(fr)
    extra = np.stack([texture(W, H, 5, 5, seed=99)] * B)
    big.load_image(extra, active=act)
    after = big.get_points()
    for b in (1, 3):
        np.testing.assert_array_equal(after[0][b], before[0][b])
        np.testing.assert_array_equal(after[1][b], before[1][b])
    assert after[2][1] == before[2][1]
    # BGR8 equals GRAY8 of the converted image; device pointers equal host pointers; invert equals pre-flipped input
    rng = np.random.default_rng(5)
    bgr = np.stack([np.stack([texture(W, H, seed=40 + b), texture(W, H, seed=50 + b), texture(W, H, seed=60 + b)], -1)
                    for b in range(B)])
    a, b_, c = _tracker(B, W, H, MF, r), _tracker(B, W, H, MF, r), _tracker(B, W, H, MF, r)
    inv, flp = _tracker(B, W, H, MF, r, invert_image=True), _tracker(B, W, H, MF, r)
    for k in range(3):
        shifted = np.roll(bgr, (k * 3, -k * 2), axis=(1, 2))
        ra = a.load_image(shifted)
        grey = np.stack([K.bgr2gray(x) for x in shifted])
        rb = b_.load_image(grey)
        rc = c.load_image(torch.from_numpy(grey).cuda())
        for u, v, w in zip(ra, rb, rc):
            np.testing.assert_array_equal(u, v)
            np.testing.assert_array_equal(v, w.cpu().numpy())
        ri = inv.load_image(grey)
        rf = flp.load_image(np.ascontiguousarray(grey[:, ::-1, ::-1]))
        for u, v in zip(ri, rf):
            np.testing.assert_array_equal(u, v)
    dm = rng.uniform(500, 5000, (B, H, W)).astype(np.float32)
    np.testing.assert_array_equal(c.sample_depth(torch.from_numpy(dm).cuda(), 1.0).cpu().numpy(), c.sample_depth(dm, 1.0))


def test_sample_depth_against_restatement():
    W, H, MF, r = 333, 251, 60, 6
    B = 3
    frames = np.stack([texture(W, H, seed=70 + b) for b in range(B)])
    rng = np.random.default_rng(8)
    dm = rng.uniform(200, 4000, (B, H, W)).astype(np.float32)
    dm[:, ::7, :] = 2e6                                     # > 1e3 m
    dm[0, :, W - 1] = 2500.0
    for inv in (False, True):
        trk = _tracker(B, W, H, MF, r, invert_image=inv)
        f, ids, cnt = trk.load_image(frames)
        d = trk.sample_depth(dm, 1.5)
        for b in range(B):
            rf = K.Tracker(W, H, MF, r, invert_image=inv)
            rf.load_image(frames[b])
            ref = rf.sample_depth(dm[b], 1.5)
            np.testing.assert_array_equal(d[b, :cnt[b]], ref)
            assert np.isnan(d[b, cnt[b]:]).all()
            assert np.isnan(ref).any() and np.isfinite(ref).any()
