"""The HIP KLT tracker (include/viekf_klt.h) where tests/test_gpu_klt.py does not reach: images smaller than the corner tile
and the LK window, pyramids of 1, 2 and 3 levels, the documented limits of max_features and radius, candidate counts
around the LDS sort's capacity, a camera activated late among cameras of very different counts, reset / set_stream / sync,
BGR8 with invert_image, and the edges of drop_features.  Everything is compared with the numpy restatement
tests/klt_ref.py on the cases of tests/klt_cases.py, or with a fresh or unbatched tracker where the claim is an invariance.

LK tolerance: every point within 0.02 px of the restatement (the suite's bound: twice the largest step a flipped stop test
can leave), and at most 5 % of a case's compared points above 1e-3 px.  The GPU's butterfly sums may differ from the
restatement's in their order alone, and tests/test_klt_cases_cpu.py shows that the restatement moves by at most 7.6e-6 px
on these cases when its sums are accumulated in float64 instead: 1e-3 px is 100 times that."""
import numpy as np
import pytest

from tests import klt_cases as KC
from tests import klt_ref as K
from tests.test_gpu_klt import _first_frame

pytestmark = pytest.mark.gpu

ATOL, FINE, SHARE = 0.02, 1e-3, 0.05


def _tracker(*a, **kw):
    from vi_ekf_amd.klt import KLTTracker
    return KLTTracker(*a, **kw)


def _np(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def _padding_ok(f, ids, cnt):
    for b in range(len(cnt)):
        assert np.isnan(f[b, cnt[b]:]).all() and (ids[b, cnt[b]:] == -1).all(), b


class _Spread:
    """|GPU - restatement| over the compared points of one case: 0.02 px on every point at once, the share at the end"""

    def __init__(self, label):
        self.label, self.d = label, []

    def add(self, gpu, ref, what=""):
        gpu, ref = np.asarray(gpu, np.float64).reshape(-1, 2), np.asarray(ref, np.float64).reshape(-1, 2)
        assert gpu.shape == ref.shape, (self.label, what, gpu.shape, ref.shape)
        d = np.abs(gpu - ref).max(1) if len(gpu) else np.zeros(0)
        self.d.append(d)
        assert (d <= ATOL).all(), "%s %s: %d of %d points off by more than %g px, worst %.4f" % (
            self.label, what, (d > ATOL).sum(), len(d), ATOL, d.max())

    def finish(self):
        d = np.concatenate(self.d) if self.d else np.zeros(0)
        share = float((d > FINE).mean()) if len(d) else 0.0
        print("LK %s: %d points compared, max |GPU - restatement| %.3e px, %.2f %% above 1e-3 px"
              % (self.label, len(d), d.max() if len(d) else 0.0, 100 * share))
        assert share <= SHARE, "%s: %.1f %% of %d points differ by more than 1e-3 px" % (self.label, 100 * share, len(d))
        return len(d)


def _resync(trk, refs):
    """the restatement continues from the GPU's own points, so a difference below the tolerance cannot grow into another
    kept set on a later frame"""
    pts, ids, nid = trk.get_points()
    for b, rf in enumerate(refs):
        rf.set_points(pts[b], ids[b])
        rf.next_id = int(nid[b])
    return pts, ids, nid


def _frame_against_restatement(trk, refs, frames, spread, what):
    """one load_image on the GPU and on one restated tracker per camera: counts and ids exact, positions within the LK
    tolerance, NaN / -1 padding"""
    f, ids, cnt = trk.load_image(np.stack(frames))
    _padding_ok(f, ids, cnt)
    for b, rf in enumerate(refs):
        first_new = rf.next_id
        rf_f, rf_i = rf.load_image(frames[b])
        assert cnt[b] == len(rf_i), (what, b, cnt[b], len(rf_i))
        np.testing.assert_array_equal(ids[b, :cnt[b]], rf_i, err_msg="%s camera %d" % (what, b))
        old = rf_i < first_new                          # carried over by LK; the others are this frame's corners: integers
        spread.add(f[b, :cnt[b]][old], rf_f[old], "%s camera %d" % (what, b))
        np.testing.assert_array_equal(f[b, :cnt[b]][~old], rf_f[~old], err_msg="%s camera %d, new corners" % (what, b))
    return f, ids, cnt


def _sequence_against_restatement(trk, refs, seq, label):
    spread = _Spread(label)
    out = []
    for k, frames in enumerate(seq):
        if k > 0:
            _resync(trk, refs)
        out.append(_frame_against_restatement(trk, refs, frames, spread, "frame %d" % k))
    spread.finish()
    return out


# -- 1. detector and pyramid on images smaller than the tile ----------------------------------------------------------------
@pytest.mark.parametrize("case", KC.SIZES, ids=KC.size_id)
def test_detector_and_pyramid_small_images(case):
    (W, H), levels, (MF, r) = case
    frames = [KC.dots(W, H, seed=s) for s in KC.SEEDS] + [KC.plateau(W, H)]
    if min(W, H) >= 40:
        frames.append(KC.squares(W, H, 4, 3))
    B = len(frames)
    trk = _first_frame(W, H, frames, MF, r)
    assert trk.levels == levels
    for b in range(B):
        ref = K.pyramid(frames[b])
        assert len(ref) == levels
        for l in range(levels):
            np.testing.assert_array_equal(trk.get_level(l)[b], ref[l], err_msg="level %d camera %d" % (l, b))
    if (W, H) == (8, 8):
        # nothing to track in the dots: empty outputs, and a second frame detects again without handing out an id
        pts, ids, nid = trk.get_points()
        for b in (0, 1):
            assert len(pts[b]) == 0 and len(ids[b]) == 0 and nid[b] == 0
        refs = [K.Tracker(W, H, MF, r) for _ in range(B)]
        for b in range(B):
            refs[b].load_image(frames[b])
        _resync(trk, refs)
        nxt = [KC.dots(W, H, 0.5, 0.25, seed=s) for s in KC.SEEDS] + frames[2:]
        spread = _Spread("8x8 second frame")
        f, ids, cnt = _frame_against_restatement(trk, refs, nxt, spread, "second frame")
        spread.finish()
        assert cnt[0] == 0 and cnt[1] == 0 and np.isnan(f[:2]).all() and (ids[:2] == -1).all()
        assert (trk.get_points()[2][:2] == 0).all()
    rng = np.random.default_rng(W * 1000 + H)
    masks = rng.integers(0, 4, (B, H, W)).astype(np.uint8) * 85          # 0 / 85 / 170 / 255, then > 1
    masks[:, H // 2:, : W // 3] = 1                                        # 1 is "not usable"
    _first_frame(W, H, frames, MF, r, masks=masks, per_camera=True)


# -- 2. LK at every pyramid depth -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", KC.SHIFTS, ids=lambda s: "%+.1f%+.1f" % s)
@pytest.mark.parametrize("case", KC.SIZES[1:], ids=KC.size_id)
def test_lk_every_pyramid_depth(case, shift):
    (W, H), levels, (MF, r) = case
    B = len(KC.SEEDS)
    f0 = [KC.dots(W, H, seed=s) for s in KC.SEEDS]
    f1 = [KC.dots(W, H, *shift, seed=s) for s in KC.SEEDS]
    trk = _tracker(B, W, H, max_features=MF, radius=r)
    assert trk.levels == levels
    trk.load_image(np.stack(f0))
    refs = [K.Tracker(W, H, MF, r) for _ in range(B)]
    for b in range(B):
        refs[b].load_image(f0[b])
    p0, i0, _ = _resync(trk, refs)
    fg, ig, cg = trk.load_image(np.stack(f1))
    p1, i1, _ = trk.get_points()
    spread = _Spread("%dx%d (%d levels) shift %s" % (W, H, levels, shift))
    for b in range(B):
        assert len(p0[b]) >= (10 if W >= 24 else 1)
        np.testing.assert_array_equal(i0[b], np.arange(len(i0[b])))
        nxt, st = K.lk(K.pyramid(f0[b]), K.pyramid(f1[b]), p0[b])
        sel = i1[b] < len(i0[b])                       # the points LK carried over (an id of frame 0 is its index there)
        assert st[i1[b][sel]].all(), "camera %d: the GPU kept a point the restatement's LK lost" % b
        spread.add(p1[b][sel], nxt[i1[b][sel]], "camera %d" % b)
        # the kept set, its order and the replenished corners are those of the restated tracker
        rf_f, rf_i = refs[b].load_image(f1[b])
        assert cg[b] == len(rf_i), (b, cg[b], len(rf_i))
        np.testing.assert_array_equal(ig[b, :cg[b]], rf_i, err_msg="camera %d" % b)
        np.testing.assert_allclose(fg[b, :cg[b]], rf_f, atol=ATOL, rtol=0)
        np.testing.assert_array_equal(fg[b, :cg[b]][~sel], rf_f[~sel])            # (new corners are integers: exact)
    _padding_ok(fg, ig, cg)
    spread.finish()


# -- 3. lifecycle on small images with shallow pyramids ---------------------------------------------------------------------
@pytest.mark.parametrize("case", [KC.SIZES[4], KC.SIZES[6], KC.SIZES[7]], ids=KC.size_id)
def test_lifecycle_small_and_shallow(case):
    (W, H), levels, (MF, r) = case
    B = 2
    trk = _tracker(B, W, H, max_features=MF, radius=r)
    assert trk.levels == levels and levels in (2, 3)
    mask = np.full((H, W), 255, np.uint8)
    mask[H // 2:H // 2 + H // 5, W // 8:W // 8 + W // 4] = 0          # a masked rectangle
    trk.set_mask(mask)
    refs = [K.Tracker(W, H, MF, r) for _ in range(B)]
    for rf in refs:
        rf.set_mask(mask)
    seq = [[KC.dots(W, H, 0.9 * k, -0.6 * k, seed=5), KC.dots(W, H, -0.9 * k, 0.6 * k, seed=5)] for k in range(8)]
    out = _sequence_against_restatement(trk, refs, seq, "lifecycle %dx%d" % (W, H))
    for f, ids, cnt in out:
        for b in range(B):
            x, y = K.round_away(f[b, :cnt[b]]).astype(int).T
            assert (mask[y, x] == 255).all()
    assert trk.get_points()[2].min() > MF                           # points left the image and were replenished


# -- 4. the documented limits of max_features and radius ----------------------------------------------------------------------
@pytest.mark.parametrize("limit", ["max_features_1024", "radius_0", "radius_1024"])
def test_limits_of_max_features_and_radius(limit):
    if limit == "max_features_1024":
        # VIEKF_KLT_MAX_FEATURES: every slot of k_prune's and k_corner's per-feature arrays and a full k_lk grid, beside a
        # camera that stays far below the limit
        W, H, MF, r = 333, 251, 1024, 3
        masks = np.full((2, H, W), 255, np.uint8)
        masks[1, :, W // 4:] = 0
        trk = _tracker(2, W, H, max_features=MF, radius=r)
        trk.set_mask(masks)
        refs = [K.Tracker(W, H, MF, r) for _ in range(2)]
        for b in range(2):
            refs[b].set_mask(masks[b])
        seq = [[KC.dots(W, H, 1.3 * k, -0.8 * k, seed=5), KC.dots(W, H, -1.3 * k, 0.8 * k, seed=6)] for k in range(3)]
        out = _sequence_against_restatement(trk, refs, seq, "max_features 1024 at 333x251")
        first = out[0][2]
        assert first[0] == MF and 64 < first[1] < MF // 2               # the first frame of camera 0 is full
        nid = trk.get_points()[2]
        assert nid[0] > MF and nid[1] > first[1]                        # both lost points and were replenished
    elif limit == "radius_0":
        # no neighbour is ever too close, and the replenish disc is the one pixel under a kept point
        for (W, H), MF in [((40, 33), 30), ((61, 47), 1024)]:
            trk = _tracker(2, W, H, max_features=MF, radius=0)
            refs = [K.Tracker(W, H, MF, 0) for _ in range(2)]
            seq = [[KC.dots(W, H, 0.9 * k, -0.6 * k, seed=s) for s in KC.SEEDS] for k in range(4)]
            out = _sequence_against_restatement(trk, refs, seq, "radius 0 at %dx%d / %d" % (W, H, MF))
            counts = [int(o[2][0]) for o in out]
            print("radius 0 at %dx%d / %d: counts %s" % (W, H, MF, counts))
            if MF == 30:
                assert counts == [30] * 4
            else:                                                       # never fills: more points every frame
                assert counts[0] > 30 and (np.diff(counts) > 0).all() and 64 < counts[-1] < MF
    else:
        # a radius larger than the image: the first corner's disc covers every pixel
        W, H, MF = 61, 47, 8
        trk = _tracker(2, W, H, max_features=MF, radius=1024)
        refs = [K.Tracker(W, H, MF, 1024) for _ in range(2)]
        seq = [[KC.dots(W, H, 0.9 * k, -0.6 * k, seed=s) for s in KC.SEEDS] for k in range(4)]
        out = _sequence_against_restatement(trk, refs, seq, "radius 1024 at 61x47")
        assert all((o[2] == 1).all() for o in out)


# -- 5. candidate counts around the LDS sort's capacity -----------------------------------------------------------------------
def test_sort_sizes_across_the_lds_boundary():
    W, H, MF, r = 333, 251, 300, 3
    img = KC.plateau(W, H)
    ns = KC.SORT_SIZES
    for group in (ns[0:4], ns[4:8], ns[8:11]):          # 8191 / 8192 / 8193 share a batch: both sort paths in one launch
        masks = np.stack([KC.exact_candidate_mask(img, n, seed=n) for n in group])
        for n, m in zip(group, masks):
            assert KC.n_candidates(img, m) == n          # (the restatement sees exactly n)
        trk = _first_frame(W, H, [img] * len(group), MF, r, masks=masks, per_camera=True)
        assert (trk.get_points()[2] >= 1).all()


# -- 6. a camera activated late, among cameras of very different counts -----------------------------------------------------------
def _ragged_masks(W, H):
    masks = np.full((4, H, W), 255, np.uint8)
    masks[1] = 0
    masks[1, 5:20, 5:22] = 255                          # a small window: a handful of corners
    masks[3, :, W // 2:] = 0                            # half the image
    return masks


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_late_activation_and_ragged_counts(device):
    import torch
    (W, H), _, (MF, r) = KC.SIZES[5]                    # 84x47, two levels
    MF = 80
    B, late, first = 4, 2, 2
    masks = _ragged_masks(W, H)
    seq = [np.stack([KC.dots(W, H, (0.8 + 0.3 * b) * k, -0.5 * k, seed=20 + b) for b in range(B)]) for k in range(5)]

    def give(x):
        return torch.from_numpy(np.ascontiguousarray(x)).cuda() if device else x

    big, plain, one = (_tracker(B, W, H, max_features=MF, radius=r), _tracker(B, W, H, max_features=MF, radius=r),
                       _tracker(1, W, H, max_features=MF, radius=r))
    gmasks = give(masks)
    big.set_mask(gmasks)
    big.sync()
    plain.set_mask(masks)
    one.set_mask(masks[late:late + 1])
    others = [b for b in range(B) if b != late]
    for k, fr in enumerate(seq):
        act = np.ones(B, np.uint8)
        act[late] = k >= first
        fb, ib, cb = (_np(x) for x in big.load_image(give(fr), active=give(act)))
        fp, ip, cp = plain.load_image(fr)
        _padding_ok(fb, ib, cb)
        # the other cameras do not notice that one of them is inactive
        np.testing.assert_array_equal(fb[others], fp[others])
        np.testing.assert_array_equal(ib[others], ip[others])
        np.testing.assert_array_equal(cb[others], cp[others])
        pts, ids, nid = big.get_points()
        if k < first:
            assert cb[late] == 0 and np.isnan(fb[late]).all() and (ib[late] == -1).all()
            assert len(pts[late]) == 0 and len(ids[late]) == 0 and nid[late] == 0
        else:
            # ... and the late camera is a fresh tracker that sees the frames from its activation on
            f1, i1, c1 = one.load_image(fr[late:late + 1])
            np.testing.assert_array_equal(fb[late], f1[0])
            np.testing.assert_array_equal(ib[late], i1[0])
            assert cb[late] == c1[0]
            p1 = one.get_points()
            np.testing.assert_array_equal(pts[late], p1[0][0])
            assert nid[late] == p1[2][0]
        if k == 0:
            # against the restatement: the first frame's corners, and counts more than a wavefront apart
            for b in others:
                ref = K.detect(fr[b], np.where(masks[b] > 1, 255, 0), MF, r)
                np.testing.assert_array_equal(fb[b, :cb[b]], ref.astype(np.float64))
            assert cb[0] - cb[1] > 64 and cb[1] > 0 and cb[1] < cb[3] < cb[0], cb
        if k == first:
            ref = K.detect(fr[late], np.where(masks[late] > 1, 255, 0), MF, r)
            np.testing.assert_array_equal(fb[late, :cb[late]], ref.astype(np.float64))
            np.testing.assert_array_equal(ib[late, :cb[late]], np.arange(len(ref)))


# -- 7. reset, a caller's stream, BGR8 with invert_image, the edges of drop_features -------------------------------------------
def test_reset_stream_and_drop_edges():
    import torch
    (W, H), _, _ = KC.SIZES[6]                          # 85x100, three levels
    MF, r, B = 40, 4, 2
    mask = np.full((H, W), 255, np.uint8)
    mask[30:60, 20:60] = 0
    seq = [np.stack([KC.dots(W, H, 0.9 * k, -0.6 * k, seed=s) for s in KC.SEEDS]) for k in range(4)]

    def masked_empty(f, cnt):
        for b in range(B):
            x, y = K.round_away(f[b, :cnt[b]]).astype(int).T
            assert (mask[y, x] == 255).all()

    # reset: the same sequence again equals a fresh tracker, bit for bit; the mask is kept
    trk, fresh = _tracker(B, W, H, max_features=MF, radius=r), _tracker(B, W, H, max_features=MF, radius=r)
    trk.set_mask(mask)
    fresh.set_mask(mask)
    for fr in seq[:3]:
        trk.load_image(fr[:, ::-1].copy())              # some other history
    trk.reset()
    pts, ids, nid = trk.get_points()
    assert all(len(p) == 0 for p in pts) and (nid == 0).all()
    for fr in seq:
        a, b_ = trk.load_image(fr), fresh.load_image(fr)
        for u, v in zip(a, b_):
            np.testing.assert_array_equal(u, v)
        masked_empty(a[0], a[2])
    ref = K.Tracker(W, H, MF, r)
    ref.set_mask(mask)
    trk.reset()
    f, ids, cnt = trk.load_image(seq[0])
    rf_f, rf_i = ref.load_image(seq[0][0])
    np.testing.assert_array_equal(f[0, :cnt[0]], rf_f)
    np.testing.assert_array_equal(ids[0, :cnt[0]], rf_i)

    # a caller's stream, device pointers and sync() equal the tracker on its own stream
    own, theirs = _tracker(B, W, H, max_features=MF, radius=r), _tracker(B, W, H, max_features=MF, radius=r)
    stream = torch.cuda.Stream()
    theirs.set_stream(stream.cuda_stream)
    dmask = torch.from_numpy(mask).cuda()
    theirs.set_mask(dmask)
    theirs.sync()
    own.set_mask(mask)
    for fr in seq:
        a = own.load_image(fr)
        b_ = theirs.load_image(torch.from_numpy(fr).cuda())
        theirs.sync()
        for u, v in zip(a, b_):
            np.testing.assert_array_equal(u, v.cpu().numpy())
    for u, v in zip(own.get_points()[0], theirs.get_points()[0]):
        np.testing.assert_array_equal(u, v)
    theirs.set_stream(None)                             # and on to the null stream
    a, b_ = own.load_image(seq[1]), theirs.load_image(seq[1])
    for u, v in zip(a, b_):
        np.testing.assert_array_equal(u, v)
    theirs.close()

    # BGR8 with invert_image equals GRAY8 of the converted, pre-flipped image, and the restatement
    bgr = [np.stack([np.stack([KC.dots(W, H, 0.7 * k, 0.4 * k, seed=40 + 3 * b + c) for c in range(3)], -1) for b in range(B)])
           for k in range(3)]
    inv, flp = _tracker(B, W, H, MF, r, invert_image=True), _tracker(B, W, H, MF, r)
    refs = [K.Tracker(W, H, MF, r, invert_image=True) for _ in range(B)]
    spread = _Spread("BGR8 inverted")
    for k, fr in enumerate(bgr):
        if k > 0:
            _resync(inv, refs)
        ri = _frame_against_restatement(inv, refs, list(fr), spread, "frame %d" % k)
        grey = np.stack([K.bgr2gray(x) for x in fr])
        rf = flp.load_image(np.ascontiguousarray(grey[:, ::-1, ::-1]))
        for u, v in zip(ri, rf):
            np.testing.assert_array_equal(u, v)
    spread.finish()

    # drop_features against the restatement's drop_feature
    trk = _tracker(B, W, H, max_features=MF, radius=r)
    refs = [K.Tracker(W, H, MF, r) for _ in range(B)]
    spread = _Spread("drop_features")
    f, ids, cnt = _frame_against_restatement(trk, refs, list(seq[0]), spread, "frame 0")
    assert (cnt == MF).all()
    before = trk.get_points()
    assert not trk.drop_features(np.full((B, 3), -1)).any()          # -1 means "none": nothing found, nothing changed
    after = trk.get_points()
    for u, v in zip(before[0] + before[1], after[0] + after[1]):
        np.testing.assert_array_equal(u, v)
    twice = np.stack([ids[b, [5, 5]] for b in range(B)])
    found = trk.drop_features(twice)                                  # the second mention finds it gone
    want = np.array([[rf.drop_feature(int(i)) for i in twice[b]] for b, rf in enumerate(refs)])
    np.testing.assert_array_equal(found, want)
    assert found.tolist() == [[True, False]] * B
    pts, pid, _ = trk.get_points()
    for b in range(B):
        np.testing.assert_array_equal(pid[b], refs[b].ids)
        np.testing.assert_array_equal(pts[b], refs[b].pts)
    _resync(trk, refs)
    f, ids, cnt = _frame_against_restatement(trk, refs, list(seq[1]), spread, "frame 1")
    # every id of camera 0 (camera 1: one real id among -1s)
    everything = np.full((B, MF), -1, np.int32)
    everything[0, :cnt[0]] = ids[0, :cnt[0]][::-1]
    everything[1, 7] = ids[1, 2]
    found = trk.drop_features(everything)
    want = np.array([[i >= 0 and rf.drop_feature(int(i)) for i in everything[b]] for b, rf in enumerate(refs)])
    np.testing.assert_array_equal(found, want)
    assert found[0, :cnt[0]].all() and found[1].sum() == 1
    pts, pid, nid = trk.get_points()
    assert len(pts[0]) == 0 and len(pid[0]) == 0 and len(pid[1]) == cnt[1] - 1
    nid0 = int(nid[0])
    _resync(trk, refs)
    f, ids, cnt = _frame_against_restatement(trk, refs, list(seq[2]), spread, "frame 2")
    # camera 0 had nothing for LK: MF fresh corners of this frame with fresh ids
    assert cnt[0] == MF
    np.testing.assert_array_equal(ids[0], np.arange(nid0, nid0 + MF))
    np.testing.assert_array_equal(f[0], K.detect(seq[2][0], KC.full(W, H), MF, r).astype(np.float64))
    spread.finish()
