"""Preconditions of tests/test_gpu_klt_edges.py, on the numpy restatement alone (no GPU): the cases of tests/klt_cases.py have
the pyramid depth, the corners and the candidate counts the GPU tests rely on, and the restatement's LK moves by far less
than the GPU tolerance when its window sums are accumulated in another order (float64 instead of float32).  If one of
these fails, the case is wrong, not the bound."""
import numpy as np
import pytest

from tests import klt_cases as KC
from tests import klt_ref as K


@pytest.mark.parametrize("case", KC.SIZES, ids=KC.size_id)
def test_levels_and_corners_at_every_size(case):
    (W, H), levels, (MF, r) = case
    lo = min(W, H)
    assert levels == (1 if lo <= 42 else 2 if lo <= 84 else 3 if lo <= 168 else 4)
    for seed in KC.SEEDS:
        img = KC.dots(W, H, seed=seed)
        assert img.shape == (H, W) and img.dtype == np.uint8
        assert len(K.pyramid(img)) == levels
        n = len(K.detect(img, KC.full(W, H), MF, r))
        assert n >= (0 if (W, H) == (8, 8) else 10 if W >= 24 and H >= 19 else 1), (seed, n)
    if (W, H) == (8, 8):                             # too small for a blob's corner to clear the threshold and the border
        assert KC.n_candidates(KC.dots(W, H, seed=KC.SEEDS[0])) == 0


def test_candidate_counts_of_the_table():
    got = [KC.n_candidates(KC.dots(W, H, seed=5)) for (W, H), _, _ in KC.SIZES]
    assert got == [0, 1, 14, 39, 61, 92, 177, 280, 616, 1686], got


def test_a_shift_moves_the_same_scene():
    a, b = KC.dots(85, 100, seed=5), KC.dots(85, 100, 3.0, -2.0, seed=5)
    # (a whole-pixel shift; 1 grey level for a blob's +-5 sigma box cut at another pixel)
    assert np.abs(a[2:, :-3].astype(int) - b[:-2, 3:].astype(int)).max() <= 1
    assert np.abs(a.astype(int) - b.astype(int)).max() > 50


def test_exact_candidate_mask_gives_exactly_n():
    img = KC.plateau(333, 251)
    xs, ys, v = K.candidates(img, KC.full(333, 251))
    assert len(xs) > 80000 and (v == v[0]).sum() > 80000          # one plateau: nearly every candidate ties at the top
    for n in KC.SORT_SIZES:
        m = KC.exact_candidate_mask(img, n, seed=n)
        assert set(np.unique(m)) <= {0, 255} and (m != 0).sum() == n
        assert KC.n_candidates(img, m) == n
    d = KC.dots(84, 47, seed=5)
    assert KC.n_candidates(d, KC.exact_candidate_mask(d, 17, seed=1)) == 17


def test_first_frame_at_the_feature_limit_is_full():
    W, H = 333, 251
    t = K.Tracker(W, H, 1024, 3)
    f, ids = t.load_image(KC.dots(W, H, seed=5))
    assert len(ids) == 1024 and t.next_id == 1024
    t.load_image(KC.dots(W, H, *KC.SHIFTS[0], seed=5))
    assert (t.ids < 1024).sum() >= 900 and 1024 < t.next_id < 1150       # most survive LK, the border and the prune; few are new


@pytest.mark.parametrize("shift", KC.SHIFTS, ids=lambda s: "%+.1f%+.1f" % s)
@pytest.mark.parametrize("case", KC.SIZES[1:], ids=KC.size_id)
def test_lk_is_insensitive_to_the_order_of_its_sums(case, shift):
    """float32 against float64 accumulation of the five window sums: the status never differs and no point moves by
    1e-3 px (measured: at most 7.6e-6 px).  The GPU's butterfly sum may differ from the restatement in nothing else, which
    is what the 1e-3 px share bound of the GPU test stands on."""
    (W, H), _, (MF, r) = case
    for seed in KC.SEEDS:
        f0, f1 = KC.dots(W, H, seed=seed), KC.dots(W, H, *shift, seed=seed)
        pts = K.detect(f0, KC.full(W, H), MF, r)
        p0, p1 = K.pyramid(f0), K.pyramid(f1)
        a, sa = K.lk(p0, p1, pts, acc=np.float32)
        b, sb = K.lk(p0, p1, pts, acc=np.float64)
        d, sd = K.lk(p0, p1, pts)
        np.testing.assert_array_equal(a, d)                       # the default is the float32 accumulation, bit for bit
        np.testing.assert_array_equal(sa, sd)
        np.testing.assert_array_equal(sa, sb)
        n, worst, share = KC.lk_spread(a, b)
        print("%dx%d shift %s seed %d: %d points (%d tracked), max |f32 - f64| %.2e px" % (W, H, shift, seed, n, sa.sum(), worst))
        assert worst <= 1e-3


@pytest.mark.parametrize("case", [KC.SIZES[4], KC.SIZES[6], KC.SIZES[7]], ids=KC.size_id)
def test_small_lifecycle_replenishes(case):
    """the pan of the GPU lifecycle test pushes points out of these small images: new ids are handed out"""
    (W, H), _, (MF, r) = case
    t = K.Tracker(W, H, MF, r)
    for k in range(8):
        t.load_image(KC.dots(W, H, 0.9 * k, -0.6 * k, seed=5))
    assert t.next_id > MF
