"""Cases for the KLT tracker's edge tests, shared by tests/test_klt_cases_cpu.py (the preconditions, on the restatement alone)
and tests/test_gpu_klt_edges.py (the HIP tracker against the restatement): a texture that has corners at every image size,
the sizes at which the pyramid depth changes, and masks that leave an exact number of candidates."""
import numpy as np

from tests import klt_ref as K
from tests.test_gpu_klt import plateau, squares  # noqa: F401  (re-exported: the same tie and plateau images)

# (W, H), pyramid levels (1 for min(W, H) <= 42, 2 up to 84, 3 up to 168, then 4), (max_features, radius).  8x8 is the
# smallest image the header allows; 16x9 and 24x19 are narrower than the 24x24 corner halo and the LK patch.
SIZES = [
    ((8, 8), 1, (10, 1)),
    ((16, 9), 1, (10, 1)),
    ((24, 19), 1, (10, 2)),
    ((42, 42), 1, (20, 2)),
    ((43, 61), 2, (60, 3)),
    ((84, 47), 2, (60, 3)),
    ((85, 100), 3, (80, 3)),
    ((168, 90), 3, (120, 4)),
    ((169, 171), 4, (200, 4)),
    ((333, 251), 4, (300, 4)),
]
SHIFTS = [(1.3, -0.8), (-4.6, 3.7)]
SEEDS = (5, 6)                      # the two `dots` cameras of every case
SORT_SIZES = [1, 2, 3, 63, 64, 65, 1023, 1025, 8191, 8192, 8193]   # around a wavefront, the power-of-two padding and the LDS limit


def size_id(case):
    return "%dx%d" % case[0]


def dots(W, H, dx=0.0, dy=0.0, seed=0, pitch=7.0):
    """u8 image of Gaussian blobs (amplitude +-60..80, sigma 1.4..1.9) on a jittered grid of `pitch` px over background 120,
    shifted by (dx, dy) px.  The grid reaches 3 pitches beyond the image, so a shift moves the same scene, and a blob every
    7 px leaves corners in an image of any size, a third to a half of them within 10 px of an edge."""
    rng = np.random.default_rng(seed)
    gx = np.arange(-3 * pitch, W + 3 * pitch, pitch)
    gy = np.arange(-3 * pitch, H + 3 * pitch, pitch)
    cy, cx = np.meshgrid(gy, gx, indexing="ij")
    cx = cx + rng.uniform(-2, 2, cx.shape)
    cy = cy + rng.uniform(-2, 2, cy.shape)
    amp = rng.choice([-1.0, 1.0], cx.shape)
    amp = amp * rng.uniform(60, 80, cx.shape)
    sg = rng.uniform(1.4, 1.9, cx.shape)
    xs = np.arange(W) - dx
    ys = np.arange(H) - dy
    img = np.full((H, W), 120.0)
    for x, y, a, s in zip(cx.ravel(), cy.ravel(), amp.ravel(), sg.ravel()):     # separable, each on its own +-5 sigma box
        x0, x1 = np.searchsorted(xs, x - 5 * s), np.searchsorted(xs, x + 5 * s)
        y0, y1 = np.searchsorted(ys, y - 5 * s), np.searchsorted(ys, y + 5 * s)
        if x1 > x0 and y1 > y0:
            img[y0:y1, x0:x1] += a * np.outer(np.exp(-(ys[y0:y1] - y) ** 2 / (2 * s * s)), np.exp(-(xs[x0:x1] - x) ** 2 / (2 * s * s)))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def full(W, H):
    return np.full((H, W), 255, np.uint8)


def n_candidates(img, mask=None):
    return len(K.candidates(img, full(img.shape[1], img.shape[0]) if mask is None else mask)[0])


_cand = {}


def exact_candidate_mask(img, n, seed):
    """a 0 / 255 mask whose usable pixels are n of the restatement's candidates of the unmasked image.  Entry 0, the
    strongest, is always among them: the masked maximum, and with it the threshold, stays what it was, and a candidate's 3x3
    maximum ignores the mask, so exactly these n pixels remain candidates."""
    key = img.tobytes()
    if key not in _cand:
        _cand.clear()                                # (one image at a time is enough)
        _cand[key] = K.candidates(img, full(img.shape[1], img.shape[0]))[:2]
    xs, ys = _cand[key]
    assert 1 <= n <= len(xs)
    pick = np.concatenate([[0], 1 + np.random.default_rng(seed).choice(len(xs) - 1, n - 1, replace=False)]).astype(int)
    m = np.zeros(img.shape, np.uint8)
    m[ys[pick], xs[pick]] = 255
    return m


def lk_spread(nxt, ref):
    """-> (points, largest |difference| in px, share of the points above 1e-3 px)"""
    if len(nxt) == 0:
        return 0, 0.0, 0.0
    d = np.abs(np.asarray(nxt, np.float64) - np.asarray(ref, np.float64)).max(1)
    return len(d), float(d.max()), float((d > 1e-3).mean())
