"""Vectorised numpy restatement of the KLT tracker: the reference's KLT_Tracker::load_image
(src/klt_tracker.cpp:54-170) -- goodFeaturesToTrack + calcOpticalFlowPyrLK, prune, replenish, ids -- as the spec
defines it.  Test infrastructure only: the tracker itself is the HIP code behind include/viekf_klt.h.

The corner detector and the pyramid are integer or correctly rounded, so the GPU must agree with them bit for bit; the
LK sums are float32 and only their order of summation differs from the GPU's.
"""
import numpy as np

QUALITY, BLOCK, WIN, HALF, MAX_LEVEL, ITERS, EPS2, MIN_EIG = 0.3, 7, 21, 10, 3, 30, 1e-4, 1e-4
FLT_EPSILON = np.float32(1.1920929e-07)
FLT_SCALE = np.float32(1.0 / (1 << 20))
F32 = np.float32


# -- image ------------------------------------------------------------------------------------------------------------
def bgr2gray(img):
    """integer BGR2GRAY: (1868 B + 9617 G + 4899 R + 8192) >> 14"""
    img = np.asarray(img, dtype=np.int32)
    return ((1868 * img[..., 0] + 9617 * img[..., 1] + 4899 * img[..., 2] + 8192) >> 14).astype(np.uint8)


def prepare(img, invert=False):
    """GRAY8 [H][W] or BGR8 [H][W][3] -> grey u8, rotated 180 degrees when invert"""
    g = bgr2gray(img) if np.ndim(img) == 3 else np.asarray(img, dtype=np.uint8)
    return np.ascontiguousarray(g[::-1, ::-1]) if invert else g


def reflect101(i, n):
    """REFLECT_101 index for any integer offset (period 2n-2)"""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i >= n, p - i, i)


def _pad(a, k):
    h, w = a.shape
    return a[reflect101(np.arange(-k, h + k), h)[:, None], reflect101(np.arange(-k, w + k), w)[None, :]]


# -- corner detector (goodFeaturesToTrack, src/klt_tracker.cpp:69,131) -----------------------------------------------------
def sobel(g):
    p = _pad(np.asarray(g, dtype=np.int32), 1)
    dx = (p[:-2, 2:] - p[:-2, :-2]) + 2 * (p[1:-1, 2:] - p[1:-1, :-2]) + (p[2:, 2:] - p[2:, :-2])
    dy = (p[2:, :-2] - p[:-2, :-2]) + 2 * (p[2:, 1:-1] - p[:-2, 1:-1]) + (p[2:, 2:] - p[:-2, 2:])
    return dx, dy


def box(a, k=BLOCK):
    r = k // 2
    p = _pad(np.asarray(a, dtype=np.int64), r)
    c = np.zeros((p.shape[0] + 1, p.shape[1] + 1), dtype=np.int64)
    c[1:, 1:] = p.cumsum(0).cumsum(1)
    return c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]


def min_eig(g):
    """lambda = max(0, 0.5 ((a + c) - sqrt((double) D))), D = (a - c)^2 + 4 b^2 in int64"""
    dx, dy = sobel(g)
    a, b, c = box(dx * dx), box(dx * dy), box(dy * dy)
    D = (a - c) * (a - c) + 4 * b * b
    return np.maximum(0.0, 0.5 * ((a + c).astype(np.float64) - np.sqrt(D.astype(np.float64))))


def candidates(g, mask):
    """-> (x, y, lambda') of every candidate, in selection order (lambda' descending, then raster order)"""
    H, W = g.shape
    lam = min_eig(g)
    m = np.asarray(mask) != 0
    mx = lam[m].max() if m.any() else 0.0
    lp = np.where(lam > QUALITY * mx, lam, 0.0)
    p = np.pad(lp, 1, constant_values=0.0)          # (lambda' >= 0: an ignored outside neighbour never raises the max)
    dil = np.max([p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], axis=0)
    c = (lp != 0) & m & (lp == dil)
    c[0, :] = c[-1, :] = False
    c[:, 0] = c[:, -1] = False
    ys, xs = np.nonzero(c)                           # raster order
    v = lp[ys, xs]
    o = np.lexsort((ys * W + xs, -v))
    return xs[o], ys[o], v[o]


def greedy(xs, ys, k, r):
    """accept a candidate when dx^2 + dy^2 >= r^2 against every accepted one; stop after k"""
    acc = []
    if k <= 0:
        return acc
    r2 = int(r) * int(r)
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    i, n, chunk = 0, len(xs), 256
    while i < n and len(acc) < k:
        cx, cy = xs[i:i + chunk], ys[i:i + chunk]
        ok = np.ones(len(cx), bool)
        if acc:
            a = np.array(acc, np.int64)
            ok = (((cx[:, None] - a[None, :, 0]) ** 2 + (cy[:, None] - a[None, :, 1]) ** 2) >= r2).all(1)
        mine = []                                    # accepted inside this chunk (the rest was tested above)
        for j in np.nonzero(ok)[0]:
            x, y = int(cx[j]), int(cy[j])
            if all((x - ax) ** 2 + (y - ay) ** 2 >= r2 for ax, ay in mine):
                mine.append((x, y))
                acc.append((x, y))
                if len(acc) == k:
                    break
        i += chunk
    return acc


def detect(g, mask, k, r):
    """-> float32 [n][2] (x, y) of at most k corners"""
    xs, ys, _ = candidates(g, mask)
    acc = greedy(xs, ys, k, r)
    return np.array(acc, dtype=np.float32).reshape(-1, 2)


# -- pyramid (buildOpticalFlowPyramid / pyrDown) -------------------------------------------------------------------------
K5 = np.array([1, 4, 6, 4, 1], dtype=np.int32)


def pyr_down(img):
    h, w = img.shape
    p = _pad(np.asarray(img, dtype=np.int32), 2)
    t = sum(K5[i] * p[:, i:i + w] for i in range(5))
    s = sum(K5[i] * t[i:i + h, :] for i in range(5))
    return ((s[::2, ::2] + 128) >> 8).astype(np.uint8)


def pyramid(g):
    lv = [np.asarray(g, dtype=np.uint8)]
    while len(lv) <= MAX_LEVEL:
        h, w = lv[-1].shape
        if (w + 1) // 2 <= WIN or (h + 1) // 2 <= WIN:
            break
        lv.append(pyr_down(lv[-1]))
    return lv


def scharr(img):
    p = _pad(np.asarray(img, dtype=np.int32), 1)
    ix = 3 * (p[:-2, 2:] - p[:-2, :-2]) + 10 * (p[1:-1, 2:] - p[1:-1, :-2]) + 3 * (p[2:, 2:] - p[2:, :-2])
    iy = 3 * (p[2:, :-2] - p[:-2, :-2]) + 10 * (p[2:, 1:-1] - p[:-2, 1:-1]) + 3 * (p[2:, 2:] - p[:-2, 2:])
    return ix.astype(np.int16), iy.astype(np.int16)


# -- pyramidal LK (calcOpticalFlowPyrLK with default arguments, src/klt_tracker.cpp:83) -----------------------------------
def _bilinear(img, X, Y, w4, reflect):
    """float32 ((w00 p00 + w01 p01) + w10 p10) + w11 p11 at integer corners X, Y (arrays [n][21][21])"""
    h, w = img.shape
    f = img.astype(np.float32)

    def rd(yy, xx):
        if reflect:
            return f[reflect101(yy, h), reflect101(xx, w)]
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, f[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], F32(0))

    w00, w01, w10, w11 = w4
    return ((w00 * rd(Y, X) + w01 * rd(Y, X + 1)) + w10 * rd(Y + 1, X)) + w11 * rd(Y + 1, X + 1)


def _window(pt, n):
    ip = np.floor(pt).astype(np.int64)
    a = (pt[:, 0] - ip[:, 0].astype(np.float32)).astype(np.float32)
    b = (pt[:, 1] - ip[:, 1].astype(np.float32)).astype(np.float32)
    one = F32(1)
    w4 = [((one - a) * (one - b))[:, None, None], (a * (one - b))[:, None, None], ((one - a) * b)[:, None, None],
          (a * b)[:, None, None]]
    r = np.arange(WIN)
    X = ip[:, 0][:, None, None] + r[None, None, :]
    Y = ip[:, 1][:, None, None] + r[None, :, None]
    return ip, w4, X, Y


def lk(prev_pyr, next_pyr, pts, acc=np.float32):
    """-> (next points float32 [n][2], status bool [n]).  `acc` is the dtype the five window sums accumulate in before they
    are cast to float32 (float64 states this restatement's own sensitivity to the order of summation)"""
    pts = np.asarray(pts, dtype=np.float32).reshape(-1, 2)
    n = len(pts)
    status = np.ones(n, bool)
    nxt_out = np.zeros((n, 2), np.float32)
    lmax = min(len(prev_pyr), len(next_pyr)) - 1
    half = F32(HALF)
    for l in range(lmax, -1, -1):
        I, J = prev_pyr[l], next_pyr[l]
        h, w = I.shape
        Ix, Iy = scharr(I)
        prev = (pts * F32(1.0 / (1 << l))).astype(np.float32)
        nxt = prev.copy() if l == lmax else (nxt_out * F32(2)).astype(np.float32)
        nxt_out = nxt.copy()
        if n == 0:
            continue
        prev = prev - half
        ip, w4, X, Y = _window(prev, n)
        inb = (ip[:, 0] >= -WIN) & (ip[:, 0] < w) & (ip[:, 1] >= -WIN) & (ip[:, 1] < h)
        ival = _bilinear(I, X, Y, w4, True) * F32(32)
        ix = _bilinear(Ix, X, Y, w4, False)
        iy = _bilinear(Iy, X, Y, w4, False)
        A11 = (ix * ix).reshape(n, -1).sum(1, dtype=acc).astype(np.float32) * FLT_SCALE
        A12 = (ix * iy).reshape(n, -1).sum(1, dtype=acc).astype(np.float32) * FLT_SCALE
        A22 = (iy * iy).reshape(n, -1).sum(1, dtype=acc).astype(np.float32) * FLT_SCALE
        D = A11 * A22 - A12 * A12
        with np.errstate(all="ignore"):
            mev = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F32(4) * A12 * A12)) / F32(2 * WIN * WIN)
            Dinv = F32(1) / D
        good = inb & ~((mev < F32(MIN_EIG)) | (D < FLT_EPSILON))
        if l == 0:
            status &= good
        run = good.copy()
        cur = nxt - half
        pdx = np.zeros(n, np.float32)
        pdy = np.zeros(n, np.float32)
        for j in range(ITERS):
            if not run.any():
                break
            inx, w4j, XJ, YJ = _window(cur, n)
            oob = (inx[:, 0] < -WIN) | (inx[:, 0] >= w) | (inx[:, 1] < -WIN) | (inx[:, 1] >= h)
            stop = run & oob
            if l == 0:
                status &= ~stop
            run &= ~oob
            jval = _bilinear(J, XJ, YJ, w4j, True) * F32(32)
            diff = jval - ival
            b1 = (diff * ix).reshape(n, -1).sum(1, dtype=acc).astype(np.float32) * FLT_SCALE
            b2 = (diff * iy).reshape(n, -1).sum(1, dtype=acc).astype(np.float32) * FLT_SCALE
            dx = ((A12 * b2 - A22 * b1) * Dinv).astype(np.float32)
            dy = ((A12 * b1 - A11 * b2) * Dinv).astype(np.float32)
            cur = np.where(run[:, None], cur + np.stack([dx, dy], 1), cur).astype(np.float32)
            nxt_out = np.where(run[:, None], cur + half, nxt_out).astype(np.float32)
            dd = dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2
            conv = run & (dd <= EPS2)
            run &= ~conv
            osc = run & (j > 0) & (np.abs(dx + pdx) < F32(0.01)) & (np.abs(dy + pdy) < F32(0.01))
            nxt_out = np.where(osc[:, None], nxt_out - np.stack([dx, dy], 1) * F32(0.5), nxt_out).astype(np.float32)
            run &= ~osc
            pdx, pdy = dx, dy
    return nxt_out, status


# -- tracker (KLT_Tracker) -------------------------------------------------------------------------------------------------
def round_away(v):
    return np.sign(v) * np.floor(np.abs(v) + 0.5)


class Tracker:
    """one camera's KLT_Tracker, with the deviations of DESIGN.md §8 (intended neighbour test, disc mask, aligned drop)"""

    def __init__(self, width, height, max_features, radius, invert_image=False):
        self.W, self.H, self.MF, self.r = int(width), int(height), int(max_features), int(radius)
        self.invert = bool(invert_image)
        self.mask = np.full((self.H, self.W), 255, np.uint8)
        self.reset()

    def reset(self):
        self.initialised = False
        self.next_id = 0
        self.pts = np.zeros((0, 2), np.float32)
        self.ids = np.zeros(0, np.int32)
        self.prev_pyr = None
        self.features = np.zeros((0, 2))

    def set_mask(self, mask):
        self.mask = np.where(np.asarray(mask) > 1, 255, 0).astype(np.uint8)

    def set_points(self, pts, ids):
        """restart from another implementation's state (the GPU's get_points)"""
        self.pts = np.asarray(pts, np.float32).reshape(-1, 2).copy()
        self.ids = np.asarray(ids, np.int32).copy()

    def _replenish_mask(self):
        m = self.mask.copy()
        yy, xx = np.mgrid[0:self.H, 0:self.W]
        for x, y in self.pts:
            cx, cy = int(np.rint(x)), int(np.rint(y))       # cvRound: halves to even
            m[(xx - cx) ** 2 + (yy - cy) ** 2 <= self.r * self.r] = 0
        return m

    def load_image(self, img):
        g = prepare(img, self.invert)
        pyr = pyramid(g)
        if not self.initialised:
            self.pts = detect(g, self.mask, self.MF, self.r)
            self.ids = np.arange(self.next_id, self.next_id + len(self.pts), dtype=np.int32)
            self.next_id += len(self.pts)
            self.initialised = True
        else:
            nxt, st = lk(self.prev_pyr, pyr, self.pts)
            keep = []
            for i in range(len(nxt) - 1, -1, -1):
                x, y = float(nxt[i, 0]), float(nxt[i, 1])
                if (not st[i] or x <= 1.0 or y <= 1.0 or x >= self.W - 1.0 or y >= self.H - 1.0
                        or self.mask[int(round_away(y)), int(round_away(x))] != 255):
                    continue
                if any(np.sqrt((float(nxt[k, 0]) - x) ** 2 + (float(nxt[k, 1]) - y) ** 2) < self.r for k in keep):
                    continue
                keep.append(i)
            keep = sorted(keep)
            self.pts = nxt[keep].astype(np.float32)
            self.ids = self.ids[keep]
            if len(self.pts) < self.MF:
                new = detect(g, self._replenish_mask(), self.MF - len(self.pts), self.r)
                self.pts = np.concatenate([self.pts, new]).astype(np.float32)
                self.ids = np.concatenate([self.ids, np.arange(self.next_id, self.next_id + len(new), dtype=np.int32)])
                self.next_id += len(new)
        self.prev_pyr = pyr
        f = self.pts.astype(np.float64)
        self.features = np.stack([np.clip(f[:, 0], 0, self.W), np.clip(f[:, 1], 0, self.H)], 1) if len(f) else f.reshape(0, 2)
        return self.features.copy(), self.ids.copy()

    def drop_feature(self, fid):
        hit = np.nonzero(self.ids == fid)[0]
        if len(hit) == 0:
            return False
        i = hit[0]
        self.pts = np.delete(self.pts, i, 0)
        self.ids = np.delete(self.ids, i)
        return True

    def sample_depth(self, depth_mm, min_depth):
        """src/vi_ekf_ros.cpp:284-297 on the last frame's (clamped) features; the read is clamped to the image"""
        d = np.asarray(depth_mm, np.float32)
        if self.invert:
            d = d[::-1, ::-1]
        f = self.features
        x = np.minimum(round_away(f[:, 0]).astype(int), self.W - 1)
        y = np.minimum(round_away(f[:, 1]).astype(int), self.H - 1)
        z = (d[y, x].astype(np.float64) * 1e-3).astype(np.float32).astype(np.float64)
        return np.where((z > 1e3) | (z < min_depth), np.nan, z)

    def outputs(self):
        """the C ABI's padded layout for this camera: features [MF][2] (NaN pad), ids [MF] (-1 pad), count"""
        f = np.full((self.MF, 2), np.nan)
        i = np.full(self.MF, -1, np.int32)
        n = len(self.features)
        f[:n], i[:n] = self.features, self.ids
        return f, i, n
