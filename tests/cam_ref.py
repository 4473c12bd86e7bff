"""numpy restatement of the camera model of include/viekf_cam.h (csrc/viekf_cam.hip), statement for statement: the forward
radial-tangential model and its Jacobian, the polar scan that derives r_valid, Newton's inverse with its validity rule, the
measurement noise R_out = J_u R J_u^T, the valid mask and the two image warps.  Vectorised over points (every lane does what the
device's lane does; a lane that has left the Newton loop is frozen), one intrinsics set per call.

Besides the results, undistort reports what the GPU tests need to show that a point is classified with margin: the number
of iterations, and per point the smallest distance to a boundary of the model met along its iterates."""
import numpy as np

MAX_ITER, STEP_TOL = 20, 1e-14
SCAN_STEP, SCAN_CAP, SCAN_DIRS = 2.0 ** -8, 4.0, 32
OK, PADDING, OUT_OF_MODEL = 0, 1, 2
RECTIFY, DISTORT = 0, 1

# the four coefficient sets of the tests: ocam.yaml's, a pure barrel, a barrel with tangential terms (both fold), a pincushion
OCAM = dict(focal=[533.013144, 533.503964], center=[316.680559, 230.660661], dist=[-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05])
DIST_SETS = [OCAM["dist"], [-0.3, 0.0, 0.0, 0.0], [-0.3, 0.02, 2e-3, -1e-3], [0.2, 0.05, 1e-3, -1e-3]]


def make(focal, center, dist=(0.0, 0.0, 0.0, 0.0), out_focal=None, out_center=None, min_det=0.0):
    """one intrinsics set with its derived r_valid"""
    k = dict(f=np.asarray(focal, float), c=np.asarray(center, float), k=np.asarray(dist, float),
             F=np.asarray(focal if out_focal is None else out_focal, float),
             C=np.asarray(center if out_center is None else out_center, float), min_det=float(min_det))
    k["r_valid"] = derive_r_valid(k)
    k["rv2"] = k["r_valid"] * k["r_valid"]
    return k


def forward(k, x, y, rv2=None):
    """-> xd, yd, j00, j01, j11, det, inside"""
    k1, k2, p1, p2 = k["k"]
    rv2 = k["rv2"] if rv2 is None else rv2
    with np.errstate(all="ignore"):
        r2 = x * x + y * y
        rad = 1.0 + k1 * r2 + k2 * r2 * r2
        drad = k1 + 2.0 * k2 * r2
        xd = x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        j00 = rad + 2.0 * x * x * drad + 2.0 * p1 * y + 6.0 * p2 * x
        j01 = 2.0 * x * y * drad + 2.0 * p1 * x + 2.0 * p2 * y
        j11 = rad + 2.0 * y * y * drad + 6.0 * p1 * y + 2.0 * p2 * x
        det = j00 * j11 - j01 * j01
        inside = (r2 <= rv2) & (det > k["min_det"])
    return xd, yd, j00, j01, j11, det, inside


def derive_r_valid(k):
    """the largest scanned radius up to which every sample of the polar scan has det > min_det"""
    rings = int(SCAN_CAP / SCAN_STEP)
    rv = 0.0
    j = np.arange(SCAN_DIRS)
    th = 2.0 * np.pi * j / SCAN_DIRS
    cs, sn = np.cos(th), np.sin(th)
    for i in range(1, rings + 1):
        r = i * SCAN_STEP
        det = forward(k, r * cs, r * sn, rv2=SCAN_CAP * SCAN_CAP)[5]
        if not (det > k["min_det"]).all():
            return rv
        rv = r
    return rv


def distort(k, z):
    """ideal pixels [..., 2] -> raw pixels [..., 2], J = d raw / d ideal [..., 4] column-major"""
    z = np.asarray(z, float)
    u, v = z[..., 0], z[..., 1]
    with np.errstate(all="ignore"):
        x, y = (u - k["C"][0]) / k["F"][0], (v - k["C"][1]) / k["F"][1]
        xd, yd, j00, j01, j11, det, _ = forward(k, x, y)
        raw = np.stack([k["f"][0] * xd + k["c"][0], k["f"][1] * yd + k["c"][1]], -1)
        J = np.stack([k["f"][0] * j00 / k["F"][0], k["f"][1] * j01 / k["F"][0], k["f"][0] * j01 / k["F"][1], k["f"][1] * j11 / k["F"][1]], -1)
    return raw, J


def undistort(k, z_raw, R=None):
    """raw pixels [..., 2], R [..., 4] column-major (broadcast over the points) or None
    -> dict(z [..., 2], R_out [..., 4] or None, status, iters, margin, Ju [..., 4] as j00 j01 j10 j11):
    margin is, for an OK point, the least of det - min_det and r_valid - r over every iterate (the solution included); for a
    point that left the model, how far beyond the boundary the iterate that left it was (the larger of r - r_valid and
    min_det - det); NaN for one that did not stop within MAX_ITER; +inf for padding."""
    z_raw = np.asarray(z_raw, float)
    shape = z_raw.shape[:-1]
    u, v = z_raw[..., 0].ravel(), z_raw[..., 1].ravel()
    n = u.size
    status = np.full(n, -1, np.int32)
    status[np.isnan(u) | np.isnan(v)] = PADDING
    margin = np.full(n, np.inf)
    iters = np.zeros(n, np.int32)
    rv, md = k["r_valid"], k["min_det"]

    def leave(live, r2, det, inside):
        out = live & ~inside
        with np.errstate(all="ignore"):
            viol = np.fmax(np.sqrt(r2) - rv, md - det)
        margin[out] = viol[out]
        status[out] = OUT_OF_MODEL
        m = np.fmin(det - md, rv - np.sqrt(r2))
        ok = live & inside
        margin[ok] = np.fmin(margin[ok], m[ok])

    with np.errstate(all="ignore"):
        xd, yd = (u - k["c"][0]) / k["f"][0], (v - k["c"][1]) / k["f"][1]
        x, y = xd.copy(), yd.copy()
        stopped = np.zeros(n, bool)
        for it in range(MAX_ITER):
            live = (status == -1) & ~stopped
            if not live.any():
                break
            fx, fy, j00, j01, j11, det, inside = forward(k, x, y)
            leave(live, x * x + y * y, det, inside)
            live = live & inside
            ex, ey = xd - fx, yd - fy
            sx, sy = (j11 * ex - j01 * ey) / det, (j00 * ey - j01 * ex) / det
            x, y = np.where(live, x + sx, x), np.where(live, y + sy, y)
            iters[live] += 1
            stopped |= live & (sx * sx + sy * sy <= STEP_TOL * STEP_TOL)
        never = (status == -1) & ~stopped
        status[never] = OUT_OF_MODEL
        margin[never] = np.nan
        live = (status == -1)
        fx, fy, j00, j01, j11, det, inside = forward(k, x, y)
        leave(live, x * x + y * y, det, inside)
        ok = live & inside
        status[ok] = OK
        nan = np.full(n, np.nan)
        z = np.stack([np.where(ok, k["F"][0] * x + k["C"][0], nan), np.where(ok, k["F"][1] * y + k["C"][1], nan)], -1)
        Ju = np.stack([k["F"][0] * j11 / det / k["f"][0], -k["F"][0] * j01 / det / k["f"][1],
                       -k["F"][1] * j01 / det / k["f"][0], k["F"][1] * j00 / det / k["f"][1]], -1)
        Ju[~ok] = np.nan
        R_out = None
        if R is not None:
            Rb = np.broadcast_to(np.asarray(R, float), shape + (4,)).reshape(n, 4)
            r00, r10, r01, r11 = Rb[:, 0], Rb[:, 1], Rb[:, 2], Rb[:, 3]
            t00, t01 = Ju[:, 0] * r00 + Ju[:, 1] * r10, Ju[:, 0] * r01 + Ju[:, 1] * r11
            t10, t11 = Ju[:, 2] * r00 + Ju[:, 3] * r10, Ju[:, 2] * r01 + Ju[:, 3] * r11
            o00 = t00 * Ju[:, 0] + t01 * Ju[:, 1]
            o10 = t10 * Ju[:, 0] + t11 * Ju[:, 1]
            o11 = t10 * Ju[:, 2] + t11 * Ju[:, 3]
            R_out = np.where(ok[:, None], np.stack([o00, o10, o10, o11], -1), Rb).reshape(shape + (4,))
    return dict(z=z.reshape(shape + (2,)), R_out=R_out, status=status.reshape(shape), iters=iters.reshape(shape),
                margin=margin.reshape(shape), Ju=Ju.reshape(shape + (4,)))


def pixel_grid(W, H):
    xs, ys = np.meshgrid(np.arange(W, dtype=float), np.arange(H, dtype=float))
    return np.stack([xs, ys], -1)


def valid_mask(k, W, H):
    """-> (mask [H][W] u8, margin [H][W])"""
    r = undistort(k, pixel_grid(W, H))
    return np.where(r["status"] == OK, 255, 0).astype(np.uint8), r["margin"]


def warp(k, direction, src, depth=None, fill=0):
    """src [H][W] u8, depth [H][W] float32 or None -> dict(val [H][W] the grey before floor(v + 0.5) (fill where nothing is
    sampled), sampled [H][W] bool, depth [H][W] float32 (+inf where nothing is sampled), sx, sy [H][W] (NaN outside the model))"""
    H, W = src.shape
    g = pixel_grid(W, H)
    with np.errstate(all="ignore"):
        if direction == RECTIFY:
            x, y = (g[..., 0] - k["C"][0]) / k["F"][0], (g[..., 1] - k["C"][1]) / k["F"][1]
            xd, yd, _, _, _, _, inside = forward(k, x, y)
            sx = np.where(inside, k["f"][0] * xd + k["c"][0], np.nan)
            sy = np.where(inside, k["f"][1] * yd + k["c"][1], np.nan)
        else:
            r = undistort(k, g)
            sx, sy = r["z"][..., 0], r["z"][..., 1]
        sampled = (sx >= 0.0) & (sx <= float(W - 1)) & (sy >= 0.0) & (sy <= float(H - 1))
        qx, qy = np.where(sampled, sx, 0.0), np.where(sampled, sy, 0.0)
        fx, fy = np.floor(qx), np.floor(qy)
        x0, y0 = fx.astype(int), fy.astype(int)
        x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
        ax, ay = qx - fx, qy - fy
        I = src.astype(float)
        v = (1.0 - ay) * ((1.0 - ax) * I[y0, x0] + ax * I[y0, x1]) + ay * ((1.0 - ax) * I[y1, x0] + ax * I[y1, x1])
        val = np.where(sampled, v, float(fill))
        dep = None
        if depth is not None:
            xn, yn = np.floor(qx + 0.5).astype(int), np.floor(qy + 0.5).astype(int)
            dep = np.where(sampled, depth[yn, xn], np.float32(np.inf)).astype(np.float32)
    return dict(val=val, sampled=sampled, depth=dep, sx=sx, sy=sy)


def warp_unclear(w, W, H, tol=1e-9):
    """the pixels a GPU test may leave out: the restated source coordinate within tol of the source's border or of a
    nearest-neighbour tie"""
    sx, sy = w["sx"], w["sy"]
    with np.errstate(all="ignore"):
        border = (np.abs(sx) < tol) | (np.abs(sx - (W - 1)) < tol) | (np.abs(sy) < tol) | (np.abs(sy - (H - 1)) < tol)
        tie = (np.abs(sx - np.floor(sx) - 0.5) < tol) | (np.abs(sy - np.floor(sy) - 0.5) < tol)
    return border | (tie & w["sampled"])
