"""Python face of the consistency diagnostics (include/viekf_diag.h): NEES, log det P and the whitened error of every
filter of a batch from one Cholesky factorisation on the device, and the innovation statistics (NIS) the update's gate
would see.  Plumbing only -- the numbers come from libviekf_hip.so (csrc/viekf_kernels_diag.hpp); there is no CPU fallback.

Arguments may be numpy arrays (host pointers, numpy results) or torch tensors on the batch's device (device pointers,
torch results).  With device tensors `consistency` returns once its work is queued on the batch's stream -- `batch.sync()` or
a stream shared with torch orders it -- while `innovation` waits for it: it hands the library re-laid-out copies of z and R
that must outlive the kernel.  (`innovation` re-lays R out itself, not with _dev.r_colmajor: rdim is general here and r_mode
may be given.)"""
import ctypes as C

import numpy as np

from . import capi
from ._dev import empty, is_torch

# every symbol include/viekf_diag.h declares (tests check the library exports exactly these)
DIAG_SYMBOLS = ["viekf_diag_consistency", "viekf_diag_innovation"]
ONCHIP_MAX_FEATURES = 61     # VIEKF_DIAG_ONCHIP_MAX_FEATURES
_SLOT_MODELS = (5, 6, 8, 9)  # QZETA, FEAT, DEPTH, INV_DEPTH (viekf_meas_type)


def _bind():
    L = capi.lib()
    if getattr(L, "_diag_bound", False):
        return L
    vp, i32 = C.c_void_p, C.c_int32
    L.viekf_diag_consistency.argtypes = [vp, vp, vp, vp, vp, vp, C.c_int]
    L.viekf_diag_innovation.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, i32, vp, vp, vp, C.c_int]
    L._diag_bound = True
    return L


def _empty(batch, shape, dtype, like):
    """an output array on the side of `like` (a torch tensor on the batch's device, or anything else) -> (array, pointer)"""
    return empty(shape, dtype, batch.device if like is not None and is_torch(like) else None)


def consistency(batch, x_true=None):
    """viekf_diag_consistency for a BatchVIEKF -> dict(logdet [B], info [B]) and, with x_true [B][nx],
    nees [B][4] (leading blocks 3, 9, 16, m) and whitened [B][n] as well."""
    L = _bind()
    batch._keep = []
    pxt, where = batch._arg(x_true, np.float64, (batch.B, batch.nx), None)
    if where is None:
        where = capi.HOST
    out = {}
    out["logdet"], pl = _empty(batch, (batch.B,), np.float64, x_true)
    out["info"], pi = _empty(batch, (batch.B,), np.int32, x_true)
    pn = pw = None
    if x_true is not None:
        out["nees"], pn = _empty(batch, (batch.B, 4), np.float64, x_true)
        out["whitened"], pw = _empty(batch, (batch.B, batch.n), np.float64, x_true)
    capi.check(L.viekf_diag_consistency(batch._h, pxt, pl, pn, pw, pi, where))
    batch._keep = []
    return out


def innovation(batch, mtype, z, R, slot=None, r_mode=None):
    """viekf_diag_innovation for a BatchVIEKF: z [B][zdim] or [B][M][zdim]; R (rdim, rdim), (B, rdim, rdim) or
    (B, M, rdim, rdim), indexed [row, col]; slot [B] or [B][M] for the feature models.  r_mode (0 one R for all, 1 one per
    filter, 2 one per filter and measurement) is read from the number of axes of R unless given; the shape is checked
    against it
    -> dict(nis [B][M], residual [B][M][rdim], S [B][M][rdim][rdim] indexed [row, col]); the M axis is dropped when z has
    none."""
    L = _bind()
    batch._keep = []
    B = batch.B
    squeeze = len(z.shape) == 2
    M = 1 if squeeze else int(z.shape[1])
    zdim = int(z.shape[-1])
    rdim = int(R.shape[-1])
    tr = (lambda t: t.transpose(-1, -2).contiguous()) if is_torch(R) else (lambda t: np.ascontiguousarray(np.swapaxes(np.asarray(t, dtype=np.float64), -1, -2)))
    if r_mode is None:
        r_mode = len(R.shape) - 2
    want = {0: (rdim, rdim), 1: (B, rdim, rdim), 2: (B, M, rdim, rdim)}.get(r_mode)
    if want is None or tuple(R.shape) != want:
        raise ValueError("R must be (rdim,rdim), (B,rdim,rdim) or (B,M,rdim,rdim), matching r_mode")
    Rc = tr(R)   # the ABI takes column-major
    zc = z.reshape(B, M, zdim) if is_torch(z) else np.asarray(z, dtype=np.float64).reshape(B, M, zdim)
    pz, where = batch._arg(zc, np.float64, (B, M, zdim), None)
    pR, where = batch._arg(Rc, np.float64, tuple(Rc.shape), where)
    ps = None
    if slot is not None:
        sc = slot.reshape(B, M) if is_torch(slot) else np.asarray(slot, dtype=np.int32).reshape(B, M)
        ps, where = batch._arg(sc, np.int32, (B, M), where)
    nis, pn = _empty(batch, (B, M), np.float64, z)
    res, pr = _empty(batch, (B, M, 3), np.float64, z)
    S, pS = _empty(batch, (B, M, 9), np.float64, z)
    keep = (zc, Rc)   # (device tensors made here stay alive until the work that reads them is done: the sync below)
    capi.check(L.viekf_diag_innovation(batch._h, int(mtype), M, pz, zdim, ps, pR, rdim, r_mode, pn, pr, pS, where))
    if where == capi.DEVICE:
        batch.sync()
    del keep
    batch._keep = []
    Sm = S[:, :, :rdim * rdim].reshape(B, M, rdim, rdim)
    Sm = Sm.transpose(-1, -2) if is_torch(Sm) else np.swapaxes(Sm, -1, -2)
    out = dict(nis=nis, residual=res[:, :, :rdim], S=Sm)
    if squeeze:
        out = {k: v[:, 0] for k, v in out.items()}
    return out
