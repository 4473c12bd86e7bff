"""What the wrappers of libviekf_hip.so share: telling a torch tensor from a host array, an output array with its pointer,
the row-major -> column-major re-layout of the pixel noise R, and the bases of the classes that own a C handle.  Plumbing
only; nothing here computes.

r_colmajor serves BatchVIEKF._meas_args and FrameIntake.intake, whose R is 2 x 2 with r_mode read from its shape.
diag.innovation keeps its own re-layout: its R is rdim x rdim for any rdim, its r_mode may be given by the caller, and it
raises another message -- fitting that in here would take a branch per difference."""
import ctypes as C

import numpy as np


def is_torch(a):
    return hasattr(a, "data_ptr") and hasattr(a, "is_cuda")


def empty(shape, dtype, device):
    """an uninitialised output: a torch tensor on cuda:<device>, or a numpy array when device is None -> (array, pointer)"""
    if device is not None:
        import torch
        t = torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device="cuda:%d" % device)
        return t, C.c_void_p(t.data_ptr())
    a = np.empty(shape, dtype=dtype)
    return a, C.c_void_p(a.ctypes.data)


def r_colmajor(R, B, M):
    """R (2,2), (B,2,2) or (B,M,2,2) indexed [row, col], numpy or torch -> (contiguous column-major copy, r_mode 0 / 1 / 2):
    the ABI takes column-major 2x2; a symmetric R is the same either way, transposed to be exact"""
    want = {(2, 2): 0, (B, 2, 2): 1, (B, M, 2, 2): 2}
    r_mode = want.get(tuple(R.shape))
    if r_mode is None:
        raise ValueError("R must be (2,2), (B,2,2) or (B,M,2,2)")
    if is_torch(R):
        return R.transpose(-1, -2).contiguous(), r_mode
    return np.ascontiguousarray(np.swapaxes(np.asarray(R, dtype=np.float64), -1, -2)), r_mode


class Handle:
    """owns one C handle: _L the library, _h the handle (None once closed), _destroy the name of its destroy function"""
    _destroy = None

    def __init__(self, lib):
        self._L = lib
        self._h = None

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise ValueError("this %s has been closed" % type(self).__name__)
        return self._h


class Companion(Handle):
    """a handle that lives on a BatchVIEKF and works on the batch's stream (its tables can go after their batch has)"""

    def __init__(self, lib, batch):
        super().__init__(lib)
        self.batch = batch      # (the batch must outlive the companion: it stays referenced from here)
        self._alive()

    def _alive(self):
        if getattr(self.batch, "_h", None) is None or not self.batch._h.value:
            raise ValueError("the batch of this %s has been closed" % type(self).__name__)

    def _handle(self):
        h = super()._handle()
        self._alive()
        return h

    def _empty(self, shape, dtype, device):
        return empty(shape, dtype, self.batch.device if device else None)

    def _ready(self, device, sync):
        """device outputs come from torch's caching allocator and the inputs may still be in torch's queue, while the
        work runs on the batch's stream (as BatchSimulator does)"""
        if device and sync:
            import torch
            torch.cuda.synchronize(self.batch.device)

    def _done(self, device, sync):
        if device and sync:
            self.batch.sync()
        self.batch._keep = []
