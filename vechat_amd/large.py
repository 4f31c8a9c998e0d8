"""The large-graph path over the C ABI `vc_large_run`: windows the fast path hands back as VC_WIN_OVERFLOW (a graph beyond its
16-bit tables, a layer too long for its LDS notes), computed on the device with 32-bit ids and tables in HBM.  Same bytes as the
fast path and the reference; slow per window.  No CPU path here either: without a device the call raises."""
import ctypes as C

import numpy as np

from . import capi


class LargeError(RuntimeError):
    def __init__(self, rc, msg):
        super().__init__(f"vc_large_run failed ({rc}): {msg}")
        self.rc = rc


def _declare(lib):
    return capi.bind(lib, ("vc_large_run", "vc_large_last_error", "vc_large_release"))


def large_consensus(batch: capi.Batch, params: capi.VcParams, lib=None):
    """-> (list of consensus bytes per window, status array), as HipContext.consensus returns them.  The capacity fields of
    params are ignored."""
    lib = _declare(lib or capi.load_hip())
    n = batch.n_windows
    cons = np.zeros(max(int(batch.bases.size), 1), np.uint8)      # a window's consensus is never longer than its sequences
    off = np.zeros(n + 1, np.uint64)
    status = np.zeros(n, np.uint8)
    r = capi.VcResult(off.ctypes.data_as(C.POINTER(C.c_uint64)), cons.ctypes.data_as(C.POINTER(C.c_uint8)), cons.size,
                      status.ctypes.data_as(C.POINTER(C.c_uint8)))
    vb = batch.as_struct()
    rc = lib.vc_large_run(C.byref(params), C.byref(vb), C.byref(r))
    if rc != 0:
        raise LargeError(rc, lib.vc_large_last_error().decode())
    return [cons[int(off[w]):int(off[w + 1])].tobytes() for w in range(n)], status


def release(lib=None):
    """vc_large_release: the large path's window tables and matrix buffer go back to the device."""
    _declare(lib or capi.load_hip()).vc_large_release()
