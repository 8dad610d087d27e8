"""The ctypes side of the index builder for tests/test_gpu_index_build.py: rvc_debug_index_append (include/rvc_mi355x_debug.h) and the rvc_index_build_*
entry points on a raw handle."""
import ctypes as C

import numpy as np

from obs_rvc_amd import _native

SZ = C.c_size_t
RVC_CONTENTVEC_NOT_LOADED = 2
RVC_SHAPE = 5


def lib():
    L = _native.lib()
    vp = C.c_void_p
    L.rvc_debug_index_append.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, SZ, SZ, vp, vp, SZ, C.POINTER(SZ), C.POINTER(SZ)]
    L.rvc_debug_index_append.restype = C.c_int
    return L


def index_append(h, cv, T, cursor, capacity, head=None):
    """cv [C][ld] float32 -> (status, the store's rows [rows][C], rows dropped)"""
    L = lib()
    cv = np.ascontiguousarray(cv, np.float32)
    Cc, ld = cv.shape
    head = None if head is None else np.ascontiguousarray(head, np.float32)
    out = np.full((cursor + T, Cc), -7.0, np.float32)
    rows, dropped = SZ(), SZ()
    rc = L.rvc_debug_index_append(h, cv.ctypes.data, Cc, T, ld, cursor, capacity, None if head is None else head.ctypes.data, out.ctypes.data, cursor + T,
                                  C.byref(rows), C.byref(dropped))
    return rc, out[: rows.value].copy(), dropped.value


def device_to_host(ptr, nbytes):
    """a copy of device memory as float32"""
    out = np.empty(nbytes // 4, np.float32)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipDeviceSynchronize() == 0
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0                 # hipMemcpyDeviceToHost
    return out
