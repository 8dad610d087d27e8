"""Who owns the retrieval index and what a failed or interleaved change leaves behind (obs_rvc_amd/csrc/retrieval.hip install_index / attach_ivf, dev_raii.h):
a load the device refuses leaves an engine with no index, no stale plans and a clear HIP error state; loads, IVF attachments, a k-means training and an aborted
index build interleaved on one engine serve the bits of a fresh engine; rvc_destroy with an index, an IVF structure and an open build live leaves the process
able to go on.  Everything is bit-compared through rvc_debug_retrieval on the engine of tests/knn_k_gpu.py with the cases of knn_ref.py / ivf_ref.py.

No infer runs on an engine whose preceding load failed before the clean-state assertions have passed."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ivf_ref as IR
import knn_ref as KR
from common import voice_signal, zoo
from debug_abi import ptr, same_bits
from knn_k_gpu import Engine as BareEngine

pytestmark = pytest.mark.gpu

SZ = C.c_size_t
RVC_BACKEND = 4
WINDOW = 4000
HUGE_N, HUGE_DIM = 1 << 28, 1024                  # 2^40 bytes of fp32: no device has them, hipMalloc refuses at once and nothing is read or written


class Engine(BareEngine):
    """knn_k_gpu's bare engine; contentvec=True: on the tiny preset with ContentVec loaded (what the index builder needs)"""

    def __init__(self, contentvec=False):
        super().__init__()
        if contentvec:
            self.close()
            self.h.h = C.c_void_p()
            assert self.L.rvc_create(str(zoo("tiny")["data"]).encode(), 0, C.byref(self.h.h)) == 0
            assert self.L.rvc_load_contentvec(self.h.h, 2) == 0, self.h.last_error()

    def layouts(self):
        return self.L.rvc_debug_index_layouts(self.h.h)

    def nprobe(self):
        return self.L.rvc_index_nprobe(self.h.h)

    def device_ptr(self):
        nbytes = SZ(12345)
        return self.L.rvc_index_device_ptr(self.h.h, C.byref(nbytes)), nbytes.value

    def serve(self, case, **kw):
        return self.run(KR.to_cv(case.q, case.T + 5), case.skip_head, case.R, case.T, **kw)


class DeviceArray:
    """a host array's copy in device memory"""

    def __init__(self, a):
        self.hip = hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), SZ]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, SZ, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        a = np.ascontiguousarray(a, np.float32)
        self.p = C.c_void_p()
        assert hip.hipMalloc(C.byref(self.p), a.nbytes) == 0
        assert hip.hipMemcpy(self.p, a.ctypes.data, a.nbytes, 1) == 0               # hipMemcpyHostToDevice

    def free(self):
        assert self.hip.hipFree(self.p) == 0


def same_result(got, want, what):
    for key in ("idx", "dist", "phone"):
        assert same_bits(got[key].view(np.float32), want[key].view(np.float32)), (what, key)


# ---- the cases, and what a fresh engine serves for them (computed once, never changed) ----
def case_a(streams):
    """1023 x 48 with ivf_ref's structure of 37 lists"""
    return IR.build_case("gaussian", 1023, streams, 16, 3100)


def case_b(streams):
    """257 x 256: another row count and another dimension"""
    case = KR.make_case("far_dups", dim=256, n=257, streams=streams, nq=16, seed=3200)
    return (case,) + IR.make_structure(case)


_FRESH = {}


def fresh(what, streams):
    """the result of one case on an engine that has seen nothing else: "a8" = A flat at k = 8, "a_ivf" = A with its structure at nprobe 3, "b" = B flat"""
    if (what, streams) not in _FRESH:
        e = Engine()
        if what == "a8":
            case, _, _ = case_a(streams)
            e.load(case.index)
            assert e.set_k(8) == 0
            res = e.serve(case)
        elif what == "a_ivf":
            res = serve_a_ivf(e, streams)
        else:
            case, _, _ = case_b(streams)
            e.load(case.index)
            res = e.serve(case)
        e.close()
        _FRESH[(what, streams)] = res
    return _FRESH[(what, streams)]


def serve_a_ivf(e, streams):
    """test 2's first case: A loaded, its structure attached, nprobe 3"""
    case, cent, assign = case_a(streams)
    e.load(case.index)
    e.attach(cent, assign, 3)
    assert e.layouts() & 4 and e.nprobe() == 3
    return e.serve(case, expect="knn_ivf")


def open_build_with_a_recording(e):
    rows = SZ()
    x = voice_signal(WINDOW + 1500, seed=77)
    assert e.L.rvc_index_build_begin(e.h.h, WINDOW, 16) == 0, e.h.last_error()
    assert e.L.rvc_index_build_add(e.h.h, x.ctypes.data_as(C.POINTER(C.c_float)), len(x), C.byref(rows)) == 0, e.h.last_error()
    assert rows.value > 0


# ---- 1. a refused load leaves a clean engine ----
@pytest.mark.parametrize("via", ["device", "host"])
def test_refused_load_leaves_a_clean_engine(via):
    case, _, _ = case_a(8)
    e = Engine()
    e.load(case.index)
    e.serve(case)
    assert e.set_k(8) == 0
    small = np.zeros(16, np.float32)
    dev = DeviceArray(small)
    if via == "device":
        rc = e.L.rvc_load_index_device(e.h.h, dev.p, HUGE_N, HUGE_DIM)
    else:
        rc = e.L.rvc_load_index(e.h.h, ptr(small), HUGE_N, HUGE_DIM)
    assert rc == RVC_BACKEND and e.h.last_error(), (rc, e.h.last_error())
    # no index, no layout, no IVF structure, flat search; the caller's k is kept
    assert e.device_ptr() == (None, 0)
    assert e.layouts() == 0 and e.nprobe() == 0 and e.k() == 8
    # the next load succeeds (the refused allocation left no error behind for its checks to find) and serves a fresh engine's bits
    assert e.load(case.index) == 0
    assert e.device_ptr()[1] == case.index.nbytes
    same_result(e.serve(case), fresh("a8", 8), via)
    dev.free()
    e.close()


# ---- 2. interleaved lifetime on one engine ----
@pytest.mark.parametrize("streams", [1, 8])
def test_interleaved_lifetime(streams):
    e = Engine(contentvec=True)
    same_result(serve_a_ivf(e, streams), fresh("a_ivf", streams), "A with its structure")
    assert e.L.rvc_train_index_ivf(e.h.h, 16, 2, None, 0) == 0, e.h.last_error()
    assert e.layouts() & 4
    # B through the device entry point: the trained structure and the probe count go with A
    b, cent, assign = case_b(streams)
    dev = DeviceArray(b.index)
    assert e.L.rvc_load_index_device(e.h.h, dev.p, b.n, b.dim) == 0, e.h.last_error()
    dev.free()
    assert e.layouts() & 4 == 0 and e.nprobe() == 0
    same_result(e.serve(b), fresh("b", streams), "B flat")
    e.attach(cent, assign, 3)
    before = e.serve(b, expect="knn_ivf")
    layouts = e.layouts()
    # a build that is opened, fed and aborted touches nothing the engine serves
    open_build_with_a_recording(e)
    e.L.rvc_index_build_abort(e.h.h)
    assert e.layouts() == layouts and layouts & 4 and e.nprobe() == 3 and e.device_ptr()[1] == b.index.nbytes
    same_result(e.serve(b, expect="knn_ivf"), before, "B with its structure behind the aborted build")
    e.close()


# ---- 3. destroy with everything live ----
def test_destroy_with_everything_live():
    e = Engine(contentvec=True)
    serve_a_ivf(e, 8)
    open_build_with_a_recording(e)
    e.close()                                           # rvc_destroy: index, layouts, IVF structure and the open build all go
    e2 = Engine()
    same_result(serve_a_ivf(e2, 8), fresh("a_ivf", 8), "a second engine behind the destroy")
    e2.close()
