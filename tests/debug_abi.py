"""The ctypes side of include/rvc_mi355x_debug.h for the GPU suites: the spec structs (test_abi_and_common.py pins their layout to the header), the
hooks' prototypes, an engine handle, and the bookkeeping on a tensor's whole allocation by its geometry
g = (size, offset of element (0, 0, 0), C, T (2-D: W), ld, bs, cs, H)."""
import ctypes as C

import numpy as np

from obs_rvc_amd import _native

RVC_SHAPE = 5


def _ints(*names):
    return [(n, C.c_int) for n in names]


class LayerSpec(C.Structure):
    """rvc_debug_layer_spec"""
    _fields_ = _ints("form", "streams", "cin", "cout", "kw", "stride", "pad", "dil", "groups", "t_in", "t_out", "x_halo", "y_halo", "r_halo", "act") + \
        [("slope", C.c_float), ("scale", C.c_float), ("accumulate", C.c_int), ("pre_act", C.c_int), ("pre_slope", C.c_float)] + \
        _ints("no_bias", "final_out", "glu", "res", "n") + [(n, C.c_int * 4) for n in ("kws", "dils", "pads")] + _ints("x_grouped", "res_grouped", "y_ws")


class OpSpec(C.Structure):
    """rvc_debug_op_spec"""
    _fields_ = _ints("op", "streams", "E", "heads", "T", "window", "C", "H", "x_halo", "y_halo", "reps", "graph")


class FrontSpec(C.Structure):
    """rvc_debug_front_spec"""
    _fields_ = _ints("op", "streams", "graph", "n", "frame") + [("bn_scale", C.c_float), ("bn_shift", C.c_float)] + \
        _ints("C", "L", "Tm", "update", "shift", "cache_start", "read_start", "R", "T", "upp", "x_halo", "f0_num", "f0_den") + \
        [("sr", C.c_float), ("lin_w", C.c_float), ("lin_b", C.c_float), ("seed", C.c_uint)]


class RmBlockSpec(C.Structure):
    """rvc_debug_rm_block_spec"""
    _fields_ = _ints("streams", "cin", "cout", "H", "W", "pool_in", "pool_out", "y_in_cat", "next", "rm_fuse", "graph", "reps")


class RetrievalSpec(C.Structure):
    """rvc_debug_retrieval_spec"""
    _fields_ = _ints("streams", "C", "T", "cv_ld", "skip_head", "R", "ph_ld") + [("rate", C.c_float)] + _ints("path", "reps", "graph")


class PostSpec(C.Structure):
    """rvc_debug_post_spec"""
    _fields_ = _ints("op", "streams", "graph", "n", "frame", "hop", "sola_len", "search", "f", "skip", "copy_begin", "rate_in", "rate_out", "chunk", "chunks") + \
        [(n, C.c_longlong) for n in ("in_bs", "out_bs", "r_bs", "sola_bs", "frame_bs", "cor_bs", "x_bs")]


class StreamState(C.Structure):
    """rvc_debug_stream_state (cache = cache_pitchf)"""
    _fields_ = [("uppower", C.c_float), ("stream_id", C.c_uint), ("chunk", C.c_uint), ("status", C.c_int), ("cache", C.c_float * 1024)]


def lib():
    """the loaded library with the prototypes of the hooks set"""
    L = _native.lib()
    vp, geo = C.c_void_p, C.POINTER(C.c_longlong)
    L.rvc_debug_layer.argtypes = [vp, C.POINTER(LayerSpec)] + [vp] * 5 + [geo]
    L.rvc_debug_op.argtypes = [vp, C.POINTER(OpSpec)] + [vp] * 5 + [geo]
    L.rvc_debug_front.argtypes = [vp, C.POINTER(FrontSpec), vp, vp, C.POINTER(vp), C.POINTER(StreamState), geo]
    L.rvc_debug_rm_block.argtypes = [vp, C.POINTER(RmBlockSpec)] + [vp] * 9 + [geo]
    L.rvc_debug_retrieval.argtypes = [vp, C.POINTER(RetrievalSpec)] + [vp] * 5
    L.rvc_debug_post.argtypes = [vp, C.POINTER(PostSpec), C.POINTER(vp), vp, vp]
    L.rvc_load_index.argtypes = [vp, vp, C.c_size_t, C.c_size_t]
    L.rvc_debug_conv_check.argtypes = L.rvc_debug_conv2d_check.argtypes = [vp] + [C.c_int] * 7
    L.rvc_debug_conv_check.restype = L.rvc_debug_conv2d_check.restype = C.c_double
    L.rvc_debug_last_kernel.restype = C.c_char_p
    L.rvc_debug_last_desc.restype = C.c_char_p
    L.rvc_debug_tap.argtypes = [vp, C.c_char_p, C.c_int, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rvc_debug_tap.restype = C.c_int
    L.rvc_set_gemm_precision.argtypes = [vp, C.c_int]
    L.rvc_set_gemm_precision.restype = C.c_int
    return L


def debug_tap(eng, name, stream, cap=1 << 22):
    """rvc_debug_tap on an RvcInfer engine -> (status, the tap of that stream of the last call)"""
    out, n = np.empty(cap, np.float32), C.c_size_t()
    rc = lib().rvc_debug_tap(eng._h, name.encode(), int(stream), out.ctypes.data, cap, C.byref(n))
    return rc, out[: n.value].copy() if rc == 0 else None


class Handle:
    """one engine without models: all a hook needs"""

    def __init__(self):
        self.L = lib()
        self.h = C.c_void_p()
        assert self.L.rvc_create(b"/tmp", 0, C.byref(self.h)) == 0

    def last_kernel(self):
        return self.L.rvc_debug_last_kernel().decode()

    def last_desc(self):
        """the whole description of the last implicit-GEMM launch queued: "reg M=.. N=.. K=.. ... split=2" """
        return self.L.rvc_debug_last_desc().decode()

    def last_error(self):
        return self.L.rvc_last_error_message(self.h).decode()

    def set_gemm_precision(self, mode):
        """rvc_set_gemm_precision: 0 = fp32, 1 = the exploratory split-bf16 GEMM wherever queue_bf3 takes a layer (rvc_debug_layer builds its plan under the engine's setting)"""
        assert self.L.rvc_set_gemm_precision(self.h, int(mode)) == 0, self.last_error()

    def close(self):
        self.L.rvc_destroy(self.h)


def ptr(a):
    return None if a is None else a.ctypes.data


def index(g, B, C0, nC, T, H=None):
    """element offsets of [B][C0:C0+nC][0:T] (2-D: [B][C0:C0+nC][0:H][0:T]) in an allocation of geometry g"""
    off, ld, bs, cs = g[1], g[4], g[5], g[6]
    b = np.arange(B)[:, None, None] * bs + np.arange(C0, C0 + nC)[None, :, None] * cs
    if H is None:
        return off + b + np.arange(T)[None, None, :]
    return off + b[..., None] + (np.arange(H) * ld)[None, None, :, None] + np.arange(T)[None, None, None, :]


def same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def stray(after, before, written):
    """positions of the floats that changed outside `written` (an index array, or a list of them)"""
    ch = after.view(np.uint32) != before.view(np.uint32)
    for w in written if isinstance(written, list) else [written]:
        ch[np.asarray(w).ravel()] = False
    return np.flatnonzero(ch)
