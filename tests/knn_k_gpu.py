"""What the k = 8 GPU suites share (tests/test_gpu_knn_k8.py, tests/test_gpu_ivf_k8.py): a bare engine with an index and a k, rvc_debug_retrieval with the
path hooks of tests/test_gpu_knn.py, and the checks of one flat-search result against tests/knn_k_ref.py and the oracle."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import knn_k_ref as R
from common import set_opt
from debug_abi import Handle, RetrievalSpec, ptr, same_bits

HOOKS = ("RVC_KNN_NO_GEMM", "RVC_KNN_EXHAUSTIVE", "RVC_KNN_WGS")
# path -> (hooks, the aid's path, what rvc_debug_last_kernel must say)
PATHS = {
    "planner": ({}, 0, None),
    "fused": ({"RVC_KNN_NO_GEMM": "1"}, 0, "knn_fused"),
    "gemm": ({}, 0, "knn_gemm"),
    "exhaustive": ({"RVC_KNN_EXHAUSTIVE": "1"}, 0, "knn_exhaustive"),
    "fallback": ({"RVC_KNN_NO_GEMM": "1"}, 1, "knn_fallback"),
}
# (order matters as in test_gpu_knn.py: "fallback" runs before a path that builds the transposed copy)
FEW = ("fused", "fallback", "exhaustive")
MANY = ("fused", "fallback", "gemm", "exhaustive")
PH_FILL = np.float32(-5.0e3)
SZ = C.c_size_t


class Engine:
    """a bare engine with an index, a k and, on request, an IVF structure"""

    def __init__(self):
        self.h = Handle()
        self.L = L = self.h.L
        L.rvc_set_index_k.argtypes = [C.c_void_p, C.c_int]
        L.rvc_index_k.argtypes = [C.c_void_p]
        L.rvc_set_index_ivf.argtypes = [C.c_void_p, C.c_void_p, SZ, SZ, C.c_void_p, SZ]
        L.rvc_set_index_nprobe.argtypes = [C.c_void_p, C.c_int]
        L.rvc_train_index_ivf.argtypes = [C.c_void_p, SZ, C.c_int, C.c_void_p, C.c_uint]
        L.rvc_get_index_ivf.argtypes = [C.c_void_p, C.c_void_p, SZ, C.c_void_p, SZ]

    def load(self, index, rc=0):
        index = np.ascontiguousarray(index, np.float32)
        got = self.L.rvc_load_index(self.h.h, ptr(index), index.shape[0], index.shape[1])
        assert got == rc, (got, self.h.last_error())
        if got == 0:
            self.index = index
        return got

    def set_k(self, k):
        return self.L.rvc_set_index_k(self.h.h, k)

    def k(self):
        return self.L.rvc_index_k(self.h.h)

    def attach(self, cent, assign, nprobe):
        cent, assign = np.ascontiguousarray(cent, np.float32), np.ascontiguousarray(assign, np.int32)
        assert self.L.rvc_set_index_ivf(self.h.h, ptr(cent), cent.shape[0], cent.shape[1], ptr(assign), assign.shape[0]) == 0, self.h.last_error()
        assert self.L.rvc_set_index_nprobe(self.h.h, nprobe) == 0, self.h.last_error()

    def run(self, cv, skip_head, R_, T, rate=0.75, path="planner", reps=1, graph=0, wgs=None, ph_pad=3, expect=None):
        """cv [streams][dim][cv_ld] -> dict(phone, cv, idx, dist, overflow, kernel, phone_in); idx / dist are [streams][R][k], k the engine's"""
        hooks, apath, kernel = PATHS[path]
        B, dim, cv_ld = cv.shape
        k = self.k()
        phone_in = np.full((B, dim, R_ + ph_pad), PH_FILL, np.float32)
        phone, cvb = phone_in.copy(), np.ascontiguousarray(cv, np.float32).copy()
        idx, dist, ovf = np.full((B, R_, k), -7, np.int32), np.full((B, R_, k), -7.0, np.float32), np.full(B, -7, np.int32)
        s = RetrievalSpec(streams=B, C=dim, T=T, cv_ld=cv_ld, skip_head=skip_head, R=R_, ph_ld=R_ + ph_pad, rate=rate, path=apath, reps=reps, graph=graph)
        try:
            for name, v in hooks.items():
                set_opt(name, v)
            if wgs is not None:
                set_opt("RVC_KNN_WGS", wgs)
            got = self.L.rvc_debug_retrieval(self.h.h, C.byref(s), ptr(cvb), ptr(phone), ptr(idx), ptr(dist), ptr(ovf))
            name = self.h.last_kernel()
        finally:
            for name_ in HOOKS:
                set_opt(name_, None)
        if got != 0 and "hip" in self.h.last_error():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % self.h.last_error(), returncode=3)
        assert got == 0, (path, got, self.h.last_error())
        want = expect or kernel
        assert want is None or name == want, (path, name)
        return dict(phone=phone, cv=cvb, idx=idx, dist=dist, overflow=ovf, kernel=name, phone_in=phone_in)

    def close(self):
        self.h.close()


def same_between(case, res, what="path"):
    """idx / dist / phone bit-identical between the results; padding and cv untouched"""
    names = list(res)
    first = res[names[0]]
    for p in names:
        r = res[p]
        for key in ("idx", "dist", "phone"):
            assert same_bits(r[key].view(np.float32), first[key].view(np.float32)), (case.name, what, p, key + " differs from " + names[0])
        assert same_bits(r["phone"][:, :, case.R:], r["phone_in"][:, :, case.R:]), (case.name, p, "phone padding written")


def check(case, cv, res, rate, K):
    """one case on several paths at K neighbours: everything tests/test_gpu_knn_k8.py's docstring lists but the k = 4 prefix"""
    from oracle import oracle as O
    same_between(case, res)
    for p, r in res.items():
        assert same_bits(r["cv"], cv), (case.name, p, "cv written")
        if r["kernel"] == "knn_gemm":
            pred = [int(R.candidates(case.index, case.used(b), K).max() > R.KNN_CAND) for b in range(case.streams)]
            assert r["overflow"].tolist() == pred, (case.name, r["overflow"].tolist(), pred)
        else:
            assert not r["overflow"].any(), (case.name, p)
    first = res[next(iter(res))]
    cols = R.col_map(case.skip_head, case.R, case.T)
    g, bb = R.gamma(case.dim), R.blend_bound(case.dim, K)
    wd = wi = wb = 0.0
    for b in range(case.streams):
        idx, dist, phone = first["idx"][b], first["dist"][b], first["phone"][b, :, :case.R].T        # [R][K], [R][K], [R][dim]
        q = case.q[b, cols]
        io, do = O.knn_search(case.index, q, K)
        assert np.array_equal(idx, io) and same_bits(dist, do), (case.name, b, "not the oracle's hits")
        d = R.d64(case.index, case.used(b))[cols - case.first_raw]
        _, D = R.topk(d, K)
        assert ((idx >= 0) & (idx < case.n)).all() and all(len(set(r)) == K for r in idx.tolist())
        assert np.all((dist[:, 1:] > dist[:, :-1]) | ((dist[:, 1:] == dist[:, :-1]) & (idx[:, 1:] > idx[:, :-1])))
        e_d, e_i = np.abs(dist - D), np.abs(np.take_along_axis(d, idx.astype(np.int64), 1) - D)
        with np.errstate(divide="ignore", invalid="ignore"):
            wd = max(wd, float(np.nanmax(np.where(D > 0, e_d / (g * D), 0.0))))
            wi = max(wi, float(np.nanmax(np.where(D > 0, e_i / (2 * g * D), 0.0))))
        assert np.all(e_d <= g * D), (case.name, b, wd)
        assert np.all(e_i <= 2 * g * D), (case.name, b, wi)
        for r in range(case.R):
            ref, mag = R.blend(case.index, q[r], idx[r], rate)
            err = np.abs(phone[r] - ref)
            wb = max(wb, float(np.max(err / (bb * mag + 1e-300))))
            assert np.all(err <= bb * mag), (case.name, b, r, wb)
            if rate == 0.0:
                assert same_bits(phone[r], q[r])
    print("k %d %s dim %d n %d streams %d nq %d [%s]: dist %.3f of gamma D, index %.3f of 2 gamma D, blend %.3f of its bound" %
          (K, case.name, case.dim, case.n, case.streams, case.nq, ",".join(res), wd, wi, wb))


def prefix_of(case, res8, res4):
    """the first four columns of the k = 8 hits are the same path's k = 4 hits, bit for bit (every hit has a row on the flat search)"""
    for p in res8:
        assert np.array_equal(res8[p]["idx"][:, :, :4], res4[p]["idx"]), (case.name, p, "idx[:4] is not the k = 4 result")
        assert same_bits(np.ascontiguousarray(res8[p]["dist"][:, :, :4]), res4[p]["dist"]), (case.name, p, "dist[:4] is not the k = 4 result")
