"""The flat-L2 retrieval alone (obs_rvc_amd/csrc/knn.hip.h, retrieval.hip build_retrieval) through rvc_debug_retrieval against tests/knn_ref.py: every case runs the
same inputs through every path that accepts them -- the one-launch form ("knn_fused"), the query GEMM + select ("knn_gemm", with its per-stream overflow
fallback), the forced exhaustive definition ("knn_exhaustive"; also the planner's choice at dim 44), the fallback list ("knn_fallback": run behind a fresh index load, so that it walks the row-major matrix) -- each forced
by hook and confirmed by rvc_debug_last_kernel, the copy of the index it scanned by rvc_debug_index_layouts.

Asserted: idx / dist / phone bit-identical between paths and idx / dist identical to oracle.knn_search; |dist[k] - D[k]| <= gamma D[k] and
|d64[idx[k]] - D[k]| <= 2 gamma D[k] against the sorted float64 distances, gamma = (dim + 2) 2^-24, no case excluded; the blend within
(4 gamma + 16 * 2^-24) max(|x|, |y|) of the float64 blend of the returned hits; padding of phone and cv untouched; the overflow words equal to the CPU prediction
(test_knn_ref.py proves what each input provokes).  The derivations are in knn_ref.py; every check prints its largest ratio to the bound before it asserts
(DESIGN.md "Retrieval: what is tested" records an MI355X run)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import knn_ref as KR
from common import set_opt
from debug_abi import RVC_SHAPE, Handle, RetrievalSpec, ptr, same_bits
from knn_ref import make_case

pytestmark = pytest.mark.gpu

HOOKS = ("RVC_KNN_NO_GEMM", "RVC_KNN_EXHAUSTIVE", "RVC_KNN_WGS")
# path -> (hooks, the aid's path, what rvc_debug_last_kernel must say)
PATHS = {
    "planner": ({}, 0, None),
    "fused": ({"RVC_KNN_NO_GEMM": "1"}, 0, "knn_fused"),
    "gemm": ({}, 0, "knn_gemm"),
    "exhaustive": ({"RVC_KNN_EXHAUSTIVE": "1"}, 0, "knn_exhaustive"),
    "fallback": ({"RVC_KNN_NO_GEMM": "1"}, 1, "knn_fallback"),
}
# (order matters: "gemm" and "exhaustive" build the transposed copy of the index, and a fallback list built after that scans it instead of the row-major matrix.
# "fallback" therefore runs behind a fresh load and "fused", which needs no transposed copy; Engine.run asserts which copy each path had)
FEW = ("fused", "fallback", "exhaustive")
MANY = ("fused", "fallback", "gemm", "exhaustive")
PH_FILL = np.float32(-5.0e3)


class Engine:
    """a bare engine with an index"""

    def __init__(self):
        self.h = Handle()
        self.L = self.h.L

    def load(self, index):
        self.index = np.ascontiguousarray(index, np.float32)
        assert self.L.rvc_load_index(self.h.h, ptr(self.index), self.index.shape[0], self.index.shape[1]) == 0, self.h.last_error()

    def run(self, cv, skip_head, R, T, rate=0.75, path="planner", reps=1, graph=0, wgs=None, ph_pad=3, expect=None, rc=0):
        """cv [streams][dim][cv_ld] -> dict(phone, cv, idx, dist, overflow, kernel, phone_in)"""
        hooks, apath, kernel = PATHS[path]
        B, dim, cv_ld = cv.shape
        phone_in = np.full((B, dim, R + ph_pad), PH_FILL, np.float32)
        phone, cvb = phone_in.copy(), np.ascontiguousarray(cv, np.float32).copy()
        idx, dist, ovf = np.full((B, R, 4), -7, np.int32), np.full((B, R, 4), -7.0, np.float32), np.full(B, -7, np.int32)
        s = RetrievalSpec(streams=B, C=dim, T=T, cv_ld=cv_ld, skip_head=skip_head, R=R, ph_ld=R + ph_pad, rate=rate, path=apath, reps=reps, graph=graph)
        try:
            for k, v in hooks.items():
                set_opt(k, v)
            if wgs is not None:
                set_opt("RVC_KNN_WGS", wgs)
            got = self.L.rvc_debug_retrieval(self.h.h, C.byref(s), ptr(cvb), ptr(phone), ptr(idx), ptr(dist), ptr(ovf))
            name = self.h.last_kernel()
            layouts = self.L.rvc_debug_index_layouts(self.h.h)
        finally:
            for k in HOOKS:
                set_opt(k, None)
        if got != rc and "hip" in self.h.last_error():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % self.h.last_error(), returncode=3)
        assert got == rc, (path, got, self.h.last_error())
        if rc == 0:
            assert name == (expect or kernel), (path, name)
            if name == "knn_fallback":
                assert not layouts & 2, "the fallback list scanned the transposed copy, not the row-major matrix"
            if name in ("knn_gemm", "knn_exhaustive"):
                assert layouts & 2
        return dict(phone=phone, cv=cvb, idx=idx, dist=dist, overflow=ovf, kernel=name, phone_in=phone_in)

    def close(self):
        self.h.close()


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


WORST = {}


def run_case(eng, case, paths, rate=0.75, wgs=None, cv_pad=5, expect=None):
    eng.load(case.index)
    cv = KR.to_cv(case.q, case.T + cv_pad)
    res = {p: eng.run(cv, case.skip_head, case.R, case.T, rate=rate, path=p, wgs=wgs, expect=(expect or {}).get(p)) for p in paths}
    check(case, cv, res, rate)
    return res


def check(case, cv, res, rate, bad_streams=(), exact_frames=None):
    """everything the module docstring lists, for the results of one case on several paths"""
    from oracle import oracle as O
    paths = list(res)
    first = res[paths[0]]
    for p in paths:
        r = res[p]
        assert same_bits(r["idx"].view(np.float32), first["idx"].view(np.float32)), (case.name, p, "idx differs from " + paths[0])
        assert same_bits(r["dist"], first["dist"]), (case.name, p, "dist differs from " + paths[0])
        assert same_bits(r["phone"], first["phone"]), (case.name, p, "phone differs from " + paths[0])
        assert same_bits(r["phone"][:, :, case.R:], r["phone_in"][:, :, case.R:]), (case.name, p, "phone padding written")
        assert same_bits(r["cv"], cv), (case.name, p, "cv written")
        # the overflow words: the CPU prediction on the many-stream path, zeros elsewhere
        if r["kernel"] == "knn_gemm":
            pred = [int(KR.candidates(case.index, case.used(b)).max() > KR.KNN_CAND) if b not in bad_streams else None for b in range(case.streams)]
            assert [o if w is not None else None for o, w in zip(r["overflow"].tolist(), pred)] == pred, (case.name, r["overflow"].tolist(), pred)
        else:
            assert not r["overflow"].any()
    cols = KR.col_map(case.skip_head, case.R, case.T)
    g, bb = KR.gamma(case.dim), KR.blend_bound(case.dim)
    wd = wi = wb = 0.0
    for b in range(case.streams):
        idx, dist, phone = first["idx"][b], first["dist"][b], first["phone"][b, :, :case.R].T        # [R][4], [R][4], [R][dim]
        if b in bad_streams:
            assert (idx == -1).all(), (case.name, b, idx)
            continue
        q = case.q[b, cols]
        io, do = O.knn_search(case.index, q, 4)
        assert np.array_equal(idx, io) and same_bits(dist, do), (case.name, b, "not the oracle's hits")
        d = KR.d64(case.index, case.used(b))[cols - case.first_raw]
        _, D = KR.topk(d)
        assert ((idx >= 0) & (idx < case.n)).all() and all(len(set(r)) == 4 for r in idx.tolist())
        assert np.all((dist[:, 1:] > dist[:, :-1]) | ((dist[:, 1:] == dist[:, :-1]) & (idx[:, 1:] > idx[:, :-1])))
        e_d, e_i = np.abs(dist - D), np.abs(np.take_along_axis(d, idx.astype(np.int64), 1) - D)
        with np.errstate(divide="ignore", invalid="ignore"):
            wd = max(wd, float(np.nanmax(np.where(D > 0, e_d / (g * D), 0.0))))
            wi = max(wi, float(np.nanmax(np.where(D > 0, e_i / (2 * g * D), 0.0))))
        assert np.all(e_d <= g * D), (case.name, b, wd)
        assert np.all(e_i <= 2 * g * D), (case.name, b, wi)
        for r in range(case.R):
            if exact_frames is not None and (b, r) in exact_frames:
                continue
            ref, mag = KR.blend(case.index, q[r], idx[r], rate)
            err = np.abs(phone[r] - ref)
            wb = max(wb, float(np.max(err / (bb * mag + 1e-300))))
            assert np.all(err <= bb * mag), (case.name, b, r, wb)
            if rate == 0.0:
                assert same_bits(phone[r], q[r])
    key = case.name
    WORST[key] = tuple(max(a, c) for a, c in zip(WORST.get(key, (0, 0, 0)), (wd, wi, wb)))
    print("%s dim %d n %d streams %d nq %d [%s]: dist %.3f of gamma D, index %.3f of 2 gamma D, blend %.3f of its bound (class so far %.3f %.3f %.3f)" %
          ((case.name, case.dim, case.n, case.streams, case.nq, ",".join(paths), wd, wi, wb) + WORST[key]))


# ---- 1. few streams: the one-launch form, the definition and the row-major list ----
@pytest.mark.parametrize("i,n", list(enumerate([4, 15, 16, 17, 63, 65, 257, 1023])))
def test_few_streams_small_indexes(eng, i, n):
    streams, nq = (1, 3, 8)[i % 3], (1, 15, 16, 17, 33)[i % 5]
    names = ["gaussian", "offset3", "offset_dim"] + (["near_runs", "far_dups"] if n >= 63 else []) + (["norm_spread"] if n >= 257 else [])
    for name in names:
        run_case(eng, make_case(name, dim=48, n=n, streams=streams, nq=nq, seed=200 + n), FEW, wgs=768)


@pytest.mark.parametrize("dim", [16, 256, 768])
def test_few_streams_every_fast_dimension(eng, dim):
    for name in ("gaussian", "offset3", "offset_dim", "near_runs", "far_dups"):
        run_case(eng, make_case(name, dim=dim, n=257, streams=3, nq=17, seed=300 + dim), FEW, wgs=768)


def test_definition_path_at_dim_44(eng):
    # 44 is no multiple of 16 (the planner itself takes the non-MFMA definition) and leaves four elements behind the eight-wide loop; such a plan has no fallback list
    for n in (257, 1023):
        for name in ("gaussian", "offset3", "near_runs", "far_dups", "norm_spread"):
            case = make_case(name, dim=44, n=n, streams=3, nq=17, seed=400 + n)
            run_case(eng, case, ("planner",), expect={"planner": "knn_exhaustive"})
    eng.run(KR.to_cv(case.q, case.T), case.skip_head, case.R, case.T, path="fallback", rc=RVC_SHAPE)


def test_forced_grid_five_tiles_per_workgroup(eng):
    # RVC_KNN_WGS = 64: G = 64 workgroups over 325 tiles (five or six each), n % 16 = 9; the runs cross a tile boundary, the wrap of the slices and the partial tile
    for name in ("gaussian", "offset_dim", "near_runs", "far_dups"):
        case = make_case(name, dim=48, n=5193, streams=1, nq=17, seed=500, wgs=64)
        assert KR.fused_grid(case.n, 1, 64) == 64
        run_case(eng, case, FEW, wgs=64)


def test_workgroup_cap_binds(eng):
    # ceil(n / 64) = 1026 > KNN_FUSED_MAXG = 1024, and the hook asks for 4096 workgroups: the cap decides
    n = 65609
    assert (n + 63) // 64 > KR.KNN_FUSED_MAXG and KR.fused_grid(n, 1, 4096) == KR.KNN_FUSED_MAXG
    for name in ("gaussian", "near_runs"):
        run_case(eng, make_case(name, dim=16, n=n, streams=1, nq=16, seed=600, wgs=4096), ("fused", "fallback"), wgs=4096)


# ---- 2. many streams: the query GEMM, its select kernel and the per-stream overflow fallback ----
# (8 x 17: the geometry whose last three frames share the last column, so the select and merge kernels' own clamp to T - 1 bites on this path too)
@pytest.mark.parametrize("dim,n,streams,nq", [(48, 4099, 8, 16), (48, 1001, 12, 11), (48, 1023, 8, 17), (256, 4096, 8, 16), (768, 1001, 12, 11)])
def test_many_streams(eng, dim, n, streams, nq):
    # offset_dim and offset_dups overflow every stream: their hits come from the overflow-gated scan + merge (offset_dups: runs of near-duplicates and far
    # duplicates among them)
    names = ["gaussian", "offset3", "offset_dim", "offset_dups", "near_runs", "far_dups"] + (["norm_spread"] if dim == 48 else [])
    for name in names:
        res = run_case(eng, make_case(name, dim=dim, n=n, streams=streams, nq=nq, seed=700 + n), MANY, wgs=768)
        assert bool(res["gemm"]["overflow"].all()) == (name in ("offset_dim", "offset_dups"))           # (the prediction itself is asserted in check)


def test_margin_constant_decides_the_overflow_words(eng):
    # an offset whose candidate count straddles KNN_CAND under the margin: more than 1 000 with the constant as it is, fewer than 300 with half of it
    # (test_knn_ref.py).  Every stream must overflow -- and, through the fallback, still return the definition's hits
    res = run_case(eng, make_case("straddle", dim=48, n=4099, streams=8, nq=16, seed=100), MANY, wgs=768)
    assert res["gemm"]["overflow"].tolist() == [1] * 8


def test_mixed_streams_overflow_per_stream(eng):
    case = make_case("mixed", dim=48, n=4099, streams=8, nq=16, seed=100)
    res = run_case(eng, case, MANY, wgs=768)
    assert res["gemm"]["overflow"].tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    # a stream that did not overflow: the bits of its single-stream run
    cv = KR.to_cv(case.q, case.T + 5)
    for b in (1, 7):
        one = eng.run(cv[b:b + 1], case.skip_head, case.R, case.T, path="planner", expect="knn_fused")
        for k in ("idx", "dist", "phone"):
            assert same_bits(one[k][0].view(np.float32), res["gemm"][k][b].view(np.float32)), (b, k)


@pytest.mark.parametrize("n", [4160, 4099])
def test_truncated_list_second_pass(eng, n):
    # one thread of knn_select_blend_kernel holds more than four values inside the margin (vector-of-four order at n % 4 == 0, scalar order otherwise)
    case = make_case("truncated", dim=48, n=n, streams=8, nq=16, seed=100)
    res = run_case(eng, case, MANY, wgs=768)
    b, j = case.meta["where"]
    frames = np.flatnonzero(KR.col_map(case.skip_head, case.R, case.T) - case.first_raw == j)
    assert set(res["gemm"]["idx"][b, frames].ravel().tolist()) <= set(case.meta["rows"]) and not res["gemm"]["overflow"].any()


def test_planner_threshold_of_128_queries(eng):
    idx, q = KR.gaussian(800, 257, 16, 128, KR.GEOMS[1][2])
    eng.load(idx)
    s, R, T = KR.GEOMS[1]
    cv = KR.to_cv(q, T)
    below = eng.run(cv[:127], s, R, T, path="planner", expect="knn_fused")
    at = eng.run(cv, s, R, T, path="planner", expect="knn_gemm")
    for k in ("idx", "dist", "phone"):
        assert same_bits(below[k].view(np.float32), at[k][:127].view(np.float32))


# ---- 3. edges of the definition ----
def test_exact_match_queries(eng):
    # d = 0 makes w infinite: the definition's arithmetic gives non-finite features for that frame, on every path the same, and touches no other frame
    for streams, nq, paths in ((3, 17, FEW), (8, 16, MANY)):
        case = make_case("gaussian", dim=48, n=1023, streams=streams, nq=nq, seed=900)
        hit = [(0, case.first_raw + 1, 77), (streams - 1, case.first_raw + nq - 1, 1022)]
        for b, t, row in hit:
            case.index[row] = case.q[b, t]
        cols = KR.col_map(case.skip_head, case.R, case.T)
        exact = {(b, int(r)) for b, t, _ in hit for r in np.flatnonzero(cols == t)}
        eng.load(case.index)
        cv = KR.to_cv(case.q, case.T + 5)
        res = {p: eng.run(cv, case.skip_head, case.R, case.T, path=p, wgs=768) for p in paths}
        first = res[paths[0]]
        for p in paths:
            assert np.array_equal(res[p]["phone"], first["phone"], equal_nan=True) and same_bits(res[p]["dist"], first["dist"])
            assert same_bits(res[p]["phone"][:, :, case.R:], res[p]["phone_in"][:, :, case.R:]), (p, "phone padding written")
            res[p]["phone"] = first["phone"]                   # (a NaN's payload is not part of the contract; check() compares the rest bit for bit)
        check(case, cv, res, 0.75, exact_frames=exact)
        bad = ~np.isfinite(first["phone"][:, :, :case.R])
        want = np.zeros_like(bad)
        for b, r in exact:
            want[b, :, r] = True
            assert first["dist"][b, r, 0] == 0.0
        assert np.array_equal(bad, want)


@pytest.mark.parametrize("rate", [0.0, 1.0])
def test_rate_zero_and_one(eng, rate):
    # rate 0: the gathered queries, bit for bit (asserted in check).  rate 1: the query term vanishes: the queries are a thousand times the index vectors, and the
    # features must stay within the blend bound taken over |y| ALONE -- a trace of x at 1e-8 of its size would already break it
    for streams, nq, paths in ((3, 17, FEW), (8, 16, MANY)):
        case = make_case("gaussian", dim=48, n=1023, streams=streams, nq=nq, seed=950)
        case.q *= np.float32(1000.0)
        res = run_case(eng, case, paths, rate=rate, wgs=768)
        if rate == 1.0:
            first = res[paths[0]]
            cols = KR.col_map(case.skip_head, case.R, case.T)
            worst = 0.0
            for b in range(streams):
                for r in range(case.R):
                    y = np.abs(case.index[first["idx"][b, r]].astype(np.float64)).max(0)
                    assert (np.abs(case.q[b, cols[r]]) > 10 * np.abs(y).max()).any()
                    ref, _ = KR.blend(case.index, case.q[b, cols[r]], first["idx"][b, r], 1.0)
                    err = np.abs(first["phone"][b, :, r] - ref)
                    worst = max(worst, float(np.max(err / (KR.blend_bound(48) * y + 1e-300))))
                    assert np.all(err <= KR.blend_bound(48) * y), (b, r, worst)
            print("rate 1, queries 1000 x the index: largest error %.3f of the bound over |y| alone" % worst)


# ---- 4. replay, and a second index ----
@pytest.mark.parametrize("path,streams,nq", [("fused", 3, 33), ("exhaustive", 3, 33), ("fallback", 3, 33), ("gemm", 8, 16), ("fused", 8, 16)])
def test_replay_gives_the_same_bits(eng, path, streams, nq):
    # three eager runs and three replays of one captured graph against one eager run; for the one-launch form the ticket words must be back at zero after every
    # launch (the aid also reads them back: non-zero words are an error)
    case = make_case("near_runs", dim=48, n=4099, streams=streams, nq=nq, seed=1000)
    eng.load(case.index)
    cv = KR.to_cv(case.q, case.T + 5)
    once = eng.run(cv, case.skip_head, case.R, case.T, path=path, wgs=768)
    for reps, graph in ((3, 0), (3, 1), (1, 1)):
        again = eng.run(cv, case.skip_head, case.R, case.T, path=path, reps=reps, graph=graph, wgs=768)
        for k in ("idx", "dist", "phone"):
            assert same_bits(again[k].view(np.float32), once[k].view(np.float32)), (path, reps, graph, k)
    check(case, cv, {path: once}, 0.75)


def test_overflow_fallback_replays(eng):
    case = make_case("mixed", dim=48, n=4099, streams=8, nq=16, seed=100)
    eng.load(case.index)
    cv = KR.to_cv(case.q, case.T + 5)
    once = eng.run(cv, case.skip_head, case.R, case.T, path="gemm")
    again = eng.run(cv, case.skip_head, case.R, case.T, path="gemm", reps=3, graph=1)
    for k in ("idx", "dist", "phone", "overflow"):
        assert same_bits(again[k].view(np.float32), once[k].view(np.float32)), k


def test_second_index_on_the_same_engine(eng):
    # another index, another dimension: plan and layout state of the first must be gone
    a = make_case("gaussian", dim=48, n=1023, streams=8, nq=16, seed=1100)
    b = make_case("far_dups", dim=256, n=257, streams=8, nq=16, seed=1101)
    c = make_case("near_runs", dim=48, n=1023, streams=8, nq=16, seed=1102)
    for case in (a, b, c):
        run_case(eng, case, MANY, wgs=768)
    eng.run(KR.to_cv(b.q, b.T), b.skip_head, b.R, b.T, rc=RVC_SHAPE)              # 256 channels against the 48 of the loaded index


# ---- 5. containment ----
def test_non_finite_queries_are_contained(eng):
    # stream 1 asks with a NaN in every query, stream 2 with an Inf: -1 on every path, and the other streams as if the two were ordinary
    for streams, nq, paths in ((4, 17, FEW), (8, 16, MANY)):
        case = make_case("gaussian", dim=48, n=1023, streams=streams, nq=nq, seed=1200)
        eng.load(case.index)
        clean = {p: eng.run(KR.to_cv(case.q, case.T + 5), case.skip_head, case.R, case.T, path=p, wgs=768) for p in paths}
        case.q[1, :, 5] = np.nan
        case.q[2, :, 7] = np.inf
        cv = KR.to_cv(case.q, case.T + 5)
        eng.load(case.index)                              # (again: the clean runs built the transposed copy, and the fallback list is to walk the row-major matrix)
        res = {p: eng.run(cv, case.skip_head, case.R, case.T, path=p, wgs=768) for p in paths}
        for p in paths:
            assert (res[p]["idx"][1:3] == -1).all(), (p, res[p]["idx"][1:3, 0])
            keep = [b for b in range(streams) if b not in (1, 2)]
            for k in ("idx", "dist", "phone"):
                assert same_bits(res[p][k][keep].view(np.float32), clean[p][k][keep].view(np.float32)), (p, k)
            assert np.array_equal(res[p]["phone"], res[paths[0]]["phone"], equal_nan=True), p
            assert same_bits(res[p]["phone"][:, :, case.R:], res[p]["phone_in"][:, :, case.R:]), (p, "phone padding written")
            res[p]["phone"] = res[paths[0]]["phone"]
        check(case, cv, res, 0.75, bad_streams=(1, 2))


# ---- 6. the aid's own arguments ----
def test_spec_is_validated(eng):
    case = make_case("gaussian", dim=48, n=257, streams=2, nq=17, seed=1300)
    eng.load(case.index)
    s, R, T = case.skip_head, case.R, case.T
    cv = KR.to_cv(case.q, T + 5)
    L, h = eng.L, eng.h.h
    bufs = lambda: (np.zeros((2, 48, R + 3), np.float32), np.zeros((2, R, 4), np.int32), np.zeros((2, R, 4), np.float32), np.zeros(2, np.int32))
    for bad in (dict(ph_ld=R - 1), dict(cv_ld=T - 1), dict(skip_head=s + 1), dict(C=32), dict(streams=0), dict(reps=0), dict(path=2), dict(rate=1.5), dict(R=0)):
        kw = dict(streams=2, C=48, T=T, cv_ld=T + 5, skip_head=s, R=R, ph_ld=R + 3, rate=0.5, path=0, reps=1, graph=0)
        kw.update(bad)
        ph, idx, dist, ovf = bufs()
        assert L.rvc_debug_retrieval(h, C.byref(RetrievalSpec(**kw)), ptr(cv.copy()), ptr(ph), ptr(idx), ptr(dist), ptr(ovf)) == RVC_SHAPE, bad
        assert not ph.any() and not idx.any()
