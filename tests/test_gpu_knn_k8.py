"""The flat-L2 retrieval at upstream's k = 8 (rvc_set_index_k) through rvc_debug_retrieval against tests/knn_k_ref.py: every case runs
the same inputs through every path that accepts them -- the one-launch form ("knn_fused"), its row-major fallback list ("knn_fallback"), the query GEMM +
select ("knn_gemm", with its per-stream overflow fallback) and the forced definition ("knn_exhaustive") -- forced by the hooks of tests/test_gpu_knn.py and
confirmed by rvc_debug_last_kernel.

Asserted per case, no case or row excluded: idx / dist / phone bit-identical between paths; idx / dist identical to oracle.knn_search(index, q, 8); eight
distinct in-range ids per row, sorted by (dist, idx); |dist[k] - D[k]| <= gamma D[k] and |d64[idx[k]] - D[k]| <= 2 gamma D[k] against the sorted float64
distances, gamma = (dim + 2) 2^-24; the blend within (4 gamma + 20 * 2^-24) max(|x|, |y|) of the float64 blend of the returned hits (knn_k_ref.py derives
both); padding of phone and cv untouched; the overflow words equal to the CPU prediction on the GEMM path (tests/test_knn_k_ref.py proves every count is far
from KNN_CAND) and zero elsewhere; the first four columns equal to the same path's k = 4 result bitwise.  Every check prints its largest ratio to the bound
before it asserts."""
from __future__ import annotations

import numpy as np
import pytest

import knn_k_ref as R
import knn_ref as KR
from debug_abi import RVC_SHAPE, same_bits
from knn_k_gpu import FEW, MANY, Engine, check, prefix_of, same_between

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    assert e.set_k(4) == 0
    e.close()


@pytest.fixture(scope="module")
def cases():
    return R.shared_cases()


def run_case(eng, case, paths, rate=0.75, wgs=768, cv_pad=5, expect=None, reps=1, graph=0):
    """k = 8 and k = 4 on every path, one index load; -> the k = 8 results"""
    eng.load(case.index)
    cv = R.to_cv(case.q, case.T + cv_pad)
    out = {}
    for k in (8, 4):
        assert eng.set_k(k) == 0 and eng.k() == k, eng.h.last_error()
        out[k] = {p: eng.run(cv, case.skip_head, case.R, case.T, rate=rate, path=p, wgs=wgs, expect=(expect or {}).get(p), reps=reps, graph=graph) for p in paths}
        assert all(r["idx"].shape[2] == k for r in out[k].values())
    check(case, cv, out[8], rate, 8)
    same_between(case, out[4])
    prefix_of(case, out[8], out[4])
    return out[8]


# ---- 1. the data classes, few streams (3 x 17 queries) and many (12 x 11 = 132 >= 128 queries) ----
@pytest.mark.parametrize("name", R.CLASSES)
def test_few_streams(eng, cases, name):
    run_case(eng, cases[name][0], FEW)


@pytest.mark.parametrize("name", R.CLASSES)
def test_many_streams(eng, cases, name):
    res = run_case(eng, cases[name][1], MANY)
    assert bool(res["gemm"]["overflow"].all()) == (name == "offset_dim")          # (the prediction itself is asserted in check)


def test_truncated_list_second_pass(eng):
    # eight near-duplicates of one query in ONE thread's stride set of knn_select_blend_kernel: exactly k, so the thread's K-th entry is inside the margin
    case = R.truncated_case()
    res = run_case(eng, case, MANY)
    b, j = case.meta["where"]
    frames = np.flatnonzero(R.col_map(case.skip_head, case.R, case.T) - case.first_raw == j)
    assert set(res["gemm"]["idx"][b, frames].ravel().tolist()) == set(case.meta["rows"]) and not res["gemm"]["overflow"].any()


def test_margin_constant_decides_the_overflow_words(eng):
    # knn_ref's `straddle` offset: at K = 8 more than 2 KNN_CAND candidates with the margin as it is, fewer than 0.6 KNN_CAND with half (test_knn_k_ref.py)
    res = run_case(eng, KR.make_case("straddle", dim=48, n=4099, streams=12, nq=11, seed=100), MANY)
    assert res["gemm"]["overflow"].tolist() == [1] * 12


# ---- 2. edge shapes on the one-launch form and the definition ----
TWO = ("fused", "exhaustive")


@pytest.mark.parametrize("n", [8, 9])
def test_index_of_k_rows(eng, n):
    # n = 8: every row is a hit of every query
    case = R.make_case("gaussian", dim=48, n=n, streams=3, nq=17, seed=1300 + n)
    res = run_case(eng, case, TWO)
    if n == 8:
        assert all(sorted(r) == list(range(8)) for r in res["fused"]["idx"].reshape(-1, 8).tolist())


@pytest.mark.parametrize("nq", [1, 33])
def test_query_groups(eng, nq):
    run_case(eng, R.make_case("near_runs12", dim=48, n=1023, streams=3, nq=nq, seed=1400 + nq), TWO)


def test_dim_16(eng):
    for name in ("gaussian", "near_runs12", "far_dups10_5"):
        run_case(eng, R.make_case(name, dim=16, n=1023, streams=3, nq=17, seed=1500), TWO)


def test_definition_path_at_dim_44(eng):
    for name in ("gaussian", "near_runs12", "far_dups10_5"):
        run_case(eng, R.make_case(name, dim=44, n=1023, streams=3, nq=17, seed=1600), ("planner",), expect={"planner": "knn_exhaustive"})


def test_forced_grids(eng):
    # RVC_KNN_WGS = 64 at one stream: G = 64 workgroups over 325 tiles (five or six each); RVC_KNN_WGS = 4096: G = ceil(n / 64), one tile in four idle
    for wgs, G in ((64, 64), (4096, 82)):
        for name in ("gaussian", "near_runs12"):
            case = R.make_case(name, dim=48, n=5193, streams=1, nq=17, seed=1700, wgs=wgs)
            assert R.fused_grid(case.n, 1, wgs) == G == min(G, (case.n + 63) // 64)
            run_case(eng, case, ("fused", "fallback"), wgs=wgs)


@pytest.mark.parametrize("rate", [0.0, 1.0])
def test_rate_edges(eng, rate):
    # rate 0: phone = the raw rows, bitwise (asserted in check)
    run_case(eng, R.make_case("far_dups10_5", dim=48, n=1023, streams=3, nq=17, seed=1800), TWO, rate=rate)


def test_graph_replay(eng, cases):
    case = cases["near_runs12"][0]
    eager = run_case(eng, case, ("fused", "exhaustive"))
    assert eng.set_k(8) == 0
    cv = R.to_cv(case.q, case.T + 5)
    for p in ("fused", "exhaustive"):
        g = eng.run(cv, case.skip_head, case.R, case.T, path=p, wgs=768, reps=3, graph=1)
        for key in ("idx", "dist", "phone"):
            assert same_bits(g[key].view(np.float32), eager[p][key].view(np.float32)), (p, key)


# ---- 2b. the file converter's default window ----
@pytest.mark.parametrize("streams", [1, 3])
def test_converter_window(eng, streams):
    """k = 14: T = 223 ContentVec columns, skip_head 48, 351 frames -- 176 raw frames, eleven query groups of the one-launch form; 1 and 3 streams, every path
    (the aid's path 0 and its fallback list, path 1, among them), eager and replayed.  Frame r reads column (48 + r) / 2: frame 350 reads column 199, and
    the duplicate runs of the index sit on columns 24 and 199, the first and the last one read"""
    case = R.make_case("near_runs12", dim=48, n=1023, streams=streams, nq=176, seed=1400 + streams)
    assert (case.skip_head, case.R, case.T) == (48, 351, 223)
    eager = run_case(eng, case, MANY)
    assert eng.set_k(8) == 0
    cv = R.to_cv(case.q, case.T + 5)
    for p in ("fused", "fallback"):
        g = eng.run(cv, case.skip_head, case.R, case.T, path=p, wgs=768, reps=2, graph=1)
        for key in ("idx", "dist", "phone"):
            assert same_bits(g[key].view(np.float32), eager[p][key].view(np.float32)), (p, key)
        raw = eng.run(cv, case.skip_head, case.R, case.T, rate=0.0, path=p, wgs=768)          # rate 0: the gather alone
        cols = R.col_map(case.skip_head, case.R, case.T)
        assert cols[350] == 199 and same_bits(raw["phone"][:, :, 350], cv[:, :, 199])
        assert same_bits(np.ascontiguousarray(raw["phone"][:, :, :case.R]), np.ascontiguousarray(cv[:, :, cols]))
    b = streams - 1                                                                              # the runs planted on the last column read: frame 350's hits
    rows = {r for pb, t, row, ln in case.meta["places"] if (pb, t) == (b, 199) for r in range(row, row + ln)}
    assert len(rows) >= 12 and set(eager["fused"]["idx"][b, 350].tolist()) <= rows


# ---- 3. the API ----
def test_api(eng):
    fresh = Engine()
    try:
        assert fresh.k() == 4                                                   # a fresh engine
        for bad in (5, 0, -8, 16):
            assert fresh.set_k(bad) == RVC_SHAPE and fresh.h.last_error() and fresh.k() == 4
        assert fresh.set_k(8) == 0 and fresh.k() == 8                           # before an index is loaded
        idx7 = KR.gaussian(1, 7, 48, 1, 4)[0]
        fresh.load(idx7, rc=RVC_SHAPE)                                          # seven rows at k = 8
        assert "at least 8" in fresh.h.last_error()
        big = R.make_case("gaussian", dim=48, n=257, streams=1, nq=17, seed=1900)
        fresh.load(big.index)
        assert fresh.k() == 8                                                   # the setting survives a load
        cv = R.to_cv(big.q, big.T)
        before = fresh.run(cv, big.skip_head, big.R, big.T, path="fused")
        fresh.load(idx7, rc=RVC_SHAPE)                                          # refused: the engine keeps the index it had
        after = fresh.run(cv, big.skip_head, big.R, big.T, path="fused")
        assert same_bits(after["dist"], before["dist"]) and np.array_equal(after["idx"], before["idx"])
        assert fresh.set_k(4) == 0
        fresh.load(idx7)                                                        # seven rows are enough at k = 4
        assert fresh.set_k(8) == RVC_SHAPE and fresh.k() == 4
        assert fresh.set_k(4) == 0
    finally:
        fresh.close()
