"""The flat-L2 retrieval with K neighbours as an argument (K = 4, or upstream's 8: rvc_set_index_k), in numpy float64: tests/knn_ref.py's
definition, candidate rule and data classes with K for 4.  The data classes, GEOMS and Case are knn_ref's own, by import.  Checked on the CPU by
tests/test_knn_k_ref.py; run on the GPU by tests/test_gpu_knn_k8.py and tests/test_gpu_ivf_k8.py.

Definition.  d[q, i] = sum_c (x_q[c] - y_i[c])^2; the hits of a query are the K smallest by (d, i); the blended feature is
rate * sum_k w^_k y_{i_k} + (1 - rate) * x, w_k = 1 / d_k^2, w^_k = w_k / sum_{k < K} w_k.  In fp32: acc = fmaf(w^_k, y_k, acc) in ascending k, then
fmaf(rate, acc, (1 - rate) x).

Tolerances (u = 2^-24).
  Distances: knn_ref's, which do not depend on K.  gamma = (dim + 2) u bounds one distance relative to its float64 value; an order statistic moves by no more
  than the largest per-element perturbation, so |dist[k] - D[k]| <= gamma D[k] for every k < K, and the float64 distance of the k-th returned index may sit on
  the other side of a near-tie: 2 gamma D[k].
  Blend: |phone - ref| <= (4 gamma + (12 + K) u) max(|x|, |y_{i_k}|) per element.
    * The weight part does not depend on K.  w_k = (1 / d_k)^2 of a distance good to gamma carries 2 gamma; the normalising sum of non-negative terms carries
      the same 2 gamma relative error whatever the number of terms, and the division by it doubles the weight's: 4 gamma.
    * knn_ref.py bounds everything else -- the O(u) roundings of the weights and their sum, the convex combination's four fmaf, the product (1 - rate) x and
      the last fmaf -- by 16 u of the largest operand at K = 4: 4 u for the four fmaf of the combination (one rounding each, every partial sum bounded by
      max |y| because the weights are non-negative and sum to 1), 12 u for the rest, which does not grow with the fmaf count.
    * Each further fmaf of the convex combination adds one rounding: (12 + K) u.  At K = 4 this is knn_ref.blend_bound exactly; at K = 8 it is 20 u.
  The bound is derived, not measured; the GPU tests print the largest ratio they see before they assert.

The candidate rule is knn.hip.h's margin with a_K, the K-th smallest approximation, for a4:
    margin = 2e-3f * (fabsf(aK + s_xn) + s_xn + 1e-3f),    candidates = { i : approx_i <= a_K + margin }.
On the one-launch form a workgroup whose K-th smallest approximation is inside the margin is "flagged" (all of its vectors are re-ranked)."""
from __future__ import annotations

import numpy as np

import knn_ref as KR
from knn_ref import GEOMS, Case, U, gamma, d64, col_map, to_cv, fused_grid, per_workgroup, KNN_CAND   # noqa: F401  (re-exported)


def topk(d, K):
    """indices [nq][K] of the K smallest by (d, index), and their distances"""
    order = np.argsort(d, axis=1, kind="stable")[:, :K]
    return order, np.take_along_axis(d, order, axis=1)


def blend(index, x, idx, rate):
    """x [dim], idx [K] -> (the blended feature in float64, max(|x|, |y_{i_k}|)); knn_ref.blend does not depend on the number of hits"""
    return KR.blend(index, x, idx, rate)


def blend_bound(dim, K):
    return 4 * gamma(dim) + (12 + K) * U


def approx64(index, q):
    y, x = np.asarray(index, np.float64), np.asarray(q, np.float64)
    return (y * y).sum(1)[None, :] - 2.0 * x @ y.T


def inside(index, q, K, c=2e-3):
    """[nq][n] bool: approx_i <= a_K + margin"""
    x = np.asarray(q, np.float64)
    approx = approx64(index, q)
    aK = np.sort(approx, axis=1)[:, K - 1]
    xn = (x * x).sum(1)
    margin = c * (np.abs(aK + xn) + xn + 1e-3)
    return approx <= (aK + margin)[:, None]


def candidates(index, q, K, c=2e-3):
    """per query: how many vectors the many-stream path collects"""
    return inside(index, q, K, c).sum(1)


def flagged(index, q, G, K):
    """[nq][G] bool: workgroups of the one-launch form whose K-th smallest approximation is inside the margin (K or more of their vectors are)"""
    return per_workgroup(inside(index, q, K), G) >= K


def probed_topk(index, q, cent, assign, nprobe, K):
    """IVF: the float64 top-K over the rows of the nprobe nearest lists (by (D, list number)); fewer rows than K: -1 / +inf.  -> (idx [nq][K], dist [nq][K],
    rows probed [nq])"""
    D = d64(cent, q)
    lists = np.argsort(D, axis=1, kind="stable")[:, :nprobe]
    d = d64(index, q)
    idx, dist, cnt = np.full((len(q), K), -1, np.int64), np.full((len(q), K), np.inf), np.zeros(len(q), int)
    for j in range(len(q)):
        rows = np.flatnonzero(np.isin(assign, lists[j]))
        cnt[j] = len(rows)
        o = rows[np.argsort(d[j, rows], kind="stable")[:K]]
        idx[j, :len(o)] = o
        dist[j, :len(o)] = d[j, o]
    return idx, dist, cnt


# ---- data classes for K = 8: knn_ref's, with runs and copy counts around 8 instead of around 4 ----
RUN = 12                      # near-duplicate runs: more than k


def make_case(name, dim=48, n=1023, streams=3, nq=17, seed=100, wgs=768):
    T = GEOMS[nq][2]
    f0 = KR.raw_range(*GEOMS[nq])[0]
    last = f0 + nq - 1
    if name == "near_runs12":
        # runs of 12 within 1e-4 of a query: inside one 16-vector tile, across a tile boundary, across the wrap of the workgroups' slices, in the partial last tile
        index, q = KR.gaussian(seed, n, dim, streams, T)
        G = fused_grid(n, streams, wgs)
        places = [(0, f0, 33, RUN), (streams - 1, last, 58, RUN)]                  # rows 33..44 (tile 2), rows 58..69 (tiles 3 | 4)
        if 16 * G - 5 >= 80 and n > 16 * G + 8 + 12:
            places.append((0, last, 16 * G - 5, RUN))                              # tile G - 1 | tile G = workgroup G - 1 | workgroup 0
        tail = n % 16
        if tail >= 9 and n - tail >= places[-1][2] + RUN:
            places.append((streams - 1, f0, n - tail, tail))                       # the whole partial tile (9 .. 15 rows: more than k)
        taken = np.zeros(n, int)
        for _, _, row, ln in places:
            taken[row:row + ln] += 1
        assert taken.max() == 1, "near-duplicate runs overlap"
        KR.near_duplicate_runs(seed + 3, index, q, places)
        return Case(name, index, q, nq, places=places)
    if name == "far_dups10_5":
        index, q = KR.gaussian(seed, n, dim, streams, T)
        rows = sorted({3, 19, 20, n // 5, n // 3, n // 2 + 1, 2 * n // 3, (n // 16) * 16 - 1, n - 17, n - 1})
        assert len(rows) == 10
        KR.far_duplicates(seed + 4, index, q, 0, f0, rows)
        rows2 = sorted({5, n // 4, n // 2 - 7, n - 40, n - 2})                    # five copies, fewer than k: hits 6-8 are ordinary vectors
        assert len(rows2) == 5 and not set(rows) & set(rows2)
        KR.far_duplicates(seed + 5, index, q, streams - 1, last, rows2)
        return Case(name, index, q, nq, rows=rows, rows2=rows2)
    return KR.make_case(name, dim=dim, n=n, streams=streams, nq=nq, seed=seed, wgs=wgs)


def offset_case(scale, dim=48, n=1023, streams=3, nq=17, seed=100):
    T = GEOMS[nq][2]
    index, q = KR.gaussian(seed, n, dim, streams, T, mu=KR.offset_per_dim(seed + 1, dim, scale))
    return Case("offset%g" % scale, index, q, nq, scale=scale)


# the shapes of tests/test_gpu_knn_k8.py (the issue's): few streams 3 x 17 queries, many streams 12 x 11 = 132 >= 128 queries
FEW_SHAPE = dict(dim=48, n=1023, streams=3, nq=17)
MANY_SHAPE = dict(dim=48, n=1023, streams=12, nq=11)
CLASSES = ("gaussian", "offset_dim", "near_runs12", "far_dups10_5", "norm_spread")


def shared_cases():
    """name -> (few-stream case, many-stream case); `truncated` needs rows up to 4127, so it has its own n"""
    out = {}
    for name in CLASSES:
        out[name] = (make_case(name, seed=1100, **FEW_SHAPE), make_case(name, seed=1200, **MANY_SHAPE))
    return out


def truncated_case():
    return KR.make_case("truncated", dim=48, n=4160, streams=12, nq=11, seed=100)
