"""The IVF-probed retrieval (obs_rvc_amd/csrc/ivf.hip.h) restated in numpy float64 on top of knn_ref, and the structures and cases
tests/test_ivf_ref.py proves fair on the CPU before tests/test_gpu_ivf.py runs them.

Definition.  D_j = d(x, c_j) to the nlist centroids; the probe set is the nprobe lists with the smallest (D_j, j); the hits are the four rows with the
smallest (d(x, y_i), i) among the rows of the probed lists.  A non-finite distance is no candidate, coarse or fine (the flat search's rule).  Fewer than four
candidates: the missing hits are idx -1 / dist +inf and the frame is not blended (it keeps the raw feature x).  Blend, column map and tolerances: knn_ref."""
from __future__ import annotations

import numpy as np

import knn_ref as KR

K = KR.K
NLIST = 37


def coarse(centroids, q):
    """[nq][nlist] float64 squared distances to the centroids"""
    return KR.d64(centroids, q)


def probe_sets(centroids, q, nprobe):
    """per query: the probed lists, nearest first (stable sort by (D, j), non-finite distances dropped), and the sorted coarse distances"""
    with np.errstate(invalid="ignore", over="ignore"):
        D = coarse(centroids, q)
    out = []
    for row in D:
        order = np.argsort(np.where(np.isfinite(row), row, np.inf), kind="stable")
        order = order[np.isfinite(row[order])]
        out.append(order[:nprobe])
    return out, D


def search(index, centroids, assign, q, nprobe):
    """-> idx [nq][4] (int64, -1 = no hit), dist [nq][4] (float64, +inf = no hit), the probe set per query, the scanned rows per query (ascending)"""
    probes, _ = probe_sets(centroids, q, nprobe)
    idx = np.full((len(q), K), -1, np.int64)
    dist = np.full((len(q), K), np.inf)
    scanned = []
    for j, lists in enumerate(probes):
        rows = np.flatnonzero(np.isin(assign, lists))            # union of the lists, ascending row number
        scanned.append(rows)
        if rows.size == 0:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            d = KR.d64(np.asarray(index)[rows], q[j:j + 1])[0]
        ok = np.isfinite(d)
        rows, d = rows[ok], d[ok]
        order = np.argsort(d, kind="stable")[:K]                 # rows ascending + stable = ties by row number
        idx[j, :order.size] = rows[order]
        dist[j, :order.size] = d[order]
    return idx, dist, probes, scanned


def blend_or_keep(index, x, idx, rate):
    """the blended feature of knn_ref.blend, or x itself when a hit is missing; and the element-wise magnitude"""
    if (np.asarray(idx) < 0).any():
        x64 = np.asarray(x, np.float64)
        return x64, np.abs(x64)
    return KR.blend(index, x, idx, rate)


def make_structure(case, nlist=NLIST, seed=77):
    """centroids = a seeded sample of nlist index rows + 0.05 N(0, 1); assign = the float64 argmin (ties: the lower list)"""
    g = KR.rng(seed)
    rows = np.sort(g.choice(case.n, nlist, replace=False))
    cent = (case.index[rows] + np.float32(0.05) * g.standard_normal((nlist, case.dim), dtype=np.float32)).astype(np.float32)
    assign = np.argmin(KR.d64(cent, case.index), axis=1).astype(np.int32)
    return np.ascontiguousarray(cent), assign


# ---- the shared cases of test 1: (class, n, streams, nq, nprobe, seed); dim 48, nlist 37.  Every value of every axis at least once; nq 33 with 12 streams once.
# Seeds: 2100, except where float64 finds a query within 4 gamma of a tie at that seed (offset3 x 12 streams: one of 132 queries), then the next hundred ----
CASES = [
    ("gaussian", 1023, 1, 1, 1, 2100),
    ("gaussian", 4099, 3, 17, 3, 2100),
    ("offset3", 1023, 12, 11, 1, 2200),
    ("offset3", 4099, 1, 17, 37, 2100),
    ("near_runs", 4099, 3, 17, 37, 2100),
    ("near_runs", 1023, 3, 11, 3, 2100),
    ("far_dups", 1023, 3, 33, 3, 2100),
    ("norm_spread", 1023, 1, 11, 3, 2100),
    ("gaussian", 1023, 12, 33, 37, 2100),
]
# classes on which exact idx equality is demanded: tests/test_ivf_ref.py asserts that NO query of their cases is ambiguous (coarse and fine gaps above 4 gamma)
CLEARED = ("gaussian", "offset3", "norm_spread")


def build_case(name, n, streams, nq, seed=2100):
    case = KR.make_case(name, dim=48, n=n, streams=streams, nq=nq, seed=seed + n + nq)
    cent, assign = make_structure(case)
    return case, cent, assign


def ambiguous_queries(index, cent, assign, q, nprobe):
    """how many of the queries q [nq][dim] have a coarse gap D_(nprobe+1) - D_(nprobe), a fine 4th/5th gap or a gap inside the first four within 4 gamma of the
    distance: where this is 0, fp32 rounding cannot change the probe set or the hits, and exact idx equality is a legitimate demand"""
    g4 = 4 * KR.gamma(np.asarray(index).shape[1])
    Ds = np.sort(coarse(cent, q), axis=1)
    _, _, _, scanned = search(index, cent, assign, q, nprobe)
    bad = 0
    for j in range(len(q)):
        amb = nprobe < Ds.shape[1] and not (Ds[j, nprobe] - Ds[j, nprobe - 1] > g4 * Ds[j, nprobe])
        d = np.sort(KR.d64(np.asarray(index)[scanned[j]], q[j:j + 1])[0])
        if d.size > K:
            amb = amb or not (d[K] - d[K - 1] > g4 * d[K])
        amb = amb or bool(np.any(~(np.diff(d[:K]) > g4 * d[1:K])))        # (the order inside the first four decides idx too)
        bad += bool(amb)
    return bad


def ambiguous(case, cent, assign, nprobe):
    """ambiguous_queries over every stream of a case"""
    return sum(ambiguous_queries(case.index, cent, assign, case.used(b), nprobe) for b in range(case.streams))


# ---- the planted structure of test 3 ----
class Planted:
    """gaussian case, 3 streams, 17 queries each, n = 1023, nlist = 37, then by hand:
      dup    lists 4 and 5 share one bit-identical centroid next to query (0, +2); its rows alternate between the two lists and the nearest row of all sits in list 5;
      empty  list 9's centroid is query (1, +3) itself and the list holds no row;
      three  list 12's centroid is query (2, +5) itself and the list holds exactly three rows;
      long   list 20's centroid is query (0, +7) itself; the list is rows 700 .. 999 and the nearest of them, a planted near-copy of the query, is row 999."""

    def __init__(self, seed=2500):
        case = KR.make_case("gaussian", dim=48, n=1023, streams=3, nq=17, seed=seed)
        cent, assign = make_structure(case)
        g = KR.rng(seed + 1)
        f0 = case.first_raw
        self.q_dup, self.q_empty, self.q_three, self.q_long = (0, f0 + 2), (1, f0 + 3), (2, f0 + 5), (0, f0 + 7)
        x = lambda bt: case.q[bt[0], bt[1]]
        # long list first (it moves the most rows)
        cent[20] = x(self.q_long)
        assign[assign == 20] = 21
        assign[700:1000] = 20
        case.index[999] = x(self.q_long) + np.float32(1e-3) * g.standard_normal(case.dim, dtype=np.float32)
        # duplicate centroid
        cent[4] = x(self.q_dup) + np.float32(0.01) * g.standard_normal(case.dim, dtype=np.float32)
        cent[5] = cent[4]
        free = np.flatnonzero((assign != 20))
        near = free[np.argsort(KR.d64(case.index[free], x(self.q_dup)[None])[0], kind="stable")[:24]]
        assign[(assign == 4) | (assign == 5)] = 6
        assign[near[0::2]] = 5                                    # the nearest row of all goes to the HIGHER list ...
        case.index[near[0]] = x(self.q_dup) + np.float32(1e-3) * g.standard_normal(case.dim, dtype=np.float32)       # ... and is a near-copy of the query
        assign[near[1::2]] = 4
        # empty list
        cent[9] = x(self.q_empty)
        assign[assign == 9] = 10
        # three rows
        cent[12] = x(self.q_three)
        assign[assign == 12] = 13
        three = np.flatnonzero((assign != 20) & (assign != 4) & (assign != 5))[[11, 301, 611]]
        assign[three] = 12
        self.three_rows = np.sort(three)
        self.case, self.cent, self.assign = case, np.ascontiguousarray(cent), np.ascontiguousarray(assign.astype(np.int32))

    def frames(self, bt):
        """the sliced frames that read raw frame t of stream b"""
        cols = KR.col_map(self.case.skip_head, self.case.R, self.case.T)
        return bt[0], np.flatnonzero(cols == bt[1])
