"""The flat-L2 retrieval (obs_rvc_amd/csrc/knn.hip.h, retrieval.hip) restated in numpy float64, the kernels' candidate rule
restated from float64 values, and the deterministic data classes of tests/test_gpu_knn.py.  Checked on the CPU by tests/test_knn_ref.py.

Definition.  d[q, i] = sum_c (x_q[c] - y_i[c])^2; the hits of a query are the four smallest by (d, i); the blended feature is
rate * sum_k w^_k y_{i_k} + (1 - rate) * x with w_k = 1 / d_k^2 and w^_k = w_k / sum w; sliced frame r of a call reads the raw frame
s = min((skip_head + r) // 2, T - 1).

Tolerances (derivations, not measurements; u = 2^-24).
  gamma = (dim + 2) u.  The fp32 definition is a dim-term sequential fmaf chain over rounded differences: each (x - y) carries one rounding, so each square
  (1 + u)^2, and the chain adds one rounding per term: (dim + 2) u to first order, all terms being non-negative.  Hence |dist[k] - D[k]| <= gamma D[k] for the
  sorted float64 distances D: an order statistic moves by no more than the largest per-element perturbation, so ties need no special case.  The float64 distance
  of the k-th returned INDEX may sit on the other side of a near-tie: 2 gamma D[k].
  blend: |phone - ref| <= (4 gamma + 16 u) max(|x|, |y_{i_k}|) per element.  Each w_k carries 2 gamma (an inverse square of a distance good to gamma), the
  normalisation doubles it; the convex combination, its four fmaf, the product (1 - rate) x and the last fmaf stay below 16 u of the largest operand.

The candidate rule (the kernels' own margin, quoted from the source):
  knn.hip.h:515 and :843   const float margin = 2e-3f * (fabsf(a4 + s_xn) + s_xn + 1e-3f);
with approx_i = |y_i|^2 - 2 x . y_i, a4 its 4th smallest value and s_xn = |x|^2; the candidates are { i : approx_i <= a4 + margin }.  `inside` evaluates it in
float64; the predictions built on it are only used where the count is far from a threshold (see test_knn_ref.py), so the kernels' fp32 rounding of approx
cannot change them."""
from __future__ import annotations

import numpy as np

K = 4
KNN_CAND = 512                 # knn.hip.h:749
KNN_FUSED_MAXG = 1024          # knn.hip.h:234
U = 2.0 ** -24


def gamma(dim):
    return (dim + 2) * U


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ---- the definition ----
def d64(index, q):
    """[nq][n] float64 squared distances of the fp32 inputs"""
    y = np.asarray(index, np.float64)
    out = np.empty((len(q), len(y)))
    for j, x in enumerate(np.asarray(q, np.float64)):
        out[j] = np.einsum("ij,ij->i", y - x, y - x)
    return out


def topk(d):
    """indices [nq][4] of the four smallest by (d, index), and their distances"""
    order = np.argsort(d, axis=1, kind="stable")[:, :K]
    return order, np.take_along_axis(d, order, axis=1)


def col_map(skip_head, R, T):
    return np.minimum((skip_head + np.arange(R)) // 2, T - 1)


def blend(index, x, idx, rate):
    """x [dim], idx [4] -> (the blended feature in float64, the element-wise magnitude max(|x|, |y_{i_k}|))"""
    y = np.asarray(index, np.float64)[idx]
    x = np.asarray(x, np.float64)
    d = np.einsum("ij,ij->i", y - x, y - x)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / (d * d)
        w = w / w.sum()
        ref = rate * (w[:, None] * y).sum(0) + (1.0 - rate) * x
    return ref, np.maximum(np.abs(x), np.abs(y).max(0))


def blend_bound(dim):
    return 4 * gamma(dim) + 16 * U


# ---- the candidate rule, from float64 ----
def inside(index, q, c=2e-3):
    """[nq][n] bool: approx_i <= a4 + margin (the formula in the module docstring; c = its constant, so that a proof can show what half of it would give)"""
    y, x = np.asarray(index, np.float64), np.asarray(q, np.float64)
    approx = (y * y).sum(1)[None, :] - 2.0 * x @ y.T
    a4 = np.sort(approx, axis=1)[:, K - 1]
    xn = (x * x).sum(1)
    margin = c * (np.abs(a4 + xn) + xn + 1e-3)
    return approx <= (a4 + margin)[:, None]


def candidates(index, q, c=2e-3):
    """per query: how many vectors the many-stream path collects"""
    return inside(index, q, c).sum(1)


def fused_grid(n, streams, wgs):
    """workgroups per stream of the one-launch form (retrieval.hip:44); wgs = the hook RVC_KNN_WGS (3 x CUs without it)"""
    return min((n + 63) // 64, max(wgs // streams, 64), KNN_FUSED_MAXG)


def per_workgroup(mask, G):
    """[nq][G]: vectors inside the margin per workgroup of the one-launch form (tiles of 16 vectors: blockIdx.x, + G, ...)"""
    n = mask.shape[1]
    wg = (np.arange(n) // 16) % G
    return np.stack([np.bincount(wg[m], minlength=G) for m in mask])


def per_thread(mask):
    """[nq][1024]: vectors inside the margin per thread of knn_select_blend_kernel in its visiting order (knn.hip.h:796-810): vectors of four while n % 4 == 0
    (thread = (i // 4) % 1024), one by one otherwise (thread = i % 1024)"""
    n = mask.shape[1]
    i = np.arange(n)
    th = (i // 4) % 1024 if n % 4 == 0 else i % 1024
    return np.stack([np.bincount(th[m], minlength=1024) for m in mask])


# ---- data classes: an index [n][dim] and queries [streams][T][dim] (one per raw frame), all fp32, seeded PCG64 as weights.make_index ----
def gaussian(seed, n, dim, streams, T, mu=0.0):
    """class 1 (mu = 0) and class 2 (a common offset: mu = 3, or a vector drawn per dimension): mu + 0.35 N"""
    g = rng(seed)
    mu = np.asarray(mu, np.float32)
    index = g.standard_normal((n, dim), dtype=np.float32) * np.float32(0.35) + mu
    q = g.standard_normal((streams, T, dim), dtype=np.float32) * np.float32(0.35) + mu
    return index, q


def offset_per_dim(seed, dim, scale=16.0):
    """mu drawn per dimension, N(0, scale^2).  scale = 16: the margin 2e-3 (|x|^2 + d^2) ~ 2e-3 dim scale^2 is then several times the spread
    0.245 sqrt(2 dim) of the squared distances for every dim >= 16, so (nearly) every vector of the index is a candidate"""
    return (rng(seed).standard_normal(dim) * scale).astype(np.float32)


def near_duplicate_runs(seed, index, q, placements):
    """class 4: for (stream, raw frame, first row, length) a run of vectors within 1e-4 relative of that query; index is changed in place"""
    g = rng(seed)
    dim = index.shape[1]
    for b, t, row, ln in placements:
        x = q[b, t]
        step = np.float32(1e-4) * np.float32(np.linalg.norm(x) / np.sqrt(dim))
        index[row:row + ln] = x + step * g.standard_normal((ln, dim), dtype=np.float32)
    return index


def far_duplicates(seed, index, q, b, t, rows):
    """class 5: one vector near query (b, t), copied bit for bit to `rows`"""
    v = q[b, t] + np.float32(0.01) * rng(seed).standard_normal(index.shape[1], dtype=np.float32)
    index[np.asarray(rows)] = v
    return index


def norm_spread(seed, n, dim, streams, T, outlier):
    """class 6: rows scaled log-uniformly from 1e-3 to 1e2, one row of norm 1e3, queries of norm ~1e-4"""
    g = rng(seed)
    index = g.standard_normal((n, dim), dtype=np.float32) * np.float32(0.35)
    index *= (10.0 ** g.uniform(-3, 2, size=(n, 1))).astype(np.float32)
    index[outlier] *= np.float32(1e3 / np.linalg.norm(index[outlier]))
    q = g.standard_normal((streams, T, dim), dtype=np.float32)
    q *= np.float32(1e-4) / np.linalg.norm(q, axis=2, keepdims=True).astype(np.float32)
    return index, q


def truncated(seed, n, dim, streams, T, b, t):
    """class 7: Gaussian data with near-duplicates of query (b, t) in ONE thread's stride set of knn_select_blend_kernel: rows 4 g .. 4 g + 3 for g = 7 and
    g = 7 + 1024 (n % 4 == 0: eight values), rows 0, 1024, ... , 4096 (otherwise: five)"""
    index, q = gaussian(seed, n, dim, streams, T)
    rows = [28, 29, 30, 31, 4124, 4125, 4126, 4127] if n % 4 == 0 else [0, 1024, 2048, 3072, 4096]
    assert max(rows) < n
    for r in rows:
        near_duplicate_runs(seed + 1 + r, index, q, [(b, t, r, 1)])
    return index, q, rows


def to_cv(q, cv_ld, pad_value=7.0e3):
    """queries [streams][T][dim] -> the ContentVec output [streams][dim][cv_ld], channel-major; the padding columns hold a value no query has"""
    B, T, dim = q.shape
    cv = np.full((B, dim, cv_ld), pad_value, np.float32)
    cv[:, :, :T] = q.transpose(0, 2, 1)
    return cv


# ---- the shared cases: what tests/test_knn_ref.py proves on the CPU is what tests/test_gpu_knn.py runs ----
# (skip_head, R, T) by the number of unique raw frames nq = the queries of a stream
GEOMS = {
    1: (3, 1, 4),           # R = 1, odd skip_head
    11: (2, 21, 12),        # the tiny preset's call
    15: (1, 29, 20),        # odd skip_head: the first raw frame feeds one sliced frame only
    16: (0, 32, 16),
    17: (5, 34, 19),        # skip_head + R = 2 T + 1: frames 36, 37 and 38 all read the last column (the clamp bites for frame 38)
    33: (0, 66, 33),        # three query groups of the one-launch form: 16, 16, 1
    176: (48, 351, 223),    # the file converter's default window (k = 14): frames 0 .. 350 read ContentVec columns 24 .. 199, eleven query groups
}


def raw_range(skip_head, R, T):
    cols = col_map(skip_head, R, T)
    return int(cols[0]), int(cols[-1] - cols[0] + 1)


class Case:
    def __init__(self, name, index, q, nq, **meta):
        self.name, self.index, self.q, self.nq, self.meta = name, np.ascontiguousarray(index, np.float32), np.ascontiguousarray(q, np.float32), nq, meta
        self.skip_head, self.R, self.T = GEOMS[nq]
        self.first_raw, n_raw = raw_range(self.skip_head, self.R, self.T)
        assert n_raw == nq and q.shape[1] == self.T
        self.streams, self.dim, self.n = q.shape[0], index.shape[1], index.shape[0]

    def used(self, b):
        """the queries of stream b the launch reads: [nq][dim]"""
        return self.q[b, self.first_raw:self.first_raw + self.nq]


def make_case(name, dim=48, n=1023, streams=3, nq=17, seed=100, wgs=768):
    """one data class at one shape.  Rows the special classes place are spread over tiles, workgroups (G = the one-launch grid the caller states) and the tail"""
    T = GEOMS[nq][2]
    f0 = raw_range(*GEOMS[nq])[0]
    last = f0 + nq - 1
    if name == "gaussian":
        index, q = gaussian(seed, n, dim, streams, T)
        return Case(name, index, q, nq)
    if name == "offset3":
        index, q = gaussian(seed, n, dim, streams, T, mu=3.0)
        return Case(name, index, q, nq)
    if name == "offset_dim":
        index, q = gaussian(seed, n, dim, streams, T, mu=offset_per_dim(seed + 1, dim))
        return Case(name, index, q, nq)
    if name == "mixed":
        # one index with a per-dimension offset; streams 0, 2, 5 ask with queries of the same class (every vector is a candidate), the others with zero-mean ones
        index, q = gaussian(seed, n, dim, streams, T, mu=offset_per_dim(seed + 1, dim))
        plain = gaussian(seed + 2, 4, dim, streams, T)[1]
        hot = [b for b in (0, 2, 5) if b < streams]
        for b in range(streams):
            if b not in hot:
                q[b] = plain[b]
        return Case(name, index, q, nq, hot=hot)
    if name in ("near_runs", "offset_dups"):
        # runs of 8 within 1e-4 of a query: inside one 16-vector tile, across a tile boundary, across the wrap of the workgroups' slices (tile G - 1 | tile G), and
        # in the last, partial tile.  offset_dups: the same runs and two sets of far duplicates planted into an index with a per-dimension offset, where every
        # vector is a candidate: the many-stream path reaches them through its overflow fallback only
        index, q = gaussian(seed, n, dim, streams, T, mu=offset_per_dim(seed + 1, dim) if name == "offset_dups" else 0.0)
        G = fused_grid(n, streams, wgs)
        places = [(0, f0, 32, 8), (streams - 1, last, 44, 8)]
        if 16 * G - 3 >= 64 and n > 16 * G + 8 + 8:
            places.append((0, last, 16 * G - 3, 8))
        if n % 16 >= 7 and n - 7 >= (places[-1][2] + 8):
            places.append((streams - 1, f0, n - 7, 7))
        taken = np.zeros(n, int)
        for _, _, row, ln in places:
            taken[row:row + ln] += 1
        assert taken.max() == 1, "near-duplicate runs overlap"
        near_duplicate_runs(seed + 3, index, q, places)
        meta = dict(places=places)
        if name == "offset_dups":
            free = np.flatnonzero(taken == 0)
            rows = sorted(set(free[[5, len(free) // 3, len(free) // 2, -2]].tolist()))
            far_duplicates(seed + 4, index, q, 1 % streams, f0 + nq // 2, rows + [int(free[-1])])
            meta["rows"] = rows
        return Case(name, index, q, nq, **meta)
    if name == "straddle":
        # a per-dimension offset of scale 5.5 at dim 48, n = 4099: the margin as it is collects more than 1 000 candidates for some query of every stream, half of
        # it fewer than 300 (test_knn_ref.py): the overflow words are what a changed margin constant would flip
        index, q = gaussian(seed, n, dim, streams, T, mu=offset_per_dim(seed + 1, dim, 5.5))
        return Case(name, index, q, nq)
    if name == "far_dups":
        index, q = gaussian(seed, n, dim, streams, T)
        rows = sorted({3, 19, n // 3, n // 2 + 1, (n // 16) * 16 - 1, n - 1})
        far_duplicates(seed + 4, index, q, 0, f0, rows)
        rows2 = sorted({5, n // 4, n - 2})                                # fewer than four copies: the fourth hit is an ordinary vector
        far_duplicates(seed + 5, index, q, streams - 1, last, rows2)
        return Case(name, index, q, nq, rows=rows, rows2=rows2)
    if name == "norm_spread":
        index, q = norm_spread(seed, n, dim, streams, T, outlier=n // 2)
        return Case(name, index, q, nq, outlier=n // 2)
    if name == "truncated":
        index, q, rows = truncated(seed, n, dim, streams, T, 1, f0 + 1)
        return Case(name, index, q, nq, rows=rows, where=(1, 1))
    raise KeyError(name)
