"""The k-means training of an IVF structure (obs_rvc_amd/csrc/kmeans.hip.h, retrieval.hip rvc_train_index_ivf) restated in numpy float64
on top of knn_ref / ivf_ref, and the cases tests/test_kmeans_ref.py proves fair on the CPU before tests/test_gpu_kmeans.py runs them.

Definition.  Inputs: the index y_0 .. y_{n-1} (fp32, dim wide), nlist, iters (the number of update steps), nlist distinct initial rows.  d is the engine's exact
distance, the fp32 sequential fmaf chain over (y[c] - c_j[c]) in ascending c (here: float64, see the tolerances).
  init     c_j = y_{init_rows[j]}, bit for bit.
  assign   assign[i] = the j with the smallest (d(y_i, c_j), j); a non-finite distance compares as +inf, so a row whose every distance is non-finite goes to
           list 0.  The step yields the objective J = sum_i d(y_i, c_assign[i]) (fp64 sum in ascending i) and moved = the rows whose list changed (first step: n).
  update   a non-empty list: c_j = fp32(sum of (double) y_i over the list's rows in ascending row number / count), rounded once; an empty list keeps its
           centroid bit for bit (no splitting, no reseeding).
  schedule assign, then (update, assign) up to iters times; training stops early after an assign step with moved == 0; iters_run = update steps done; the
           objectives of all iters_run + 1 assign steps are kept.  Training always ends with an assign step against the final centroids.
  default nlist (argument 0): min(floor(16 sqrt(n)), n // 39), clamped to [1, 65536] (upstream's rule for "IVF<n>,Flat").
  default init: the nlist rows with the smallest (h(seed, i), i), taken in ascending row number, h(seed, i) = m(i ^ m(seed + 0x9e3779b9)) in 32-bit arithmetic
           with the mixer m(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.

Tolerances (derivations; gamma = (dim + 2) 2^-24 as in knn_ref).  An fp32 chain distance is within gamma D of the float64 D, so the list a kernel picks has a
float64 distance within (1 + 2 gamma) of the float64 minimum, and equals the float64 argmin wherever the two smallest distances of the row differ by more than
4 gamma D (`ambiguous_rows` counts the others).  The objective, an fp64 sum of non-negative fp32 distances each within gamma, is within gamma relative (the
fp64 summation error, n 2^-53, is far below).  The mean is an fp64 sum of at most 2^29 fp32 values (relative error below n 2^-53 of sum |y|) rounded once: within
1 fp32 ulp of fp32(mean64) whatever the order of the sum."""
from __future__ import annotations

import numpy as np

import ivf_ref as IR
import knn_ref as KR

NLIST = IR.NLIST


# ---- defaults ----
def default_nlist(n):
    return int(min(max(min(int(np.floor(16.0 * np.sqrt(float(n)))), n // 39), 1), 65536))


def mix(x):
    x = np.asarray(x, np.uint64) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xffffffff)
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xffffffff)
    return x ^ (x >> np.uint64(16))


def h(seed, i):
    return mix(np.asarray(i, np.uint64) ^ mix((int(seed) + 0x9e3779b9) & 0xffffffff))


def seeded_rows(n, nlist, seed):
    key = (h(seed, np.arange(n)) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return np.sort(np.argsort(key, kind="stable")[:nlist]).astype(np.int32)


# ---- the two steps ----
def distances(index, cent):
    """[n][nlist] float64; non-finite entries as +inf (the comparison rule)"""
    with np.errstate(invalid="ignore", over="ignore"):
        D = KR.d64(cent, index)
    return np.where(np.isfinite(D), D, np.inf)


def assign_step(index, cent, prev=None):
    """-> assign (int32), the float64 distance of every row to its list, the objective, moved"""
    D = distances(index, cent)
    a = np.argmin(D, axis=1).astype(np.int32)                     # (the first minimum: the lower list on a tie)
    d = D[np.arange(len(a)), a]
    J = 0.0
    for v in d:                                                   # ascending i
        J += float(v)
    return a, d, J, len(a) if prev is None else int((a != prev).sum())


def means(index, assign, cent):
    """the update step over `assign`: [nlist][dim] fp32; an empty list keeps its row of `cent`"""
    out = np.array(cent, np.float32, copy=True)
    y = np.asarray(index, np.float64)
    for j in range(len(cent)):
        rows = np.flatnonzero(assign == j)
        if rows.size:
            acc = np.zeros(y.shape[1])
            for i in rows:                                        # ascending row number
                acc += y[i]
            out[j] = (acc / rows.size).astype(np.float32)
    return out


def train(index, nlist, iters, init_rows):
    """-> dict: cents[s] = the centroids assign step s ran against, assigns[s], dists[s], objective[s], moved[s] (s = 0 .. iters_run), iters_run"""
    index = np.asarray(index, np.float32)
    cent = np.ascontiguousarray(index[np.asarray(init_rows)])
    assert len(cent) == nlist
    a, d, J, moved = assign_step(index, cent)
    out = dict(cents=[cent], assigns=[a], dists=[d], objective=[J], moved=[moved], iters_run=0)
    while out["iters_run"] < iters and moved != 0:
        cent = means(index, a, cent)
        a, d, J, moved = assign_step(index, cent, a)
        out["cents"].append(cent); out["assigns"].append(a); out["dists"].append(d); out["objective"].append(J); out["moved"].append(moved)
        out["iters_run"] += 1
    return out


def ambiguous_rows(index, cent):
    """bool [n]: the two smallest distances of the row are within 4 gamma of each other: fp32 rounding may pick either list"""
    D = np.sort(distances(index, cent), axis=1)
    if D.shape[1] < 2:
        return np.zeros(len(D), bool)
    g4 = 4 * KR.gamma(np.asarray(index).shape[1])
    with np.errstate(invalid="ignore"):
        return ~(D[:, 1] - D[:, 0] > g4 * D[:, 1])


def chain32(index, cent):
    """[n][nlist] the fp32 sequential chain, emulated: each link is computed in float64 (the product of two fp32 differences is exact there) and rounded to
    fp32 -- the device's fmaf up to a double rounding of the sum, which the CPU checks that use this do not depend on"""
    y, c = np.asarray(index, np.float32), np.asarray(cent, np.float32)
    acc = np.zeros((len(y), len(c)), np.float32)
    for k in range(y.shape[1]):
        df = (y[:, k, None] - c[None, :, k]).astype(np.float64)
        acc = (df * df + acc.astype(np.float64)).astype(np.float32)
    return acc


# ---- cases ----
SEED = 3100


def init37(n, seed=SEED, nlist=NLIST):
    return np.sort(KR.rng(seed + 5).choice(n, nlist, replace=False)).astype(np.int32)


def case_index(name, n, dim=48, seed=SEED):
    return KR.make_case(name, dim=dim, n=n, streams=1, nq=1, seed=seed).index


def blobs(n=1023, dim=48, nlist=NLIST, seed=SEED):
    """37 separated clusters: mu_b = 4 N(0, 1), row i = mu_{i mod 37} + 0.3 N(0, 1)"""
    g = KR.rng(seed)
    mu = np.float32(4.0) * g.standard_normal((nlist, dim), dtype=np.float32)
    return np.ascontiguousarray(mu[np.arange(n) % nlist] + np.float32(0.3) * g.standard_normal((n, dim), dtype=np.float32))


# trajectory cases: name -> (index, init rows).  test_kmeans_ref.py asserts that no row is ambiguous at any assign step of 6 update steps (seed 3100 passes for all
# three: no seed had to be moved)
def trajectory_case(name):
    if name == "blobs":
        return blobs(), np.arange(NLIST, dtype=np.int32)
    index = case_index(name, 1023)
    return index, init37(1023)


TRAJECTORY = ("gaussian", "offset3", "blobs")
TRAJ_ITERS = 6


def blobs_random_init():
    """the blobs with a random init: some blobs get no initial row, some two -- lists end up empty (test_kmeans_ref.py confirms how many)"""
    return blobs(), init37(1023)


# one-step cases: name -> (index, nlist, init rows).  Ambiguous rows stay under 1 % at each of the steps used (a cap, not a tolerance)
def step_case(name):
    if name == "gaussian4099":
        return case_index("gaussian", 4099), NLIST, init37(4099)
    if name == "norm_spread":
        return case_index("norm_spread", 1023), NLIST, init37(1023)
    if name == "tail":                                            # nothing a multiple of any tile
        return case_index("gaussian", 257, dim=45), 5, np.sort(KR.rng(SEED + 6).choice(257, 5, replace=False)).astype(np.int32)
    if name == "nlist130":                                        # two centroid tiles of 64 and a remainder of 2
        return case_index("gaussian", 1023), 130, np.sort(KR.rng(SEED + 7).choice(1023, 130, replace=False)).astype(np.int32)
    if name == "dim70":                                           # two staged chunks of 32 dimensions and a remainder of 6; 65 rows: one row tile of 64 and one row
        return case_index("gaussian", 65, dim=70), 7, np.sort(KR.rng(SEED + 8).choice(65, 7, replace=False)).astype(np.int32)
    raise KeyError(name)


STEP_CASES = ("gaussian4099", "norm_spread", "tail", "nlist130", "dim70")
STEP_ITERS = 2                                                    # the one-step tests feed the centroids of assign steps 0 .. 2


_CACHE: dict = {}


def reference(kind, name):
    """the reference trajectory of a case, computed once per process and shared (read-only)"""
    key = (kind, name)
    if key not in _CACHE:
        if kind == "traj":
            index, init = trajectory_case(name)
            _CACHE[key] = (index, NLIST, init, train(index, NLIST, TRAJ_ITERS, init))
        elif kind == "empty":
            index, init = blobs_random_init()
            _CACHE[key] = (index, NLIST, init, train(index, NLIST, STEP_ITERS, init))
        else:
            index, nlist, init = step_case(name)
            _CACHE[key] = (index, nlist, init, train(index, nlist, STEP_ITERS, init))
    return _CACHE[key]
