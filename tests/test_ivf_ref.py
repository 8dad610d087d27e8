"""CPU checks behind tests/test_gpu_ivf.py: the inputs are fair (no query of a cleared class sits within 4 gamma of a coarse or fine tie, so exact idx equality
is a legitimate demand there), the planted structure is what the GPU test relies on, and the Faiss reader returns an IndexIVFFlat file's structure."""
from __future__ import annotations

import os

import numpy as np
import pytest

import ivf_ref as IR
import knn_ref as KR
from obs_rvc_amd import faiss_index as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.mark.parametrize("name,n,streams,nq,nprobe,seed", [c for c in IR.CASES if c[0] in IR.CLEARED])
def test_cleared_cases_have_no_ambiguous_query(name, n, streams, nq, nprobe, seed):
    case, cent, assign = IR.build_case(name, n, streams, nq, seed)
    assert IR.ambiguous(case, cent, assign, nprobe) == 0


def test_every_axis_value_is_covered():
    assert {c[2] for c in IR.CASES} == {1, 3, 12} and {c[3] for c in IR.CASES} == {1, 11, 17, 33} and {c[4] for c in IR.CASES} == {1, 3, 37}
    assert {c[1] for c in IR.CASES} == {1023, 4099} and any(c[2] == 12 and c[3] == 33 for c in IR.CASES)
    assert {c[0] for c in IR.CASES} == {"gaussian", "offset3", "near_runs", "far_dups", "norm_spread"}


def test_probe_of_every_list_is_the_flat_search():
    case, cent, assign = IR.build_case("gaussian", 1023, 3, 17)
    q = case.used(1)
    idx, dist, probes, scanned = IR.search(case.index, cent, assign, q, IR.NLIST)
    fi, fd = KR.topk(KR.d64(case.index, q))
    assert np.array_equal(idx, fi) and np.array_equal(dist, fd) and all(len(s) == case.n for s in scanned)
    # one list: the hits are that list's rows
    idx1, _, probes1, _ = IR.search(case.index, cent, assign, q, 1)
    assert all(set(assign[i[i >= 0]].tolist()) <= set(p.tolist()) for i, p in zip(idx1, probes1))


def test_non_finite_query_has_no_hit():
    case, cent, assign = IR.build_case("gaussian", 1023, 1, 11)
    q = case.used(0).copy()
    q[0, 3] = np.nan
    q[1, 5] = np.inf
    idx, dist, probes, _ = IR.search(case.index, cent, assign, q, 3)
    assert (idx[:2] == -1).all() and np.isinf(dist[:2]).all() and len(probes[0]) == 0 and (idx[2:] >= 0).all()
    ref, _ = IR.blend_or_keep(case.index, q[2], idx[0], 0.75)
    assert np.array_equal(ref, q[2].astype(np.float64))


def test_planted_structure():
    p = IR.Planted()
    case, cent, assign = p.case, p.cent, p.assign
    x = lambda bt: case.q[bt[0], bt[1]][None]
    # dup: bit-identical centroids, equal and smallest coarse distances; both lists hold rows and the nearest row of all is in list 5
    assert np.array_equal(cent[4].view(np.uint32), cent[5].view(np.uint32))
    D = IR.coarse(cent, x(p.q_dup))[0]
    assert D[4] == D[5] and np.argsort(D, kind="stable")[0] == 4 and np.sort(D)[2] > 10 * D[4]
    assert (assign == 4).sum() == 12 and (assign == 5).sum() == 12
    flat = KR.topk(KR.d64(case.index, x(p.q_dup)))[0][0]
    assert assign[flat[0]] == 5
    idx, _, probes, _ = IR.search(case.index, cent, assign, x(p.q_dup), 1)
    assert probes[0].tolist() == [4] and (assign[idx[0]] == 4).all()
    # empty: the nearest list holds nothing
    D = IR.coarse(cent, x(p.q_empty))[0]
    assert D[9] == 0.0 and (assign == 9).sum() == 0
    idx, dist, _, _ = IR.search(case.index, cent, assign, x(p.q_empty), 1)
    assert (idx == -1).all() and np.isinf(dist).all()
    # three rows
    D = IR.coarse(cent, x(p.q_three))[0]
    assert D[12] == 0.0 and np.array_equal(np.flatnonzero(assign == 12), p.three_rows)
    idx, dist, _, _ = IR.search(case.index, cent, assign, x(p.q_three), 1)
    assert sorted(idx[0, :3].tolist()) == p.three_rows.tolist() and idx[0, 3] == -1 and np.isinf(dist[0, 3]) and np.isfinite(dist[0, :3]).all()
    # long list: 300 rows, the best one last
    D = IR.coarse(cent, x(p.q_long))[0]
    assert D[20] == 0.0 and np.array_equal(np.flatnonzero(assign == 20), np.arange(700, 1000))
    idx, dist, _, _ = IR.search(case.index, cent, assign, x(p.q_long), 1)
    assert idx[0, 0] == 999 and dist[0, 1] > 100 * dist[0, 0]
    # the four planted queries are distinct raw frames, and every list number is in range
    assert len({p.q_dup, p.q_empty, p.q_three, p.q_long}) == 4 and assign.min() >= 0 and assign.max() < IR.NLIST


@pytest.mark.parametrize("name", ["faiss_ivf.index", "faiss_ivf_sparse.index"])
def test_read_index_ivf_on_the_golden_files(name):
    path = os.path.join(GOLDEN, name)
    v, cent, assign = F.read_index_ivf(path)
    assert np.array_equal(v.view(np.uint32), F.read_index(path).view(np.uint32))
    assert cent is not None and cent.dtype == np.float32 and cent.shape[1] == v.shape[1] and assign.dtype == np.int32 and assign.shape == (v.shape[0],)
    # assign reproduces the file's lists: the file stores list after list, each as (vectors, ids)
    ivf = {}
    with open(path, "rb") as f:
        stored, ids = F._read(F._R(f), ivf)
    sizes = ivf["sizes"]
    assert sizes.size == cent.shape[0] and np.array_equal(np.bincount(assign, minlength=sizes.size), sizes)
    at = 0
    for l, n in enumerate(sizes.tolist()):
        assert (assign[ids[at:at + n]] == l).all() and np.array_equal(v[ids[at:at + n]], stored[at:at + n])
        at += n
    assert F.read_index_nprobe(path) == ivf["nprobe"] >= 1


def test_flat_file_has_no_structure():
    path = os.path.join(GOLDEN, "faiss_flat.index")
    v, cent, assign = F.read_index_ivf(path)
    assert cent is None and assign is None and np.array_equal(v, F.read_index(path)) and F.read_index_nprobe(path) == 0


@pytest.mark.parametrize("sparse", [False, True])
def test_write_ivf_flat_round_trip(tmp_path, sparse):
    case, cent, assign = IR.build_case("gaussian", 1023, 1, 1)
    cent = cent.copy()
    cent[7] = 1.0e3                                               # an empty list
    path = str(tmp_path / "rt.index")
    F.write_ivf_flat(path, case.index, cent, sparse_sizes=sparse)
    v, c2, a2 = F.read_index_ivf(path)
    want = np.argmin(((case.index[:, None, :] - cent[None]) ** 2).sum(-1), axis=1)          # write_ivf_flat's own assignment
    assert np.array_equal(v.view(np.uint32), case.index.view(np.uint32)) and np.array_equal(c2.view(np.uint32), cent.view(np.uint32))
    assert np.array_equal(a2, want) and (a2 == 7).sum() == 0
