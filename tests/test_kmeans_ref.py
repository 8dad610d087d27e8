"""tests/kmeans_ref.py on the CPU: the inputs of tests/test_gpu_kmeans.py are proven fair before the GPU sees them, the reference's own properties, the defaults,
and the Faiss writer for a given assignment.  gamma = (dim + 2) 2^-24 (knn_ref)."""
from __future__ import annotations

import numpy as np
import pytest

import kmeans_ref as M
import knn_ref as KR
from obs_rvc_amd import faiss_index as F


def _empty(assign, nlist):
    return int((np.bincount(assign, minlength=nlist) == 0).sum())


@pytest.mark.parametrize("name", M.TRAJECTORY)
def test_trajectory_cases_have_no_ambiguous_row(name):
    # seed 3100 clears all three cases at every assign step: no seed was moved
    index, nlist, init, ref = M.reference("traj", name)
    assert len(set(init.tolist())) == nlist
    for s, (cent, a) in enumerate(zip(ref["cents"], ref["assigns"])):
        amb = int(M.ambiguous_rows(index, cent).sum())
        print("%s step %d: %d ambiguous rows, moved %d, J %.9g" % (name, s, amb, ref["moved"][s], ref["objective"][s]))
        assert amb == 0, (name, s)
        assert np.array_equal(np.argmin(M.chain32(index, cent), axis=1), a), (name, s, "the fp32 chain's argmin differs from float64")
    if name == "blobs":
        # init rows 0 .. 36 are one row of every blob: the second assign step moves nothing
        assert ref["iters_run"] == 1 and ref["moved"] == [1023, 0]
    else:
        assert ref["iters_run"] == M.TRAJ_ITERS and min(ref["moved"]) > 0          # never converges within the steps the tests run


@pytest.mark.parametrize("name", M.STEP_CASES)
def test_step_cases_stay_under_the_ambiguity_cap(name):
    index, nlist, init, ref = M.reference("step", name)
    assert ref["iters_run"] == M.STEP_ITERS
    for s, cent in enumerate(ref["cents"]):
        amb = int(M.ambiguous_rows(index, cent).sum())
        print("%s step %d: %d ambiguous rows of %d" % (name, s, amb, len(index)))
        assert amb < 0.01 * len(index), (name, s, amb)


def test_blobs_with_a_random_init_leave_lists_empty():
    # a random init misses some blobs and hits others twice: with seed 3100 two lists are empty from the second assign step on (the lists of the doubly hit blobs'
    # losers), and an empty list's centroid never changes
    index, nlist, init, ref = M.reference("empty", "blobs")
    empties = [_empty(a, nlist) for a in ref["assigns"]]
    print("empty lists per assign step:", empties)
    assert empties == [0, 2, 2]
    for s in (1, 2):
        dead = np.flatnonzero(np.bincount(ref["assigns"][s], minlength=nlist) == 0)
        if s + 1 < len(ref["cents"]):
            assert np.array_equal(ref["cents"][s + 1][dead].view(np.uint32), ref["cents"][s][dead].view(np.uint32))
    assert all(int(M.ambiguous_rows(index, c).sum()) == 0 for c in ref["cents"])


@pytest.mark.parametrize("kind,name", [("traj", n) for n in M.TRAJECTORY] + [("step", n) for n in M.STEP_CASES] + [("empty", "blobs")])
def test_objective_never_rises(kind, name):
    ref = M.reference(kind, name)[3]
    J = np.array(ref["objective"])
    assert len(J) == ref["iters_run"] + 1 and np.all(np.diff(J) <= 0), J
    assert ref["moved"][0] == len(ref["assigns"][0])


def test_update_step_is_the_mean():
    index, nlist, init, ref = M.reference("traj", "gaussian")
    c1 = M.means(index, ref["assigns"][0], ref["cents"][0])
    for j in (0, 17, 36):
        rows = np.flatnonzero(ref["assigns"][0] == j)
        assert np.array_equal(c1[j], index[rows].astype(np.float64).mean(0).astype(np.float32)) or np.allclose(c1[j], index[rows].mean(0), rtol=1e-6)
    assert np.array_equal(c1, ref["cents"][1])
    # init is a copy of the rows, bit for bit
    assert np.array_equal(ref["cents"][0].view(np.uint32), index[init].view(np.uint32))


def test_ties_and_non_finite_distances():
    index = M.case_index("gaussian", 65)
    cent = index[[3, 3, 9]].copy()                                 # lists 0 and 1 bit-identical
    a, d, J, moved = M.assign_step(index, cent)
    assert not (a == 1).any() and moved == 65
    # a row whose every distance is non-finite: each compares as +inf, and the smallest (+inf, j) is list 0
    with np.errstate(all="ignore"):
        far = np.concatenate([index, np.full((1, 48), 1.7e308 ** 0.5 * 4.0)]).astype(np.float64)
        D = M.distances(far, -far[-1:].repeat(3, 0))
    assert np.isposinf(D[-1]).all() and np.argmin(D, axis=1)[-1] == 0


def test_default_nlist_rule():
    assert M.default_nlist(100000) == 2564 and M.default_nlist(1000000) == 16000 and M.default_nlist(1023) == 26
    assert M.default_nlist(4) == 1 and M.default_nlist(38) == 1 and M.default_nlist(78) == 2 and M.default_nlist(10 ** 8) == 65536
    assert M.default_nlist(3000) == 76                               # n // 39 binds below n = 389 376, 16 sqrt(n) above
    assert M.default_nlist(400000) == min(int(16 * np.sqrt(400000.0)), 400000 // 39) == 10119


def test_seeded_init_is_distinct_sorted_and_reproducible():
    for n, nlist, seed in ((1023, 37, 0), (4099, 130, 1), (257, 257, 7), (65, 1, 0xffffffff)):
        rows = M.seeded_rows(n, nlist, seed)
        assert rows.shape == (nlist,) and np.all(np.diff(rows) > 0) and rows.min() >= 0 and rows.max() < n
        assert np.array_equal(rows, M.seeded_rows(n, nlist, seed))
    assert not np.array_equal(M.seeded_rows(1023, 37, 0), M.seeded_rows(1023, 37, 1))
    # the mixer, pinned: lowbias32 on a few words, and the sample of two seeds
    x = 1
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16
    assert int(M.mix(1)) == x and int(M.mix(0)) == 0
    assert M.seeded_rows(1023, 5, 0).tolist() == [125, 271, 310, 538, 942] and M.seeded_rows(1023, 5, 1).tolist() == [65, 70, 493, 616, 870]
    # a prefix property the definition implies: the sample of nlist + 1 contains the sample of nlist
    assert set(M.seeded_rows(1023, 37, 3).tolist()) <= set(M.seeded_rows(1023, 38, 3).tolist())


def test_write_ivf_flat_assigned_round_trips(tmp_path):
    index, nlist, init, ref = M.reference("empty", "blobs")          # (two empty lists)
    cent, assign = ref["cents"][-1], ref["assigns"][-1]
    path = str(tmp_path / "t.index")
    F.write_ivf_flat_assigned(path, index, cent, assign, nprobe=3)
    v, c, a, k = F.read_index_ivf(path, with_nprobe=True)
    assert k == 3 and np.array_equal(a, assign) and a.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), index.view(np.uint32)) and np.array_equal(c.view(np.uint32), cent.view(np.uint32))
    assert np.array_equal(F.read_index(path).view(np.uint32), index.view(np.uint32)) and F.read_index_nprobe(path) == 3
    with pytest.raises(F.IndexFormatError):
        F.write_ivf_flat_assigned(path, index, cent, np.where(assign == 0, nlist, assign))
    with pytest.raises(F.IndexFormatError):
        F.write_ivf_flat_assigned(path, index, cent[:, :-1], assign)


def test_write_ivf_flat_assigned_equals_the_old_writer(tmp_path):
    # a small case where the old writer's own fp32 numpy argmin IS the given assignment (asserted first): the two files are byte-identical
    index = M.case_index("gaussian", 257, dim=45)
    cent = np.ascontiguousarray(index[[5, 50, 100, 150, 250]] + np.float32(0.05))
    assign = np.argmin(((index[:, None, :] - cent[None]) ** 2).sum(-1), axis=1)
    assert np.array_equal(assign, np.argmin(KR.d64(cent, index), axis=1))
    old, new = str(tmp_path / "old.index"), str(tmp_path / "new.index")
    F.write_ivf_flat(old, index, cent)
    F.write_ivf_flat_assigned(new, index, cent, assign.astype(np.int32))
    assert open(old, "rb").read() == open(new, "rb").read()
