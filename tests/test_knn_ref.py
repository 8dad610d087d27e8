"""tests/knn_ref.py on the CPU: (a) the float64 restatement against the project's fp32 definition (oracle.knn_search), (b) the proofs that the adversarial
inputs of tests/test_gpu_knn.py do what they are meant to do -- candidate, flag and truncation counts from float64 with the kernels' own margin formula --,
(c) the determinism of the generated data.  Every proof prints its counts before it asserts.

A count only proves a path when it is far from the threshold the kernel compares it with: the kernels evaluate approx in fp32, good to ~1e-4 (|x|^2 + |y|^2)
(knn.hip.h:841), a twentieth of the margin.  "Far" here: outside [3/4, 5/4] of KNN_CAND."""
import numpy as np
import pytest

import knn_ref as KR
from knn_ref import make_case

CLASSES = ["gaussian", "offset3", "offset_dim", "mixed", "near_runs", "far_dups", "norm_spread", "offset_dups", "straddle"]
# the shapes of tests/test_gpu_knn.py's many-stream cases
GEMM = dict(dim=48, n=4099, streams=8, nq=16)


def _frames(case, b):
    cols = KR.col_map(case.skip_head, case.R, case.T)
    return case.q[b, cols]


# ---- (a) ----
@pytest.mark.parametrize("name", CLASSES)
@pytest.mark.parametrize("dim", [48, 44])
def test_oracle_search_agrees_with_float64_ranking(name, dim):
    from oracle import oracle as O
    O.build()
    case = make_case(name, dim=dim, n=257, streams=3, nq=17)
    g = KR.gamma(dim)
    for b in range(case.streams):
        q = _frames(case, b)
        io, do = O.knn_search(case.index, q, 4)
        d = KR.d64(case.index, q)
        _, D = KR.topk(d)
        assert ((io >= 0) & (io < case.n)).all() and all(len(set(r)) == 4 for r in io.tolist())
        assert np.all(np.abs(do - D) <= g * D), (name, b, float(np.max(np.abs(do - D) / np.maximum(D, 1e-300))))
        assert np.all(np.abs(np.take_along_axis(d, io.astype(np.int64), 1) - D) <= 2 * g * D)


def test_reference_pieces():
    # ranking by (d, index); the column map with an odd skip_head and the clamp; the blend's weights
    d = np.array([[3.0, 1.0, 1.0, 2.0, 1.0, 0.5]])
    idx, D = KR.topk(d)
    assert idx.tolist() == [[5, 1, 2, 4]] and D.tolist() == [[0.5, 1.0, 1.0, 1.0]]
    assert KR.col_map(5, 34, 19).tolist()[:3] == [2, 3, 3] and KR.col_map(5, 34, 19).tolist()[-4:] == [17, 18, 18, 18]
    assert KR.col_map(3, 1, 4).tolist() == [1]
    for nq, (s, R, T) in KR.GEOMS.items():
        assert s + R <= 2 * T + 1 and KR.raw_range(s, R, T)[1] == nq
    index = np.array([[1.0, 0.0], [0.0, 2.0], [3.0, 3.0], [-1.0, 0.0]], np.float32)
    x = np.array([0.0, 0.0], np.float32)
    ref, mag = KR.blend(index, x, np.array([0, 1, 2, 3]), 0.5)
    w = np.array([1.0, 1 / 16.0, 1 / 324.0, 1.0]); w /= w.sum()
    assert np.allclose(ref, 0.5 * (w[:, None] * index).sum(0), rtol=1e-15) and mag.tolist() == [3.0, 3.0]
    assert KR.fused_grid(5193, 1, 64) == 64 and KR.fused_grid(65609, 1, 4096) == 1024 and KR.fused_grid(1023, 3, 768) == 16


# ---- (b) ----
def test_overflow_inputs_overflow_and_the_others_do_not():
    lo, hi = KR.KNN_CAND * 3 // 4, KR.KNN_CAND * 5 // 4
    for name in ("gaussian", "offset3", "offset_dim", "offset_dups", "straddle", "mixed", "near_runs", "far_dups", "truncated"):
        case = make_case(name, **GEMM)
        cnt = np.stack([KR.candidates(case.index, case.used(b)) for b in range(case.streams)])
        print("%s: candidates per stream, min .. max over its queries: %s" % (name, [(int(c.min()), int(c.max())) for c in cnt]))
        if name in ("offset_dim", "offset_dups"):
            assert (cnt.max(1) > hi).all()
        elif name == "straddle":
            half = np.stack([KR.candidates(case.index, case.used(b), c=1e-3) for b in range(case.streams)])
            print("straddle: with half the margin constant: %s" % half.max(1).tolist())
            assert (cnt.max(1) > hi).all() and (half.max(1) < lo).all()         # the margin constant decides the overflow word of every stream
        elif name == "mixed":
            hot = case.meta["hot"]
            assert hot == [0, 2, 5]
            for b in range(case.streams):
                assert cnt[b].max() > hi if b in hot else cnt[b].max() < lo, (b, cnt[b])
        else:
            # (offset3: a common offset of 3 widens the margin to ~0.9 at dim 48 against a spread of 2.4 of the squared distances: tens of candidates, no overflow
            # at an index of a few thousand vectors.  The class that overflows at this size is the per-dimension offset)
            assert (cnt.max(1) < lo).all()
    for shape in (dict(dim=768, n=1001, streams=12, nq=11), dict(dim=256, n=4096, streams=8, nq=16)):
        case = make_case("offset_dim", **shape)
        cnt = np.stack([KR.candidates(case.index, case.used(b)) for b in range(case.streams)])
        print("offset_dim %s: %d .. %d" % (shape, cnt.min(), cnt.max()))
        assert (cnt.max(1) > hi).all()


def test_flagged_inputs_put_five_in_one_workgroup():
    # the one-launch form at the grids test_gpu_knn.py forces: G = 64 at n = 5193 (five or six tiles per workgroup), the default 16 at n = 1023, three streams
    for name, shape, wgs in (("offset_dim", dict(dim=48, n=5193, streams=1, nq=17), 64), ("near_runs", dict(dim=48, n=5193, streams=1, nq=17), 64),
                             ("offset_dim", dict(dim=48, n=1023, streams=3, nq=17), 768), ("near_runs", dict(dim=48, n=1023, streams=3, nq=17), 768)):
        case = make_case(name, **shape)
        G = KR.fused_grid(case.n, case.streams, wgs)
        tiles = -(-case.n // 16)
        worst = [int(KR.per_workgroup(KR.inside(case.index, case.used(b)), G).max()) for b in range(case.streams)]
        print("%s n %d: G %d, %d tiles (%d .. %d per workgroup), most vectors inside the margin in one workgroup per stream: %s" % (name, case.n, G, tiles, tiles // G, -(-tiles // G), worst))
        assert max(worst) >= 5
        if wgs == 64:
            assert tiles // G >= 5 and case.n % 16 != 0


def test_truncated_input_truncates_one_thread():
    for n in (4160, 4099):
        case = make_case("truncated", **dict(GEMM, n=n))
        b, j = case.meta["where"]
        m = KR.inside(case.index, case.used(b))
        per = KR.per_thread(m)
        print("truncated n %d: query (%d, %d): %d inside the margin, %d of them in thread %d's stride set" % (n, b, j, m[j].sum(), per[j].max(), per[j].argmax()))
        assert per[j].max() > 4 and m[j].sum() <= KR.KNN_CAND
        assert set(np.flatnonzero(m[j]).tolist()) == set(case.meta["rows"])
        assert per[np.arange(len(per)) != j].max() <= 4


def test_norm_spread_outlier_is_never_a_hit():
    case = make_case("norm_spread", **GEMM)
    out = case.meta["outlier"]
    assert abs(np.linalg.norm(case.index[out]) - 1e3) < 1.0 and abs(np.linalg.norm(case.q[0, 0]) - 1e-4) < 1e-6
    for b in range(case.streams):
        idx, _ = KR.topk(KR.d64(case.index, case.used(b)))
        assert out not in idx


def test_near_duplicate_runs_keep_six_each():
    # every run the class places has at least six vectors within 1e-4 relative of its query, at every index size the GPU file uses
    for n, streams, nq in ((63, 3, 15), (65, 3, 1), (257, 1, 16), (1023, 3, 17), (4099, 8, 16), (5193, 1, 17)):
        case = make_case("near_runs", dim=48, n=n, streams=streams, nq=nq, wgs=64 if n == 5193 else 768)
        for b, t, row, ln in case.meta["places"]:
            d = np.sqrt(KR.d64(case.index[row:row + ln], case.q[b, t][None])[0]) / np.linalg.norm(case.q[b, t])
            assert ln >= 6 and (d < 3e-4).all(), (n, row, d)


# ---- (c) ----
@pytest.mark.parametrize("name", CLASSES + ["truncated"])
def test_data_classes_are_deterministic(name):
    a, b = make_case(name, **GEMM), make_case(name, **GEMM)
    assert a.index.dtype == np.float32 and a.q.dtype == np.float32
    assert a.index.tobytes() == b.index.tobytes() and a.q.tobytes() == b.q.tobytes()
    assert np.isfinite(a.index).all() and np.isfinite(a.q).all()
    cv = KR.to_cv(a.q, a.T + 3)
    assert cv.shape == (a.streams, a.dim, a.T + 3) and np.array_equal(cv[1, :, 2], a.q[1, 2]) and (cv[:, :, a.T:] == np.float32(7.0e3)).all()
