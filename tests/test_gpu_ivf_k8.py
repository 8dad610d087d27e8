"""The IVF-probed retrieval at k = 8 (rvc_set_index_k; obs_rvc_amd/csrc/ivf.hip.h ivf_scan_blend_kernel<8>) on the shapes of tests/test_gpu_ivf.py (dim 48,
n 1023, nlist 37) through rvc_debug_retrieval: a probe of every list returns the flat k = 8 search's bits; a small nprobe returns the float64 top-8 over the
probed lists (knn_k_ref.probed_topk); a query whose probed lists hold five rows has five hits, three -1 / +inf, and is not blended, while the same query at
k = 4 is; a structure trained on the device is searched at k = 8."""
from __future__ import annotations

import numpy as np
import pytest

import ivf_ref as IR
import knn_k_ref as R
import knn_ref as KR
from debug_abi import ptr, same_bits
from knn_k_gpu import Engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def built():
    # ivf_ref's gaussian case (a class tests/test_ivf_ref.py cleared: no coarse or fine gap within 4 gamma at k = 4; the k = 8 gaps are asserted where used)
    return IR.build_case("gaussian", 1023, 3, 17, 2100)


def test_probe_of_every_list_is_the_flat_search(eng, built):
    case, cent, assign = built
    cv = R.to_cv(case.q, case.T + 5)
    eng.load(case.index)
    assert eng.set_k(8) == 0
    flat = eng.run(cv, case.skip_head, case.R, case.T, path="fused")
    eng.attach(cent, assign, IR.NLIST)
    assert eng.k() == 8                                                         # the setting survives rvc_set_index_ivf
    ivf = eng.run(cv, case.skip_head, case.R, case.T, expect="knn_ivf")
    assert ivf["idx"].shape[2] == 8 and (ivf["idx"] >= 0).all()
    for key in ("idx", "dist", "phone"):
        assert same_bits(ivf[key].view(np.float32), flat[key].view(np.float32)), key
    assert same_bits(ivf["phone"][:, :, case.R:], ivf["phone_in"][:, :, case.R:]) and same_bits(ivf["cv"], cv)


@pytest.mark.parametrize("nprobe", [1, 3])
def test_small_nprobe_against_float64(eng, built, nprobe):
    case, cent, assign = built
    cv = R.to_cv(case.q, case.T + 5)
    eng.load(case.index)
    assert eng.set_k(8) == 0
    eng.attach(cent, assign, nprobe)
    res = eng.run(cv, case.skip_head, case.R, case.T, expect="knn_ivf")
    cols = R.col_map(case.skip_head, case.R, case.T)
    g, bb = R.gamma(case.dim), R.blend_bound(case.dim, 8)
    wd = wb = 0.0
    for b in range(case.streams):
        q = case.used(b)
        ri, rd, cnt = R.probed_topk(case.index, q, cent, assign, nprobe, 8)
        # exact idx equality is demanded where float64 sees no gap within 4 gamma among the first nine distances (and the coarse order is knn_ref-cleared)
        d = R.d64(case.index, q)
        for r in range(case.R):
            j = cols[r] - case.first_raw
            idx, dist = res["idx"][b, r].astype(np.int64), res["dist"][b, r].astype(np.float64)
            have = ri[j] >= 0
            assert np.array_equal(idx >= 0, have) and np.all(np.isposinf(dist[~have])) and np.all(idx[~have] == -1), (b, r, idx, ri[j])
            D = rd[j][have]
            e_d = np.abs(dist[have] - D)
            wd = max(wd, float(np.max(e_d / (g * D))) if D.size else 0.0)
            assert np.all(e_d <= g * D), (b, r, wd)
            assert np.all(np.abs(d[j, idx[have]] - D) <= 2 * g * D)
            ph, x = res["phone"][b, :, r], q[j]
            if not have.all():
                assert same_bits(ph, x), (b, r, "a frame with fewer than eight hits was blended")
            else:
                ref, mag = R.blend(case.index, x, idx, 0.75)
                err = np.abs(ph - ref)
                wb = max(wb, float(np.max(err / (bb * mag))))
                assert np.all(err <= bb * mag), (b, r, wb)
    print("ivf k 8 nprobe %d: dist %.3f of gamma D, blend %.3f of its bound" % (nprobe, wd, wb))


def test_five_probed_rows(eng):
    # list 0 = rows 0..4 around a centroid of their own, far from everything else; query 0 of stream 0 sits on that centroid: nprobe = 1 probes five rows
    case = R.make_case("gaussian", dim=48, n=1023, streams=1, nq=17, seed=2300)
    far = np.float32(40.0)
    case.index[:5] = far + np.float32(0.01) * KR.rng(5).standard_normal((5, 48), dtype=np.float32)
    case.q[0, case.first_raw] = far
    g = KR.rng(6)
    rows = np.sort(g.choice(np.arange(5, case.n), 36, replace=False))
    cent = np.concatenate([np.full((1, 48), far, np.float32), case.index[rows]]).astype(np.float32)
    assign = np.argmin(R.d64(cent, case.index), axis=1).astype(np.int32)
    assert np.flatnonzero(assign == 0).tolist() == [0, 1, 2, 3, 4]
    cv = R.to_cv(case.q, case.T + 5)
    eng.load(case.index)
    frames = np.flatnonzero(R.col_map(case.skip_head, case.R, case.T) == case.first_raw)
    assert frames.size >= 1
    out = {}
    for k in (8, 4):
        assert eng.set_k(k) == 0
        eng.attach(cent, assign, 1)
        out[k] = eng.run(cv, case.skip_head, case.R, case.T, expect="knn_ivf")
    x = case.q[0, case.first_raw]
    for r in frames:
        i8, d8 = out[8]["idx"][0, r], out[8]["dist"][0, r]
        assert sorted(i8[:5].tolist()) == [0, 1, 2, 3, 4] and i8[5:].tolist() == [-1] * 3 and np.all(np.isposinf(d8[5:])) and np.all(np.isfinite(d8[:5]))
        assert same_bits(out[8]["phone"][0, :, r], x), "five hits at k = 8: the frame keeps its raw feature"
        i4 = out[4]["idx"][0, r]
        assert np.array_equal(i4, i8[:4]) and same_bits(out[4]["dist"][0, r], np.ascontiguousarray(d8[:4]))
        assert not same_bits(out[4]["phone"][0, :, r], x), "the same query at k = 4 is blended"
        ref, mag = R.blend(case.index, x, i4.astype(np.int64), 0.75)
        assert np.all(np.abs(out[4]["phone"][0, :, r] - ref) <= R.blend_bound(48, 4) * mag)


def test_trained_structure_at_k8(eng, built):
    case, _, _ = built
    cv = R.to_cv(case.q, case.T + 5)
    eng.load(case.index)
    assert eng.set_k(8) == 0
    assert eng.L.rvc_train_index_ivf(eng.h.h, 16, 4, None, 11) == 0, eng.h.last_error()
    assert eng.k() == 8                                                         # the setting survives rvc_train_index_ivf
    cent, assign = np.empty((16, 48), np.float32), np.empty(case.n, np.int32)
    assert eng.L.rvc_get_index_ivf(eng.h.h, ptr(cent), cent.size, ptr(assign), case.n) == 0
    assert eng.L.rvc_set_index_nprobe(eng.h.h, 3) == 0
    res = eng.run(cv, case.skip_head, case.R, case.T, expect="knn_ivf")
    cols = R.col_map(case.skip_head, case.R, case.T)
    g = R.gamma(case.dim)
    for b in range(case.streams):
        q = case.used(b)
        ri, rd, cnt = R.probed_topk(case.index, q, cent, assign, 3, 8)
        assert (cnt >= 8).all()
        for r in range(case.R):
            j = cols[r] - case.first_raw
            idx, dist = res["idx"][b, r], res["dist"][b, r].astype(np.float64)
            assert len(set(idx.tolist())) == 8 and np.all(np.abs(dist - rd[j]) <= g * rd[j]), (b, r)
    # and a probe of all 16 lists is the flat search
    assert eng.L.rvc_set_index_nprobe(eng.h.h, 16) == 0
    full = eng.run(cv, case.skip_head, case.R, case.T, expect="knn_ivf")
    assert eng.L.rvc_set_index_nprobe(eng.h.h, 0) == 0
    flat = eng.run(cv, case.skip_head, case.R, case.T, path="fused")
    for key in ("idx", "dist", "phone"):
        assert same_bits(full[key].view(np.float32), flat[key].view(np.float32)), key
