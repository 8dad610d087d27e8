"""The IVF-probed retrieval (obs_rvc_amd/csrc/ivf.hip.h, retrieval.hip build_ivf) against tests/ivf_ref.py: the section alone through
rvc_debug_retrieval on a bare engine (dim 48, n 1023 / 4099, nlist 37), then the public path on the tiny preset.

Asserted everywhere: |dist[k] - D[k]| <= gamma D[k] against the reference's sorted distances over the reference probe set, the float64 distance of the returned
row within 2 gamma D[k], every returned row in a reference-probed list, phone within knn_ref.blend_bound(dim) of blend() on the returned rows (bit-equal to the
raw feature where a hit is missing), padding untouched; on the classes tests/test_ivf_ref.py cleared, idx equal to the reference.  gamma = (dim + 2) 2^-24
(knn_ref.py).  Every check prints its largest ratio to the bound before it asserts."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ivf_ref as IR
import knn_ref as KR
from debug_abi import RVC_SHAPE, Handle, RetrievalSpec, ptr, same_bits

pytestmark = pytest.mark.gpu

PH_FILL = np.float32(-5.0e3)
SZ = C.c_size_t


class Engine:
    """a bare engine with an index and, on request, an IVF structure"""

    def __init__(self):
        self.h = Handle()
        self.L = L = self.h.L
        L.rvc_set_index_ivf.argtypes = [C.c_void_p, C.c_void_p, SZ, SZ, C.c_void_p, SZ]
        L.rvc_set_index_nprobe.argtypes = [C.c_void_p, C.c_int]
        L.rvc_index_nprobe.argtypes = [C.c_void_p]
        L.rvc_index_ivf_info.argtypes = [C.c_void_p, C.POINTER(SZ), C.POINTER(SZ), C.POINTER(SZ)]
        L.rvc_retrieval_recoveries.argtypes = [C.c_void_p]
        L.rvc_retrieval_recoveries.restype = C.c_longlong

    def load(self, index, cent=None, assign=None, nprobe=0):
        self.index = np.ascontiguousarray(index, np.float32)
        assert self.L.rvc_load_index(self.h.h, ptr(self.index), self.index.shape[0], self.index.shape[1]) == 0, self.h.last_error()
        if cent is not None:
            assert self.attach(cent, assign) == 0, self.h.last_error()
        assert self.nprobe(nprobe) == 0, self.h.last_error()

    def attach(self, cent, assign, dim=None, n=None, nlist=None):
        cent, assign = np.ascontiguousarray(cent, np.float32), np.ascontiguousarray(assign, np.int32)
        return self.L.rvc_set_index_ivf(self.h.h, ptr(cent), cent.shape[0] if nlist is None else nlist, cent.shape[1] if dim is None else dim, ptr(assign),
                                        assign.shape[0] if n is None else n)

    def nprobe(self, k):
        return self.L.rvc_set_index_nprobe(self.h.h, k)

    def info(self):
        a, b, c = SZ(), SZ(), SZ()
        rc = self.L.rvc_index_ivf_info(self.h.h, C.byref(a), C.byref(b), C.byref(c))
        return rc, a.value, b.value, c.value

    def run(self, cv, skip_head, R, T, rate=0.75, reps=1, graph=0, ph_pad=3, path=0, rc=0):
        B, dim, cv_ld = cv.shape
        phone_in = np.full((B, dim, R + ph_pad), PH_FILL, np.float32)
        phone, cvb = phone_in.copy(), np.ascontiguousarray(cv, np.float32).copy()
        idx, dist, ovf = np.full((B, R, 4), -7, np.int32), np.full((B, R, 4), -7.0, np.float32), np.full(B, -7, np.int32)
        s = RetrievalSpec(streams=B, C=dim, T=T, cv_ld=cv_ld, skip_head=skip_head, R=R, ph_ld=R + ph_pad, rate=rate, path=path, reps=reps, graph=graph)
        got = self.L.rvc_debug_retrieval(self.h.h, C.byref(s), ptr(cvb), ptr(phone), ptr(idx), ptr(dist), ptr(ovf))
        name = self.h.last_kernel()
        if got != rc and "hip" in self.h.last_error():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % self.h.last_error(), returncode=3)
        assert got == rc, (got, self.h.last_error())
        return dict(phone=phone, cv=cvb, idx=idx, dist=dist, overflow=ovf, kernel=name, phone_in=phone_in)

    def close(self):
        self.h.close()


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def check(case, cent, assign, nprobe, cv, res, rate, exact):
    """everything the module docstring lists, for one result"""
    assert res["kernel"] == "knn_ivf" and not res["overflow"].any()
    assert same_bits(res["phone"][:, :, case.R:], res["phone_in"][:, :, case.R:]), "phone padding written"
    assert same_bits(res["cv"], cv), "cv written"
    cols = KR.col_map(case.skip_head, case.R, case.T)
    g, bb = KR.gamma(case.dim), KR.blend_bound(case.dim)
    wd = wi = wb = 0.0
    for b in range(case.streams):
        q = case.used(b)
        ri, rd, probes, _ = IR.search(case.index, cent, assign, q, nprobe)
        for r in range(case.R):
            j = cols[r] - case.first_raw
            idx, dist, x = res["idx"][b, r].astype(np.int64), res["dist"][b, r].astype(np.float64), q[j]
            have = ri[j] >= 0
            assert np.array_equal(idx >= 0, have), (case.name, b, r, idx, ri[j])
            assert np.all(np.isposinf(dist[~have])) and np.all(idx[~have] == -1)
            D = rd[j][have]
            got = idx[have]
            assert len(set(got.tolist())) == len(got) and np.all((got >= 0) & (got < case.n))
            d_ret = KR.d64(case.index[got], x[None])[0] if got.size else np.zeros(0)
            e_d, e_i = np.abs(dist[have] - D), np.abs(d_ret - D)
            with np.errstate(divide="ignore", invalid="ignore"):
                if D.size:
                    wd = max(wd, float(np.nanmax(np.where(D > 0, e_d / (g * D), 0.0))))
                    wi = max(wi, float(np.nanmax(np.where(D > 0, e_i / (2 * g * D), 0.0))))
            assert np.all(e_d <= g * D), (case.name, b, r, wd)
            assert np.all(e_i <= 2 * g * D), (case.name, b, r, wi)
            assert np.all(np.isin(assign[got], probes[j])), (case.name, b, r, "a hit outside the reference probe set")
            if exact:
                assert np.array_equal(idx, ri[j]), (case.name, b, r, idx, ri[j])
            ref, mag = IR.blend_or_keep(case.index, x, idx, rate)
            ph = res["phone"][b, :, r]
            if not have.all() or rate == 0.0:
                assert same_bits(ph, x), (case.name, b, r, "the frame does not hold the raw feature")
            else:
                err = np.abs(ph - ref)
                wb = max(wb, float(np.max(err / (bb * mag + 1e-300))))
                assert np.all(err <= bb * mag), (case.name, b, r, wb)
    print("%s n %d streams %d nq %d nprobe %d: dist %.3f of gamma D, index %.3f of 2 gamma D, blend %.3f of its bound" %
          (case.name, case.n, case.streams, case.nq, nprobe, wd, wi, wb))


# ---- 1. hits and blend against float64 ----
@pytest.mark.parametrize("name,n,streams,nq,nprobe,seed", IR.CASES)
def test_hits_and_blend_against_float64(eng, name, n, streams, nq, nprobe, seed):
    case, cent, assign = IR.build_case(name, n, streams, nq, seed)
    eng.load(case.index, cent, assign, nprobe)
    assert eng.L.rvc_index_nprobe(eng.h.h) == nprobe and eng.L.rvc_debug_index_layouts(eng.h.h) & 4
    rc, nlist, longest, empty = eng.info()
    sizes = np.bincount(assign, minlength=IR.NLIST)
    assert (rc, nlist, longest, empty) == (0, IR.NLIST, int(sizes.max()), int((sizes == 0).sum()))
    cv = KR.to_cv(case.q, case.T + 5)
    res = eng.run(cv, case.skip_head, case.R, case.T)
    check(case, cent, assign, nprobe, cv, res, 0.75, exact=name in IR.CLEARED)


# ---- 2. a probe of every list is the flat search ----
@pytest.mark.parametrize("name", ["gaussian", "near_runs"])
def test_nprobe_nlist_is_the_flat_search(eng, name):
    case, cent, assign = IR.build_case(name, 4099, 3, 17)
    eng.load(case.index, cent, assign, 0)
    cv = KR.to_cv(case.q, case.T + 5)
    flat = eng.run(cv, case.skip_head, case.R, case.T)
    assert flat["kernel"] == "knn_fused"
    assert eng.nprobe(64) == 0 and eng.L.rvc_index_nprobe(eng.h.h) == IR.NLIST           # clamped to nlist
    ivf = eng.run(cv, case.skip_head, case.R, case.T)
    assert ivf["kernel"] == "knn_ivf"
    for k in ("idx", "dist", "phone"):
        assert same_bits(ivf[k].view(np.float32), flat[k].view(np.float32)), (name, k)
    assert eng.nprobe(0) == 0
    again = eng.run(cv, case.skip_head, case.R, case.T)
    assert again["kernel"] == "knn_fused" and same_bits(again["phone"], flat["phone"])


# ---- 3. tie-break and corners ----
def test_planted_structure(eng):
    p = IR.Planted()
    case, cent, assign = p.case, p.cent, p.assign
    eng.load(case.index, cent, assign, 1)
    cv = KR.to_cv(case.q, case.T + 5)
    res = eng.run(cv, case.skip_head, case.R, case.T)
    check(case, cent, assign, 1, cv, res, 0.75, exact=False)
    # two bit-identical centroids: the lower list wins, although the nearest row of all sits in the higher one
    b, fr = p.frames(p.q_dup)
    assert fr.size and (assign[res["idx"][b, fr]] == 4).all()
    # an empty nearest list: no hit, the raw feature, and the neighbouring frames still blended
    b, fr = p.frames(p.q_empty)
    assert fr.size and (res["idx"][b, fr] == -1).all() and np.isposinf(res["dist"][b, fr]).all()
    for r in fr:
        assert same_bits(res["phone"][b, :, r], case.q[b, p.q_empty[1]])
    for r in (fr.min() - 1, fr.max() + 1):
        assert (res["idx"][b, r] >= 0).all() and not np.array_equal(res["phone"][b, :, r], case.q[b, KR.col_map(case.skip_head, case.R, case.T)[r]])
    # a probed union of three rows: three hits, one -1, no blend
    b, fr = p.frames(p.q_three)
    for r in fr:
        assert sorted(res["idx"][b, r, :3].tolist()) == p.three_rows.tolist() and res["idx"][b, r, 3] == -1 and np.isposinf(res["dist"][b, r, 3])
        assert same_bits(res["phone"][b, :, r], case.q[b, p.q_three[1]])
    # a list of 300 rows, the best one last
    b, fr = p.frames(p.q_long)
    assert fr.size and (res["idx"][b, fr, 0] == 999).all()
    ref = IR.search(case.index, cent, assign, case.q[b, p.q_long[1]][None], 1)[0][0]
    assert all(np.array_equal(res["idx"][b, r], ref) for r in fr)
    # rate 0: phone = x bit for bit (asserted per frame in check)
    zero = eng.run(cv, case.skip_head, case.R, case.T, rate=0.0)
    check(case, cent, assign, 1, cv, zero, 0.0, exact=False)


# ---- 4. launch mechanics ----
def test_replay_and_bookkeeping(eng):
    case, cent, assign = IR.build_case("near_runs", 4099, 3, 17)
    eng.load(case.index, cent, assign, 3)
    cv = KR.to_cv(case.q, case.T + 5)
    before = eng.L.rvc_retrieval_recoveries(eng.h.h)
    once = eng.run(cv, case.skip_head, case.R, case.T)
    again = eng.run(cv, case.skip_head, case.R, case.T, reps=3, graph=1)
    assert once["kernel"] == again["kernel"] == "knn_ivf"
    for k in ("idx", "dist", "phone"):
        assert same_bits(again[k].view(np.float32), once[k].view(np.float32)), k
    assert eng.L.rvc_retrieval_recoveries(eng.h.h) == before == 0
    eng.run(cv, case.skip_head, case.R, case.T, path=1, rc=RVC_SHAPE)                   # there is no exhaustive list
    assert eng.h.last_error()


# ---- 5. the public path ----
def _full_engine(streams):
    from common import zoo
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method("yin")
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    return e


@pytest.mark.parametrize("streams", [1, 3])
def test_public_path(streams):
    from common import BASELINE_160MS as g, voice_signal
    from obs_rvc_amd import weights as W
    index = W.make_index(3000, 48, seed=5)
    gq = KR.rng(31)
    rows = np.sort(gq.choice(3000, IR.NLIST, replace=False))
    cent = np.ascontiguousarray(index[rows] + np.float32(0.05) * gq.standard_normal((IR.NLIST, 48), dtype=np.float32))
    assign = np.argmin(KR.d64(cent, index), axis=1).astype(np.int32)
    e = _full_engine(streams)
    e.load_index(index); e.set_index_rate(0.75); e.enable_taps(2)
    e.set_index_ivf(cent, assign); e.set_index_nprobe(2)
    assert e.index_nprobe() == 2 and e.index_ivf_info()[0] == IR.NLIST
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=3 + s) for s in range(streams)])
    R, skip = g.model_return_length, g.skip_head

    def run():
        e.reset_state(); e.set_noise_seed(1234, 0)                      # (every run is the engine's first chunk: pitch cache, chunk counter, noise)
        return e.infer_batch(xs, g.sample_frame_16k, [12, 0, -12][:streams], skip, R) if streams > 1 else e.infer(xs[0], g.sample_frame_16k, 12, skip, R)

    if streams > 1:
        e.set_protect(0.33)                                             # (the plans with the protection stage tap every stream's ContentVec output: "cv.out_all")
    y0 = np.array(run())
    idx, dist = e.knn()
    assert idx.shape == (streams * R, 4)
    # every stream's queries from the tap of the ContentVec output [B][C][T]; the hits are not touched by the protection stage
    cvo = (e.tap("cv.out_all") if streams > 1 else e.tap("cv.out")).reshape(streams, 48, -1)
    cols = KR.col_map(skip, R, cvo.shape[2])
    gm = KR.gamma(48)
    for b in range(streams):
        q = np.ascontiguousarray(cvo[b].T[cols])
        assert IR.ambiguous_queries(index, cent, assign, q, 2) == 0, "the seed is not cleared: a coarse or fine gap within 4 gamma"
        ri, rd, _, _ = IR.search(index, cent, assign, q, 2)
        assert (ri >= 0).all()
        assert np.all(np.abs(dist[b * R:(b + 1) * R] - rd) <= gm * rd) and np.array_equal(idx[b * R:(b + 1) * R], ri), b
    b0 = e.plan_cache_info()["builds"]
    e.set_index_nprobe(0)
    y1 = np.array(run())
    assert e.plan_cache_info()["builds"] == b0 + 1 and not np.array_equal(y1, y0)
    e.set_index_nprobe(2)
    y2 = np.array(run())
    assert e.plan_cache_info()["builds"] == b0 + 1 and same_bits(np.ascontiguousarray(y2, np.float32), np.ascontiguousarray(y0, np.float32))
    # a new index: flat again
    e.load_index(index)
    assert e.index_nprobe() == 0
    e.close()


def test_load_index_keeps_a_files_structure(tmp_path):
    import os
    from obs_rvc_amd import faiss_index as F
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.rvc_common import RvcInferError
    from common import zoo
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    ivf, flat = os.path.join(golden, "faiss_ivf.index"), os.path.join(golden, "faiss_flat.index")
    v, cent, assign = F.read_index_ivf(ivf)
    e = RvcInfer(zoo("tiny")["data"])
    e.load_index(ivf)
    assert e.index_nprobe() == 0 and not e._L.rvc_debug_index_layouts(e._h) & 4          # nprobe=None: today's behaviour
    e.load_index(ivf, nprobe="file")
    assert e.index_nprobe() == F.read_index_nprobe(ivf) >= 1 and e.index_ivf_info()[0] == cent.shape[0]
    e.load_index(ivf, nprobe=2)
    assert e.index_nprobe() == min(2, cent.shape[0])
    # sources without a structure: the RVC_SHAPE error, and the engine keeps the index and the probe count it had
    np.save(str(tmp_path / "m.npy"), v)
    for src in (flat, v, str(tmp_path / "m.npy")):
        for k in (1, "file"):
            with pytest.raises(RvcInferError) as ei:
                e.load_index(src, nprobe=k)
            assert ei.value.code == RVC_SHAPE and e.index_nprobe() == min(2, cent.shape[0]) and e._L.rvc_debug_index_layouts(e._h) & 4
    with pytest.raises(RvcInferError):
        e.load_index(ivf, nprobe=65)
    e.load_index(flat, nprobe=0)
    assert e.index_nprobe() == 0
    e.close()


def test_session_chunk_equals_the_engine_call():
    # the native session (rvc_session_process) against the Python state machine, which makes the engine call rvc_infer on its own 16 kHz ring: same settings,
    # nprobe = 2 on both.  What the retrieval produced is compared bit for bit (hits and the blended features), the finished frames within the bound
    # tests/test_gpu_crossfade.py uses for this pair of chains
    from common import zoo
    from obs_rvc_amd import weights as W
    from obs_rvc_amd.geometry import derive
    from obs_rvc_amd.resample import FftFixedInOut
    from obs_rvc_amd.rvc import RvcInfer
    from obs_rvc_amd.streaming import NativeStreamingSession, StreamingSession
    from common import voice_signal
    index = W.make_index(3000, 48, seed=5)
    gq = KR.rng(31)
    rows = np.sort(gq.choice(3000, IR.NLIST, replace=False))
    cent = np.ascontiguousarray(index[rows] + np.float32(0.05) * gq.standard_normal((IR.NLIST, 48), dtype=np.float32))
    assign = np.argmin(KR.d64(cent, index), axis=1).astype(np.int32)
    z = zoo("tiny")

    def engine():
        e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_f0(); e.load_model(z["model"]); e.set_noise_seed(3, 0)
        e.load_index(index); e.set_index_rate(0.75); e.set_index_ivf(cent, assign); e.set_index_nprobe(2); e.enable_taps(2)
        return e
    e1, e2 = engine(), engine()
    g = derive(48000, 0.16, 0.07, 2.0, 4800)
    nat = NativeStreamingSession(e1, 48000, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    pys = StreamingSession(e2, g, 12, 0.6, 4800, lambda ri, ro, n: FftFixedInOut(e2, ri, ro, n))
    F = 7680
    a = np.interp(np.arange(F * 3) / 48000.0, np.arange(2560 * 3) / 16000.0, voice_signal(2560 * 3, seed=10)).astype(np.float32)
    R = nat.model_return_length
    for c in range(3):
        ch = a[c * F:(c + 1) * F]
        fn, fp = nat.process_one_frame(ch), pys.process_one_frame(ch)
        (i1, d1), (i2, d2) = e1.knn(), e2.knn()
        assert i1.shape == (R, 4) and (i1 >= 0).all() and np.array_equal(i1, i2) and same_bits(d1, d2), c
        assert same_bits(e1.tap("cv.out"), e2.tap("cv.out")) and same_bits(e1.tap("phone_ct"), e2.tap("phone_ct")), c
        err = float(np.abs(fn - fp).max())
        print("chunk %d: hits and blended features bit-identical, frames differ by %.3e" % (c, err))
        assert nat.last_sola_offset == pys.last_sola_offset and err < 2e-5, (c, err)
        # and they are the IVF search's hits: every row lies in one of the two lists nearest to its query
        cvo = e1.tap("cv.out").reshape(48, -1)
        q = np.ascontiguousarray(cvo.T[KR.col_map(nat.skip_head, R, cvo.shape[1])])
        probes, _ = IR.probe_sets(cent, q, 2)
        assert all(np.isin(assign[i1[r]], probes[r]).all() for r in range(R)), c
    assert e1.index_nprobe() == 2 and e1.retrieval_recoveries() == 0
    del nat
    e1.close(); e2.close()


# ---- 5b. non-finite queries ----
def test_non_finite_queries_are_contained(eng):
    # stream 1 asks with a NaN in every query, stream 2 with an Inf: no list is probed, the hits are -1 / +inf, the frames keep their raw features (the flat search
    # writes (1 - rate) x there: DESIGN.md section 15), and the other streams come out as if the two were ordinary
    case, cent, assign = IR.build_case("gaussian", 1023, 4, 17)
    eng.load(case.index, cent, assign, 3)
    clean = eng.run(KR.to_cv(case.q, case.T + 5), case.skip_head, case.R, case.T)
    case.q[1, :, 5] = np.nan
    case.q[2, :, 7] = np.inf
    cv = KR.to_cv(case.q, case.T + 5)
    res = eng.run(cv, case.skip_head, case.R, case.T)
    assert res["kernel"] == "knn_ivf"
    assert (res["idx"][1:3] == -1).all() and np.isposinf(res["dist"][1:3]).all()
    cols = KR.col_map(case.skip_head, case.R, case.T)
    for b in (1, 2):
        raw = case.q[b, cols].T                                       # [dim][R]
        got = res["phone"][b, :, :case.R]
        assert np.array_equal(got, raw, equal_nan=True) and same_bits(got[np.isfinite(raw)], raw[np.isfinite(raw)]), b
    for k in ("idx", "dist", "phone"):
        assert same_bits(res[k][[0, 3]].view(np.float32), clean[k][[0, 3]].view(np.float32)), k
    assert same_bits(res["phone"][:, :, case.R:], res["phone_in"][:, :, case.R:]) and np.array_equal(res["cv"], cv, equal_nan=True)
    # the flat search on the same engine: the same hits, another feature for these frames
    assert eng.nprobe(0) == 0
    flat = eng.run(cv, case.skip_head, case.R, case.T)
    assert (flat["idx"][1:3] == -1).all()
    fin = np.isfinite(case.q[2, cols].T)
    assert same_bits(flat["phone"][2, :, :case.R][fin], (np.float32(1.0 - np.float32(0.75)) * case.q[2, cols].T)[fin])


# ---- 6. errors ----
def test_errors_and_lifetime():
    e = Engine()
    case, cent, assign = IR.build_case("gaussian", 1023, 1, 1)

    def shape(rc):
        assert rc == RVC_SHAPE and e.h.last_error(), (rc, e.h.last_error())

    shape(e.attach(cent, assign))                                        # no index loaded
    shape(e.nprobe(1))
    e.load(case.index)
    shape(e.nprobe(1))                                                   # no structure attached
    shape(e.info()[0])
    shape(e.attach(cent[:, :47], assign))                                # dim
    shape(e.attach(cent, assign[:-1]))                                   # n
    shape(e.attach(cent, assign, nlist=0))
    big = np.zeros((65537, 48), np.float32)
    shape(e.attach(big, assign))                                         # nlist above 65 536
    bad = assign.copy(); bad[17] = IR.NLIST
    shape(e.attach(cent, bad))
    bad[17] = -1
    shape(e.attach(cent, bad))
    for v in (np.nan, np.inf):
        c2 = cent.copy(); c2[3, 5] = v
        shape(e.attach(c2, assign))
    assert not e.L.rvc_debug_index_layouts(e.h.h) & 4
    assert e.attach(cent, assign) == 0 and e.L.rvc_debug_index_layouts(e.h.h) & 4
    shape(e.nprobe(-1)); shape(e.nprobe(65))
    assert e.nprobe(3) == 0 and e.L.rvc_index_nprobe(e.h.h) == 3
    e.load(case.index)                                                   # a new index drops the structure
    assert e.L.rvc_index_nprobe(e.h.h) == 0 and not e.L.rvc_debug_index_layouts(e.h.h) & 4
    e.close()
