"""The k-means training of an IVF structure (obs_rvc_amd/csrc/kmeans.hip.h, retrieval.hip rvc_train_index_ivf) against tests/kmeans_ref.py:
one assign + update step through rvc_debug_kmeans_step on the centroids of the reference trajectory, then the public call, the structure it attaches, and the
Python layer on the tiny preset.  Bounds (derived in kmeans_ref.py, gamma = (dim + 2) 2^-24): the chosen list's float64 distance within (1 + 2 gamma) of the
float64 minimum; assign equal to the reference on rows that are not ambiguous; dist within gamma D; objective within gamma relative; centroids within 1 fp32 ulp
of fp32(mean64).  The cases were proven fair by tests/test_kmeans_ref.py.  Every check prints its largest ratio to the bound before it asserts.  A HIP error ends
the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import ivf_ref as IR
import kmeans_ref as M
import knn_ref as KR
from debug_abi import RVC_SHAPE, Handle, RetrievalSpec, ptr, same_bits

pytestmark = pytest.mark.gpu

SZ = C.c_size_t
PH_FILL = np.float32(-5.0e3)


class Engine:
    """a bare engine with an index"""

    def __init__(self):
        self.h = Handle()
        self.L = L = self.h.L
        vp = C.c_void_p
        L.rvc_debug_kmeans_step.argtypes = [vp, vp, SZ, vp, vp, vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_longlong)]
        L.rvc_train_index_ivf.argtypes = [vp, SZ, C.c_int, vp, C.c_uint32]
        L.rvc_index_ivf_train_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(SZ), C.POINTER(C.c_double), SZ, C.POINTER(SZ), C.POINTER(C.c_double)]
        L.rvc_get_index_ivf.argtypes = [vp, vp, SZ, vp, SZ]
        L.rvc_set_index_ivf.argtypes = [vp, vp, SZ, SZ, vp, SZ]
        L.rvc_set_index_nprobe.argtypes = [vp, C.c_int]
        L.rvc_index_nprobe.argtypes = [vp]
        L.rvc_index_ivf_info.argtypes = [vp, C.POINTER(SZ), C.POINTER(SZ), C.POINTER(SZ)]

    def ok(self, rc, want=0):
        if rc != want and "hip" in self.h.last_error().lower():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % self.h.last_error(), returncode=3)
        assert rc == want, (rc, self.h.last_error())

    def load(self, index):
        self.index = np.ascontiguousarray(index, np.float32)
        self.ok(self.L.rvc_load_index(self.h.h, ptr(self.index), self.index.shape[0], self.index.shape[1]))

    def step(self, cent, prev=None):
        cent = np.ascontiguousarray(cent, np.float32)
        n = self.index.shape[0]
        a, d, c = np.full(n, -7, np.int32), np.full(n, -7.0, np.float32), np.full(cent.shape, -7.0, np.float32)
        J, mv = C.c_double(-7.0), C.c_longlong(-7)
        pv = None if prev is None else np.ascontiguousarray(prev, np.int32)
        self.ok(self.L.rvc_debug_kmeans_step(self.h.h, ptr(cent), cent.shape[0], ptr(pv), ptr(a), ptr(d), ptr(c), C.byref(J), C.byref(mv)))
        return dict(assign=a, dist=d, cent=c, J=J.value, moved=mv.value)

    def train(self, nlist, iters, init=None, seed=0, want=0):
        init = None if init is None else np.ascontiguousarray(init, np.int32)
        self.ok(self.L.rvc_train_index_ivf(self.h.h, nlist, iters, ptr(init), seed), want)

    def train_info(self):
        it, mv, no = C.c_int(), SZ(), SZ()
        obj, ms = (C.c_double * 101)(), (C.c_double * 3)()
        self.ok(self.L.rvc_index_ivf_train_info(self.h.h, C.byref(it), C.byref(mv), obj, 101, C.byref(no), ms))
        return it.value, mv.value, [obj[i] for i in range(no.value)], list(ms)

    def info(self):
        a, b, c = SZ(), SZ(), SZ()
        rc = self.L.rvc_index_ivf_info(self.h.h, C.byref(a), C.byref(b), C.byref(c))
        return rc, a.value, b.value, c.value

    def get(self, nlist):
        n, dim = self.index.shape
        cent, assign = np.full((nlist, dim), -7.0, np.float32), np.full(n, -7, np.int32)
        self.ok(self.L.rvc_get_index_ivf(self.h.h, ptr(cent), cent.size, ptr(assign), n))
        return cent, assign

    def attach(self, cent, assign):
        cent, assign = np.ascontiguousarray(cent, np.float32), np.ascontiguousarray(assign, np.int32)
        self.ok(self.L.rvc_set_index_ivf(self.h.h, ptr(cent), cent.shape[0], cent.shape[1], ptr(assign), assign.shape[0]))

    def nprobe(self, k):
        self.ok(self.L.rvc_set_index_nprobe(self.h.h, k))

    def layouts(self):
        return self.L.rvc_debug_index_layouts(self.h.h)

    def search(self, q, skip_head, R, T, rate=0.75):
        """q [B][T][dim] -> idx, dist, phone of rvc_debug_retrieval"""
        cv = KR.to_cv(np.ascontiguousarray(q, np.float32), T + 5)
        B, dim, cv_ld = cv.shape
        phone = np.full((B, dim, R + 3), PH_FILL, np.float32)
        idx, dist, ovf = np.full((B, R, 4), -7, np.int32), np.full((B, R, 4), -7.0, np.float32), np.full(B, -7, np.int32)
        s = RetrievalSpec(streams=B, C=dim, T=T, cv_ld=cv_ld, skip_head=skip_head, R=R, ph_ld=R + 3, rate=rate, path=0, reps=1, graph=0)
        self.ok(self.L.rvc_debug_retrieval(self.h.h, C.byref(s), ptr(cv), ptr(phone), ptr(idx), ptr(dist), ptr(ovf)))
        return dict(idx=idx, dist=dist, phone=phone, kernel=self.h.last_kernel())

    def close(self):
        self.h.close()


@pytest.fixture(scope="module")
def eng():
    e = Engine()
    yield e
    e.close()


def ulps(got, ref):
    """|got - ref| in units of ref's fp32 spacing"""
    ref = np.asarray(ref, np.float32)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.maximum(np.abs(ref), np.float32(1e-30))).astype(np.float64)


def check_step(tag, index, cent, prev, res, ref_assign):
    n, dim = index.shape
    nlist = len(cent)
    g = KR.gamma(dim)
    D = M.distances(index, cent)
    a = res["assign"]
    assert a.min() >= 0 and a.max() < nlist
    chosen, best = D[np.arange(n), a], D.min(axis=1)
    r_min = float(np.max((chosen - best) / (2 * g * best + 1e-300)))
    clear = ~M.ambiguous_rows(index, cent)
    r_dist = float(np.max(np.abs(res["dist"].astype(np.float64) - chosen) / (g * chosen + 1e-300)))
    J64 = float(chosen.sum())
    r_obj = abs(res["J"] - J64) / (g * J64)
    want_moved = n if prev is None else int((a != prev).sum())
    mean = M.means(index, a, cent)
    u = ulps(res["cent"], mean)
    print("%s: chosen list %.3f of 2 gamma D over the minimum, dist %.3f of gamma D, objective %.3f of gamma J, centroids %.2f ulp, %d rows not clear, moved %d" %
          (tag, r_min, r_dist, r_obj, float(u.max()), int((~clear).sum()), res["moved"]))
    assert np.all(chosen <= (1 + 2 * g) * best), tag
    assert np.array_equal(a[clear], ref_assign[clear]), (tag, np.flatnonzero(clear & (a != ref_assign))[:8])
    assert np.all(np.abs(res["dist"].astype(np.float64) - chosen) <= g * chosen), tag
    assert res["moved"] == want_moved, (tag, res["moved"], want_moved)
    assert np.all(u <= 1.0), (tag, float(u.max()))
    empty = np.bincount(a, minlength=nlist) == 0
    assert same_bits(res["cent"][empty], np.ascontiguousarray(cent, np.float32)[empty]), (tag, "an empty list's centroid changed")
    assert r_obj <= 1.0, (tag, res["J"], J64)
    return int(empty.sum())


# ---- 1. one assign + update step on the reference trajectory's centroids ----
STEP_PARAMS = [("traj", "gaussian", (0, 3, 6)), ("traj", "offset3", (0, 1, 6)), ("traj", "blobs", (0, 1))] + [("step", n, (0, 1, 2)) for n in M.STEP_CASES]


@pytest.mark.parametrize("kind,name,steps", STEP_PARAMS)
def test_one_step_against_float64(eng, kind, name, steps):
    index, nlist, init, ref = M.reference(kind, name)
    eng.load(index)
    for s in steps:
        cent = ref["cents"][s]
        prev = None if s == 0 else ref["assigns"][s - 1]
        res = eng.step(cent, prev)
        check_step("%s step %d" % (name, s), index, cent, prev, res, ref["assigns"][s])
        again = eng.step(cent, prev)
        for k in ("assign", "dist", "cent"):
            assert same_bits(again[k].view(np.float32), res[k].view(np.float32)), (name, s, k)
        assert again["J"] == res["J"] and again["moved"] == res["moved"]
    assert not eng.layouts() & 4                                    # nothing was attached


def test_empty_lists_and_identical_centroids(eng):
    # the blobs with a random init: two lists are empty from the second assign step on, and their centroids come back with the bits that went in
    index, nlist, init, ref = M.reference("empty", "blobs")
    eng.load(index)
    for s in (1, 2):
        res = eng.step(ref["cents"][s], ref["assigns"][s - 1])
        assert check_step("blobs, random init, step %d" % s, index, ref["cents"][s], ref["assigns"][s - 1], res, ref["assigns"][s]) == 2
    # two bit-identical centroids: the lower list takes every tied row, the higher one is empty and keeps its bits
    index, nlist, init, ref = M.reference("traj", "gaussian")
    eng.load(index)
    cent = ref["cents"][1].copy()
    cent[5] = cent[4]
    a64 = M.assign_step(index, cent)[0]
    res = eng.step(cent)
    check_step("gaussian, lists 4 = 5", index, cent, None, res, a64)
    assert (a64 == 4).sum() > 0 and not (res["assign"] == 5).any() and same_bits(res["cent"][5], cent[5])


# ---- 2. the public call ----
@pytest.mark.parametrize("name", M.TRAJECTORY)
@pytest.mark.parametrize("iters", [0, 1, 6])
def test_training_follows_the_reference(eng, name, iters):
    index, nlist, init, ref = M.reference("traj", name)
    run = min(iters, ref["iters_run"])
    eng.load(index)
    eng.train(nlist, iters, init)
    it, moved, obj, ms = eng.train_info()
    cent, assign = eng.get(nlist)
    g = KR.gamma(index.shape[1])
    J = np.array(ref["objective"][:run + 1])
    u = ulps(cent, ref["cents"][run])
    r_obj = float(np.max(np.abs(np.array(obj[:len(J)]) - J) / (g * J))) if len(obj) >= len(J) else np.inf
    print("%s iters %d: ran %d, moved %d, centroids %.2f ulp, objectives %.3f of gamma J, ms %s" % (name, iters, it, moved, float(u.max()), r_obj, ms))
    assert it == run and moved == ref["moved"][run] and len(obj) == run + 1
    assert np.array_equal(assign, ref["assigns"][run])
    assert np.all(u <= 1.0)
    assert r_obj <= 1.0
    assert np.all(np.diff(obj) <= 1e-6 * np.array(obj[:-1]))
    assert ms[2] >= ms[0] > 0 and (ms[1] > 0) == (run > 0)
    # attachment: the structure is reported, and the search is flat until a probe count is set
    sizes = np.bincount(assign, minlength=nlist)
    assert eng.info() == (0, nlist, int(sizes.max()), int((sizes == 0).sum())) and eng.layouts() & 4 and eng.L.rvc_index_nprobe(eng.h.h) == 0


def test_early_stop(eng):
    index, nlist, init, ref = M.reference("traj", "blobs")
    eng.load(index)
    eng.train(nlist, 10, init)
    it, moved, obj, _ = eng.train_info()
    assert (it, moved, len(obj)) == (1, 0, 2)


def _case(streams, nq):
    case = KR.make_case("gaussian", dim=48, n=1023, streams=streams, nq=nq, seed=M.SEED)
    assert same_bits(case.index, M.case_index("gaussian", 1023))          # (the index of a case does not depend on its queries)
    return case


def test_trained_structure_searches_like_an_attached_one(eng):
    index, nlist, init, ref = M.reference("traj", "gaussian")
    eng.load(index)
    eng.train(nlist, M.TRAJ_ITERS, init)
    cent, assign = eng.get(nlist)
    other = Engine()
    other.load(index)
    other.attach(cent, assign)
    for streams in (1, 3):
        case = _case(streams, 17)
        for k in (1, 3):
            eng.nprobe(k); other.nprobe(k)
            a, b = eng.search(case.q, case.skip_head, case.R, case.T), other.search(case.q, case.skip_head, case.R, case.T)
            assert a["kernel"] == b["kernel"] == "knn_ivf"
            for key in ("idx", "dist", "phone"):
                assert same_bits(a[key].view(np.float32), b[key].view(np.float32)), (streams, k, key)
    other.close()
    # full probe = the flat search, bit for bit
    case = _case(3, 17)
    eng.nprobe(0)
    flat = eng.search(case.q, case.skip_head, case.R, case.T)
    eng.nprobe(64)
    assert eng.L.rvc_index_nprobe(eng.h.h) == nlist
    full = eng.search(case.q, case.skip_head, case.R, case.T)
    assert flat["kernel"] == "knn_fused" and full["kernel"] == "knn_ivf"
    for key in ("idx", "dist", "phone"):
        assert same_bits(full[key].view(np.float32), flat[key].view(np.float32)), key
    # self-retrieval: every row as a query finds itself in the one list it probes, at distance exactly 0 (31 streams x 33 raw frames = the 1 023 rows)
    eng.nprobe(1)
    skip, R, T = KR.GEOMS[33]
    res = eng.search(index.reshape(31, 33, 48), skip, R, T)
    rows = np.arange(1023).reshape(31, 33)[:, KR.col_map(skip, R, T)]
    assert np.all(res["dist"][:, :, 0] == 0.0) and np.array_equal(res["idx"][:, :, 0], rows)


def test_training_is_deterministic_and_defaults(eng):
    index = M.case_index("gaussian", 4099)
    eng.load(index)
    nlist = M.default_nlist(4099)
    eng.train(0, 3, None, seed=11)
    first = eng.get(nlist) + (eng.train_info()[:3],)
    assert eng.info()[1] == nlist == 105
    eng.train(0, 3, None, seed=11)
    second = eng.get(nlist) + (eng.train_info()[:3],)
    assert same_bits(first[0], second[0]) and np.array_equal(first[1], second[1]) and first[2] == second[2]
    # the seeded sample is kmeans_ref's: the same training with the rows spelt out
    eng.train(nlist, 3, M.seeded_rows(4099, nlist, 11))
    third = eng.get(nlist) + (eng.train_info()[:3],)
    assert same_bits(first[0], third[0]) and np.array_equal(first[1], third[1]) and first[2] == third[2]
    eng.train(nlist, 0, None, seed=12)
    assert same_bits(eng.get(nlist)[0], index[M.seeded_rows(4099, nlist, 12)])


# ---- 3. errors, replacement, lifetime ----
def test_errors_keep_the_structure():
    e = Engine()
    e.train(4, 1, want=RVC_SHAPE)                                    # no index loaded
    assert "no index" in e.h.last_error()
    index, nlist, init, ref = M.reference("traj", "gaussian")
    case = _case(3, 17)
    e.load(index)
    it = C.c_int()
    assert e.L.rvc_index_ivf_train_info(e.h.h, C.byref(it), None, None, 0, None, None) == RVC_SHAPE       # nothing trained yet
    assert e.L.rvc_get_index_ivf(e.h.h, None, 0, None, 0) == RVC_SHAPE                                    # nothing attached
    e.train(nlist, 2, init)
    e.nprobe(2)
    kept = e.get(nlist)
    base = e.search(case.q, case.skip_head, case.R, case.T)

    def refused(msg, *args, **kw):
        e.train(*args, want=RVC_SHAPE, **kw)
        assert msg in e.h.last_error(), e.h.last_error()
        assert e.L.rvc_index_nprobe(e.h.h) == 2 and e.layouts() & 4
        now = e.search(case.q, case.skip_head, case.R, case.T)
        assert all(same_bits(now[k].view(np.float32), base[k].view(np.float32)) for k in ("idx", "dist", "phone")), msg

    refused("nlist", 1024, 1)
    refused("nlist", 65537, 1)
    refused("iters", nlist, -1, init)
    refused("iters", nlist, 101, init)
    bad = init.copy(); bad[7] = 1023
    refused("outside", nlist, 1, bad)
    bad[7] = -1
    refused("outside", nlist, 1, bad)
    bad[7] = bad[30]
    refused("twice", nlist, 1, bad)
    got = e.get(nlist)
    assert same_bits(got[0], kept[0]) and np.array_equal(got[1], kept[1])
    small = np.zeros((3, 48), np.float32)
    assert e.L.rvc_get_index_ivf(e.h.h, ptr(small), small.size, ptr(got[1]), 1023) == RVC_SHAPE          # a short capacity
    assert e.L.rvc_get_index_ivf(e.h.h, ptr(got[0]), got[0].size, ptr(got[1]), 1022) == RVC_SHAPE
    # a non-finite row: the first one is named, and a structure set by hand stays
    for value, row in ((np.nan, 77), (np.inf, 500)):
        dirty = index.copy()
        dirty[row, 5] = value
        dirty[900, 0] = -np.inf
        e.load(dirty)
        e.attach(kept[0], kept[1])
        e.nprobe(2)
        base = e.search(case.q, case.skip_head, case.R, case.T)
        refused("row %d " % row, nlist, 1, init)
    # a finite row whose norm overflows is no such row: its distances compare as +inf, and it goes to list 0
    huge = index.copy()
    huge[300] = np.float32(3e19)
    free = init[init != 300]
    e.load(huge)
    e.train(len(free), 0, free)
    assert e.get(len(free))[1][300] == 0
    e.close()


def test_replacement_and_lifetime(eng):
    index, nlist, init, ref = M.reference("traj", "gaussian")
    eng.load(index)
    eng.train(nlist, 1, init)
    eng.nprobe(3)
    assert eng.info()[1] == nlist and eng.L.rvc_index_nprobe(eng.h.h) == 3
    eng.train(5, 1, None, seed=1)                                    # a second training replaces the first, and the search is flat again
    assert eng.info()[1] == 5 and eng.L.rvc_index_nprobe(eng.h.h) == 0 and eng.get(5)[1].max() == 4
    eng.load(index)                                                  # a new index drops it
    assert not eng.layouts() & 4 and eng.L.rvc_index_nprobe(eng.h.h) == 0 and eng.info()[0] == RVC_SHAPE


# ---- 4. the Python layer on the tiny preset ----
def _full_engine(streams):
    from common import zoo
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method("yin")
    if streams > 1:
        e.set_streams(streams)
        e.set_protect(0.33)                                          # (the plans with the protection stage tap every stream's ContentVec output: "cv.out_all")
    e.set_noise_seed(1234, 0)
    return e


@pytest.mark.parametrize("streams", [1, 3])
def test_python_train_save_load(streams, tmp_path):
    from common import BASELINE_160MS as g, voice_signal
    from obs_rvc_amd import weights as W
    from obs_rvc_amd.rvc_common import RvcInferError
    index = W.make_index(3000, 48, seed=5)
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=3 + s) for s in range(streams)])
    R, skip = g.model_return_length, g.skip_head

    def run(e):
        e.reset_state(); e.set_noise_seed(1234, 0)
        y = e.infer_batch(xs, g.sample_frame_16k, [12, 0, -12][:streams], skip, R) if streams > 1 else e.infer(xs[0], g.sample_frame_16k, 12, skip, R)
        return np.array(y), e.knn()

    e = _full_engine(streams)
    e.set_index_rate(0.75); e.enable_taps(2)
    with pytest.raises(RvcInferError) as ei:                         # the default: refused as before, nothing loaded
        e.load_index(index, nprobe=2)
    assert ei.value.code == RVC_SHAPE and e.index_device_ptr()[1] == 0
    e.load_index(index, nprobe=2, train=dict(iters=4, seed=9))
    info = e.index_ivf_train_info()
    assert e.index_nprobe() == 2 and info["nlist"] == M.default_nlist(3000) == 76 and 1 <= info["iters_run"] <= 4 and len(info["objective"]) == info["iters_run"] + 1
    cent, assign = e.index_ivf()
    assert cent.shape == (76, 48) and assign.shape == (3000,) and np.array_equal(np.bincount(assign, minlength=76).max(), info["longest_list"])
    y0, (idx, dist) = run(e)
    assert idx.shape == (streams * R, 4)
    cvo = (e.tap("cv.out_all") if streams > 1 else e.tap("cv.out")).reshape(streams, 48, -1)
    cols = KR.col_map(skip, R, cvo.shape[2])
    gm = KR.gamma(48)
    for b in range(streams):
        q = np.ascontiguousarray(cvo[b].T[cols])
        ri, rd, _, _ = IR.search(index, cent, assign, q, 2)
        assert (ri >= 0).all() and np.all(np.abs(dist[b * R:(b + 1) * R] - rd) <= gm * rd), b
        clear = np.array([IR.ambiguous_queries(index, cent, assign, q[r:r + 1], 2) == 0 for r in range(R)])
        print("stream %d: %d of %d queries clear of a 4 gamma tie" % (b, int(clear.sum()), R))
        assert np.array_equal(idx[b * R:(b + 1) * R][clear], ri[clear]), b
    # export: the file upstream's Faiss reads, and a fresh engine that loads it finds the same hits
    path = str(tmp_path / "trained.index")
    e.save_index(path)
    from obs_rvc_amd import faiss_index as F
    v, c2, a2, k = F.read_index_ivf(path, with_nprobe=True)
    assert k == 2 and same_bits(v, index) and same_bits(c2, cent) and np.array_equal(a2, assign)
    e.close()
    f = _full_engine(streams)
    f.set_index_rate(0.75)
    f.load_index(path, nprobe="file")
    assert f.index_nprobe() == 2
    y1, (idx1, dist1) = run(f)
    assert np.array_equal(idx1, idx) and same_bits(dist1, dist) and same_bits(np.ascontiguousarray(y1, np.float32), np.ascontiguousarray(y0, np.float32))
    # a flat file when nothing is attached
    f.load_index(index)
    f.save_index(str(tmp_path / "flat.index"))
    assert F.read_index_ivf(str(tmp_path / "flat.index"))[1] is None and same_bits(F.read_index(str(tmp_path / "flat.index")), index)
    f.close()
