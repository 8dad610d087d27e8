"""The index builder (obs_rvc_amd/csrc/index_build.hip.h, retrieval.hip rvc_index_build_*) on the tiny zoo: the rows of a build against
rvc_hubert's frames bit for bit, the append kernel alone with planted NaN / Inf rows, the installed index under retrieval against tests/knn_ref.py, the
k-means reduction against rvc_train_index_ivf and tests/kmeans_ref.py, serving while a build is open, the refusals, and RvcInfer.build_index end to end.
A HIP error ends the session: nothing more is started on the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import index_build_ref as B
import kmeans_ref as M
import knn_ref as KR
from common import BASELINE_160MS as g, voice_signal, zoo
from debug_abi import Handle, same_bits
from index_build_abi import RVC_CONTENTVEC_NOT_LOADED, RVC_SHAPE, device_to_host, index_append
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

WINDOW = 4000
DIMS = {2: 48, 1: 16}


def recording(n, seed, f=220.0):
    """seeded noise plus a sine"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / 16000.0
    return (0.1 * np.sin(2 * np.pi * f * t) + 0.02 * r.standard_normal(n)).astype(np.float32)


# three windows and a kept tail of 1 500 samples (4 frames); one window and a tail of 200 samples, dropped: 52 rows
RECS = [recording(3 * WINDOW + 1500, 41), recording(WINDOW + 200, 42, 330.0)]


def guard(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except RvcInferError as x:
        if "hip" in str(x).lower():
            pytest.exit("a HIP call failed (%s): nothing more is started on this device" % x, returncode=3)
        raise


def engine(version=2, full=False):
    z = zoo("tiny", version)
    e = RvcInfer(z["data"])
    e.load_contentvec(version)
    if full:
        e.load_model(z["model"]); e.load_f0_method("yin"); e.set_noise_seed(1234, 0)
    return e


def installed(e, dim):
    p, nbytes = e.index_device_ptr()
    return device_to_host(p, nbytes).reshape(-1, dim)


def infer(e):
    e.reset_state(); e.set_noise_seed(1234, 0)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    return np.array(guard(e.infer, x, g.sample_frame_16k, 12, g.skip_head, g.model_return_length))


_BUILT = {}


def built(version):
    """test 1's build, once per version and shared: (engine with the build installed, rvc_hubert's rows computed before begin, what add returned, info)"""
    if version not in _BUILT:
        e = engine(version, full=version == 2)
        want = B.rows_of(RECS, WINDOW, e.hubert)                    # rvc_hubert in the same process, before begin: the yardstick
        guard(e.index_build_begin, WINDOW, 16)
        added = [guard(e.index_build_add, x) for x in RECS]
        info = e.index_build_info()
        n = guard(e.index_build_finish, 1 << 40)
        _BUILT[version] = (e, want, added, info, n)
    return _BUILT[version]


# ---- 1. rows equal rvc_hubert's, bit for bit ----
@pytest.mark.parametrize("version", [2, 1])
def test_rows_are_huberts_frames(version):
    e, want, added, info, n = built(version)
    dim = DIMS[version]
    assert want.shape == (52, dim) and added == [40, 12] and n == 52
    assert info["rows"] == 52 and info["windows"] == 5 and info["dropped_nonfinite"] == 0
    assert info["capacity"] == 64                                   # 16 -> 32 -> 64: grown twice
    assert info["ms_contentvec"] > 0 and info["ms_append"] > 0 and info["ms_reduce"] == 0
    got = installed(e, dim)
    assert got.shape == want.shape and np.array_equal(got, want) and same_bits(got, want)
    with pytest.raises(RvcInferError):                              # the build is closed
        e.index_build_info()


# ---- 2. the append kernel alone ----
@pytest.mark.parametrize("cursor", [0, 7])
@pytest.mark.parametrize("Cc,T,ld", [(33, 65, 72), (48, 12, 12), (16, 1, 8), (768, 149, 152)])
def test_append_kernel(Cc, T, ld, cursor):
    h = Handle()
    r = np.random.default_rng(1000 * Cc + T + cursor)
    cv = np.full((Cc, ld), 9.0e3, np.float32)
    cv[:, :T] = r.standard_normal((Cc, T), dtype=np.float32)
    bad = {0: [(0, np.nan)], T - 1: [(Cc - 1, np.inf)]}
    if T >= 3:
        bad[T // 2] = [(Cc // 3, np.nan), (Cc // 2, -np.inf)]
    for t, items in bad.items():
        for c, v in items:
            cv[c, t] = v
    head = r.standard_normal((cursor, Cc), dtype=np.float32)
    keep = np.array([t for t in range(T) if t not in bad], int)
    want = np.concatenate([head, np.ascontiguousarray(cv[:, :T].T)[keep]], axis=0)
    capacity = max(cursor, 1) + T // 2                              # below cursor + T: the append overflows it and the store grows (T = 1 at cursor 0 cannot: a store has a row)
    rc, rows, dropped = index_append(h.h, cv, T, cursor, capacity, head if cursor else None)
    if rc != 0 and "hip" in h.last_error().lower():
        pytest.exit("a HIP call failed (%s): nothing more is started on this device" % h.last_error(), returncode=3)
    assert rc == 0, h.last_error()
    assert dropped == len(bad) and rows.shape == want.shape
    assert same_bits(rows[:cursor], head)                           # rows before the cursor are untouched
    assert same_bits(rows, want)
    # a clean window: nothing dropped, nothing moved
    clean = np.where(np.isfinite(cv), cv, np.float32(1.0))
    rc, rows, dropped = index_append(h.h, clean, T, cursor, cursor + T, head if cursor else None)
    assert rc == 0 and dropped == 0 and same_bits(rows, np.concatenate([head, np.ascontiguousarray(clean[:, :T].T)], axis=0))
    h.close()


# ---- 3. the index is usable ----
def test_built_index_serves_retrieval():
    e, want, _, _, _ = built(2)
    index = installed(e, 48)
    e.set_index_rate(1.0); e.enable_taps(2)
    infer(e)
    idx, dist = e.knn()
    R, skip = g.model_return_length, g.skip_head
    assert idx.shape == (R, KR.K)
    cvo = e.tap("cv.out").reshape(48, -1)
    q = np.ascontiguousarray(cvo.T[KR.col_map(skip, R, cvo.shape[1])])
    d = KR.d64(index, q)
    ri, rd = KR.topk(d)
    gm = KR.gamma(48)
    ds = np.sort(d, axis=1)
    gap = (ds[:, 1:KR.K + 1] - ds[:, :KR.K]) / ds[:, 1:KR.K + 1]
    print("smallest relative gap among the first %d sorted distances: %.3e (4 gamma = %.3e); dist error %.3f of gamma D" %
          (KR.K + 1, gap.min(), 4 * gm, float(np.max(np.abs(dist - rd) / (gm * rd)))))
    assert gap.min() > 4 * gm                                       # the reference alone leaves no query undecided (checked with the CPU oracle's features: 1.2e-3)
    assert np.all(np.abs(dist - rd) <= gm * rd)
    assert np.array_equal(idx, ri)
    e.enable_taps(False); e.set_index_rate(0.0)


# ---- 4. reduction ----
def test_reduction_is_the_trainer():
    e = engine(2)
    recs = [recording(8 * WINDOW, 50 + i, 200.0 + 40 * i) for i in range(3)] + [recording(2 * WINDOW + 2640, 53, 150.0)]
    guard(e.index_build_begin, WINDOW, 0)
    assert sum(guard(e.index_build_add, x) for x in recs) == 320
    # the same 320 rows, read back from a build that keeps every row
    assert guard(e.index_build_finish, 1 << 40) == 320
    rows = installed(e, 48)
    assert rows.shape == (320, 48) and np.isfinite(rows).all()
    guard(e.index_build_begin, WINDOW, 0)
    for x in recs:
        guard(e.index_build_add, x)
    assert guard(e.index_build_finish, 100, 16, 10, 3) == 16
    got = installed(e, 48)
    assert got.shape == (16, 48)
    assert e.index_nprobe() == 0
    # the parent's path: the rows loaded on a second engine, trained, read back
    o = engine(2)
    o.load_index(rows)
    tinfo = guard(o.train_index_ivf, 16, 10, None, 3)
    cent, assign = o.index_ivf()
    assert same_bits(got, cent)
    # kmeans_ref, under the conditions tests/test_gpu_kmeans.py applies: the reference trajectory where no row is ambiguous at any step, and in any case the last
    # assign step's rules (chosen list within (1 + 2 gamma) of the minimum, equal to the float64 argmin on rows that are not ambiguous)
    init = M.seeded_rows(320, 16, 3)
    ref = M.train(rows, 16, 10, init)
    amb = [int(M.ambiguous_rows(rows, c).sum()) for c in ref["cents"]]
    run = ref["iters_run"]
    gm = KR.gamma(48)
    D = M.distances(rows, cent)
    chosen, best = D[np.arange(320), assign], D.min(axis=1)
    clear = ~M.ambiguous_rows(rows, cent)
    print("reference ran %d update steps, ambiguous rows per assign step %s; engine ran %d" % (run, amb, tinfo["iters_run"]))
    assert np.all(chosen <= (1 + 2 * gm) * best)
    assert np.array_equal(assign[clear], M.assign_step(rows, cent)[0][clear])
    if not any(amb):
        u = np.abs(cent.astype(np.float64) - ref["cents"][run].astype(np.float64)) / np.spacing(np.maximum(np.abs(ref["cents"][run]), np.float32(1e-30))).astype(np.float64)
        print("centroids within %.2f ulp of the reference trajectory" % float(u.max()))
        assert tinfo["iters_run"] == run and np.array_equal(assign, ref["assigns"][run]) and np.all(u <= 1.0)
    # deterministic bit for bit: the same build again
    guard(e.index_build_begin, WINDOW, 0)
    for x in recs:
        guard(e.index_build_add, x)
    guard(e.index_build_finish, 100, 16, 10, 3)
    assert same_bits(installed(e, 48), got)
    e.close(); o.close()


# ---- 5. serving while building ----
def test_serving_while_building():
    from obs_rvc_amd import weights as W
    e = engine(2, full=True)
    e.load_index(W.make_index(300, 48, seed=5))
    e.set_index_rate(1.0)
    y0 = infer(e)
    hits0 = e.knn()
    guard(e.index_build_begin, WINDOW, 16)
    assert guard(e.index_build_add, RECS[0]) == 40
    y1 = infer(e)
    hits1 = e.knn()
    assert np.array_equal(y1, y0) and np.array_equal(hits1[0], hits0[0]) and same_bits(hits1[1], hits0[1])
    assert e.index_build_info()["rows"] == 40 and e.index_device_ptr()[1] == 300 * 48 * 4
    assert guard(e.index_build_add, RECS[1]) == 12                 # the build goes on behind the call it served
    e.index_build_abort()
    assert np.array_equal(infer(e), y0)
    e.close()


# ---- 6. errors ----
def test_errors():
    z = zoo("tiny")
    e = RvcInfer(z["data"])

    def refused(code, msg, fn, *a):
        with pytest.raises(RvcInferError) as ei:
            fn(*a)
        assert ei.value.code == code and (msg in str(ei.value)), (code, msg, str(ei.value))

    with pytest.raises(RvcInferError) as ei:                        # no ContentVec
        e.index_build_begin(WINDOW, 0)
    assert ei.value.code == RVC_CONTENTVEC_NOT_LOADED and "ContentVec is not loaded" in str(ei.value)
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method("yin")
    refused(RVC_SHAPE, "no build is open", e.index_build_add, RECS[1])
    refused(RVC_SHAPE, "no build is open", e.index_build_finish, 0, 0)
    refused(RVC_SHAPE, "no build is open", e.index_build_info)
    refused(RVC_SHAPE, "too short", e.index_build_begin, 399, 0)   # a window the plan cannot be built for
    refused(RVC_SHAPE, "no build is open", e.index_build_info)
    e.index_build_begin(WINDOW, 0)
    refused(RVC_SHAPE, "already open", e.index_build_begin, WINDOW, 0)
    refused(RVC_SHAPE, "at least 4", e.index_build_finish, 0, 0)   # no rows yet
    assert e.index_build_add(recording(1040, 1)) == 3               # one run of 3 frames: still fewer than k
    refused(RVC_SHAPE, "at least 4", e.index_build_finish, 0, 0)
    assert e.index_build_info()["rows"] == 3                        # the build stayed open
    assert e.index_build_add(RECS[1]) == 12
    refused(RVC_SHAPE, "reduce_to", e.index_build_finish, 10, 16)  # reduce_to above the 15 rows held
    refused(RVC_SHAPE, "at least 4", e.index_build_finish, 10, 3)  # the reduced index would be below k
    refused(RVC_SHAPE, "iters", e.index_build_finish, 10, 8, 101)
    e.set_index_k(8)
    refused(RVC_SHAPE, "at least 8", e.index_build_finish, 10, 5)
    e.set_index_k(4)
    assert e.index_build_info()["rows"] == 15 and e.index_device_ptr()[1] == 0
    assert e.index_build_finish(0, 0) == 15
    # afterwards the engine still infers, with and without the index it has just built
    e.set_noise_seed(1234, 0)
    assert np.isfinite(infer(e)).all()
    e.set_index_rate(1.0)
    assert np.isfinite(infer(e)).all() and e.knn()[0].max() < 15
    # rvc_destroy aborts an open build
    e.index_build_begin(WINDOW, 0)
    e.index_build_add(RECS[1])
    e.close()


# ---- 7. RvcInfer.build_index end to end ----
def test_build_index_end_to_end(tmp_path):
    e = engine(2, full=True)
    e.set_streams(2)                                                # the builder uses its one-stream plan whatever the stream count
    recs = [recording(40000, 60), (recording(36000, 61, 180.0), 16000), (recording(64000, 62, 260.0), 32000)]
    info = guard(e.build_index, recs, window=WINDOW, iters=5, seed=9, train=True, nprobe=2)
    e.set_streams(1)
    n16 = len(e._to_16k(recs[2][0], 32000))
    want_rows = B.total_rows([40000, 36000, n16], WINDOW)
    assert abs(n16 - 32000) <= 400 and info["rows"] == info["index_rows"] == want_rows and info["dropped_nonfinite"] == 0
    assert e.index_nprobe() == 2 and info["ivf"]["nlist"] == M.default_nlist(want_rows)
    # the first two recordings' rows are rvc_hubert's
    v = e.index_vectors()
    head = B.rows_of([recs[0], recs[1][0]], WINDOW, e.hubert)
    assert v.shape == (want_rows, 48) and same_bits(v[: len(head)], head)
    cent, assign = e.index_ivf()
    path = str(tmp_path / "added.index")
    e.save_index(path)
    f = engine(2, full=True)
    f.load_index(path, nprobe="file")
    assert f.index_nprobe() == 2 and same_bits(f.index_vectors(), v)
    c2, a2 = f.index_ivf()
    assert same_bits(c2, cent) and np.array_equal(a2, assign)
    f.set_index_rate(0.75); e.set_index_rate(0.75)
    assert np.array_equal(infer(f), infer(e))
    e.close(); f.close()
