"""Upstream's k = 8 through the public path (RvcInfer.set_index_k) on the tiny preset with a seeded index and index rate 0.75: the hits of
get_knn() are (R, 8), start with a k = 4 engine's hits on the same input and equal oracle.knn_search of the tapped ContentVec rows at 8; the audio differs
from the k = 4 audio and is finite; the same for stream 1 of a two-stream batch; one chunk through the native streaming session; k is part of a plan's
identity (rvc_plan_cache_info counts the builds)."""
from __future__ import annotations

import numpy as np
import pytest

import knn_ref as KR
from debug_abi import same_bits

pytestmark = pytest.mark.gpu


def _engine(streams=1, k=None):
    from common import zoo
    from obs_rvc_amd import weights as W
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_f0(); e.load_model(z["model"])
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(1234, 0)
    index = W.make_index(3000, 48, seed=5)
    e.load_index(index, k=k); e.set_index_rate(0.75); e.enable_taps(2)
    return e, index


@pytest.mark.parametrize("streams", [1, 2])
def test_public_path(streams):
    from common import BASELINE_160MS as g, voice_signal
    from oracle import oracle as O
    e8, index = _engine(streams)
    e4, _ = _engine(streams)
    assert e8.index_k() == 4
    e8.set_index_k(8)
    assert e8.index_k() == 8 and e4.index_k() == 4
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=3 + s) for s in range(streams)])
    R, skip = g.model_return_length, g.skip_head

    def run(e):
        e.reset_state(); e.set_noise_seed(1234, 0)
        if streams > 1:
            return np.array(e.infer_batch(xs, g.sample_frame_16k, [12, 0][:streams], skip, R))
        return np.array(e.infer(xs[0], g.sample_frame_16k, 12, skip, R))

    if streams > 1:
        e8.set_protect(0.33); e4.set_protect(0.33)                      # (plans with the protection stage tap every stream's ContentVec output)
    y8, y4 = run(e8), run(e4)
    (i8, d8), (i4, d4) = e8.get_knn(), e4.get_knn()
    assert i8.shape == d8.shape == (streams * R, 8) and i4.shape == (streams * R, 4)
    assert np.array_equal(i8[:, :4], i4) and same_bits(np.ascontiguousarray(d8[:, :4]), d4)
    cvo = (e8.tap("cv.out_all") if streams > 1 else e8.tap("cv.out")).reshape(streams, 48, -1)
    cols = KR.col_map(skip, R, cvo.shape[2])
    for b in range(streams):
        q = np.ascontiguousarray(cvo[b].T[cols])
        io, do = O.knn_search(index, q, 8)
        assert np.array_equal(i8[b * R:(b + 1) * R], io) and same_bits(np.ascontiguousarray(d8[b * R:(b + 1) * R]), do), b
    assert np.isfinite(y8).all() and y8.shape == y4.shape and not np.array_equal(y8, y4)
    # k is part of a plan's identity: another k builds a plan, the first k finds its own again
    b0 = e8.plan_cache_info()["builds"]
    e8.set_index_k(4)
    y4b = run(e8)
    assert e8.plan_cache_info()["builds"] == b0 + 1 and e8.get_knn()[0].shape == (streams * R, 4)
    assert same_bits(np.ascontiguousarray(y4b, np.float32), np.ascontiguousarray(y4, np.float32))
    e8.set_index_k(8)
    y8b = run(e8)
    assert e8.plan_cache_info()["builds"] == b0 + 1 and same_bits(np.ascontiguousarray(y8b, np.float32), np.ascontiguousarray(y8, np.float32))
    # the setting is the caller's: a new index keeps it
    e8.load_index(index)
    assert e8.index_k() == 8
    e8.close(); e4.close()


def test_load_index_k_argument():
    from obs_rvc_amd.rvc_common import RvcInferError
    e, index = _engine(k="upstream")
    assert e.index_k() == 8
    e.load_index(index)                                                 # None leaves the engine's value
    assert e.index_k() == 8
    with pytest.raises(RvcInferError):
        e.load_index(index[:7], k=8)
    assert e.index_k() == 8 and e._index_dims()[0] == 3000             # refused: the engine keeps the index it had
    e.load_index(index[:7], k=4)
    assert e.index_k() == 4
    with pytest.raises(RvcInferError):
        e.set_index_k(8)
    with pytest.raises(RvcInferError):
        e.set_index_k(5)
    e.close()


def test_one_chunk_through_the_native_session():
    from common import voice_signal
    from obs_rvc_amd.streaming import NativeStreamingSession
    e, index = _engine(k="upstream")
    nat = NativeStreamingSession(e, 48000, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    F = 7680
    a = np.interp(np.arange(F) / 48000.0, np.arange(2560) / 16000.0, voice_signal(2560, seed=10)).astype(np.float32)
    out = nat.process_one_frame(a)
    i8, d8 = e.get_knn()
    assert i8.shape == (nat.model_return_length, 8) and (i8 >= 0).all() and np.all(d8[:, 1:] >= d8[:, :-1]) and np.isfinite(np.asarray(out)).all()
    e.close()
