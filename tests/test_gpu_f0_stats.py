"""f0_select_kernel (obs_rvc_amd/csrc/f0_select.hip.h) through rvc_f0_stats and rvc_f0_stats_stream against the numpy definition of
tests/f0_stats_ref.py, bit for bit: every size around the vector width, the wave, the one-workgroup launch's 1024 rows, and 70 001 rows -- 18 workgroups per
pass, one launch per digit pass -- on every kind of input; a stream's pitch cache after two batched chunks; every refusal."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import f0_stats_ref as S
from common import BASELINE_160MS as g, voice_signal, zoo
from obs_rvc_amd.rvc import RvcInfer
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu

_FP, _DP = C.POINTER(C.c_float), C.POINTER(C.c_double)
SIZES = [1, 2, 63, 64, 65, 1023, 1024, 1025, 70001]
EIGHT = (0.0, 0.05, 0.5, 0.95, 1.0, 0.25, 0.75, 0.5)          # nq = 8: the five of the definition's tests, two more, and one of them twice


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.fixture(scope="module")
def bare():
    e = RvcInfer(zoo("tiny")["data"])
    yield e
    e.close()


@pytest.mark.parametrize("n", SIZES)
def test_select_is_the_definition(bare, n):
    for name, x in S.select_inputs(n).items():
        for q in (S.QUANTILES, EIGHT, (0.5,)):
            want, v = S.select(x, q)
            got, gv = bare.f0_stats(x, q)
            assert gv == v, (name, n, gv, v)
            assert same_bits(got, want), (name, n, q, got, want)
            if v:          # an element of the input, bit for bit
                assert all(np.any(x.view(np.uint32) == b) for b in got.view(np.uint32)), (name, n)


def test_select_crosses_every_digit_pass(bare):
    # rows that agree in the first one, two and three digits of their bit patterns: the answer is decided in the last pass a pair differs in
    base = np.float32(261.6256).view(np.uint32)
    for n in (1024, 70001):
        r = np.random.default_rng(n)
        for low_bits in (8, 16, 24):
            keys = (base & np.uint32(~((1 << low_bits) - 1) & 0xFFFFFFFF)) | r.integers(0, 1 << low_bits, n, dtype=np.uint32)
            x = keys.astype(np.uint32).view(np.float32)
            assert np.all(np.isfinite(x) & (x > 0))
            want, v = S.select(x, EIGHT)
            got, gv = bare.f0_stats(x, EIGHT)
            assert gv == v == n and same_bits(got, want), (n, low_bits)


def test_stats_of_a_stream_are_its_pitch_cache():
    z = zoo("tiny")
    e = RvcInfer(z["data"])
    e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method("rmvpe"); e.set_streams(3); e.set_noise_seed(1234, 0)
    L, R = g.input_buffer_16k_size, g.model_return_length
    for c in range(2):
        x = np.stack([voice_signal(L, seed=10 * c + s + 1) for s in range(3)])
        e.infer_batch(x, g.sample_frame_16k, (12, 0, -12), g.skip_head, R)
    for s in (0, 2):
        cache = e.pitch_cache(s)
        want, v = S.select(cache, S.QUANTILES)
        got, gv = e.f0_stats_stream(s, S.QUANTILES)
        assert v > 0 and gv == v and same_bits(got, want), s
    assert not same_bits(e.f0_stats_stream(0)[0], e.f0_stats_stream(2)[0])          # (an octave up against an octave down)
    with pytest.raises(RvcInferError):
        e.f0_stats_stream(3)
    with pytest.raises(RvcInferError):
        e.f0_stats_stream(-1)
    e.close()


def test_refusals(bare):
    L, h = bare._L, bare._h
    x = np.float32([100.0, 200.0])
    out, v = np.zeros(8, np.float32), C.c_size_t()
    call = lambda n, q: L.rvc_f0_stats(h, x.ctypes.data_as(_FP), n, np.float64(q).ctypes.data_as(_DP), len(q), out.ctypes.data_as(_FP), C.byref(v))
    assert call(2, [0.5]) == 0 and out[0] == 100.0 and v.value == 2
    assert call(0, [0.5]) == 5                                        # no rows
    assert call((1 << 30) + 1, [0.5]) == 5                            # (refused before anything is read)
    assert call(2, []) == 5 and call(2, [0.5] * 9) == 5               # nq outside 1..8
    for q in (-0.01, 1.01, np.nan, np.inf):
        assert call(2, [0.5, q]) == 5, q
    assert b"f0_stats" in L.rvc_last_error_message(h)
    assert L.rvc_f0_stats_stream(h, 1, np.float64([0.5]).ctypes.data_as(_DP), 1, out.ctypes.data_as(_FP), C.byref(v)) == 5          # one stream: 1 is none
    assert L.rvc_f0_stats_stream(h, 0, np.float64([2.0]).ctypes.data_as(_DP), 1, out.ctypes.data_as(_FP), C.byref(v)) == 5
    got, v0 = bare.f0_stats_stream(0)                                 # a fresh engine's cache: nothing voiced
    assert v0 == 0 and got[0] == 0.0
    with pytest.raises(RvcInferError):
        bare.f0_stats(x, [0.5] * 9)
