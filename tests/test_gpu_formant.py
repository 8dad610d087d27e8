"""Formant shift (the plugin's resonance shift) on the GPU: stage by stage against the definition (DESIGN.md "Formant shift"; the numpy
restatements of tests/test_formant.py), every entry point against single-stream runs, plan and graph behaviour, the native session."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from common import BASELINE_160MS as g, rel_rms, rms, voice_signal, zoo
from obs_rvc_amd import weights as W
from oracle import oracle as O
from test_formant import back_to_model_rate, geometry, interp

pytestmark = pytest.mark.gpu

PCM_TOL = 1e-3
R = g.model_return_length
SEED = (1234, 0)


def _engine(z, phi=None, streams=1, seed=SEED, taps=False):
    from obs_rvc_amd.rvc import RvcInfer
    e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_f0(); e.load_model(z["model"])
    if streams > 1:
        e.set_streams(streams)
    e.set_noise_seed(*seed)
    if phi is not None:
        e.set_formant_shift(phi)
    if taps:
        e.enable_taps(True)
    return e


def _coarse_pitch(f0):
    # get_f0_post, rvc/src/f0/mod.rs:7-12 (f32 arithmetic, round half away from zero)
    f0 = f0.astype(np.float32)
    mn, mx = np.float32(1127.0) * np.log(np.float32(1.0) + np.float32(50.0 / 700.0)), np.float32(1127.0) * np.log(np.float32(1.0) + np.float32(500.0 / 700.0))
    mel = np.float32(1127.0) * np.log(np.float32(1.0) + f0 / np.float32(700.0))
    mel = np.where(mel > 0, (mel - mn) * np.float32(254.0) / (mx - mn) + np.float32(1.0), mel)
    return np.floor(np.clip(mel, 1.0, 255.0) + 0.5).astype(np.int64)


def _nsf(f0, T, upp, sr, lin, noise):
    """oracle/rvc_oracle.c nsf_source restated in numpy (fp32, sequential phase)."""
    f32 = np.float32
    f0 = f0.astype(f32)
    N = T * upp
    rad = np.fmod(f0 / f32(sr), f32(1.0)).astype(f32)
    cum = (np.cumsum(rad, dtype=f32) * f32(upp)).astype(f32)
    i = np.arange(N)
    pos = (i.astype(f32) * f32(T - 1) / f32(N - 1)).astype(f32) if N > 1 else np.zeros(N, f32)
    i0 = np.minimum(np.floor(pos).astype(np.int64), T - 1)
    i1 = np.where(i0 + 1 < T, i0 + 1, T - 1)
    w = (pos - i0.astype(f32)).astype(f32)
    tmp = np.fmod(cum[i0] * (f32(1) - w) + cum[i1] * w, f32(1.0)).astype(f32)
    shift = np.zeros(N, f32)
    shift[1:] = np.where(tmp[1:] - tmp[:-1] < 0, f32(-1.0), f32(0.0))
    t = i // upp
    phase = np.cumsum((rad[t] + shift).astype(f32), dtype=f32)
    sine = np.sin(phase * f32(6.28318530717958647692)).astype(f32) * f32(0.1)
    uv = (f0[t] > 0).astype(f32)
    namp = uv * f32(0.003) + (f32(1) - uv) * f32(0.1) / f32(3)
    return np.tanh(f32(lin[0]) * (sine * uv + namp * noise) + f32(lin[1])).astype(f32)


def _stage_case(preset, synth_preset, phi):
    import torch_ref as TR
    z = zoo(preset, 2, synth_preset)
    cfg, tens = W.read_blob(z["model"])
    sr = int(cfg["sr"]); upp = sr // 100; I = int(cfg["inter"])
    R2, ures = geometry(R, sr, phi)
    eng = _engine(z, phi, taps=True)
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(*SEED)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    ye = eng.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    ora.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    assert ye.shape == (R * upp,)
    # pitch: the cache holds f0 x uppower x (float)2^(-phi / 12)
    m = np.float32(2.0 ** (-phi / 12.0))
    cache = eng.pitch_cache()
    assert np.allclose(cache, ora.pitch_cache() * m, rtol=1e-5, atol=1e-3)
    # the latent, stretched
    zt = eng.tap("sy.z").reshape(I, R)
    zi = eng.tap("sy.zi").reshape(I, R2)
    zi_ref = torch.nn.functional.interpolate(torch.from_numpy(np.ascontiguousarray(zt))[None], size=R2, mode="linear", align_corners=False)[0].numpy()
    assert rel_rms(zi, zi_ref) < 1e-4
    # the harmonic source at f0 x R2 / R, then stretched
    pitchf = cache[1024 - 223 + g.skip_head:1024 - 223 + g.skip_head + R]          # rvc.rs:176-177 at the 160 ms geometry
    pn = (pitchf * np.float32(R2)) / np.float32(R) if R2 != R else pitchf
    noise = O.philox_normal(SEED[0], SEED[1], 0, 1, R * upp)
    src_ref = _nsf(pn, R, upp, sr, tens["sy.src"], noise)
    src = eng.tap("sy.src")
    assert rel_rms(src, src_ref) < 5e-4          # (the device's phase is a block prefix scan, the restatement's a sequential sum)
    srci = eng.tap("sy.srci")
    assert srci.shape == (R2 * upp,) and rel_rms(srci, interp(src, R2 * upp)) < 1e-4
    # the decoder on R2 frames, then back to the model rate
    dec = eng.tap("sy.dec")
    assert dec.shape == (R2 * upp,)
    assert rel_rms(dec, TR.synth_decoder(cfg, tens, zi, srci)) < 1e-4
    assert rel_rms(ye, back_to_model_rate(dec, R, upp, ures)) < 1e-4
    # end to end: the reference chain fed with the device's phone features and f0
    C_ = int(cfg["phone_dim"])
    phone = np.ascontiguousarray(eng.tap("phone_ct").reshape(C_, R).T)
    eps = O.philox_normal(SEED[0], SEED[1], 0, 0, I * R).reshape(I, R)
    z_ref = TR.synth_until_z(cfg, tens, phone, _coarse_pitch(pitchf), eps)[2]
    y2 = TR.synth_decoder(cfg, tens, interp(z_ref, R2), interp(src_ref, R2 * upp))
    assert rms(ye - back_to_model_rate(y2, R, upp, ures)) < PCM_TOL
    eng.close()


@pytest.mark.parametrize("phi", [0.07, -0.07, 0.01, 3.5, 5.0, -5.0])
def test_stages_full_48k(phi):
    _stage_case("full", None, phi)


def test_stages_full_40k():
    _stage_case("full", "full40k", 3.5)


@pytest.mark.parametrize("phi", [-5.0, -2.3, 0.07, 1.7, 5.0])
def test_stages_tiny(phi):
    _stage_case("tiny", None, phi)


@pytest.mark.parametrize("phi", [3.5, -2.3])
def test_stages_tiny_32k(phi):
    # upstream's v2 32k decoder layout (10 * 8 * 2 * 2, upp = 320): the stretch and the resample back at a model rate of 32000, both directions
    _stage_case("tiny", "tiny32k", phi)


def test_zero_is_todays_path():
    z = zoo("tiny")
    x = voice_signal(g.input_buffer_16k_size, seed=5)
    fresh = _engine(z)
    y0 = fresh.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    back = _engine(z, 3.0)
    y3 = back.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    back.set_formant_shift(0.0)
    back.reset_state()
    y = back.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    assert y.shape == y0.shape == y3.shape
    assert np.array_equal(y, y0) and not np.array_equal(y3, y0)
    assert back.plan_ops() == fresh.plan_ops()
    for e in (fresh, back):
        e.close()


PHIS8 = [0.0, 0.07, 5.0, -5.0, 3.5, 0.0, -0.07, 0.01]


def _alone(z, phis, xs, shifts, seed=SEED):
    """every stream run alone on a one-stream engine: same seed, same stream id, same settings"""
    one = _engine(z)
    ys = []
    for s, phi in enumerate(phis):
        one.set_noise_seed(seed[0], seed[1] + s); one.reset_state(); one.set_formant_shift(phi)
        ys.append(one.infer(xs[s], g.sample_frame_16k, int(shifts[s]), g.skip_head, R))
    one.close()
    return ys


def test_mixed_shifts_every_entry_point():
    from obs_rvc_amd import _native
    z = zoo("full")
    S = len(PHIS8)
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=40 + s) for s in range(S)])
    shifts = np.array([12, 0, 7, -12, 12, 5, 12, 0], np.int32)
    alone = _alone(z, PHIS8, xs, shifts)
    plain = _alone(z, [0.0] * S, xs, shifts)
    eng = _engine(z, streams=S)
    for s, phi in enumerate(PHIS8):
        eng.set_formant_shift(phi, stream=s)
    yv = eng.infer_batch(xs, g.sample_frame_16k, shifts, g.skip_head, R)
    eng.reset_state()
    L = _native.lib()
    d_in = torch.from_numpy(xs).cuda()
    cap = g.model_return_size + 64
    d_out = torch.zeros((S, cap), dtype=torch.float32, device="cuda")
    n = C.c_size_t()
    rc = L.rvc_infer_device_v(eng._h, C.c_void_p(d_in.data_ptr()), xs.shape[1], g.sample_frame_16k, shifts.ctypes.data_as(C.POINTER(C.c_int32)),
                              g.skip_head, R, C.c_void_p(d_out.data_ptr()), cap, C.byref(n), 1)
    assert rc == 0 and n.value == g.model_return_size
    yd = d_out[:, :n.value].cpu().numpy()
    eng.reset_state()
    yg = eng.infer_batch_g(list(xs), [g.sample_frame_16k] * S, list(shifts), [g.skip_head] * S, [R] * S)
    for s in range(S):
        for name, y in (("batch_v", yv[s]), ("device_v", yd[s]), ("batch_g", yg[s])):
            assert y.shape == alone[s].shape == (g.model_return_size,)
            assert rms(y - alone[s]) < PCM_TOL, (name, s, PHIS8[s], rms(y - alone[s]))
            if PHIS8[s] == 0.0:
                assert rms(y - plain[s]) < PCM_TOL, (name, s)
    eng.close()


def test_64_streams_uniform_shift():
    z = zoo("tiny")
    S = 64
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=200 + s) for s in range(S)])
    eng = _engine(z, 0.07, streams=S)
    y = eng.infer_batch(xs, g.sample_frame_16k, 12, g.skip_head, R)
    alone = _alone(z, [0.07] * S, xs, [12] * S)
    for s in range(S):
        assert rms(y[s] - alone[s]) < PCM_TOL, (s, rms(y[s] - alone[s]))
    eng.close()


def test_same_decoder_length_builds_no_plan():
    z = zoo("full")
    assert geometry(R, 48000, 0.07)[0] == geometry(R, 48000, 0.08)[0] and geometry(R, 48000, 0.07)[1] != geometry(R, 48000, 0.08)[1]
    x = voice_signal(g.input_buffer_16k_size, seed=6)
    eng = _engine(z, 0.07)
    y1 = eng.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    builds = eng.plan_cache_info()["builds"]
    eng.set_formant_shift(0.08); eng.reset_state()
    y2 = eng.infer(x, g.sample_frame_16k, 12, g.skip_head, R)
    assert eng.plan_cache_info()["builds"] == builds
    assert y1.shape == y2.shape and rms(y1 - y2) > 1e-5
    eng.close()


def test_graph_replay():
    from obs_rvc_amd.rvc_common import RvcInferError
    z = zoo("tiny")
    xs = np.stack([voice_signal(g.input_buffer_16k_size, seed=70 + s) for s in range(2)])
    eager = _engine(z, 0.07, streams=2)
    graph = _engine(z, 0.07, streams=2)
    graph.set_use_graph(True)
    for c in range(3):
        ye = eager.infer_batch(xs, g.sample_frame_16k, 12, g.skip_head, R)
        yg = graph.infer_batch(xs, g.sample_frame_16k, 12, g.skip_head, R)
        assert np.array_equal(ye, yg), c
    graph.set_formant_shift(5.0, stream=1)          # R2 22 and 29: two buckets
    with pytest.raises(RvcInferError) as ei:
        graph.infer_batch(xs, g.sample_frame_16k, 12, g.skip_head, R)
    assert ei.value.code == 5
    for e in (eager, graph):
        e.close()


def test_native_session_per_stream_shift():
    from oracle import resample_oracle as RO  # noqa: F401
    from obs_rvc_amd.geometry import derive
    from obs_rvc_amd.resample import FftFixedInOut
    from obs_rvc_amd.streaming import NativeStreamingSession, StreamingSession
    gg = derive(48000, 0.16, 0.07, 2.0, 4800)
    z = zoo("tiny")
    e1 = _engine(z, streams=2, seed=(3, 0))
    e1.set_formant_shift(0.07, stream=0)
    e0 = _engine(z, streams=2, seed=(3, 0))                       # the same session without formant shift
    e2 = _engine(z, 0.07, seed=(3, 0))                            # the host-side state machine, stream 0's settings
    nat = NativeStreamingSession(e1, 48000, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    nat0 = NativeStreamingSession(e0, 48000, 0.16, 0.07, 2.0, 4800, 12, 0.6)
    pys = StreamingSession(e2, gg, 12, 0.6, 4800, lambda ri, ro, n: FftFixedInOut(e2, ri, ro, n))
    a = [np.interp(np.arange(7680 * 8) / 48000.0, np.arange(2560 * 8) / 16000.0, voice_signal(2560 * 8, seed=10 + s)).astype(np.float32) for s in range(2)]
    for c in range(8):
        ch = np.stack([a[s][c * 7680:(c + 1) * 7680] for s in range(2)])
        fn = nat.process_one_frame(ch)
        f0 = nat0.process_one_frame(ch)
        fp = pys.process_one_frame(ch[0])
        assert np.abs(fn[0] - fp).max() < 2e-5, (c, float(np.abs(fn[0] - fp).max()))
        assert np.abs(fn[1] - f0[1]).max() < 2e-5, (c, float(np.abs(fn[1] - f0[1]).max()))
    del nat, nat0
    for e in (e1, e0, e2):
        e.close()
