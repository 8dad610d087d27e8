"""Pins tests/front_ref.py (the float64 references of test_gpu_front.py) against independent implementations: torch in float64 where torch has the
operation, the fp32 CPU oracle for the reference's own quirks (decode window, cache moves, coarse pitch rounding, noise layout).  No GPU."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import front_ref as R
from common import BASELINE_160MS as g, GOLDEN, W, chunk_stream, voice_signal, zoo
from oracle import oracle as O


def _mk(seed=(1, 0)):
    z = zoo("tiny")
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(*seed)
    ora.enable_taps(True)
    return z, ora


def test_logmel_against_torch_stft_and_the_oracle():
    rng = np.random.default_rng(1)
    for frame, extra in ((4960, 0), (10080, 37)):
        x = np.concatenate([voice_signal(frame + extra, seed=3)[:extra], voice_signal(frame, seed=4) + 0.05 * rng.standard_normal(frame)]).astype(np.float32)
        s, norm = R.mel_linear(x, frame)
        sig = torch.from_numpy(x[extra:].astype(np.float64))
        spec = torch.stft(sig, 1024, hop_length=160, win_length=1024, window=torch.hann_window(1024, periodic=True, dtype=torch.float64), center=True,
                          pad_mode="reflect", return_complex=True).abs().numpy()
        assert spec.shape == (513, 1 + frame // 160)
        st = R.mel_basis() @ spec
        assert np.max(np.abs(s - st)) <= 1e-12 * np.max(st)
        # the fp32 oracle on a signal with energy in every band: logarithms agree to fp32 accuracy
        lm_o = O.mel_extract(x[extra:]).astype(np.float64)
        assert np.max(np.abs(R.logmel(x, frame) - lm_o)) < 1e-4
        assert norm.shape == (1 + frame // 160,) and np.all(norm > 0)
    # reflection and frame origin: an impulse at sample 0 reaches frame 0 only through the centre tap (hann(512) = 1) -- a flat spectrum of 1
    imp = np.zeros(4960, np.float32); imp[0] = 1.0
    s, _ = R.mel_linear(imp, 4960)
    assert np.allclose(s[:, 0], R.mel_basis().sum(axis=1), rtol=1e-12)
    assert np.all(s[:, 4:] == 0.0)                                           # frames from 640 on do not see sample 0 or its mirror image
    assert np.all(R.logmel(np.zeros(4960, np.float32), 4960) == np.log(1e-5))


def test_conv0_gn_gelu_against_torch():
    rng = np.random.default_rng(2)
    for B, C, L in ((2, 6, 10), (3, 5, 1297), (1, 16, 5 * 299 + 13)):
        x = rng.standard_normal((B, L)).astype(np.float32)
        w = rng.standard_normal((C, 10)).astype(np.float32) * 0.3
        ga, be = rng.uniform(0.5, 1.5, C), rng.uniform(-0.5, 0.5, C)
        y = F.conv1d(torch.from_numpy(x.astype(np.float64))[:, None], torch.from_numpy(w.astype(np.float64))[:, None], stride=5)
        assert y.shape[2] == (L - 10) // 5 + 1
        y = F.gelu(F.group_norm(y, C, torch.from_numpy(ga), torch.from_numpy(be), eps=1e-5)).numpy()
        got = R.conv0_gn_gelu(x, w, 5, ga, be)
        assert got.shape == y.shape and np.max(np.abs(got - y)) < 1e-12
    # a constant input has variance 0: gelu(beta) for every t
    got = R.conv0_gn_gelu(np.full((1, 60), 0.25), w, 5, ga, be)
    assert np.allclose(got, R.gelu(be)[None, :, None] * np.ones((1, 1, 11)), atol=1e-9)


def _salience(rng, T, peaks):
    sal = rng.uniform(0.001, 0.003, (360, T))
    for t, p in enumerate(peaks):
        k = np.arange(360)
        sal[:, t] += 0.9 * np.where(np.abs(k - p) < 16, 0.5 * (1 + np.cos(np.pi * (k - p) / 16)), 0.0)
    return sal.astype(np.float32)


def test_decode_against_the_oracle():
    rng = np.random.default_rng(3)
    peaks = [0, 3, 4, 44, 45, 100, 179, 180, 300, 347]
    sal = _salience(rng, len(peaks), peaks)
    sal[:, 5] = 0.0                                                          # nothing positive: 0 Hz through the threshold, not NaN
    sal[:, 6] *= np.float32(0.029)
    sal[np.argmax(sal[:, 6]), 6] = np.float32(0.03)                          # maximum at the threshold (strict >): unvoiced
    rc, f_o = O.decode(sal.T.copy())
    f, panic = R.decode_pitch(sal)
    assert rc == 0 and not panic.any()
    assert f[5] == 0.0 and f[6] == 0.0 and f_o[5] == 0.0 and f_o[6] == 0.0
    assert np.allclose(f, f_o, rtol=2e-6, atol=0)
    # the window sits 4 bins above the peak: a peak at bin p is read at p + 4 .. p + 12, so the estimate lies above the peak's own pitch
    assert f[5 + 0] == 0 and f[7] > 10.0 * 2 ** ((180 * 20 + R.CENTS0) / 1200)
    # first of two equal maxima wins
    sal2 = _salience(rng, 1, [120]); sal2[200, 0] = sal2[120, 0]
    assert np.allclose(R.decode_pitch(sal2)[0], O.decode(sal2.T.copy())[1], rtol=2e-6)
    assert np.allclose(R.decode_pitch(sal2)[0], R.decode_pitch(_salience(np.random.default_rng(3), 1, [120]))[0], rtol=0.05)
    # argmax at bin 348 (start 352, start + 8 = 360): the reference panics
    sal3 = _salience(rng, 2, [347, 348])
    rc, _ = O.decode(sal3.T.copy())
    assert rc != 0 and R.decode_pitch(sal3)[1].tolist() == [False, True]
    for k in (-24, -13, -12, -1, 0, 7, 12, 23, 24):
        assert O.uppower(k) == 2.0 ** int(k / 12)                            # truncating division


def test_coarse_pitch_against_the_oracle():
    f = np.concatenate([[0.0, 49.9, 50.0, 500.0, 1100.0, 5000.0], np.geomspace(20.0, 2000.0, 20000)]).astype(np.float32)
    want, _ = O.get_f0_post(f)
    got, dist = R.coarse_pitch(f)
    clear = dist > 1e-3
    assert np.array_equal(got[clear], want[clear]) and np.mean(~clear) < 0.01
    assert got[0] == 1 and got[1] == 1 and got[2] == 1 and got[3] == 255 and got[4] == 255 and got[5] == 255


def test_cache_against_the_oracle_and_the_golden_chain():
    _, ora = _mk()
    audio = voice_signal(g.sample_frame_16k * 20, seed=5)
    cache = np.zeros(1024)
    hubert_length = min(g.input_buffer_16k_size // 160, 2 * 111 + 1)
    for ring in list(chunk_stream(audio, g.input_buffer_16k_size, g.sample_frame_16k))[-4:]:
        ora.infer(ring, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
        f0 = ora.tap("f0")
        cache, pitchf = R.update_cache(cache, f0, g.sample_frame_16k // 160, 1028 - len(f0), 1024 - hubert_length + g.skip_head, g.model_return_length)
        assert np.array_equal(ora.pitch_cache(), cache.astype(np.float32))
        assert np.array_equal(ora.tap("pitchf"), pitchf.astype(np.float32))
        assert np.array_equal(ora.tap("pitch").astype(np.int64)[R.coarse_pitch(pitchf)[1] > 1e-3], R.coarse_pitch(pitchf)[0][R.coarse_pitch(pitchf)[1] > 1e-3])
    # the committed chain: the same four moves on the oracle's f0 of each ring reproduce the recorded cache
    d = np.load(os.path.join(GOLDEN, "tiny_chain.npz"))
    _, ora = _mk((99, 5))
    cache = np.zeros(1024)
    for i, r in enumerate(list(chunk_stream(d["audio"], g.input_buffer_16k_size, g.sample_frame_16k))[-4:]):
        ora.infer(r, g.sample_frame_16k, 7 if i % 2 else -12, g.skip_head, g.model_return_length)
        f0 = ora.tap("f0")
        cache, _ = R.update_cache(cache, f0, g.sample_frame_16k // 160, 1028 - len(f0), 1024 - hubert_length + g.skip_head, g.model_return_length)
    assert np.allclose(cache, d["cache"], rtol=1e-5, atol=1e-4)
    # a shift of the whole cache keeps the old values; the last legal read offset
    c0 = np.arange(1024.0)
    c1, pf = R.update_cache(c0, np.arange(100.0, 132.0), 1024, 1028 - 32, 1024 - 21, 21)
    assert np.array_equal(c1[:996], c0[:996]) and np.array_equal(c1[996:], np.arange(103.0, 131.0)) and np.array_equal(pf, c1[1003:])


def test_nsf_source_against_the_oracle():
    z, ora = _mk((7, 3))
    cfg, tens = W.read_blob(z["model"])
    sr, upp = int(cfg["sr"]), int(np.prod([int(cfg["up_rate%d" % i]) for i in range(int(cfg["n_ups"]))]))
    lin_w, lin_b = [float(v) for v in tens["sy.src"]]
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    for chunk in range(2):
        ora.infer(x, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
        pitchf, src = ora.tap("pitchf"), ora.tap("sy.src")
        noise = O.philox_normal(7, 3, chunk, 1, len(src))
        ref = R.nsf_source(pitchf, upp, sr, lin_w, lin_b, noise)
        assert len(src) == len(pitchf) * upp and (pitchf > 0).any()
        # fp32 phase accumulation over R upp samples in the oracle: a few 1e-5 of a turn, times 2 pi x 0.1 x lin_w
        assert np.max(np.abs(ref - src)) < 5e-4, np.max(np.abs(ref - src))
    # the single-precision restatement of the phase follows the float64 one (the measure test_gpu_front.py takes its tolerance from)
    f0 = np.full(35, 440.0, np.float32)
    d = R.sine_phase(f0, 400, 40000, np.float32).astype(np.float64) - R.sine_phase(f0, 400, 40000)
    assert np.max(np.abs(d - np.round(d))) < 1e-3


def test_alternating_tracks_lose_the_phase_in_single_precision():
    """Where voiced and unvoiced frames alternate, the wraps counted on the interpolated phase do not follow the increments that are summed: the running
    phase climbs to hundreds or thousands of turns, and single precision (the oracle's arithmetic, restated by sine_phase(..., float32)) no longer holds
    its fraction.  test_gpu_front.py measures its sine allowance from this difference, so on these tracks the allowance says nothing; on steady and
    gliding tracks the phase stays within a few turns and the two precisions agree to a few hundredths of a turn at the longest window."""
    def measure(f, upp):
        f = np.asarray(f, np.float32)
        p64, p32 = R.sine_phase(f.astype(np.float64), upp, upp * 100), R.sine_phase(f, upp, upp * 100, np.float32).astype(np.float64)
        d = p32 - p64
        return float(np.max(np.abs(p64))), float(np.max(np.abs(d - np.round(d))))
    for T, upp in ((155, 320), (512, 480)):
        t = np.arange(T)
        for f in (np.where(t % 2 == 0, 220.0, 0.0), np.where((t // 7) % 2 == 0, 330.0, 0.0)):
            turns, diff = measure(f, upp)
            assert turns > 500 and diff > 0.03, (T, turns, diff)
        for f in (np.full(T, 55.0), np.full(T, 440.0), np.full(T, 1100.0), np.geomspace(80.0, 800.0, T)):
            turns, diff = measure(f, upp)
            assert turns < 20 and diff < 0.02, (T, turns, diff)
