"""The YIN f0 method of DESIGN.md section 11 restated in numpy, written from the definition and not from the kernel's indexing: frames, the
difference function d, the cumulative-mean-normalised d', the pick, the parabola.  dtype = float64 is the reference of tests/test_gpu_yin.py;
dtype = float32 runs the same recipe in single precision (the measure of what fp32 costs, from which that test derives its bound).  The tail
behind it -- uppower, the pitch cache -- is the one RMVPE feeds: uppower here, the cache update in tests/front_ref.py."""
import numpy as np

from front_ref import update_cache  # noqa: F401  (the cache tail, rvc.rs:168-179)

FRAME, HOP, PAD = 1024, 160, 512
TAU_MIN, TAU_MAX, THRESHOLD = 14, 320, 0.15
N = FRAME - TAU_MAX
SR = 16000.0


def f0_frame(sample_frame_16k_size):
    """f0_extractor_frame (rmvpe.rs:256)"""
    return 5120 * ((sample_frame_16k_size + 799) // 5120 + 1) - 160


def pad_reflect(x, pad):
    """rmvpe.rs:47-67: pad samples mirrored about the first and about the last sample (the edge samples are not repeated)"""
    x = np.asarray(x)
    return np.concatenate([x[1:pad + 1][::-1], x, x[-pad - 1:-1][::-1]])


def frames(audio, sample_frame_16k_size):
    """the last f0_extractor_frame samples, reflect-padded by 512 -> [Tm][1024], frame t = padded[160 t : 160 t + 1024]"""
    fr = f0_frame(sample_frame_16k_size)
    audio = np.asarray(audio)
    assert fr <= len(audio)
    p = pad_reflect(audio[len(audio) - fr:], PAD)
    Tm = 1 + fr // HOP
    return np.stack([p[HOP * t:HOP * t + FRAME] for t in range(Tm)])


def cmnd(x, dtype=np.float64):
    """one frame x [1024] -> d' [321]"""
    x = np.asarray(x, dtype)
    d = np.array([np.sum((x[:N] - x[tau:tau + N]) ** 2, dtype=dtype) for tau in range(TAU_MAX + 1)], dtype=dtype)
    S = np.cumsum(d[1:], dtype=dtype)
    dp = np.ones(TAU_MAX + 1, dtype)
    nz = S > 0
    tau = np.arange(1, TAU_MAX + 1).astype(dtype)
    dp[1:][nz] = d[1:][nz] * tau[nz] / S[nz]
    return dp


def pick(dp):
    """d' [321] -> f0 in Hz (0 = unvoiced), in the precision of dp"""
    dt = dp.dtype.type
    for tau in range(TAU_MIN, TAU_MAX):
        if dp[tau] < dt(THRESHOLD):
            while tau + 1 < TAU_MAX and dp[tau + 1] < dp[tau]:
                tau += 1
            a, b, c = dp[tau - 1], dp[tau], dp[tau + 1]
            den = a - dt(2) * b + c
            off = dt(0.5) * (a - c) / den if den > 0 else dt(0)
            return dt(SR) / (dt(tau) + off)
    return dt(0)


def yin(audio, sample_frame_16k_size, dtype=np.float64):
    """-> (f0 [Tm] in Hz, decision margin [Tm] = min over the searched lags of |d' - 0.15|)"""
    F = frames(np.asarray(audio, np.float32), sample_frame_16k_size)
    f0, margin = [], []
    for x in F:
        dp = cmnd(x, dtype)
        f0.append(pick(dp))
        margin.append(np.min(np.abs(dp[TAU_MIN:TAU_MAX].astype(np.float64) - THRESHOLD)))
    return np.array(f0, dtype), np.array(margin)


def uppower(pitch_shift):
    """rvc.rs:121: 2^(pitch_shift / 12) with Rust's integer division (towards zero: -7 / 12 = 0)"""
    return 2.0 ** int(pitch_shift / 12)


def composite_signal(n=6000, seed=0):
    """The input of tests/test_gpu_yin.py: n samples whose last 4960 (the f0 window at sample_frame_16k_size = 2560, 32 frames) hold silence, a
    noise burst, a glide of five partials (120 -> 170 Hz) on a 1e-3 noise floor, 100 Hz (a period of exactly 160 samples), 800 Hz (20 samples) and,
    after a short silence, a 200 Hz tone that starts inside a frame.  tests/test_yin_ref.py checks what the reference makes of it: which frames
    are voiced, and that few enough of them sit within 1e-4 of the threshold (the tones' phases were chosen so that none does)."""
    rng = np.random.default_rng(seed)
    fr = f0_frame(2560)
    t = lambda m: np.arange(m) / SR
    x = np.zeros(fr)
    x[520:920] = 0.1 * rng.standard_normal(400)
    f = 120.0 * 2.0 ** np.linspace(0.0, 0.5, 1480)
    ph = 2.0 * np.pi * np.cumsum(f) / SR
    x[920:2400] = 0.2 * sum(np.sin(k * ph) / k for k in range(1, 6)) + 1e-3 * rng.standard_normal(1480)
    x[2400:3600] = 0.3 * np.sin(2.0 * np.pi * 100.0 * t(1200) + 0.4)
    x[3600:4400] = 0.3 * np.sin(2.0 * np.pi * 800.0 * t(800) + 0.5)
    x[4560:] = 0.25 * sum(np.sin(2.0 * np.pi * 200.0 * k * t(400)) / k for k in range(1, 4))
    return np.concatenate([0.05 * rng.standard_normal(n - fr), x]).astype(np.float32)


def whole_window_signal(frame16k=5120, seed=5):
    """A whole converter window: exactly f0_frame(frame16k) samples, so the f0 window starts at sample 0 of the buffer (n == frame) and the first and last
    frames' reflection (YIN) or zero extension (CREPE) touches the buffer's own ends.  voice_signal (a harmonic glide, voiced from the first sample to the
    last) with the composite's 4960 samples spliced into the middle and a DC step of +0.05 / -0.04 over the first / last 512 samples."""
    from common import voice_signal
    n = f0_frame(frame16k)
    x = voice_signal(n, seed=seed).astype(np.float64)
    at = (n - 4960) // 2 // 160 * 160
    x[at:at + 4960] = composite_signal()[-4960:]
    x[:512] += 0.05
    x[-512:] -= 0.04
    return x.astype(np.float32)
