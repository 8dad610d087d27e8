"""The "pm" f0 method (Praat's autocorrelation tracker, Boersma 1993) restated in numpy from the definition and not from the
kernels' indexing: YIN's frames, the intensity, the Hanning-windowed autocorrelation divided by the window's own, the parabola and the windowed-sinc
strength of every peak, the best 14 candidates, the local scores, and one Viterbi path over the frames of the window.  dtype = float64 is the
reference of tests/test_gpu_pm.py; dtype = float32 runs the same recipe in single precision (what fp32 costs, from which that test derives its bound).

Praat's Brent refinement of a peak on the sinc interpolant is LEFT OUT: a candidate's lag is the vertex of the parabola through r[i-1], r[i], r[i+1]
and its strength is the sinc interpolant at that lag.  tests/test_pm_ref.py measures what that gives on tones.

Every candidate array is [Tm][15]: entry 0 is the unvoiced candidate (f = 0, s = 0), entries 1 .. n the voiced ones in ascending lag."""
import numpy as np

from yin_ref import FRAME, HOP, PAD, SR, f0_frame, frames, uppower  # noqa: F401  (YIN's frame geometry, unchanged)

FLOOR, CEILING = 50.0, 1100.0
W, OFF = 960, 32                      # the analysis window: three periods of the floor, centred in the 1024-sample frame
VT, ST, OC, OJ, VUV = 0.6, 0.03, 0.01, 0.35, 0.14
MAXC, D, NLAG = 14, 30, 353
I_LO, I_HI = 14, 321                  # peak lags searched
NC = MAXC + 1


def rw_table():
    """the normalised autocorrelation of the Hanning window at the 353 lags, evaluated in double and rounded to float once: the rounded table is the definition"""
    u = np.arange(NLAG) / float(W)
    return ((1.0 - u) * (2.0 / 3.0 + np.cos(2.0 * np.pi * u) / 3.0) + np.sin(2.0 * np.pi * u) / (2.0 * np.pi)).astype(np.float32)


RW = rw_table()
H = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(W) + 0.5) / W)


def global_peak(audio, sample_frame_16k_size, dtype=np.float64):
    """G = max |s - mean| over the f0 window (Praat: over the whole sound)"""
    fr = f0_frame(sample_frame_16k_size)
    s = np.asarray(audio, np.float32)[len(audio) - fr:].astype(dtype)
    mu = np.sum(s, dtype=dtype) / dtype(fr)
    return np.max(np.abs(s - mu))


def correlogram(x, G, dtype=np.float64):
    """one frame x [1024] -> (r [353] or None when ra(0) == 0, intensity I)"""
    dt = dtype
    w = np.asarray(x, dt)[OFF:OFF + W]
    mu = np.sum(w, dtype=dt) / dt(W)
    P = np.max(np.abs(w[320:640] - mu))
    inten = min(dt(1), P / dt(G))
    a = (w - mu) * H.astype(dt)
    ra = np.array([np.sum(a[:W - tau] * a[tau:], dtype=dt) for tau in range(NLAG)], dt)
    if ra[0] == 0:
        return None, inten
    return ra / (ra[0] * RW.astype(dt)), inten


def sinc_strength(r, i, off, dtype=np.float64):
    """Praat's raised-cosine windowed sinc interpolation of r (r(-k) = r(k)) at lag tau = i + off, |off| <= 0.5, depth D.  With m = floor(tau) and
    phi = tau - m: sin(pi (tau - k)) is (-1)^(m - k) sin(pi phi), and phi and 1 - phi are taken from off (off and 1 - off, or 1 + off and -off), not from
    the rounded sum i + off: the same numbers, written so that single precision neither rounds an argument of pi * 30 nor cancels 1 - phi"""
    dt = dtype
    if off == 0:
        return r[i]
    one, half, pi = dt(1), dt(0.5), dt(np.pi)
    m, phi, omphi = (i, off, one - off) if off > 0 else (i - 1, one + off, -off)
    sp = np.sin(pi * min(phi, omphi))
    j = np.arange(D)
    sign = np.where(j % 2 == 0, 1.0, -1.0).astype(dt)
    dl = phi + j.astype(dt)                       # tau - k for k = m, m - 1, ..., m - D + 1
    left = r[np.abs(m - j)] * (sign * sp / (pi * dl)) * (half + half * np.cos(pi * (dl / (phi + dt(D)))))
    dr = omphi + j.astype(dt)                     # k - tau for k = m + 1, ..., m + D
    right = r[m + 1 + j] * (sign * sp / (pi * dr)) * (half + half * np.cos(pi * (dr / (omphi + dt(D)))))
    sl, sr = dt(0), dt(0)
    for v in left:
        sl += v
    for v in right:
        sr += v
    return sl + sr


def frame_candidates(x, G, dtype=np.float64):
    """one frame -> (n, lag index i [15], f [15], s [15], delta [15], decision margin).  The margin is the smallest, over the peaks and near-peaks of
    the frame, of what separates a decision from its alternative: r[i] - 0.3, r[i] - r[i-1], r[i] - r[i+1], |f - 50| / 50, |f - 1100| / 1100 (relative, so that
    all are of one scale) and the score gap between the 14th and the 15th candidate; always measured in float64 terms of the dtype's own numbers"""
    dt = dtype
    lag, f, s, delta = np.zeros(NC, int), np.zeros(NC, dt), np.zeros(NC, dt), np.zeros(NC, dt)
    margin = np.inf
    n = 0
    r, inten = (None, dt(0)) if G == 0 else correlogram(x, G, dt)
    if r is not None:
        cand = []
        for i in range(I_LO, I_HI + 1):
            a, b, c = r[i - 1], r[i], r[i + 1]
            # every lag is one decision: how far it is from changing sides
            ispeak = b > dt(0.5 * VT) and b > a and b >= c
            if b > a and b >= c:
                margin = min(margin, abs(float(b) - 0.5 * VT))
            if b > dt(0.5 * VT):
                margin = min(margin, abs(float(b) - float(a)), abs(float(b) - float(c)))
            if not ispeak:
                continue
            off = dt(0.5) * (c - a) / (dt(2) * b - a - c)
            fc = dt(SR) / (dt(i) + off)
            margin = min(margin, abs(float(fc) - FLOOR) / FLOOR, abs(float(fc) - CEILING) / CEILING)
            if not (fc >= dt(FLOOR) and fc <= dt(CEILING)):
                continue
            sc = sinc_strength(r, i, off, dt)
            if sc > 1:
                sc = dt(1) / sc
            cand.append((i, fc, sc, sc + dt(OC) * np.log2(fc / dt(FLOOR))))
        if len(cand) > MAXC:
            order = sorted(range(len(cand)), key=lambda k: (-cand[k][3], cand[k][0]))
            margin = min(margin, float(cand[order[MAXC - 1]][3]) - float(cand[order[MAXC]][3]))
            cand = [cand[k] for k in sorted(order[:MAXC])]
        n = len(cand)
        for k, (i, fc, sc, _) in enumerate(cand):
            lag[k + 1], f[k + 1], s[k + 1] = i, fc, sc
            delta[k + 1] = sc - dt(OC) * np.log2(dt(CEILING) / fc)
    delta[0] = dt(VT) + max(dt(0), dt(2) - inten / (dt(ST) / (dt(1) + dt(VT))))
    return n, lag, f, s, delta, margin


def candidates(audio, sample_frame_16k_size, dtype=np.float64):
    """-> dict of n [Tm], lag / f / s / delta [Tm][15], margin [Tm]"""
    audio = np.asarray(audio, np.float32)
    G = global_peak(audio, sample_frame_16k_size, dtype)
    out = [frame_candidates(x, G, dtype) for x in frames(audio, sample_frame_16k_size)]
    return {"n": np.array([o[0] for o in out]), "lag": np.stack([o[1] for o in out]), "f": np.stack([o[2] for o in out]), "s": np.stack([o[3] for o in out]),
            "delta": np.stack([o[4] for o in out]), "margin": np.array([o[5] for o in out])}


def transition(f1, f2):
    if f1 == 0 and f2 == 0:
        return 0.0
    if f1 == 0 or f2 == 0:
        return VUV
    return OJ * abs(np.log2(f1 / f2))


def path(n, f, delta):
    """One forward Viterbi over the frames (ties to the lowest candidate index), backtracked from the best candidate of the last frame.
    -> (chosen index [Tm], f0 [Tm], path margin [Tm], sum of the absolute terms along the best path).  The path margin of frame t is the best total
    minus the best total over the paths that pass through another candidate at t (inf where the frame has no other), from a forward and a backward pass."""
    n, f, delta = np.asarray(n), np.asarray(f, np.float64), np.asarray(delta, np.float64)
    Tm = len(n)
    NEG = -np.inf
    fwd = np.full((Tm, NC), NEG)
    bp = np.zeros((Tm, NC), int)
    fwd[0, :n[0] + 1] = delta[0, :n[0] + 1]
    for t in range(1, Tm):
        for c in range(n[t] + 1):
            best, arg = NEG, 0
            for p in range(n[t - 1] + 1):
                v = fwd[t - 1, p] - transition(f[t - 1, p], f[t, c])
                if v > best:
                    best, arg = v, p
            fwd[t, c] = best + delta[t, c]
            bp[t, c] = arg
    idx = np.zeros(Tm, int)
    idx[-1] = int(np.argmax(fwd[-1]))          # (the first of equal maxima)
    for t in range(Tm - 1, 0, -1):
        idx[t - 1] = bp[t, idx[t]]
    bwd = np.full((Tm, NC), NEG)               # the best sum of what follows frame t, given candidate c at t
    bwd[-1, :n[-1] + 1] = 0.0
    for t in range(Tm - 2, -1, -1):
        for c in range(n[t] + 1):
            bwd[t, c] = max(bwd[t + 1, q] + delta[t + 1, q] - transition(f[t, c], f[t + 1, q]) for q in range(n[t + 1] + 1))
    through = fwd + bwd
    total = through[np.arange(Tm), idx]
    margin = np.full(Tm, np.inf)
    for t in range(Tm):
        others = [through[t, c] for c in range(n[t] + 1) if c != idx[t]]
        if others:
            margin[t] = total[t] - max(others)
    terms = sum(abs(delta[t, idx[t]]) for t in range(Tm)) + sum(abs(transition(f[t - 1, idx[t - 1]], f[t, idx[t]])) for t in range(1, Tm))
    return idx, f[np.arange(Tm), idx], margin, terms


def pm(audio, sample_frame_16k_size, dtype=np.float64):
    """-> (f0 [Tm] in Hz, 0 = unvoiced; the candidates' dict; chosen index; path margin; sum of absolute terms)"""
    c = candidates(audio, sample_frame_16k_size, dtype)
    idx, f0, pmargin, terms = path(c["n"], c["f"], c["delta"])
    return f0.astype(dtype), c, idx, pmargin, terms


def composite_signal(n=6000, seed=0):
    """The input of tests/test_gpu_pm.py: n samples whose last 4960 (the f0 window at sample_frame_16k_size = 2560, 32 frames) hold silence, a noise
    burst, a glide of five partials (120 -> 170 Hz) on a 1e-3 noise floor, 100 Hz, 800 Hz and, after a short silence, a 200 Hz tone that starts inside a
    frame: the parts of yin_ref.composite_signal.  tests/test_pm_ref.py checks what the reference makes of it."""
    rng = np.random.default_rng(seed)
    fr = f0_frame(2560)
    t = lambda m: np.arange(m) / SR
    x = np.zeros(fr)
    x[520:920] = 0.1 * rng.standard_normal(400)
    f = 120.0 * 2.0 ** np.linspace(0.0, 0.5, 1480)
    ph = 2.0 * np.pi * np.cumsum(f) / SR
    x[920:2400] = 0.2 * sum(np.sin(k * ph) / k for k in range(1, 6)) + 1e-3 * rng.standard_normal(1480)
    x[2400:3600] = 0.3 * sum(np.sin(2.0 * np.pi * 101.0 * k * t(1200) + 0.4 * k) / k for k in range(1, 4))
    x[3600:4400] = 0.3 * np.sin(2.0 * np.pi * 800.0 * t(800) + 0.5) * np.exp(-np.arange(800) / 1000.0)
    x[4560:] = 0.25 * sum(np.sin(2.0 * np.pi * 200.0 * k * t(400)) / k for k in range(1, 4))
    return np.concatenate([0.05 * rng.standard_normal(n - fr), x]).astype(np.float32)


def stream_signals(n=6000):
    """three streams with different audio for tests/test_gpu_pm.py: the composite, a 110 -> 220 Hz glide of eight partials on a noise floor (common.voice_signal),
    and the composite played backwards (its onset becomes an offset)"""
    from common import voice_signal
    a = composite_signal(n)
    return np.stack([a, voice_signal(n, seed=2), np.ascontiguousarray(a[::-1])])


def tone(f, n=6000, partials=5, weights=None, phase=0.3):
    """partials of f with amplitudes 1 / k (or `weights`), 0.2 in all"""
    t = np.arange(n) / SR
    w = weights if weights is not None else [1.0 / k for k in range(1, partials + 1)]
    return (0.2 * sum(a * np.sin(2.0 * np.pi * f * k * t + phase * k) for k, a in enumerate(w, 1))).astype(np.float32)


def synthetic_candidates(Tm=1024, seed=11):
    """candidate arrays for the path alone at the longest window: a slow random walk in log-frequency with a weaker decoy an octave up and up to 12 weak
    candidates per frame, every seventh frame with all 14; every third stretch of 97 frames unvoiced.  -> (n [Tm], f [Tm][15], delta [Tm][15])"""
    rng = np.random.default_rng(seed)
    n = np.zeros(Tm, np.int32)
    f, d = np.zeros((Tm, NC)), np.zeros((Tm, NC))
    lf = np.log2(140.0) + np.cumsum(0.01 * rng.standard_normal(Tm))
    for t in range(Tm):
        voiced = (t // 97) % 3 != 2
        d[t, 0] = 0.2 + 0.05 * rng.random() if voiced else 1.8
        k = int(rng.integers(2, MAXC + 1)) if t % 7 else MAXC
        fs = np.concatenate([[2.0 ** lf[t], 2.0 ** (lf[t] + 1.0)], 2.0 ** rng.uniform(np.log2(50.0), np.log2(1100.0), k - 2)])
        ds = np.concatenate([[0.9 + 0.1 * rng.random(), 0.45 + 0.1 * rng.random()], 0.2 + 0.2 * rng.random(k - 2)])
        order = np.argsort(-fs)          # ascending lag = descending frequency
        n[t], f[t, 1:k + 1], d[t, 1:k + 1] = k, fs[order], ds[order]
    return n, f, d
