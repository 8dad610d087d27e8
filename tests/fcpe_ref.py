"""The FCPE f0 method of DESIGN.md section 23 restated in numpy, written from the definition and not from the kernels' indexing: the Slaney log-mel on
RMVPE's frame grid, the input stack, the conv layers, the classifier, the local arg-max decoder.  dtype = float64 is the reference of
tests/test_gpu_fcpe.py; dtype = float32 runs the same recipe in single precision (the measure of what fp32 costs, from which that test derives its bounds).
No torch here: tests/test_fcpe_ref.py holds a torch restatement of the network and compares.  The filterbank is the blob's (fc.mel_basis), so the kernel and
this file cannot disagree about it; tests/test_fcpe_ref.py checks it against its closed form.  The tail behind the raw f0 -- uppower, the pitch cache -- is
the one RMVPE and YIN feed (yin_ref.uppower, front_ref.update_cache)."""
import numpy as np
import scipy.fft

from yin_ref import f0_frame, pad_reflect

FRAME, HOP, PAD, MELS, BINS = 1024, 160, 512, 128, 360
DW_K, DW_PAD = 31, 15
EPS = 1e-5
THRESHOLD = 0.006
F0_FLOOR = 50.0
CENTS = np.linspace(1200.0 * np.log2(32.70 / 10.0), 1200.0 * np.log2(1975.5 / 10.0), BINS)
STAGES = ("mel", "stack", "l0.dw")          # + "l0" .. "l{N-1}", "prob", "f0"


def n_layers(t):
    n = 0
    while "fc.l%d.ln.g" % n in t:
        n += 1
    return n


def stage_names(t):
    return STAGES + tuple("l%d" % l for l in range(n_layers(t))) + ("prob", "f0")


# ------------------------------------------------------------------------------------------------ front end
def logmel(t, audio, sample_frame_16k_size, dtype=np.float64):
    """the last f0_extractor_frame samples, reflect-padded by 512; frame i = the 1024 samples centred on sample 160 i, periodic Hann, 513 plain magnitudes,
    the blob's filterbank, log(max(x, 1e-5)) -> [128][Tm]"""
    fr = f0_frame(sample_frame_16k_size)
    audio = np.asarray(audio, np.float32)
    assert fr <= len(audio)
    p = pad_reflect(audio[len(audio) - fr:], PAD).astype(dtype)
    Tm = 1 + fr // HOP
    win = (0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(FRAME) / FRAME))).astype(dtype)
    F = np.stack([p[HOP * i:HOP * i + FRAME] for i in range(Tm)]) * win
    mag = np.abs(scipy.fft.rfft(F, axis=1)).astype(dtype)          # (scipy keeps single precision; numpy.fft may not)
    s = t["fc.mel_basis"].astype(dtype) @ mag.T
    return np.log(np.maximum(s, dtype(1e-5))).astype(dtype)


# ------------------------------------------------------------------------------------------------ network
def conv1d(x, w, b, pad):
    """x [cin][T], w [cout][cin][k], zero padding pad either side -> [cout][T + 2 pad - k + 1]"""
    cin, T = x.shape
    cout, _, k = w.shape
    xp = np.zeros((cin, T + 2 * pad), x.dtype)
    xp[:, pad:pad + T] = x
    win = np.lib.stride_tricks.sliding_window_view(xp, k, axis=1)          # [cin][Tout][k]
    cols = np.ascontiguousarray(win.transpose(1, 0, 2)).reshape(win.shape[1], cin * k)
    return (cols @ w.reshape(cout, cin * k).T).T + b[:, None]


def sigmoid(x):
    return x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))


def group_norm(x, g, b, groups=4):
    """each group: its C / groups channels over all frames; biased variance about the mean"""
    C, T = x.shape
    dt = x.dtype.type
    xg = x.reshape(groups, -1)
    mean = xg.mean(axis=1, keepdims=True, dtype=x.dtype)
    var = np.mean((xg - mean) ** 2, axis=1, keepdims=True, dtype=x.dtype)
    return ((xg - mean) / np.sqrt(var + dt(EPS))).reshape(C, T) * g[:, None] + b[:, None]


def layer_norm(x, g, b):
    """over the channels of every frame"""
    dt = x.dtype.type
    mean = x.mean(axis=0, keepdims=True, dtype=x.dtype)
    var = np.mean((x - mean) ** 2, axis=0, keepdims=True, dtype=x.dtype)
    return (x - mean) / np.sqrt(var + dt(EPS)) * g[:, None] + b[:, None]


def glu_dw_silu(z, w, b):
    """z [2 I][T] -> silu(b + depthwise(w [I][31], zero padding 15)(z[:I] * sigmoid(z[I:]))) [I][T]"""
    I = z.shape[0] // 2
    u = z[:I] * sigmoid(z[I:])
    T = u.shape[1]
    up = np.zeros((I, T + 2 * DW_PAD), z.dtype)
    up[:, DW_PAD:DW_PAD + T] = u
    win = np.lib.stride_tricks.sliding_window_view(up, DW_K, axis=1)          # [I][T][31]: win[c][t][k] = u[c][t + k - 15]
    y = np.einsum("ctk,ck->ct", win, w).astype(z.dtype) + b[:, None]
    return y * sigmoid(y)


def network(t, mel, dtype=np.float64):
    """t: the blob's tensors (weights.make_fcpe / importers.import_fcpe), mel [128][Tm] -> {"stack", "l0.dw", "l0" .., "prob" [Tm][360]}"""
    g = lambda k: t[k].astype(dtype)
    out = {}
    x = conv1d(np.asarray(mel, dtype), g("fc.in0.w"), g("fc.in0.b"), 1)
    x = group_norm(x, g("fc.gn.g"), g("fc.gn.b"))
    x = np.where(x >= 0, x, x * dtype(0.01))
    x = conv1d(x, g("fc.in1.w"), g("fc.in1.b"), 1)
    out["stack"] = x
    for l in range(n_layers(t)):
        p = "fc.l%d." % l
        n = layer_norm(x, g(p + "ln.g"), g(p + "ln.b"))
        z = g(p + "pw1.w") @ n + g(p + "pw1.b")[:, None]
        d = glu_dw_silu(z, g(p + "dw.w"), g(p + "dw.b"))
        if l == 0:
            out["l0.dw"] = d
        x = x + (g(p + "pw2.w") @ d + g(p + "pw2.b")[:, None])
        out["l%d" % l] = x
    n = layer_norm(x, g("fc.norm.g"), g("fc.norm.b"))
    out["prob"] = sigmoid(g("fc.out.w") @ n + g("fc.out.b")[:, None]).T.astype(dtype)
    return out


# ------------------------------------------------------------------------------------------------ decoder
def decode(p, threshold=THRESHOLD, dtype=np.float64):
    """upstream's local_argmax.  p [T][360] -> dict(bins = arg-max per frame (ties to the lower bin), f0 [T], cents [T] before the two gates): the nine indices clamp(k* - 4 + j, 0, 359),
    a clamped index counting as often as it occurs; cents = sum p c / sum p over them; f0 = 10 * 2^(cents / 1200); 0 where p[k*] <= threshold, 0 below 50 Hz"""
    p = np.asarray(p, dtype)
    T = len(p)
    bins = np.argmax(p, axis=1)
    idx = np.clip(bins[:, None] - 4 + np.arange(9)[None, :], 0, BINS - 1)
    w = p[np.arange(T)[:, None], idx]
    c = CENTS.astype(dtype)[idx]
    with np.errstate(invalid="ignore", divide="ignore"):
        cents = np.sum(w * c, axis=1, dtype=dtype) / np.sum(w, axis=1, dtype=dtype)
        f0 = dtype(10) * np.exp2(cents / dtype(1200))
    peak = p[np.arange(T), bins]
    f0 = np.where((peak.astype(np.float64) <= threshold) | ~(f0 >= F0_FLOOR), dtype(0), f0)
    return dict(bins=bins, f0=f0.astype(dtype), peak=peak, cents=cents)


def fcpe(t, audio, sample_frame_16k_size, threshold=THRESHOLD, dtype=np.float64):
    """the whole method on one stream: -> dict(mel, stack, l0.dw, l0 .., prob, bins, f0, peak)"""
    mel = logmel(t, audio, sample_frame_16k_size, dtype)
    out = network(t, mel, dtype)
    out["mel"] = mel
    out.update(decode(out["prob"], threshold, dtype))
    return out


# ------------------------------------------------------------------------------------------------ constructed posteriors of the decoder tests
def ridge_case(Tm, seed):
    """a bump of width 2 bins wandering over the bins, and in every eighth frame a decoy spike more than 40 bins away that beats it (local arg-max follows the
    decoy: the decoder has no memory).  The bump peaks 0.3 bins above its integer centre, so no two bins tie"""
    rng = np.random.default_rng(seed)
    c = np.clip(170 + np.cumsum(rng.integers(-3, 4, Tm)), 100, 240)
    i = np.arange(BINS)
    p = 0.02 + 0.78 * np.exp(-0.5 * ((i[None, :] - c[:, None] - 0.3) / 2.0) ** 2)
    decoy = {}
    for t in range(3, Tm, 8):
        decoy[t] = int(c[t] + (50 if t % 16 == 3 else -45))
        p[t, decoy[t]] = 0.97
    return p.astype(np.float32), c, decoy
