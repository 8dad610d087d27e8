"""The CREPE f0 method of DESIGN.md section 21 restated in numpy, written from the definition and not from the kernels' indexing: frames, the six
conv -> ReLU -> BatchNorm -> max-pool layers, the classifier, the Viterbi / arg-max decoder, the two width-3 filters and the threshold.  dtype = float64
is the reference of tests/test_gpu_crepe.py; dtype = float32 runs the same recipe in single precision (the measure of what fp32 costs, from which that
test derives its bounds).  No torch here: tests/test_crepe_ref.py holds a torch restatement of the network and compares.  The tail behind the raw f0 --
uppower, the pitch cache -- is the one RMVPE and YIN feed (yin_ref.uppower, front_ref.update_cache)."""
import numpy as np

from yin_ref import f0_frame

FRAME, HOP, PAD, BINS = 1024, 160, 512, 360
CENTS_OFFSET = 1997.3794084376191
BN_EPS = 0.0010000000474974513
CAPACITY = {"full": 32, "tiny": 4, "micro": 1}
CHANNELS = (32, 4, 4, 4, 8, 16)
KERNELS = (512, 64, 64, 64, 64, 64)
STRIDES = (4, 1, 1, 1, 1, 1)
PADS = ((254, 254), (31, 32), (31, 32), (31, 32), (31, 32), (31, 32))
LENGTHS = (1024, 128, 64, 32, 16, 8)                   # what each layer reads: 1024 -> 256 -> 128 -> 64 -> 32 -> 16 -> 8 -> 4 counts the strided conv and every pool
TRANSITION_WIDTH = 12                                  # max(12 - |i - j|, 0)
VOICED = 0.1


def bin_of(f):
    return (1200.0 * np.log2(f / 10.0) - CENTS_OFFSET) / 20.0


LO, HI = int(np.floor(bin_of(50.0))), int(np.ceil(bin_of(1100.0)))          # bins [LO, HI) are decoded: 39, 308
F0_OF_BIN = 10.0 * 2.0 ** ((20.0 * np.arange(BINS) + CENTS_OFFSET) / 1200.0)


# ------------------------------------------------------------------------------------------------ frames
def frames(audio, sample_frame_16k_size, dtype=np.float64):
    """the last f0_extractor_frame samples, zero-padded by 512 -> [Tm][1024]: frame t is centred on sample 160 t; mean removed, over max(1e-10, std),
    std unbiased"""
    fr = f0_frame(sample_frame_16k_size)
    audio = np.asarray(audio, np.float32)
    assert fr <= len(audio)
    p = np.concatenate([np.zeros(PAD, dtype), audio[len(audio) - fr:].astype(dtype), np.zeros(PAD, dtype)])
    Tm = 1 + fr // HOP
    F = np.stack([p[HOP * t:HOP * t + FRAME] for t in range(Tm)])
    F = F - F.mean(axis=1, keepdims=True, dtype=dtype)
    sd = np.sqrt(np.sum(F * F, axis=1, keepdims=True, dtype=dtype) / dtype(FRAME - 1))
    return (F / np.maximum(dtype(1e-10), sd)).astype(dtype)


# ------------------------------------------------------------------------------------------------ network
def conv1d(x, w, b, stride, pad):
    """x [n][cin][L], w [cout][cin][k], zero padding (left, right) -> [n][cout][Lout], in x's dtype"""
    n, cin, L = x.shape
    cout, _, k = w.shape
    xp = np.zeros((n, cin, L + pad[0] + pad[1]), x.dtype)
    xp[:, :, pad[0]:pad[0] + L] = x
    Lout = (L + pad[0] + pad[1] - k) // stride + 1
    w2 = w.reshape(cout, cin * k)
    out = np.empty((n, cout, Lout), x.dtype)
    step = max(1, (1 << 23) // (cin * k * Lout))          # frames per block: the window matrix stays under 64 MB
    for i in range(0, n, step):
        win = np.lib.stride_tricks.sliding_window_view(xp[i:i + step], k, axis=2)[:, :, ::stride][:, :, :Lout]          # [m][cin][Lout][k]
        cols = np.ascontiguousarray(win.transpose(0, 2, 1, 3)).reshape(-1, cin * k)
        out[i:i + step] = (cols @ w2.T).reshape(-1, Lout, cout).transpose(0, 2, 1)
    return out + b[None, :, None]


def layer_shapes(preset):
    """[(cout, cin, k, length in, conv length, pooled length)] of the six layers"""
    m = CAPACITY[preset]
    out, cin = [], 1
    for l in range(6):
        co = CHANNELS[l] * m
        conv_len = (LENGTHS[l] + PADS[l][0] + PADS[l][1] - KERNELS[l]) // STRIDES[l] + 1
        out.append((co, cin, KERNELS[l], LENGTHS[l], conv_len, conv_len // 2))
        cin = co
    return out


def network(t, F, dtype=np.float64):
    """t: the blob's tensors (weights.make_crepe / importers.import_crepe), F [n][1024] -> {"p1" .. "p6": [n][c][len], "prob": [n][360]}"""
    x = np.asarray(F, dtype)[:, None, :]
    out = {}
    for l in range(6):
        w, b = t["cr.conv%d.w" % (l + 1)].astype(dtype), t["cr.conv%d.b" % (l + 1)].astype(dtype)
        sc, sh = t["cr.bn%d.scale" % (l + 1)].astype(dtype), t["cr.bn%d.shift" % (l + 1)].astype(dtype)
        y = conv1d(x, w, b, STRIDES[l], PADS[l])
        y = np.maximum(y, dtype(0)) * sc[None, :, None] + sh[None, :, None]          # ReLU, then BatchNorm: a scale may be negative
        x = np.maximum(y[:, :, 0::2], y[:, :, 1::2])
        out["p%d" % (l + 1)] = x
    feat = x.transpose(0, 2, 1).reshape(len(x), -1)          # time major, channel minor
    z = feat @ t["cr.fc.w"].astype(dtype).T + t["cr.fc.b"].astype(dtype)
    out["prob"] = (dtype(1) / (dtype(1) + np.exp(-z))).astype(dtype)
    return out


# ------------------------------------------------------------------------------------------------ decoder
def log_transition(n=BINS, width=TRANSITION_WIDTH, dtype=np.float64):
    """log of max(width - |i - j|, 0), row-normalised: [i][j] = from i to j"""
    i = np.arange(n)
    w = np.maximum(width - np.abs(i[:, None] - i[None, :]), 0).astype(dtype)
    w = w / w.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore"):
        return np.log(w).astype(dtype)


def log_observation(p, lo=LO, hi=HI, dtype=np.float64):
    """softmax over the bins [lo, hi) of each row of p [T][n], as logs; -inf outside"""
    p = np.asarray(p, dtype)
    q = p[:, lo:hi]
    mx = q.max(axis=1, keepdims=True)
    lse = mx + np.log(np.sum(np.exp(q - mx), axis=1, keepdims=True, dtype=dtype))
    out = np.full(p.shape, -np.inf, dtype)
    out[:, lo:hi] = q - lse
    return out


def viterbi(logobs, logtrans, lo=LO, hi=HI):
    """the best path through logobs [T][n] from a uniform prior over [lo, hi); logtrans [n][n] or None (arg-max: no transition term).  Ties go to the lower
    bin (np.argmax returns the first).  Scores are kept relative to each frame's best.  -> bins [T]"""
    T, n = logobs.shape
    dt = logobs.dtype.type
    if logtrans is None:
        return np.argmax(logobs, axis=1)
    score = np.full(n, -np.inf, logobs.dtype)
    score[lo:hi] = dt(-np.log(hi - lo)) + logobs[0, lo:hi]
    bp = np.zeros((T, n), np.int64)
    for t in range(1, T):
        cand = score[:, None] + logtrans
        bp[t] = np.argmax(cand, axis=0)
        score = cand[bp[t], np.arange(n)] + logobs[t]
        score = score - score.max()          # relative to the frame's best: a constant per frame, which no arg-max sees, and float32 keeps its digits
    path = np.zeros(T, np.int64)
    path[-1] = np.argmax(score)
    for t in range(T - 1, 0, -1):
        path[t - 1] = bp[t, path[t]]
    return path


def path_score(logobs, logtrans, path, lo=LO, hi=HI):
    """the log probability of a path under the model viterbi() maximises (float64 in, float64 out)"""
    s = -np.log(hi - lo) + logobs[0, path[0]]
    for t in range(1, len(path)):
        s = s + (logtrans[path[t - 1], path[t]] if logtrans is not None else 0.0) + logobs[t, path[t]]
    return float(s)


def filter3(x, kind):
    """width-3 median or mean; at either end the two entries that exist (the median of two is their mean)"""
    x = np.asarray(x)
    dt = x.dtype.type
    out = np.empty_like(x)
    if len(x) == 1:
        return x.copy()
    out[0], out[-1] = (x[0] + x[1]) * dt(0.5), (x[-1] + x[-2]) * dt(0.5)
    a, b, c = x[:-2], x[1:-1], x[2:]
    out[1:-1] = np.maximum(np.minimum(a, b), np.minimum(np.maximum(a, b), c)) if kind == "median" else ((a + b) + c) / dt(3)
    return out


def decode(p, decoder="viterbi", dtype=np.float64):
    """p [T][360] -> dict(bins, pd = p[t][bin] unfiltered, f0 = the raw f0 handed to the pitch tail, margin = |median-filtered pd - 0.1| in float64)"""
    p = np.asarray(p, dtype)
    lo = log_observation(p, dtype=dtype)
    bins = viterbi(lo, log_transition(dtype=dtype) if decoder == "viterbi" else None)
    pd = p[np.arange(len(p)), bins]
    pdm = filter3(pd, "median")
    f0 = filter3(F0_OF_BIN.astype(dtype)[bins], "mean")
    f0 = np.where(pdm < dtype(VOICED), dtype(0), f0)
    return dict(bins=bins, pd=pd, f0=f0.astype(dtype), margin=np.abs(pdm.astype(np.float64) - VOICED))


def crepe(t, audio, sample_frame_16k_size, decoder="viterbi", dtype=np.float64):
    """the whole method on one stream: -> dict(frames, p1 .. p6, prob, bins, pd, f0, margin)"""
    F = frames(audio, sample_frame_16k_size, dtype)
    out = network(t, F, dtype)
    out["frames"] = F
    out.update(decode(out["prob"], decoder, dtype))
    return out


# ------------------------------------------------------------------------------------------------ constructed posteriors of the decoder tests
def ridge_case(Tm, seed):
    """a Gaussian bump of width 2 bins wandering by <= 3 bins per frame, and in every eighth frame a decoy spike more than 40 bins away that beats it.  The
    bump peaks 0.3 bins above its integer centre: a symmetric one leaves exact ties between mirror-image paths, which rounding then decides"""
    rng = np.random.default_rng(seed)
    c = np.clip(170 + np.cumsum(rng.integers(-3, 4, Tm)), 100, 240)
    for t in range(1, Tm):          # (the clip may not create a larger step)
        c[t] = c[t - 1] + np.clip(c[t] - c[t - 1], -3, 3)
    i = np.arange(360)
    p = 0.02 + 0.78 * np.exp(-0.5 * ((i[None, :] - c[:, None] - 0.3) / 2.0) ** 2)
    decoy = {}
    for t in range(3, Tm, 8):
        decoy[t] = int(c[t] + (50 if t % 16 == 3 else -45))
        p[t, decoy[t]] = 0.97
    return p.astype(np.float32), c, decoy


def smooth_case(Tm, seed):
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    z = gaussian_filter(rng.standard_normal((Tm, 360)), (2.0, 6.0))
    return (1.0 / (1.0 + np.exp(-3.0 * z / z.std()))).astype(np.float32)
