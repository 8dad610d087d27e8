"""Double-precision reference of the convolution layers the models are built from, written in the operations' definitional form: a direct loop
over the taps of a convolution (zero padding, stride, dilation, groups as PyTorch defines them) and a scatter-add over the input positions of a
transposed convolution.  It shares nothing with the kernels' polyphase decomposition or gather tables, and tests/test_layer_ref.py pins it to
torch.float64 on the CPU.  Weights are in PyTorch layout; inputs are [B][C][T] (2-D: [B][C][H][W])."""
import numpy as np
from scipy.special import erf

ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_TANH, ACT_SIGMOID = range(6)


def act(v, kind, slope=0.0):
    v = np.asarray(v, np.float64)
    if kind == ACT_NONE:
        return v
    if kind == ACT_RELU:
        return np.where(v > 0, v, 0.0)
    if kind == ACT_LRELU:
        return np.where(v > 0, v, v * slope)
    if kind == ACT_GELU:
        return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))
    if kind == ACT_TANH:
        return np.tanh(v)
    if kind == ACT_SIGMOID:
        return 1.0 / (1.0 + np.exp(-v))
    raise ValueError(kind)


def conv1d(x, w, bias=None, stride=1, pad=0, dil=1, groups=1):
    """out[b, o, t] = bias[o] + sum_{c in group(o), k} w[o, c, k] * x[b, c, t * stride + k * dil - pad] (zero outside [0, T))."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    B, Cin, T = x.shape
    Cout, cig, K = w.shape
    assert Cin == cig * groups and Cout % groups == 0
    cog = Cout // groups
    Tout = (T + 2 * pad - dil * (K - 1) - 1) // stride + 1
    need = (Tout - 1) * stride + (K - 1) * dil + 1
    xp = np.zeros((B, Cin, max(need, T + 2 * pad)), np.float64)
    xp[:, :, pad:pad + T] = x
    out = np.zeros((B, Cout, Tout), np.float64)
    for g in range(groups):
        xg = xp[:, g * cig:(g + 1) * cig]
        for k in range(K):
            tap = xg[:, :, k * dil:k * dil + (Tout - 1) * stride + 1:stride]          # x at t * stride + k * dil - pad, t = 0 .. Tout-1
            out[:, g * cog:(g + 1) * cog] += np.matmul(np.ascontiguousarray(w[g * cog:(g + 1) * cog, :, k]), tap)      # (a contiguous tap matrix: the strided view takes matmul's slow path)
    if bias is not None:
        out += np.asarray(bias, np.float64)[None, :, None]
    return out


def conv_transpose1d(x, w, bias=None, stride=1, pad=0):
    """Every input position scatters its taps: out[b, o, t * stride + k - pad] += w[c, o, k] * x[b, c, t]; w is [Cin][Cout][K]."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    B, Cin, T = x.shape
    _, Cout, K = w.shape
    full = np.zeros((B, Cout, (T - 1) * stride + K), np.float64)
    for k in range(K):
        full[:, :, k:k + (T - 1) * stride + 1:stride] += np.matmul(np.ascontiguousarray(w[:, :, k].T), x)      # tap k of every input position t lands on t * stride + k
    Tout = (T - 1) * stride - 2 * pad + K
    out = full[:, :, pad:pad + Tout].copy()
    if bias is not None:
        out += np.asarray(bias, np.float64)[None, :, None]
    return out


def conv2d_3x3(x, w, bias=None):
    """3x3 convolution, padding 1: out[b, o, h, v] = bias[o] + sum_{c, i, j} w[o, c, i, j] * x[b, c, h + i - 1, v + j - 1]."""
    x = np.asarray(x, np.float64); w = np.asarray(w, np.float64)
    B, Cin, H, W = x.shape
    Cout = w.shape[0]
    xp = np.zeros((B, Cin, H + 2, W + 2), np.float64)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    out = np.zeros((B, Cout, H, W), np.float64)
    for i in range(3):
        for j in range(3):
            out += np.einsum("oc,bchw->bohw", w[:, :, i, j], xp[:, :, i:i + H, j:j + W])
    if bias is not None:
        out += np.asarray(bias, np.float64)[None, :, None, None]
    return out


def glu_gate(a):
    """WaveNet gate on [B][2H][T] pre-activations: tanh of the first H channels times sigmoid of the last H."""
    h = a.shape[1] // 2
    return np.tanh(a[:, :h]) * (1.0 / (1.0 + np.exp(-a[:, h:])))
