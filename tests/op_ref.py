"""fp64 definitional references of the transformer and recurrent ops of the models (tests/test_gpu_ops.py), pinned to torch float64 by
tests/test_op_ref.py.  Layouts are the engine's: [streams][channels][time].  Plain numpy, written from the operations' definitions, not from the
kernels' indexing."""
import numpy as np

LN_EPS = 1e-5


def _softmax(s):
    s = s - s.max(axis=-1, keepdims=True)
    e = np.exp(s)
    return e / e.sum(axis=-1, keepdims=True)


def _split(qkv, heads, dtype=np.float64):
    qkv = np.asarray(qkv, dtype)
    B, E3, T = qkv.shape
    E = E3 // 3
    hd = E // heads
    q, k, v = (qkv[:, i * E:(i + 1) * E].reshape(B, heads, hd, T) for i in range(3))
    return q, k, v, hd


def mha(qkv, heads, dtype=np.float64):
    """multi-head self-attention: qkv [B][3E][T] (q, k, v rows) -> [B][E][T]; softmax(q_i . k_j / sqrt(hd)) over j, times v_j.
    dtype = np.float32: the same definition evaluated in single precision (what a tolerance is judged against, never a reference)"""
    q, k, v, hd = _split(qkv, heads, dtype)
    B, H, _, T = q.shape
    p = _softmax(np.einsum("bhdi,bhdj->bhij", q, k) / np.sqrt(dtype(hd)))
    return np.einsum("bhij,bhdj->bhdi", p, v).reshape(B, H * hd, T)


def relpos_mha(qkv, heads, rel_k, rel_v, window, dtype=np.float64):
    """VITS windowed relative attention: rel_k / rel_v [2w + 1][hd], row r = offset j - i + w.  Scores q_i . (k_j + rel_k[j - i + w]) / sqrt(hd),
    output sum_j p_ij (v_j + rel_v[j - i + w]); both relative terms are zero outside |j - i| <= w"""
    q, k, v, hd = _split(qkv, heads, dtype)
    B, H, _, T = q.shape
    rk, rv = np.asarray(rel_k, dtype), np.asarray(rel_v, dtype)
    off = np.arange(T)[None, :] - np.arange(T)[:, None]               # [i][j] = j - i
    inside = np.abs(off) <= window
    idx = np.clip(off + window, 0, 2 * window)
    relk = rk[idx] * inside[..., None]                                 # [i][j][hd]
    relv = rv[idx] * inside[..., None]
    s = (np.einsum("bhdi,bhdj->bhij", q, k) + np.einsum("bhdi,ijd->bhij", q, relk)) / np.sqrt(dtype(hd))
    p = _softmax(s)
    o = np.einsum("bhij,bhdj->bhdi", p, v) + np.einsum("bhij,ijd->bhdi", p, relv)
    return o.reshape(B, H * hd, T)


def layernorm(x, g, b):
    """LayerNorm over channels of x [B][C][T] at every time step: (x - mean) / sqrt(var + eps) * g + b, biased variance"""
    x = np.asarray(x, np.float64)
    m = x.mean(axis=1, keepdims=True)
    var = ((x - m) ** 2).mean(axis=1, keepdims=True)
    return (x - m) / np.sqrt(var + LN_EPS) * np.asarray(g, np.float64)[None, :, None] + np.asarray(b, np.float64)[None, :, None]


def _sigmoid(a):
    return 1 / (1 + np.exp(-a))


def gru_bidir(gi, whh, bhh, dtype=np.float64):
    """bidirectional GRU over gate pre-activations: gi [B][6H][T] = W_ih x + b_ih (forward r, z, n rows, then reverse), whh [2][3H][H]
    (weight_hh_l0, _reverse), bhh [2][3H]; h_0 = 0.  -> [B][2H][T] (forward h, then reverse h, at each input position)
        r = s(gi_r + W_hr h + b_hr), z = s(gi_z + W_hz h + b_hz), n = tanh(gi_n + r (W_hn h + b_hn)), h' = (1 - z) n + z h"""
    gi = np.asarray(gi, dtype)
    B, H6, T = gi.shape
    H = H6 // 6
    out = np.zeros((B, 2 * H, T), dtype)
    for d in range(2):
        W, bh = np.asarray(whh[d], dtype), np.asarray(bhh[d], dtype)
        h = np.zeros((B, H), dtype)
        for step in range(T):
            t = step if d == 0 else T - 1 - step
            gx = gi[:, d * 3 * H:(d + 1) * 3 * H, t]
            gh = h @ W.T + bh
            r = _sigmoid(gx[:, :H] + gh[:, :H])
            z = _sigmoid(gx[:, H:2 * H] + gh[:, H:2 * H])
            n = np.tanh(gx[:, 2 * H:] + r * gh[:, 2 * H:])
            h = (1 - z) * n + z * h
            out[:, d * H:(d + 1) * H, t] = h
    return out
