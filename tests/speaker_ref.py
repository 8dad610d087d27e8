"""Run-time speaker selection in float64: the mix rule and the fold of cond(g) into the conditioned biases.

The speaker enters the synthesizer as g = sum_i w_i emb_g[id_i] through cond(g) = cond_w g + cond_b, a per-channel constant of every WaveNet in-layer of the
flows and of dec_pre.  `fold` gives, for every conditioned layer in model row order -- flow 0 in-layer 0 [2 hidden], flow 0 in-layer 1, ..., dec_pre [up_init],
the order of rvc_debug_speaker_biases -- the bias base_b + cond_b + cond_w g and the magnitude |base_b| + |cond_b| + sum_q |cond_w g| that a bound on an
fp32 evaluation is stated in.  Test infrastructure; never imported by the product."""
from __future__ import annotations

import numpy as np

MAX_MIX = 8


def normalise_mix(mix, n_spk: int):
    """{id: weight} or [(id, weight)] -> (ids, float64 weights summing to 1); ValueError for what rvc_set_speaker_mix answers with RVC_SHAPE"""
    items = list(mix.items()) if isinstance(mix, dict) else [(int(k), float(v)) for k, v in mix]
    if not 1 <= len(items) <= MAX_MIX:
        raise ValueError("1 to 8 (id, weight) pairs")
    ids = [int(k) for k, _ in items]
    w = np.array([float(v) for _, v in items], np.float64)
    if any(not 0 <= i < n_spk for i in ids):
        raise ValueError("an id outside [0, n_spk)")
    if len(set(ids)) != len(ids):
        raise ValueError("a repeated id")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("a weight is negative or not finite")
    s = float(np.sum(w))
    if not s > 0.0 or not np.isfinite(s):
        raise ValueError("the weights sum to 0")
    return ids, w / s


def mix_g(emb, ids, w):
    """g = sum_i w_i emb[id_i] in float64"""
    emb = np.asarray(emb, np.float64)
    return sum(float(wi) * emb[i] for i, wi in zip(ids, w))


def layers(cfg, t):
    """(base_b, cond_w, cond_b) of every conditioned layer, in the order above"""
    H, nl, fn = int(cfg["hidden"]), int(cfg["wn_layers"]), int(cfg["flow_n"])
    out = []
    for i in range(fn):
        cw, cb = t["sy.flow%d.cond.w" % i], t["sy.flow%d.cond.b" % i]
        for j in range(nl):
            out.append((t["sy.flow%d.in%d.b" % (i, j)], cw[j * 2 * H:(j + 1) * 2 * H], cb[j * 2 * H:(j + 1) * 2 * H]))
    out.append((t["sy.dec.pre.b"], t["sy.dec.cond.w"], t["sy.dec.cond.b"]))
    return out


def fold(cfg, t, g):
    """-> (bias, magnitude), both float64 and flat over every conditioned row"""
    g = np.asarray(g, np.float64)
    bias, mag = [], []
    for bb, cw, cb in layers(cfg, t):
        bb, cw, cb = np.asarray(bb, np.float64), np.asarray(cw, np.float64), np.asarray(cb, np.float64)
        prod = cw * g[None, :]
        bias.append(bb + cb + prod.sum(axis=1))
        mag.append(np.abs(bb) + np.abs(cb) + np.abs(prod).sum(axis=1))
    return np.concatenate(bias), np.concatenate(mag)


def fold_bound(cfg, mag):
    """per element: (gin + 8) 2^-24 magnitude -- a sum of gin + 2 fp32 terms whose g is itself a sum of up to 8 (the length of the sums, nothing tuned)"""
    return (int(cfg["gin"]) + 8) * 2.0 ** -24 * np.asarray(mag, np.float64)


def baked(cfg, t, g):
    """the blob a converter would have written for the speaker g: sy.g = g rounded to f32, no table"""
    cfg = {k: v for k, v in cfg.items() if k != "n_spk"}
    t = {k: v for k, v in t.items() if k != "sy.emb_g"}
    t["sy.g"] = np.asarray(g, np.float64).astype(np.float32)
    return cfg, t
