"""ContentVec and RMVPE split at the engine's tap boundaries, one function per stage, evaluated in float64.  The layers
are torch_ref.py's, run under torch_ref.precision(), as synth_ref.py does for the synthesizer: nothing is restated here but what the engine adds to the
models -- the not yet normalised ("raw") taps of plans that fold their LayerNorms into the neighbouring GEMMs, and that folded form itself, restated in
torch as the second yardstick of those stages.

Every function takes a blob's config and tensors (PyTorch layout) and numpy arrays shaped like the taps -- ContentVec [C][T], RMVPE images [C][H = Tm][W = 128],
the GRU's side [C][Tm] -- and returns a float64 array.  `dtype=torch.float32` evaluates the same stage in fp32 (synth_ref.stage_delta32).  The keyword
arguments `pad`, `drop`, `pick`, `swap` and `skip_pending` plant the mistakes of tests/test_front_stage_ref.py's bite check; nothing else sets them.
Test infrastructure; never imported by the product."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import front_ref as FR
import torch_ref as TR
from synth_ref import F64, _run, max_over_rms, stage_delta32  # noqa: F401  (the metrics are the synthesizer's)

EPS = 1e-5


# ---- ContentVec -----------------------------------------------------------------------------------------------------------------------------
def cv_conv0(cfg, t, audio, dtype=F64):
    """the stream's input audio [L] -> cv.conv0"""
    return _run(dtype, lambda x: TR.cv_conv0(cfg, t, x), np.asarray(audio).reshape(-1))


def cv_stem(cfg, t, conv0, dtype=F64):
    """cv.conv0 -> cv.feat"""
    return _run(dtype, lambda x: TR.cv_stem(cfg, t, x), conv0)


def cv_proj(cfg, t, feat, dtype=F64):
    """cv.feat -> cv.proj"""
    return _run(dtype, lambda x: TR.cv_proj(cfg, t, x), feat)


def cv_pos(cfg, t, proj, dtype=F64, **flaw):
    """cv.proj -> cv.pos"""
    return _run(dtype, lambda x: TR.cv_pos(cfg, t, x, True, **flaw), proj)


def cv_pos_raw(cfg, t, proj, dtype=F64, **flaw):
    """cv.proj -> cv.pos.raw: the same without the encoder's LayerNorm"""
    return _run(dtype, lambda x: TR.cv_pos(cfg, t, x, False, **flaw), proj)


def cv_layer(cfg, t, l, x, dtype=F64):
    """cv.l{l-1} (cv.pos) -> cv.l{l}"""
    return _run(dtype, lambda a: TR.cv_layer(cfg, t, l, a), x)


def cv_layer_raw(cfg, t, l, x_raw, dtype=F64, norm=False, skip_pending=False):
    """cv.l{l-1}.raw (cv.pos.raw) -> cv.l{l}.raw: the pending LayerNorm on the input, then the layer without its ln2 (norm=True: with it -- the last layer
    of a folded plan publishes cv.l{last}).  skip_pending: the planted mistake -- the residual takes the raw input, the projections the normalised one"""
    g, b = TR.cv_pending_ln(cfg, t, l)

    def f(a):
        x = TR._ln_c(a, TR._t(g), TR._t(b))
        if not skip_pending:
            return TR.cv_layer(cfg, t, l, x, norm)
        pre = "cv.l%d." % l
        h = TR._ln_c(a + TR.cv_attention(cfg, t, l, x), TR._t(t[pre + "ln1.g"]), TR._t(t[pre + "ln1.b"]))
        y = h + TR._lin_c(F.gelu(TR._lin_c(h, t[pre + "ff1.w"], t[pre + "ff1.b"])), t[pre + "ff2.w"], t[pre + "ff2.b"])
        return TR._ln_c(y, TR._t(t[pre + "ln2.g"]), TR._t(t[pre + "ln2.b"])) if norm else y
    return _run(dtype, f, x_raw)


def cv_layer_raw_last(cfg, t, l, x_raw, dtype=F64):
    """cv.l{l-1}.raw -> cv.l{l}: the last layer of a folded plan"""
    return cv_layer_raw(cfg, t, l, x_raw, dtype, norm=True)


def cv_final_proj(cfg, t, x, dtype=F64):
    """cv.l{last} -> cv.out of a v1 model"""
    return _run(dtype, lambda a: TR.cv_final_proj(cfg, t, a), x)


def layer_norm_ct(x, g, b):
    """LayerNorm over the channels of [C][T] in float64"""
    return _run(F64, lambda a: TR._ln_c(a, TR._t(g), TR._t(b)), x)


# ---- the folded form: LayerNorm + Linear as ONE product on the not yet normalised columns ---------------------------------------------------------
# LN(x)[k] = (x[k] - mean) rstd g[k] + beta[k] per column, so W LN(x) + b = rstd (W diag(g) x - mean wsum) + (b + W beta), wsum[m] = sum_k W[m][k] g[k]:
# the product runs on the raw columns, their mean and rstd are applied to its result.  Written here as the algebra says, not as the kernels index.
def _col_stats(x):
    mean = x.mean(1, keepdim=True)
    return mean, torch.rsqrt(((x - mean) ** 2).mean(1, keepdim=True) + EPS)


def folded_linear(x, w, b, g, beta):
    """x (1, K, T) not normalised -> Linear(LayerNorm(x; g, beta); w, b) in the folded form"""
    w, b, g, beta = TR._t(w), TR._t(b), TR._t(g), TR._t(beta)
    wf = w * g[None, :]
    wsum, bf = wf.sum(1), b + w @ beta
    mean, rstd = _col_stats(x)
    return rstd * (F.conv1d(x, wf[:, :, None]) - mean * wsum[None, :, None]) + bf[None, :, None]


def _ln_from_stats(x, g, beta):
    mean, rstd = _col_stats(x)
    return (x - mean) * rstd * TR._t(g)[None, :, None] + TR._t(beta)[None, :, None]


def cv_proj_folded(cfg, t, feat, dtype=F64):
    """cv.feat -> cv.proj as one folded product"""
    return _run(dtype, lambda x: folded_linear(x, t["cv.proj.w"], t["cv.proj.b"], t["cv.ln0.g"], t["cv.ln0.b"]), feat)


def cv_layer_folded(cfg, t, l, x_raw, dtype=F64, norm=False):
    """cv.l{l-1}.raw -> cv.l{l}.raw as a folded plan computes it: q / k / v folded with the pending LayerNorm, the residual behind the output projection
    normalised from the same column statistics, ff1 folded with ln1, ff2's residual normalised from ln1's statistics"""
    g, b = TR.cv_pending_ln(cfg, t, l)
    pre, heads = "cv.l%d." % l, int(cfg["heads"])

    def f(a):
        _, E, T = a.shape
        d = E // heads
        q, k, v = (folded_linear(a, t[pre + n + ".w"], t[pre + n + ".b"], g, b) for n in "qkv")
        q, k, v = (z.view(1, heads, d, T).transpose(2, 3) for z in (q * d ** -0.5, k, v))
        att = torch.matmul(F.softmax(torch.matmul(q, k.transpose(-2, -1)), dim=-1), v).transpose(2, 3).contiguous().view(1, E, T)
        h = TR._lin_c(att, t[pre + "o.w"], t[pre + "o.b"]) + _ln_from_stats(a, g, b)
        ff = F.gelu(folded_linear(h, t[pre + "ff1.w"], t[pre + "ff1.b"], t[pre + "ln1.g"], t[pre + "ln1.b"]))
        y = TR._lin_c(ff, t[pre + "ff2.w"], t[pre + "ff2.b"]) + _ln_from_stats(h, t[pre + "ln1.g"], t[pre + "ln1.b"])
        return TR._ln_c(y, TR._t(t[pre + "ln2.g"]), TR._t(t[pre + "ln2.b"])) if norm else y
    return _run(dtype, f, x_raw)


def cv_layer_folded_last(cfg, t, l, x_raw, dtype=F64):
    return cv_layer_folded(cfg, t, l, x_raw, dtype, norm=True)


def folded_delta32(plain, folded, *args):
    """(ref64, delta32) of a stage a plan runs in folded form: the fp64 value is the layer-by-layer one; delta32 is the larger of torch's fp32 evaluation
    layer by layer and of the fp32 folded algebra above, both against it.  Neither involves the engine."""
    r64, d_plain = stage_delta32(plain, *args)
    return r64, max(d_plain, max_over_rms(folded(*args, dtype=torch.float32), r64))


# ---- RMVPE ----------------------------------------------------------------------------------------------------------------------------------
def rm_mel(audio, frame):
    """the stream's audio -> rm.mel [128][Tm]: front_ref's float64 log-mel of the last `frame` samples"""
    return FR.logmel(np.asarray(audio), int(frame))


def rm_enc0(cfg, t, mel, dtype=F64):
    """rm.mel [128][Tm] -> rm.enc0 [C][Tm][128]"""
    return _run(dtype, lambda m: TR.rm_enc(cfg, t, 0, TR.rm_input(cfg, t, m)), mel)


def rm_enc(cfg, t, lv, x, dtype=F64, **flaw):
    """rm.enc{lv-1} -> rm.enc{lv}, lv >= 1"""
    return _run(dtype, lambda a: TR.rm_enc(cfg, t, lv, a, **flaw), x)


def rm_int(cfg, t, x, dtype=F64, **flaw):
    """rm.enc{last} -> rm.int"""
    return _run(dtype, lambda a: TR.rm_int(cfg, t, a, **flaw), x)


def rm_dec(cfg, t, lv, x, skip, dtype=F64, **flaw):
    """(rm.dec{lv-1} or rm.int, rm.enc{levels-1-lv}) -> rm.dec{lv}"""
    return _run(dtype, lambda a, s: TR.rm_dec(cfg, t, lv, a, s, **flaw), x, skip)


def rm_cnn(cfg, t, x, dtype=F64):
    """rm.dec{last} -> rm.cnn_ct [3 * 128][Tm]"""
    return _run(dtype, lambda a: TR.rm_cnn(cfg, t, a), x)


def rm_gru(cfg, t, feat, dtype=F64):
    """rm.cnn_ct -> rm.gru_ct [2 H][Tm]"""
    return _run(dtype, lambda a: TR.rm_gru(cfg, t, a), feat)


def rm_sal(cfg, t, y, dtype=F64):
    """rm.gru_ct -> rm.sal_ct [360][Tm]"""
    return _run(dtype, lambda a: TR.rm_sal(cfg, t, a), y)


def rm_shapes(cfg, Tm, n_mels=128):
    """[C][H][W] of rm.enc{lv}, rm.int and rm.dec{lv}"""
    levels, co = int(cfg["levels"]), int(cfg["en_out"])
    out = {}
    for lv in range(levels):
        out["rm.enc%d" % lv] = (co << lv, Tm >> lv, n_mels >> lv)
    out["rm.int"] = (co << levels, Tm >> levels, n_mels >> levels)
    for lv in range(levels):
        sl = levels - 1 - lv
        out["rm.dec%d" % lv] = (co << sl, Tm >> sl, n_mels >> sl)
    return out


def mel_frame(sample_frame_16k):
    """the samples RMVPE analyses (the reference's f0_extractor_frame) and the mel frame count"""
    fr = 5120 * ((int(sample_frame_16k) + 800 - 1) // 5120 + 1) - 160
    return fr, 1 + fr // 160


# ---- the stages of one stream, from its taps --------------------------------------------------------------------------------------------------------
# One list for the CPU pin (the oracle's taps) and the GPU test (the engine's): (stage, kind, got, fn, args, folded fn or None).  kind: "single" (one
# launch: the per-layer bound), "multi" (bound from the stage's own delta32), "bits" (got must equal args[0] bit for bit).  get(name, shape) returns the
# tap reshaped (-1 for one free dimension); has(name) says whether the plan published it.
def cv_stages(cfg, t, audio, get, has):
    C, E, n = int(cfg["conv_dim"]), int(cfg["embed"]), int(cfg["run_layers"])
    conv0, feat, proj = get("cv.conv0", (C, -1)), get("cv.feat", (C, -1)), get("cv.proj", (E, -1))
    raw = has("cv.pos.raw")
    out = [("cv.conv0", "single", conv0, cv_conv0, (cfg, t, audio), None),
           ("cv.stem", "multi", feat, cv_stem, (cfg, t, conv0), None),
           ("cv.proj", "multi", proj, cv_proj, (cfg, t, feat), cv_proj_folded if raw else None)]
    x = get("cv.pos.raw" if raw else "cv.pos", (E, -1))
    out.append(("cv.pos.raw" if raw else "cv.pos", "multi", x, cv_pos_raw if raw else cv_pos, (cfg, t, proj), None))
    for l in range(n):
        to_raw = has("cv.l%d.raw" % l)
        assert not to_raw or (raw and l + 1 < n), "a raw tap behind a normalised one, or on the last layer"
        y = get("cv.l%d.raw" % l if to_raw else "cv.l%d" % l, (E, -1))
        if raw:
            fn, fold = (cv_layer_raw, cv_layer_folded) if to_raw else (cv_layer_raw_last, cv_layer_folded_last)
        else:
            fn, fold = cv_layer, None
        out.append(("cv.l%d.raw" % l if to_raw else "cv.l%d" % l, "multi", y, fn, (cfg, t, l, x), fold))
        x, raw = y, to_raw
    assert not raw
    o = get("cv.out", (int(cfg["out_dim"]), -1))
    if int(cfg["out_dim"]) == E:
        out.append(("cv.out", "bits", o, None, (x,), None))
    else:
        out.append(("cv.out", "single", o, cv_final_proj, (cfg, t, x), None))
    return out


def rm_stages(cfg, t, audio, frame, get):
    fr, Tm = mel_frame(frame)
    levels, shp = int(cfg["levels"]), rm_shapes(cfg, Tm)

    def img(name):
        return get(name, (-1,) + shp[name][1:])
    mel = get("rm.mel", (128, Tm))
    out = [("rm.mel", "single", mel, lambda a, dtype=F64: rm_mel(a, fr), (audio,), None)]
    enc = [img("rm.enc%d" % lv) for lv in range(levels)]
    out.append(("rm.enc0", "multi", enc[0], rm_enc0, (cfg, t, mel), None))
    for lv in range(1, levels):
        out.append(("rm.enc%d" % lv, "multi", enc[lv], rm_enc, (cfg, t, lv, enc[lv - 1]), None))
    x = img("rm.int")
    out.append(("rm.int", "multi", x, rm_int, (cfg, t, enc[-1]), None))
    for lv in range(levels):
        y = img("rm.dec%d" % lv)
        out.append(("rm.dec%d" % lv, "multi", y, rm_dec, (cfg, t, lv, x, enc[levels - 1 - lv]), None))
        x = y
    cnn, gru, sal = get("rm.cnn_ct", (3 * 128, Tm)), get("rm.gru_ct", (2 * int(cfg["gru_hidden"]), Tm)), get("rm.sal_ct", (int(cfg["n_out"]), Tm))
    out += [("rm.cnn", "single", cnn, rm_cnn, (cfg, t, x), None), ("rm.gru", "multi", gru, rm_gru, (cfg, t, cnn), None),
            ("rm.sal", "single", sal, rm_sal, (cfg, t, gru), None)]
    return out


TOL = 2e-5                 # the per-layer bound of tests/test_gpu_tiles.py


def judge(kind, got, fn, args, fold):
    """-> (e, bound, delta32 or None) of one stage of the lists above ("single" / "multi")"""
    if kind == "single":
        return max_over_rms(got, fn(*args)), TOL, None
    ref, d32 = folded_delta32(fn, fold, *args) if fold else stage_delta32(fn, *args)
    return max_over_rms(got, ref), max(TOL, 4 * d32), d32
