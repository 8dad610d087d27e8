"""Independent torch-CPU implementations of the three networks, used ONLY to
pin the C oracle's dense layers (the oracle's im2col+sgemm code vs torch's conv/linear/GRU kernels, and
ContentVec vs the HuggingFace HuBERT class).  Test infrastructure; never imported by the product."""
from __future__ import annotations

import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F


_DTYPE = [torch.float32]


@contextlib.contextmanager
def precision(dtype):
    """Evaluate the layers below in `dtype` (synth_ref.py: torch.float64); the default is fp32, what the oracle is pinned against."""
    _DTYPE.append(dtype)
    try:
        yield
    finally:
        _DTYPE.pop()


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype or _DTYPE[-1])


# ------------------------------------------------------------------------------------------------
# ContentVec through transformers.HubertModel with the blob's weights copied in
# ------------------------------------------------------------------------------------------------
def contentvec_hf(cfg, tens, wav: np.ndarray) -> np.ndarray:
    """Returns (C_out, T) like the oracle's contentvec_forward."""
    from transformers import HubertConfig, HubertModel

    E, C = int(cfg["embed"]), int(cfg["conv_dim"])
    hc = HubertConfig(
        hidden_size=E, num_hidden_layers=int(cfg["run_layers"]), num_attention_heads=int(cfg["heads"]),
        intermediate_size=int(cfg["ffn"]), hidden_act="gelu", hidden_dropout=0.0, activation_dropout=0.0,
        attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, feat_proj_layer_norm=True,
        feat_extract_norm="group", feat_extract_activation="gelu", conv_dim=[C] * 7,
        conv_stride=[int(cfg["conv_s%d" % i]) for i in range(7)], conv_kernel=[int(cfg["conv_k%d" % i]) for i in range(7)],
        conv_bias=False, num_conv_pos_embeddings=int(cfg["pos_k"]), num_conv_pos_embedding_groups=int(cfg["pos_groups"]),
        do_stable_layer_norm=False, apply_spec_augment=False, layer_norm_eps=1e-5)
    m = HubertModel(hc).eval()
    sd = {}
    for i in range(7):
        sd["feature_extractor.conv_layers.%d.conv.weight" % i] = _t(tens["cv.conv%d.w" % i])
    sd["feature_extractor.conv_layers.0.layer_norm.weight"] = _t(tens["cv.gn.g"])
    sd["feature_extractor.conv_layers.0.layer_norm.bias"] = _t(tens["cv.gn.b"])
    sd["feature_projection.layer_norm.weight"] = _t(tens["cv.ln0.g"])
    sd["feature_projection.layer_norm.bias"] = _t(tens["cv.ln0.b"])
    sd["feature_projection.projection.weight"] = _t(tens["cv.proj.w"])
    sd["feature_projection.projection.bias"] = _t(tens["cv.proj.b"])
    sd["encoder.layer_norm.weight"] = _t(tens["cv.enc_ln.g"])
    sd["encoder.layer_norm.bias"] = _t(tens["cv.enc_ln.b"])
    for l in range(int(cfg["run_layers"])):
        p, q = "encoder.layers.%d." % l, "cv.l%d." % l
        for hf, mine in (("q_proj", "q"), ("k_proj", "k"), ("v_proj", "v"), ("out_proj", "o")):
            sd[p + "attention.%s.weight" % hf] = _t(tens[q + mine + ".w"])
            sd[p + "attention.%s.bias" % hf] = _t(tens[q + mine + ".b"])
        sd[p + "layer_norm.weight"] = _t(tens[q + "ln1.g"]); sd[p + "layer_norm.bias"] = _t(tens[q + "ln1.b"])
        sd[p + "feed_forward.intermediate_dense.weight"] = _t(tens[q + "ff1.w"]); sd[p + "feed_forward.intermediate_dense.bias"] = _t(tens[q + "ff1.b"])
        sd[p + "feed_forward.output_dense.weight"] = _t(tens[q + "ff2.w"]); sd[p + "feed_forward.output_dense.bias"] = _t(tens[q + "ff2.b"])
        sd[p + "final_layer_norm.weight"] = _t(tens[q + "ln2.g"]); sd[p + "final_layer_norm.bias"] = _t(tens[q + "ln2.b"])
    missing, unexpected = m.load_state_dict(sd, strict=False)
    # the positional conv is weight-normed in HF; bypass the parametrisation by calling the conv functionally below
    missing = [k for k in missing if "pos_conv_embed" not in k and "masked_spec_embed" not in k]
    assert not missing and not unexpected, (missing, unexpected)
    pos_w, pos_b = _t(tens["cv.pos.w"]), _t(tens["cv.pos.b"])
    with torch.no_grad():
        x = _t(wav)[None]
        feats = m.feature_extractor(x).transpose(1, 2)        # (1, T, C)
        h = m.feature_projection(feats)
        if isinstance(h, tuple):
            h = h[0]
        pk = int(cfg["pos_k"])
        pc = F.conv1d(h.transpose(1, 2), pos_w, pos_b, padding=pk // 2, groups=int(cfg["pos_groups"]))
        if pk % 2 == 0:
            pc = pc[:, :, :-1]
        h = h + F.gelu(pc).transpose(1, 2)
        h = m.encoder.layer_norm(h)
        for layer in m.encoder.layers:
            out = layer(h)
            h = out[0] if isinstance(out, tuple) else out
        if int(cfg["out_dim"]) != E:
            h = F.linear(h, _t(tens["cv.final_proj.w"]), _t(tens["cv.final_proj.b"]))
    return h[0].transpose(0, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------------
# RMVPE network
# ------------------------------------------------------------------------------------------------
def _cbr(t, pre, x):
    y = F.relu(F.conv2d(x, _t(t[pre + "c1.w"]), _t(t[pre + "c1.b"]), padding=1))
    y = F.relu(F.conv2d(y, _t(t[pre + "c2.w"]), _t(t[pre + "c2.b"]), padding=1))
    if pre + "sc.w" in t:
        w = _t(t[pre + "sc.w"])
        return y + F.conv2d(x, w[:, :, None, None], _t(t[pre + "sc.b"]))
    return y + x


def rmvpe_salience(cfg, t, mel: np.ndarray) -> np.ndarray:
    """mel (128, Tm) -> salience (Tm, 360)."""
    levels, nb, inter = int(cfg["levels"]), int(cfg["n_blocks"]), int(cfg["inter_layers"])
    H = int(cfg["gru_hidden"])
    with torch.no_grad():
        x = _t(mel).transpose(0, 1)[None, None] * float(t["rm.bn0"][0]) + float(t["rm.bn0"][1])
        skips = []
        for lv in range(levels):
            for j in range(nb):
                x = _cbr(t, "rm.enc%d.b%d." % (lv, j), x)
            skips.append(x)
            x = F.avg_pool2d(x, 2)
        for lv in range(inter):
            for j in range(nb):
                x = _cbr(t, "rm.int%d.b%d." % (lv, j), x)
        for lv in range(levels):
            x = F.relu(F.conv_transpose2d(x, _t(t["rm.dec%d.up.w" % lv]), _t(t["rm.dec%d.up.b" % lv]), stride=2, padding=1, output_padding=1))
            x = torch.cat([x, skips[-1 - lv]], dim=1)
            for j in range(nb):
                x = _cbr(t, "rm.dec%d.b%d." % (lv, j), x)
        x = F.conv2d(x, _t(t["rm.cnn.w"]), _t(t["rm.cnn.b"]), padding=1)
        x = x.transpose(1, 2).flatten(-2)                 # (1, Tm, 3*n_mels)
        gru = torch.nn.GRU(x.shape[-1], H, num_layers=1, batch_first=True, bidirectional=True)
        gru.weight_ih_l0.copy_(_t(t["rm.gru.w_ih_f"])); gru.weight_hh_l0.copy_(_t(t["rm.gru.w_hh_f"]))
        gru.bias_ih_l0.copy_(_t(t["rm.gru.b_ih_f"])); gru.bias_hh_l0.copy_(_t(t["rm.gru.b_hh_f"]))
        gru.weight_ih_l0_reverse.copy_(_t(t["rm.gru.w_ih_b"])); gru.weight_hh_l0_reverse.copy_(_t(t["rm.gru.w_hh_b"]))
        gru.bias_ih_l0_reverse.copy_(_t(t["rm.gru.b_ih_b"])); gru.bias_hh_l0_reverse.copy_(_t(t["rm.gru.b_hh_b"]))
        y, _ = gru(x)
        y = torch.sigmoid(F.linear(y, _t(t["rm.fc.w"]), _t(t["rm.fc.b"])))
    return y[0].numpy()


def _ln_c(x, g, b):
    return F.layer_norm(x.transpose(1, 2), (x.shape[1],), g, b, 1e-5).transpose(1, 2)


# ------------------------------------------------------------------------------------------------
# ContentVec and RMVPE in pieces, each a function of torch tensors with a leading batch axis of 1, written with torch.nn.functional alone
# (tests/front_stage_ref.py evaluates them one at a time in fp64 under precision(); tests/test_front_stage_ref.py pins their fp32 chain
# to contentvec_hf / rmvpe_salience above and to the oracle's taps).  The keyword arguments that are not None / True / "back" / False by
# default exist for the planted mistakes of that test only.
# ------------------------------------------------------------------------------------------------
def _lin_c(x, w, b=None):
    """a Linear layer on [1][C][T]"""
    return F.conv1d(x, _t(w)[:, :, None], None if b is None else _t(b))


def cv_conv0(cfg, t, wav):
    """wav (1, L) -> (1, C, T0): Conv1d(1 -> C, no bias) + GroupNorm with one group per channel + GELU"""
    C = int(cfg["conv_dim"])
    y = F.conv1d(wav[:, None], _t(t["cv.conv0.w"]), stride=int(cfg["conv_s0"]))
    return F.gelu(F.group_norm(y, C, _t(t["cv.gn.g"]), _t(t["cv.gn.b"]), 1e-5))


def cv_stem(cfg, t, x):
    """the six strided convolutions behind the first, each followed by GELU"""
    for i in range(1, 7):
        x = F.gelu(F.conv1d(x, _t(t["cv.conv%d.w" % i]), stride=int(cfg["conv_s%d" % i])))
    return x


def cv_proj(cfg, t, x):
    return _lin_c(_ln_c(x, _t(t["cv.ln0.g"]), _t(t["cv.ln0.b"])), t["cv.proj.w"], t["cv.proj.b"])


def cv_pos(cfg, t, h, norm=True, pad=None, drop="back"):
    """h + GELU(grouped positional convolution), then the encoder's LayerNorm (norm=False: the sum alone)"""
    pk = int(cfg["pos_k"])
    pc = F.conv1d(h, _t(t["cv.pos.w"]), _t(t["cv.pos.b"]), padding=pk // 2 if pad is None else pad, groups=int(cfg["pos_groups"]))
    if pk % 2 == 0:
        pc = pc[:, :, :-1] if drop == "back" else pc[:, :, 1:]
    if pc.shape[2] != h.shape[2]:                       # (a planted padding mistake shortens the convolution: aligned at the front)
        pc = F.pad(pc, (0, h.shape[2] - pc.shape[2]))
    x = h + F.gelu(pc)
    return _ln_c(x, _t(t["cv.enc_ln.g"]), _t(t["cv.enc_ln.b"])) if norm else x


def cv_attention(cfg, t, l, x):
    """HuBERT self-attention of layer l including the output projection, without the residual"""
    pre, heads = "cv.l%d." % l, int(cfg["heads"])
    b, E, T = x.shape
    d = E // heads
    q = _lin_c(x, t[pre + "q.w"], t[pre + "q.b"]) * d ** -0.5
    k = _lin_c(x, t[pre + "k.w"], t[pre + "k.b"])
    v = _lin_c(x, t[pre + "v.w"], t[pre + "v.b"])
    q, k, v = (a.view(b, heads, d, T).transpose(2, 3) for a in (q, k, v))
    p = F.softmax(torch.matmul(q, k.transpose(-2, -1)), dim=-1)
    a = torch.matmul(p, v).transpose(2, 3).contiguous().view(b, E, T)
    return _lin_c(a, t[pre + "o.w"], t[pre + "o.b"])


def cv_layer(cfg, t, l, x, norm=True):
    """post-LN HuBERT layer l (norm=False: up to and including the residual sum behind ff2, without its LayerNorm)"""
    pre = "cv.l%d." % l
    h = _ln_c(x + cv_attention(cfg, t, l, x), _t(t[pre + "ln1.g"]), _t(t[pre + "ln1.b"]))
    y = h + _lin_c(F.gelu(_lin_c(h, t[pre + "ff1.w"], t[pre + "ff1.b"])), t[pre + "ff2.w"], t[pre + "ff2.b"])
    return _ln_c(y, _t(t[pre + "ln2.g"]), _t(t[pre + "ln2.b"])) if norm else y


def cv_pending_ln(cfg, t, l):
    """the LayerNorm a not yet normalised input of layer l is waiting for: the encoder's for layer 0, ln2 of layer l - 1 otherwise"""
    return (t["cv.enc_ln.g"], t["cv.enc_ln.b"]) if l == 0 else (t["cv.l%d.ln2.g" % (l - 1)], t["cv.l%d.ln2.b" % (l - 1)])


def cv_final_proj(cfg, t, x):
    return _lin_c(x, t["cv.final_proj.w"], t["cv.final_proj.b"])


def rm_input(cfg, t, mel):
    """log-mel (1, 128, Tm) -> the network's image (1, 1, Tm, 128)"""
    return mel.transpose(1, 2)[:, None] * float(t["rm.bn0"][0]) + float(t["rm.bn0"][1])


def rm_blocks(t, fmt, n, x):
    for j in range(n):
        x = _cbr(t, fmt % j, x)
    return x


def rm_pool(x, pick=False):
    """AvgPool2d(2) (pick: the planted mistake, the top left pixel of every 2 x 2 square)"""
    return x[:, :, ::2, ::2] if pick else F.avg_pool2d(x, 2)


def rm_enc(cfg, t, lv, x, pick=False):
    """encoder level lv from the previous level's output before its pooling (level 0: from rm_input's image)"""
    if lv > 0:
        x = rm_pool(x, pick)
    return rm_blocks(t, "rm.enc%d.b%%d." % lv, int(cfg["n_blocks"]), x)


def rm_int(cfg, t, x, pick=False):
    x = rm_pool(x, pick)
    for lv in range(int(cfg["inter_layers"])):
        x = rm_blocks(t, "rm.int%d.b%%d." % lv, int(cfg["n_blocks"]), x)
    return x


def rm_dec(cfg, t, lv, x, skip, swap=False):
    """decoder level lv: transposed convolution + ReLU, concat (up first, skip second; swap: the planted mistake), blocks"""
    up = F.relu(F.conv_transpose2d(x, _t(t["rm.dec%d.up.w" % lv]), _t(t["rm.dec%d.up.b" % lv]), stride=2, padding=1, output_padding=1))
    return rm_blocks(t, "rm.dec%d.b%%d." % lv, int(cfg["n_blocks"]), torch.cat([skip, up] if swap else [up, skip], dim=1))


def rm_cnn(cfg, t, x):
    """the head convolution in the GRU's layout: (1, 3 * 128, Tm), row c * 128 + mel"""
    y = F.conv2d(x, _t(t["rm.cnn.w"]), _t(t["rm.cnn.b"]), padding=1)           # (1, 3, Tm, 128)
    return y.permute(0, 1, 3, 2).reshape(y.shape[0], -1, y.shape[2])


def rm_gru(cfg, t, feat):
    """(1, 384, Tm) -> (1, 2 H, Tm): input projection + bidirectional GRU"""
    H = int(cfg["gru_hidden"])
    gru = torch.nn.GRU(feat.shape[1], H, num_layers=1, batch_first=True, bidirectional=True).to(feat.dtype)
    for sfx, mine in (("", "f"), ("_reverse", "b")):
        for hf, nm in (("weight_ih", "w_ih"), ("weight_hh", "w_hh"), ("bias_ih", "b_ih"), ("bias_hh", "b_hh")):
            getattr(gru, hf + "_l0" + sfx).copy_(_t(t["rm.gru.%s_%s" % (nm, mine)]))
    return gru(feat.transpose(1, 2))[0].transpose(1, 2)


def rm_sal(cfg, t, y):
    return torch.sigmoid(_lin_c(y, t["rm.fc.w"], t["rm.fc.b"]))


# ------------------------------------------------------------------------------------------------
# synthesizer
# ------------------------------------------------------------------------------------------------


def _rel_attn(t, l, x, heads, window):
    pre = "sy.enc.l%d." % l
    q = F.conv1d(x, _t(t[pre + "q.w"])[:, :, None], _t(t[pre + "q.b"]))
    k = F.conv1d(x, _t(t[pre + "k.w"])[:, :, None], _t(t[pre + "k.b"]))
    v = F.conv1d(x, _t(t[pre + "v.w"])[:, :, None], _t(t[pre + "v.b"]))
    b, d, T = q.shape
    kc = d // heads
    q = q.view(b, heads, kc, T).transpose(2, 3)
    k = k.view(b, heads, kc, T).transpose(2, 3)
    v = v.view(b, heads, kc, T).transpose(2, 3)
    scores = torch.matmul(q / math.sqrt(kc), k.transpose(-2, -1))
    rk, rv = _t(t[pre + "rel_k"]), _t(t[pre + "rel_v"])
    idx = torch.arange(T)[None, :] - torch.arange(T)[:, None]           # j - i
    valid = (idx.abs() <= window)
    e = (idx + window).clamp(0, 2 * window)
    relk = rk[e] * valid[..., None]                                      # (T, T, kc)
    scores = scores + torch.einsum("bhid,ijd->bhij", q / math.sqrt(kc), relk)
    p = F.softmax(scores, dim=-1)
    out = torch.matmul(p, v)
    relv = rv[e] * valid[..., None]
    out = out + torch.einsum("bhij,ijd->bhid", p, relv)
    out = out.transpose(2, 3).contiguous().view(b, d, T)
    return F.conv1d(out, _t(t[pre + "o.w"])[:, :, None], _t(t[pre + "o.b"]))


# The synthesizer in pieces, each a function of torch tensors with a leading batch axis of 1 (synth_until_z / synth_decoder chain them in fp32;
# tests/synth_ref.py evaluates them one at a time in fp64 under precision()).
def sy_embed(cfg, t, phone, pitch):
    """phone (R, C), pitch int (R,) -> (1, H, R)"""
    Hd = int(cfg["hidden"])
    x = F.linear(_t(phone)[None], _t(t["sy.enc.phone.w"]), _t(t["sy.enc.phone.b"])) + _t(t["sy.enc.pitch_emb"])[torch.from_numpy(np.asarray(pitch).astype(np.int64))][None]
    return F.leaky_relu(x * math.sqrt(Hd), 0.1).transpose(1, 2)


def sy_encoder(cfg, t, x):
    heads, window, ek = int(cfg["heads"]), int(cfg["window"]), int(cfg["enc_k"])
    for l in range(int(cfg["enc_layers"])):
        pre = "sy.enc.l%d." % l
        x = _ln_c(x + _rel_attn(t, l, x, heads, window), _t(t[pre + "ln1.g"]), _t(t[pre + "ln1.b"]))
        y = F.conv1d(F.relu(F.conv1d(x, _t(t[pre + "ff1.w"]), _t(t[pre + "ff1.b"]), padding=ek // 2)), _t(t[pre + "ff2.w"]), _t(t[pre + "ff2.b"]), padding=ek // 2)
        x = _ln_c(x + y, _t(t[pre + "ln2.g"]), _t(t[pre + "ln2.b"]))
    return x


def sy_stats(cfg, t, x):
    return F.conv1d(x, _t(t["sy.enc.proj.w"])[:, :, None], _t(t["sy.enc.proj.b"]))


def sy_prior(cfg, stats, eps):
    I = int(cfg["inter"])
    m, logs = stats[:, :I], stats[:, I:]
    return m + torch.exp(logs) * _t(eps)[None] * 0.66666


def sy_wavenet(cfg, t, fi, x0):
    """the coupling layer's network: x0 (1, I/2, R) -> m (1, I/2, R)"""
    Hd, wk, wl = int(cfg["hidden"]), int(cfg["wn_k"]), int(cfg["wn_layers"])
    g = _t(t["sy.g"])[None, :, None]
    pre = "sy.flow%d." % fi
    h = F.conv1d(x0, _t(t[pre + "pre.w"])[:, :, None], _t(t[pre + "pre.b"]))
    cond = F.conv1d(g, _t(t[pre + "cond.w"])[:, :, None], _t(t[pre + "cond.b"]))
    out = torch.zeros_like(h)
    for j in range(wl):
        a = F.conv1d(h, _t(t[pre + "in%d.w" % j]), _t(t[pre + "in%d.b" % j]), padding=(wk - 1) // 2) + cond[:, j * 2 * Hd:(j + 1) * 2 * Hd]
        acts = torch.tanh(a[:, :Hd]) * torch.sigmoid(a[:, Hd:])
        rs = F.conv1d(acts, _t(t[pre + "rs%d.w" % j])[:, :, None], _t(t[pre + "rs%d.b" % j]))
        if j < wl - 1:
            h = h + rs[:, :Hd]
            out = out + rs[:, Hd:]
        else:
            out = out + rs
    return F.conv1d(out, _t(t[pre + "post.w"])[:, :, None], _t(t[pre + "post.b"]))


def sy_flow(cfg, t, fi, z):
    """Flip, then the reverse coupling layer fi (the reference's module order at inference)"""
    half = int(cfg["inter"]) // 2
    z = torch.flip(z, [1])
    x0, x1 = z[:, :half], z[:, half:]
    return torch.cat([x0, x1 - sy_wavenet(cfg, t, fi, x0)], 1)


def sy_dec_pre(cfg, t, z):
    g = _t(t["sy.g"])[None, :, None]
    return F.conv1d(z, _t(t["sy.dec.pre.w"]), _t(t["sy.dec.pre.b"]), padding=3) + F.conv1d(g, _t(t["sy.dec.cond.w"])[:, :, None], _t(t["sy.dec.cond.b"]))


def sy_dec_up(cfg, t, i, x, s):
    """upsampling stage i of x plus its strided convolution of the harmonic source s (1, 1, N)"""
    n_ups = int(cfg["n_ups"])
    rates = [int(cfg["up_rate%d" % q]) for q in range(n_ups)]
    kerns = [int(cfg["up_kernel%d" % q]) for q in range(n_ups)]
    x = F.leaky_relu(x, 0.1)
    x = F.conv_transpose1d(x, _t(t["sy.dec.up%d.w" % i]), _t(t["sy.dec.up%d.b" % i]), stride=rates[i], padding=(kerns[i] - rates[i]) // 2)
    if i + 1 < n_ups:
        sf = int(np.prod(rates[i + 1:]))
        return x + F.conv1d(s, _t(t["sy.dec.nc%d.w" % i]), _t(t["sy.dec.nc%d.b" % i]), stride=sf, padding=sf // 2)
    return x + F.conv1d(s, _t(t["sy.dec.nc%d.w" % i]), _t(t["sy.dec.nc%d.b" % i]))


def sy_dec_rb(cfg, t, i, x):
    """the ResBlock chains of stage i and their mean"""
    n_rb, n_rbd = int(cfg["n_rb"]), int(cfg["n_rbd"])
    xs = None
    for j in range(n_rb):
        k = int(cfg["rb_k%d" % j])
        r = x
        for m in range(n_rbd):
            d = int(cfg["rb_d%d" % m])
            xt = F.conv1d(F.leaky_relu(r, 0.1), _t(t["sy.dec.rb%d_%d.c1_%d.w" % (i, j, m)]), _t(t["sy.dec.rb%d_%d.c1_%d.b" % (i, j, m)]), dilation=d, padding=(k * d - d) // 2)
            xt = F.conv1d(F.leaky_relu(xt, 0.1), _t(t["sy.dec.rb%d_%d.c2_%d.w" % (i, j, m)]), _t(t["sy.dec.rb%d_%d.c2_%d.b" % (i, j, m)]), padding=(k - 1) // 2)
            r = xt + r
        xs = r if xs is None else xs + r
    return xs / n_rb


def sy_dec_post(cfg, t, x):
    return torch.tanh(F.conv1d(F.leaky_relu(x, 0.01), _t(t["sy.dec.post.w"]), None, padding=3))


def synth_until_z(cfg, t, phone: np.ndarray, pitch: np.ndarray, eps: np.ndarray):
    """TextEncoder + prior + reverse flow.  phone (R, C), pitch int (R,), eps (inter, R) -> (enc_out, stats, z)."""
    with torch.no_grad():
        enc = sy_encoder(cfg, t, sy_embed(cfg, t, phone, pitch))
        stats = sy_stats(cfg, t, enc)
        z = sy_prior(cfg, stats, eps)
        for fi in reversed(range(int(cfg["flow_n"]))):
            z = sy_flow(cfg, t, fi, z)
    return enc[0].numpy(), stats[0].numpy(), z[0].numpy()


def synth_decoder(cfg, t, z: np.ndarray, src: np.ndarray) -> np.ndarray:
    """NSF-HiFiGAN decoder given the latent z (inter, R) and the harmonic source (N,)."""
    with torch.no_grad():
        x = sy_dec_pre(cfg, t, _t(z)[None])
        s = _t(src)[None, None]
        for i in range(int(cfg["n_ups"])):
            x = sy_dec_rb(cfg, t, i, sy_dec_up(cfg, t, i, x, s))
        x = sy_dec_post(cfg, t, x)
    return x[0, 0].numpy()
