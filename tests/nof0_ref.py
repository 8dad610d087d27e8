"""A synthesizer trained without pitch guidance (upstream's SynthesizerTrnMs{256,768}NSFsid_nono), stage by stage in float64.

The stages are synth_ref.py's (which are torch_ref.py's layers under torch_ref.precision()); a no-f0 model differs in two of them, stated here:
the text encoder's front has no pitch term, and an upsampling stage of the decoder -- a plain HiFi-GAN generator -- adds no convolution of a harmonic
source.  `synth` chains the stages the way the engine's plan does: on the latent in the engine's physical channel order (synth_ref.flow), flips
materialised once at the end (synth_ref.final_flip), the formant stage's latent stretch in front of the decoder when R2 is given.
tests/test_nof0_ref.py pins the chain to an nn.Module written after upstream's _nono classes.  Test infrastructure; never imported by the product."""
from __future__ import annotations

import hashlib
import math

import numpy as np
import torch
import torch.nn.functional as F

import synth_ref as SR
import torch_ref as TR

F64 = SR.F64


def embed(cfg, t, phone_ct, dtype=F64):
    """phone_ct [C][R] -> sy.emb [H][R]: lrelu(emb_phone(phone) * sqrt(H), 0.1)"""
    Hd = int(cfg["hidden"])
    with torch.no_grad(), TR.precision(dtype):
        x = F.linear(TR._t(np.asarray(phone_ct).T)[None], TR._t(t["sy.enc.phone.w"]), TR._t(t["sy.enc.phone.b"]))
        return F.leaky_relu(x * math.sqrt(Hd), 0.1).transpose(1, 2)[0].to(F64).numpy()


def dec_up(cfg, t, i, x, dtype=F64):
    """sy.pre / sy.rb{i-1} -> sy.up{i}: lrelu(0.1), then the transposed convolution; nothing is added"""
    n_ups = int(cfg["n_ups"])
    rates = [int(cfg["up_rate%d" % q]) for q in range(n_ups)]
    kerns = [int(cfg["up_kernel%d" % q]) for q in range(n_ups)]

    def f(a):
        return F.conv_transpose1d(F.leaky_relu(a, 0.1), TR._t(t["sy.dec.up%d.w" % i]), TR._t(t["sy.dec.up%d.b" % i]), stride=rates[i], padding=(kerns[i] - rates[i]) // 2)
    return SR._run(dtype, f, x)


def synth(cfg, t, phone_ct, eps, R2=None):
    """phone_ct [C][R], the stream's normals eps [I][R] -> dict of every stage's float64 value under the engine's tap names ("pcm": the output, [N]).
    R2: the decoder's frame count when the formant stage stretches the latent (None: R)."""
    n_ups, fn = int(cfg["n_ups"]), int(cfg["flow_n"])
    out = {"sy.emb": embed(cfg, t, phone_ct)}
    out["sy.enc"] = SR.encoder(cfg, t, out["sy.emb"])
    out["sy.stats"] = SR.stats(cfg, t, out["sy.enc"])
    z = out["sy.zp"] = SR.prior(cfg, out["sy.stats"], eps)
    for fi in reversed(range(fn)):
        z = out["sy.flow%d" % fi] = SR.flow(cfg, t, fi, z)
    z = out["sy.z"] = np.ascontiguousarray(SR.final_flip(cfg, z))
    if R2 is not None and int(R2) != z.shape[1]:
        z = out["sy.zi"] = SR.latent_stretch(z, int(R2))
    x = out["sy.pre"] = SR.dec_pre(cfg, t, z)
    for i in range(n_ups):
        u = out["sy.up%d" % i] = dec_up(cfg, t, i, x)
        x = out["sy.rb%d" % i] = SR.dec_rb(cfg, t, i, u)
    out["sy.dec"] = SR.dec_post(cfg, t, x)
    out["pcm"] = out["sy.dec"][0]
    return out


def blob_digest(cfg, tens) -> str:
    """sha256 over a blob's content in the order make_synth emits it: every config key and value, every tensor's name, shape and fp32 bytes"""
    h = hashlib.sha256()
    for k, v in cfg.items():
        h.update(("%s=%r;" % (k, float(v))).encode())
    for k, a in tens.items():
        a = np.ascontiguousarray(a, dtype="<f4")
        h.update(("%s%r:" % (k, tuple(a.shape))).encode())
        h.update(a.tobytes())
    return h.hexdigest()
