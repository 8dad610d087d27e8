"""The synthesizer split at the engine's tap boundaries, one function per stage, evaluated in float64.  The layers are
torch_ref.py's, run under torch_ref.precision(): nothing is restated here but what the engine adds to the model -- the phone gather's column rule, the
coarse pitch, the physical channel order it keeps the latent in (flips folded into the weights) and the formant stage's stretch.

Every function takes the blob's config and tensors (PyTorch layout) and numpy arrays shaped like the taps, [C][T], and returns a float64 array.
`dtype=torch.float32` evaluates the same stage in fp32: stage_delta32 measures how far that is from the fp64 value, the yardstick of the multi-layer
stages' tolerance in test_gpu_stream_taps.py.  Test infrastructure; never imported by the product."""
from __future__ import annotations

import numpy as np
import torch

import torch_ref as TR

F64 = torch.float64


def _run(dtype, fn, *arrays):
    """fn(*tensors with a leading batch axis) under the precision `dtype` -> numpy float64 [C][T]"""
    with torch.no_grad(), TR.precision(dtype):
        out = fn(*[TR._t(np.asarray(a))[None] for a in arrays])
    return out[0].to(F64).numpy()


# ---- what the engine adds around the model ----------------------------------------------------------------------------------------------------
def phone_gather(cv_out, skip_head, R):
    """cv.out [C][T] -> phone_ct [C][R]: the features repeated twice and sliced [skip_head : skip_head + R] (no index loaded): a pure gather, bitwise"""
    T = cv_out.shape[1]
    cols = np.minimum((int(skip_head) + np.arange(int(R))) // 2, T - 1)
    return cv_out[:, cols]


def coarse_pitch(f0):
    """pitchf (Hz) -> the pitch embedding's row (rule of _coarse_pitch in test_gpu_formant.py: f32 arithmetic, round half away from zero)"""
    f32 = np.float32
    f0 = np.asarray(f0, f32)
    mn, mx = f32(1127.0) * np.log(f32(1.0) + f32(50.0 / 700.0)), f32(1127.0) * np.log(f32(1.0) + f32(500.0 / 700.0))
    mel = f32(1127.0) * np.log(f32(1.0) + f0 / f32(700.0))
    mel = np.where(mel > 0, (mel - mn) * f32(254.0) / (mx - mn) + f32(1.0), mel)
    return np.floor(np.clip(mel, 1.0, 255.0) + 0.5).astype(np.int64)


def flow_flipped(cfg, fi):
    """does the engine see flow fi through an odd number of flips (flow_n - fi of them)?  Then its tap is the reference's latent upside down."""
    return (int(cfg["flow_n"]) - fi) % 2 == 1


def final_flip(cfg, flow0):
    """sy.flow0 -> sy.z: an odd flow count leaves one flip to materialise, an even one none.  Bitwise."""
    return flow0[::-1] if int(cfg["flow_n"]) % 2 else flow0


def latent_stretch(z, R2):
    """sy.z [I][R] -> sy.zi [I][R2]: F.interpolate(mode="linear", align_corners=False) (interp of tests/test_formant.py, in float64)"""
    dt = np.float64
    x = np.asarray(z, dt)
    nin = x.shape[-1]
    s = dt(nin) / dt(R2)
    i = np.arange(R2, dtype=dt)
    xs = np.maximum(s * (i + 0.5) - 0.5, 0.0)
    i0 = np.minimum(xs.astype(np.int64), nin - 1)
    i1 = i0 + (i0 < nin - 1)
    lam = np.clip(xs - i0, 0.0, 1.0)
    return (1.0 - lam) * x[..., i0] + lam * x[..., i1]


# ---- the model's stages -------------------------------------------------------------------------------------------------------------------
def embed(cfg, t, phone_ct, pitchf, dtype=F64):
    """phone_ct [C][R], pitchf [R] -> sy.emb [H][R]"""
    pitch = coarse_pitch(pitchf)
    with torch.no_grad(), TR.precision(dtype):
        return TR.sy_embed(cfg, t, np.asarray(phone_ct).T, pitch)[0].to(F64).numpy()


def encoder(cfg, t, emb, dtype=F64):
    """sy.emb -> sy.enc"""
    return _run(dtype, lambda x: TR.sy_encoder(cfg, t, x), emb)


def stats(cfg, t, enc, dtype=F64):
    """sy.enc -> sy.stats [2I][R]"""
    return _run(dtype, lambda x: TR.sy_stats(cfg, t, x), enc)


def encoder_stats(cfg, t, emb, dtype=F64):
    """sy.emb -> sy.stats: plans that fold the encoder's last LayerNorm into the projection have no normalised sy.enc in between"""
    return _run(dtype, lambda x: TR.sy_stats(cfg, t, TR.sy_encoder(cfg, t, x)), emb)


def prior(cfg, stats_, eps, dtype=F64):
    """sy.stats, the stream's normals [I][R] -> sy.zp"""
    with torch.no_grad(), TR.precision(dtype):
        return TR.sy_prior(cfg, TR._t(np.asarray(stats_))[None], np.asarray(eps))[0].to(F64).numpy()


def flow_reference(cfg, t, fi, z, dtype=F64):
    """flip, then reverse coupling layer fi: the reference's form, on the latent in the reference's channel order"""
    return _run(dtype, lambda x: TR.sy_flow(cfg, t, fi, x), z)


def flow(cfg, t, fi, z, dtype=F64):
    """Flow fi on the latent in the engine's PHYSICAL channel order (the tap of the flow before it, sy.zp for the first) -> sy.flow{fi}.  The engine never
    moves a channel: a flow behind an odd number of flips reads x0 from the upper half with its channels reversed and takes the coupling's output, reversed,
    off the lower half; behind an even number it is the plain coupling layer."""
    half = int(cfg["inter"]) // 2
    flipped = flow_flipped(cfg, fi)

    def f(x):
        if flipped:
            m = TR.sy_wavenet(cfg, t, fi, torch.flip(x[:, half:], [1]))
            return torch.cat([x[:, :half] - torch.flip(m, [1]), x[:, half:]], 1)
        return torch.cat([x[:, :half], x[:, half:] - TR.sy_wavenet(cfg, t, fi, x[:, :half])], 1)
    return _run(dtype, f, z)


def dec_pre(cfg, t, z, dtype=F64):
    """sy.z / sy.zi -> sy.pre"""
    return _run(dtype, lambda x: TR.sy_dec_pre(cfg, t, x), z)


def dec_up(cfg, t, i, x, src, dtype=F64):
    """sy.pre / sy.rb{i-1} and the harmonic source [N] -> sy.up{i}"""
    return _run(dtype, lambda a, s: TR.sy_dec_up(cfg, t, i, a, s), x, np.asarray(src).reshape(1, -1))


def dec_rb(cfg, t, i, x, dtype=F64):
    """sy.up{i} -> sy.rb{i}"""
    return _run(dtype, lambda a: TR.sy_dec_rb(cfg, t, i, a), x)


def dec_post(cfg, t, x, dtype=F64):
    """sy.rb{last} -> sy.dec / the PCM, [1][N]"""
    return _run(dtype, lambda a: TR.sy_dec_post(cfg, t, a), x)


# ---- metrics ----------------------------------------------------------------------------------------------------------------------------------
def rms64(a):
    a = np.asarray(a, np.float64)
    return float(np.sqrt(np.mean(a * a))) if a.size else 0.0


def max_over_rms(got, ref64):
    """the per-layer metric: max |got - ref| / rms(ref)"""
    ref64 = np.asarray(ref64, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(ref64.shape) - ref64).max()) / max(rms64(ref64), 1e-30)


def stage_delta32(stage, *args):
    """(ref64, delta32) of one stage on the given inputs: how far torch's own fp32 evaluation lies from the fp64 one, in the per-layer metric"""
    r64 = stage(*args, dtype=F64)
    r32 = stage(*args, dtype=torch.float32)
    return r64, max_over_rms(r32, r64)
