"""synth_ref.py (the synthesizer in float64, one function per tap interval) against the references the suite already trusts: chained, its stages
reproduce torch_ref's fp32 synthesizer and the C oracle's taps; teacher-forced, torch's fp32 evaluation of a stage stays within 1e-5 (max / rms) of the
fp64 one, so the inputs the GPU tests use do not widen their own tolerance; and the engine's physical-channel-order form of a flow is the reference's
flip-then-couple form for both parities.  No GPU."""
import functools

import numpy as np
import pytest

import synth_ref as SR
import torch_ref as TR
from common import BASELINE_160MS as g, rel_rms, synth_zoo, voice_signal
from obs_rvc_amd import weights as W
from oracle import oracle as O

torch = pytest.importorskip("torch")

PRESETS = ["tiny", "tiny5", "full", "tiny_v1_48k", "tiny_v1_32k", "tiny32k"]       # (the last three: upstream's v1 48k / v1 32k / v2 32k decoder layouts)
SEED, STREAM = 3, 1


@functools.lru_cache(maxsize=None)
def _case(preset):
    """one oracle chunk with taps: (cfg, tensors, taps by name as [C][T] arrays, PCM)"""
    z, version = synth_zoo(preset)
    cfg, tens = W.read_blob(z["model"])
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(version); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(SEED, STREAM)
    ora.enable_taps(True)
    R = g.model_return_length
    pcm = ora.infer(voice_signal(35840, seed=4), g.sample_frame_16k, 12, g.skip_head, R)
    n_ups, fn = int(cfg["n_ups"]), int(cfg["flow_n"])
    names = ["sy.emb", "sy.enc", "sy.stats", "sy.zp", "sy.z", "sy.pre"] + ["sy.flow%d" % i for i in range(fn)] + ["sy.up%d" % i for i in range(n_ups)] + ["sy.rb%d" % i for i in range(n_ups)]
    taps = {}
    for nm in names:
        a = ora.tap(nm)
        taps[nm] = a.reshape(-1, R if nm in ("sy.emb", "sy.enc", "sy.stats", "sy.zp", "sy.z", "sy.pre") or nm.startswith("sy.flow") else 1)
    for nm in names:                    # decoder stages: [C][T] from the channel counts
        if nm.startswith(("sy.up", "sy.rb")):
            i = int(nm[5:])
            taps[nm] = taps[nm].reshape(int(cfg["up_init"]) >> (i + 1), -1)
    taps["phone"] = ora.tap("phone").reshape(R, -1)
    taps["pitch"] = ora.tap("pitch").astype(np.int64)
    taps["sy.src"] = ora.tap("sy.src")
    taps["eps"] = O.philox_normal(SEED, STREAM, 0, 0, int(cfg["inter"]) * R).reshape(int(cfg["inter"]), R)
    ora.close()
    return cfg, tens, taps, pcm


def _embed64(cfg, tens, taps):
    # with the oracle's own coarse pitch (SR.embed derives it from pitchf, as the engine does)
    with torch.no_grad(), TR.precision(torch.float64):
        return TR.sy_embed(cfg, tens, taps["phone"], taps["pitch"])[0].numpy()


@pytest.mark.parametrize("preset", PRESETS)
def test_chained_stages_reproduce_torch_ref_and_the_oracle(preset):
    cfg, tens, taps, pcm = _case(preset)
    fn, n_ups = int(cfg["flow_n"]), int(cfg["n_ups"])
    got = {}
    got["sy.emb"] = _embed64(cfg, tens, taps)
    got["sy.enc"] = SR.encoder(cfg, tens, got["sy.emb"])
    got["sy.stats"] = SR.stats(cfg, tens, got["sy.enc"])
    assert rel_rms(SR.encoder_stats(cfg, tens, got["sy.emb"]), got["sy.stats"]) < 1e-12
    got["sy.zp"] = SR.prior(cfg, got["sy.stats"], taps["eps"])
    zz = got["sy.zp"]
    for fi in reversed(range(fn)):
        zz = SR.flow(cfg, tens, fi, zz)                      # physical order, as the engine's taps
        got["sy.flow%d" % fi] = zz[::-1] if SR.flow_flipped(cfg, fi) else zz      # ... the oracle's are in the reference's order
    got["sy.z"] = SR.final_flip(cfg, zz)
    # the fp32 reference the oracle is pinned to
    enc, stats, z32 = TR.synth_until_z(cfg, tens, taps["phone"], taps["pitch"], taps["eps"])
    for nm, ref in (("sy.enc", enc), ("sy.stats", stats), ("sy.z", z32)):
        e = rel_rms(got[nm], ref)
        print("%s chained vs torch_ref fp32 %-9s %.2e" % (preset, nm, e))
        assert e < 1e-5, (nm, e)
    # decoder: from the oracle's latent, as test_oracle_vs_torch does
    x = SR.dec_pre(cfg, tens, taps["sy.z"]); got["sy.pre"] = x
    for i in range(n_ups):
        x = SR.dec_up(cfg, tens, i, x, taps["sy.src"]); got["sy.up%d" % i] = x
        x = SR.dec_rb(cfg, tens, i, x); got["sy.rb%d" % i] = x
    y = SR.dec_post(cfg, tens, x)[0]
    ref_audio = TR.synth_decoder(cfg, tens, taps["sy.z"], taps["sy.src"])
    assert y.shape == ref_audio.shape == pcm.shape == (g.model_return_length * int(cfg["sr"]) // 100,)
    assert rel_rms(y, ref_audio) < 1e-5 and rel_rms(pcm, y) < 1e-5, (rel_rms(y, ref_audio), rel_rms(pcm, y))
    for nm, a in got.items():
        e = rel_rms(taps[nm], a)
        print("%s oracle tap vs chained fp64 %-9s %.2e" % (preset, nm, e))
        assert taps[nm].shape == a.shape and e < 1e-5, (nm, e)


def _stages(cfg, tens, taps):
    """(name, stage function, inputs) of every teacher-forced stage, inputs = the oracle's taps in the engine's physical channel order"""
    fn, n_ups = int(cfg["flow_n"]), int(cfg["n_ups"])
    phys = {fi: (taps["sy.flow%d" % fi][::-1] if SR.flow_flipped(cfg, fi) else taps["sy.flow%d" % fi]) for fi in range(fn)}
    out = [("encoder", SR.encoder, (cfg, tens, taps["sy.emb"])), ("stats", SR.stats, (cfg, tens, taps["sy.enc"])),
           ("encoder+stats", SR.encoder_stats, (cfg, tens, taps["sy.emb"])), ("prior", SR.prior, (cfg, taps["sy.stats"], taps["eps"]))]
    for fi in reversed(range(fn)):
        out.append(("flow%d" % fi, SR.flow, (cfg, tens, fi, taps["sy.zp"] if fi == fn - 1 else phys[fi + 1])))
    out.append(("pre", SR.dec_pre, (cfg, tens, taps["sy.z"])))
    for i in range(n_ups):
        out.append(("up%d" % i, SR.dec_up, (cfg, tens, i, taps["sy.pre"] if i == 0 else taps["sy.rb%d" % (i - 1)], taps["sy.src"])))
        out.append(("rb%d" % i, SR.dec_rb, (cfg, tens, i, taps["sy.up%d" % i])))
    out.append(("post", SR.dec_post, (cfg, tens, taps["sy.rb%d" % (n_ups - 1)])))
    return out


@pytest.mark.parametrize("preset", PRESETS)
def test_fp32_evaluation_of_every_stage_is_within_1e5_of_fp64(preset):
    cfg, tens, taps, _ = _case(preset)
    for name, fnc, args in _stages(cfg, tens, taps):
        _, d = SR.stage_delta32(fnc, *args)
        print("%s delta32 %-14s %.2e" % (preset, name, d))
        assert d <= 1e-5, (name, d)


@pytest.mark.parametrize("preset", ["tiny", "tiny5"])       # even and odd flow counts: every flow index meets both parities
def test_physical_order_flow_is_flip_then_couple(preset):
    cfg, tens, taps, _ = _case(preset)
    fn = int(cfg["flow_n"])
    z = taps["sy.zp"].astype(np.float64)                     # the latent in the reference's order
    for fi in reversed(range(fn)):
        ref = SR.flow_reference(cfg, tens, fi, z)
        z_phys = z[::-1] if SR.flow_flipped(cfg, fi + 1) else z      # flow_n - fi - 1 flips so far (none at the prior sample: both orders coincide)
        got = SR.flow(cfg, tens, fi, z_phys)
        got_ref_order = got[::-1] if SR.flow_flipped(cfg, fi) else got
        assert np.abs(got_ref_order - ref).max() <= 1e-13 * max(1.0, np.abs(ref).max()), fi
        assert rel_rms(taps["sy.flow%d" % fi], ref) < 1e-5
        z = ref
    assert np.array_equal(SR.final_flip(cfg, got), ref)      # sy.z is in the reference's order


def test_gather_and_pitch_rules():
    cv = np.arange(3 * 7, dtype=np.float32).reshape(3, 7)
    assert np.array_equal(SR.phone_gather(cv, 4, 5)[0], [2, 2, 3, 3, 4]) and np.array_equal(SR.phone_gather(cv, 11, 5)[0], [5, 6, 6, 6, 6])
    assert list(SR.coarse_pitch(np.array([0.0, 50.0, 500.0, 2000.0], np.float32))) == [1, 1, 255, 255]
    x = np.random.default_rng(0).standard_normal((4, 21))
    from test_formant import interp
    assert np.array_equal(SR.latent_stretch(x, 25), interp(x, 25, np.float64))
