"""Models trained without pitch guidance, the parts that need no GPU: the staged float64 reference of tests/nof0_ref.py against an
nn.Module written after upstream's _nono classes, the importer's handling of such state dicts, and make_synth's two kinds.

The module: upstream's SynthesizerTrnMs*NSFsid_nono is the f0 synthesizer with (a) a TextEncoder whose forward gets pitch = None -- no emb_pitch term in
front of the leaky ReLU -- and (b) `Generator`, the plain HiFi-GAN decoder, in place of GeneratorNSF: no m_source, no noise_convs, nothing added behind an
upsampling convolution.  The blocks the two kinds share (relative-position encoder, WaveNet coupling layers and flips, weight-normed ResBlocks) are the ones
tests/test_importers.py writes out for the f0 module; the two classes that differ are written here.

Bound of the torch-against-staged comparison: both sides are float64 evaluations of the same function with different groupings (true flips against folded
ones, weight-norm pairs against plain weights, one forward against stage functions).  A rounding is 2^-53 = 1.1e-16; the chain is about 60 layers deep with
dot products of at most 16 * 11 * 3 terms and gains of order one per layer, so a relative difference in max-over-rms of 1e-12 .. 1e-11 is what round-off can
make.  The bound is 1e-9: two orders above that, and still 60 times below one float32 rounding (6e-8), the smallest error a wrong operand could hide behind."""
import math

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import nof0_ref as NR
import synth_ref as SR
import test_importers as TI
from obs_rvc_amd import importers as IM
from obs_rvc_amd import weights as W

ROUNDOFF = 1e-9
# weight-normed tensors come back from the importer as v * (g / |v|) with g stored in fp32: one rounding of g and one of the product, 2 * 2^-24
WN_RTOL = 2.0 ** -23
# tests/nof0_ref.blob_digest of make_synth(preset, phone_dim) on the parent commit
PARENT_DIGEST = {
    ("tiny", 48): "0ee7220613a110ee39e5379e0ea8ee6d47cf2e7adc09e18a82ff4089bfc3612c",
    ("tiny5", 48): "38f3954861876ba699ec370c2c3c646193e83839b330d045fe2aa0a2278b999c",
    ("full40k", 768): "d1ef483a7eabccf4ab5d287a3baf224eacd47e2b5569193359479c54f80f9f00",
}


def _dims(preset):
    p = W.SYNTH_PRESETS[preset]
    return dict(phone_dim=48, inter=p["inter"], hidden=p["hidden"], filt=p["filter"], heads=p["heads"], layers=p["enc_layers"], k=p["enc_k"], window=p["window"],
                n_flows=p["flow_n"], wn_layers=p["wn_layers"], gin=p["gin"], up_init=p["up_init"], rates=p["up_rates"], kernels=p["up_kernels"], rb_k=p["rb_k"], rb_d=p["rb_d"])


def nono_module(preset, seed=0):
    """upstream's SynthesizerTrnMs768NSFsid_nono at the preset's sizes, random weights"""
    d = _dims(preset)
    f0m = TI._upstream_synth(seed=seed, **d)
    hidden, inter, nk = d["hidden"], d["inter"], len(d["rb_k"])

    class TextEncoder(nn.Module):              # models.py TextEncoder.forward(phone, pitch=None, lengths)
        def __init__(self):
            super().__init__()
            self.emb_phone, self.encoder, self.proj = f0m.enc_p.emb_phone, f0m.enc_p.encoder, f0m.enc_p.proj

        def forward(self, phone):
            x = F.leaky_relu(self.emb_phone(phone) * math.sqrt(hidden), 0.1).transpose(1, -1)
            mask = torch.ones(1, 1, x.shape[-1], dtype=x.dtype)
            x = self.encoder(x, mask)
            return torch.split(self.proj(x) * mask, inter, dim=1)

    class Generator(nn.Module):                # models.py Generator: HiFi-GAN, conditioned on g
        def __init__(self):
            super().__init__()
            self.conv_pre, self.ups, self.resblocks, self.conv_post, self.cond = f0m.dec.conv_pre, f0m.dec.ups, f0m.dec.resblocks, f0m.dec.conv_post, f0m.dec.cond

        def forward(self, x, g):
            x = self.conv_pre(x) + self.cond(g)
            for i in range(len(self.ups)):
                x = self.ups[i](F.leaky_relu(x, 0.1))
                x = sum(self.resblocks[i * nk + j](x) for j in range(nk)) / nk
            return torch.tanh(self.conv_post(F.leaky_relu(x)))

    class SynthNono(nn.Module):
        def __init__(self):
            super().__init__()
            self.enc_p, self.dec, self.flow, self.emb_g = TextEncoder(), Generator(), f0m.flow, f0m.emb_g

        def infer(self, phone, eps, sid):
            g = self.emb_g(torch.tensor([sid])).unsqueeze(-1)
            m_p, logs_p = self.enc_p(phone)
            z_p = m_p + torch.exp(logs_p) * eps * 0.66666
            z = self.flow(z_p, torch.ones(1, 1, phone.shape[1], dtype=phone.dtype), g, reverse=True)
            return self.dec(z, g)

    return SynthNono().eval()


def _set(p, a):
    assert tuple(p.shape) == tuple(a.shape), (tuple(p.shape), a.shape)
    p.data = torch.from_numpy(np.ascontiguousarray(a)).to(p.dtype)


def _set_wn(mod, w):
    """a weight-normed layer's pair: v = w, g = |v| over all axes but the first, evaluated in float64 and rounded once to the module's dtype"""
    _set(mod.weight_v, w)
    mod.weight_g.data = torch.norm_except_dim(mod.weight_v.data.double(), 2, 0).to(mod.weight_v.dtype)


def load_blob(m, cfg, t, sid):
    """the inverse of import_synth's name table: the blob's tensors into the module's parameters"""
    n_rb, n_rbd = int(cfg["n_rb"]), int(cfg["n_rbd"])
    with torch.no_grad():
        m.emb_g.weight.data[sid] = torch.from_numpy(t["sy.g"]).to(m.emb_g.weight.dtype)
        _set(m.enc_p.emb_phone.weight, t["sy.enc.phone.w"]); _set(m.enc_p.emb_phone.bias, t["sy.enc.phone.b"])
        e = m.enc_p.encoder
        for i in range(int(cfg["enc_layers"])):
            q = "sy.enc.l%d." % i
            for n in "qkvo":
                c = getattr(e.attn_layers[i], "conv_" + n)
                _set(c.weight, t[q + n + ".w"][:, :, None]); _set(c.bias, t[q + n + ".b"])
            _set(e.attn_layers[i].emb_rel_k, t[q + "rel_k"][None]); _set(e.attn_layers[i].emb_rel_v, t[q + "rel_v"][None])
            for k, ln in (("ln1", e.norm_layers_1[i]), ("ln2", e.norm_layers_2[i])):
                _set(ln.gamma, t[q + k + ".g"]); _set(ln.beta, t[q + k + ".b"])
            for k, c in (("ff1", e.ffn_layers[i].conv_1), ("ff2", e.ffn_layers[i].conv_2)):
                _set(c.weight, t[q + k + ".w"]); _set(c.bias, t[q + k + ".b"])
        _set(m.enc_p.proj.weight, t["sy.enc.proj.w"][:, :, None]); _set(m.enc_p.proj.bias, t["sy.enc.proj.b"])
        for i in range(int(cfg["flow_n"])):
            f, q = m.flow.flows[2 * i], "sy.flow%d." % i
            _set(f.pre.weight, t[q + "pre.w"][:, :, None]); _set(f.pre.bias, t[q + "pre.b"])
            _set_wn(f.enc.cond_layer, t[q + "cond.w"][:, :, None]); _set(f.enc.cond_layer.bias, t[q + "cond.b"])
            for j in range(int(cfg["wn_layers"])):
                _set_wn(f.enc.in_layers[j], t[q + "in%d.w" % j]); _set(f.enc.in_layers[j].bias, t[q + "in%d.b" % j])
                _set_wn(f.enc.res_skip_layers[j], t[q + "rs%d.w" % j][:, :, None]); _set(f.enc.res_skip_layers[j].bias, t[q + "rs%d.b" % j])
            _set(f.post.weight, t[q + "post.w"][:, :, None]); _set(f.post.bias, t[q + "post.b"])
        d = m.dec
        _set(d.conv_pre.weight, t["sy.dec.pre.w"]); _set(d.conv_pre.bias, t["sy.dec.pre.b"])
        _set(d.cond.weight, t["sy.dec.cond.w"][:, :, None]); _set(d.cond.bias, t["sy.dec.cond.b"])
        for i in range(int(cfg["n_ups"])):
            _set_wn(d.ups[i], t["sy.dec.up%d.w" % i]); _set(d.ups[i].bias, t["sy.dec.up%d.b" % i])
            for j in range(n_rb):
                r, q = d.resblocks[i * n_rb + j], "sy.dec.rb%d_%d." % (i, j)
                for k in range(n_rbd):
                    _set_wn(r.convs1[k], t[q + "c1_%d.w" % k]); _set(r.convs1[k].bias, t[q + "c1_%d.b" % k])
                    _set_wn(r.convs2[k], t[q + "c2_%d.w" % k]); _set(r.convs2[k].bias, t[q + "c2_%d.b" % k])
        _set(d.conv_post.weight, t["sy.dec.post.w"])
    return m


def _state_dict(m):
    return {k: v.detach().to(torch.float32).numpy() for k, v in m.state_dict().items()}


def _rates(preset):
    return [int(r) for r in W.SYNTH_PRESETS[preset]["up_rates"]]


# ---- make_synth -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,phone_dim", sorted(PARENT_DIGEST))
def test_make_synth_with_f0_is_the_parent_commits_bytes(preset, phone_dim):
    cfg, tens = W.make_synth(preset, phone_dim)
    assert "f0" not in cfg                                    # an absent key means 1: every existing blob keeps its meaning
    assert NR.blob_digest(cfg, tens) == PARENT_DIGEST[(preset, phone_dim)]
    cfg1, tens1 = W.make_synth(preset, phone_dim, f0=True)
    assert NR.blob_digest(cfg1, tens1) == PARENT_DIGEST[(preset, phone_dim)]


@pytest.mark.parametrize("preset", ["tiny", "tiny5"])
def test_make_synth_without_f0_shares_every_other_tensor(preset, tmp_path):
    cfg1, t1 = W.make_synth(preset, 48, seed=5)
    cfg0, t0 = W.make_synth(preset, 48, seed=5, f0=False)
    gone = sorted(set(t1) - set(t0))
    assert gone == sorted(["sy.enc.pitch_emb", "sy.src"] + ["sy.dec.nc%d.%s" % (i, s) for i in range(int(cfg1["n_ups"])) for s in "wb"])
    assert not set(t0) - set(t1) and all(W.is_f0_only(k) for k in gone) and not any(W.is_f0_only(k) for k in t0)
    assert list(t0) == [k for k in t1 if k in t0]             # the same order
    assert all(t0[k].tobytes() == t1[k].tobytes() and t0[k].shape == t1[k].shape for k in t0)
    assert cfg0["f0"] == 0 and {k: v for k, v in cfg0.items() if k != "f0"} == cfg1
    p = str(tmp_path / "m.rvcw")
    W.write_blob(p, cfg0, t0)
    c, t = W.read_blob(p)
    assert c["f0"] == 0.0 and set(t) == set(t0)


# ---- the staged reference against the module --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["tiny", "tiny5"])          # tiny5: an odd flow count, the final flip is materialised
def test_staged_reference_is_the_nono_module(preset):
    sid, R = 1, 21
    cfg, tens = W.make_synth(preset, 48, f0=False)
    m = load_blob(nono_module(preset).double(), cfg, tens, sid)
    rng = np.random.default_rng(17)
    phone = rng.standard_normal((48, R)) * 0.5
    eps = rng.standard_normal((int(cfg["inter"]), R))
    with torch.no_grad():
        ref = m.infer(torch.from_numpy(phone.T.copy())[None], torch.from_numpy(eps)[None], sid)[0, 0].numpy()
        mp, logs = m.enc_p(torch.from_numpy(phone.T.copy())[None])
    st = NR.synth(cfg, tens, phone, eps)
    e_stats = SR.max_over_rms(st["sy.stats"], torch.cat([mp, logs], 1)[0].numpy())
    e_pcm = SR.max_over_rms(st["pcm"], ref)
    print("%s: stats %.2e  pcm %.2e  (bound %.0e)" % (preset, e_stats, e_pcm, ROUNDOFF))
    assert st["pcm"].shape == ref.shape == (R * int(np.prod(_rates(preset))),)
    assert e_stats <= ROUNDOFF and e_pcm <= ROUNDOFF
    # the two stages this file's subject changes are not no-ops of the f0 stages: with the f0 twin's tensors the f0 stage functions differ from them
    cfg1, t1 = W.make_synth(preset, 48)
    x = st["sy.pre"]
    assert SR.max_over_rms(SR.dec_up(cfg1, t1, 0, x, np.full(st["pcm"].shape[0], 0.3)), st["sy.up0"]) > 1e-3
    assert SR.max_over_rms(SR.embed(cfg1, t1, phone, np.full(R, 220.0)), st["sy.emb"]) > 1e-3


# ---- the importer -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["tiny", "tiny5"])
def test_import_round_trip_of_a_nono_state_dict(preset):
    sid = 2
    cfg, tens = W.make_synth(preset, 48, f0=False)
    sd = _state_dict(load_blob(nono_module(preset), cfg, tens, sid))
    assert not any("emb_pitch" in k or "m_source" in k or "noise_convs" in k for k in sd)
    assert any(k.endswith("weight_g") or "parametrizations" in k for k in sd)
    c2, t2 = IM.import_synth(sd, sid=sid, up_rates=_rates(preset), heads=int(cfg["heads"]))
    assert c2["f0"] == 0 and {k: int(v) for k, v in c2.items()} == {k: int(v) for k, v in cfg.items()}
    assert set(t2) == set(tens) and not any(W.is_f0_only(k) for k in t2)
    for k in tens:
        a, b = np.asarray(t2[k], np.float32), tens[k]
        assert a.shape == b.shape, k
        weight_normed = k.startswith("sy.flow") and (".in" in k or ".rs" in k or ".cond." in k) and k.endswith(".w") or \
            k.startswith(("sy.dec.up", "sy.dec.rb")) and k.endswith(".w")
        if weight_normed:
            assert np.all(np.abs(a.astype(np.float64) - b) <= WN_RTOL * np.abs(b)), k
        else:
            assert a.tobytes() == b.tobytes(), k
    # the checkpoint's own list gives the rates as well, and an f0 entry that agrees is accepted
    config = [0, 0, 0, 0, 0, int(cfg["heads"]), 0, 0, 0, "1", [], [], _rates(preset), 0, [int(k) for k in W.SYNTH_PRESETS[preset]["up_kernels"]], 0, 0, int(cfg["sr"])]
    c3, _ = IM.import_synth(sd, sid=sid, config=config, f0=0)
    assert c3["f0"] == 0 and c3["sr"] == cfg["sr"] and [c3["up_rate%d" % i] for i in range(int(cfg["n_ups"]))] == _rates(preset)


def _f0_state_dict(sid=0):
    cfg, tens = W.make_synth("tiny", 48)
    m = TI._upstream_synth()
    return {k: v.detach().numpy() for k, v in m.state_dict().items()}


def test_import_failures():
    cfg, tens = W.make_synth("tiny", 48, f0=False)
    nono = _state_dict(load_blob(nono_module("tiny"), cfg, tens, 0))
    full = _f0_state_dict()
    IM.import_synth(full, up_rates=[4, 3, 2, 2], heads=2)                  # the f0 dict itself imports, with or without an agreeing entry
    c, _ = IM.import_synth(full, up_rates=[4, 3, 2, 2], heads=2, f0=1)
    assert "f0" not in c
    # mixtures: one of the three groups present without the others, or one missing
    for drop in ("enc_p.emb_pitch", "dec.m_source", "dec.noise_convs"):
        mixed = {k: v for k, v in full.items() if drop not in k}
        with pytest.raises(IM.ImportError_) as ei:
            IM.import_synth(mixed, up_rates=[4, 3, 2, 2], heads=2)
        assert drop in str(ei.value) and "but not" in str(ei.value), str(ei.value)
        only = dict(nono, **{k: v for k, v in full.items() if drop in k})
        with pytest.raises(IM.ImportError_) as ei:
            IM.import_synth(only, up_rates=[4, 3, 2, 2], heads=2)
        assert drop in str(ei.value), str(ei.value)
    # a no-f0 model has no noise convs: sr alone gives no rates
    with pytest.raises(IM.ImportError_) as ei:
        IM.import_synth(nono, sr=4800, heads=2)
    assert "sr alone" in str(ei.value) and "up_rates" in str(ei.value), str(ei.value)
    with pytest.raises(IM.ImportError_):
        IM.import_synth(nono, heads=2)
    with pytest.raises(IM.ImportError_):                                  # ... and rates that do not multiply to sr / 100 are still refused
        IM.import_synth(nono, sr=4800, up_rates=[4, 3, 2, 4], heads=2)
    # the checkpoint's f0 entry against its tensors, both ways
    with pytest.raises(IM.ImportError_) as ei:
        IM.import_synth(nono, up_rates=[4, 3, 2, 2], heads=2, f0=1)
    assert "f0 = 1" in str(ei.value), str(ei.value)
    with pytest.raises(IM.ImportError_) as ei:
        IM.import_synth(full, up_rates=[4, 3, 2, 2], heads=2, f0=0)
    assert "f0 = 0" in str(ei.value), str(ei.value)


def test_checkpoint_file_with_a_contradicting_f0_entry(tmp_path):
    # through the file path the CLI takes: {"weight": sd, "config": [...], "f0": ..} as upstream's extract_small_model writes it
    cfg, tens = W.make_synth("tiny", 48, f0=False)
    m = load_blob(nono_module("tiny"), cfg, tens, 0)
    config = [0, 0, 16, 16, 32, 2, 2, 3, 0, "1", [3, 5], [[1, 3], [1, 3]], [4, 3, 2, 2], 32, [8, 7, 4, 4], 3, 8, 4800]
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    good, bad = str(tmp_path / "nono.pth"), str(tmp_path / "bad.pth")
    torch.save({"weight": sd, "config": config, "f0": 0, "version": "v2"}, good)
    torch.save({"weight": sd, "config": config, "f0": 1, "version": "v2"}, bad)
    assert IM.load_checkpoint_f0(good) == 0 and IM.load_checkpoint_f0(bad) == 1
    out = str(tmp_path / "nono.rvcw")
    IM.main(["synth", good, out])
    c, t = W.read_blob(out)
    assert c["f0"] == 0.0 and not any(W.is_f0_only(k) for k in t) and c["sr"] == 4800.0
    with pytest.raises(IM.ImportError_):
        IM.convert("synth", bad, str(tmp_path / "bad.rvcw"))
