"""CPU checks of the FCPE definition (tests/fcpe_ref.py): the Slaney filterbank against its closed form, the numpy network against
torch.nn modules loaded with the same weights, the decoder against a loop written from the text, the importer's round trip, the seeded zoo's peakiness, the
command line, and every assumption tests/test_gpu_fcpe.py makes of its inputs."""
from __future__ import annotations

import numpy as np
import pytest

import fcpe_ref as R
import yin_ref as Y
from obs_rvc_amd import importers as IM
from obs_rvc_amd import weights as W

FRAME16K = 2560


@pytest.fixture(scope="module")
def micro():
    return W.make_fcpe("micro")[1]


# ------------------------------------------------------------------------------------------------ the filterbank
def test_slaney_scale_and_edges():
    assert W.slaney_hz_to_mel(1000.0) == 15.0 and abs(W.slaney_hz_to_mel(500.0) - 7.5) < 1e-12
    assert abs(W.slaney_hz_to_mel(6400.0) - 42.0) < 1e-9          # ln(6.4) / (ln(6.4) / 27) above 15
    f = W.fcpe_mel_edges()
    assert f.shape == (130,) and f[0] == 0.0 and abs(f[-1] - 8000.0) < 1e-9 and np.all(np.diff(f) > 0)
    assert np.max(np.abs(W.slaney_mel_to_hz(W.slaney_hz_to_mel(f)) - f)) < 1e-9


def _triangle_sum(f0, f1, f2, step=8000.0 / 512):
    """sum over the bin centres k * step of the triangle (f0, f1, f2) of height 2 / (f2 - f0), by two arithmetic series"""
    total = 0.0
    k0, k1 = int(np.floor(f0 / step)) + 1, int(np.floor(f1 / step))          # f0 < k step <= f1: the rising side
    if k1 >= k0:
        n = k1 - k0 + 1
        total += (n * (k0 + k1) / 2.0 * step - n * f0) / (f1 - f0)
    k2, k3 = k1 + 1, int(np.ceil(f2 / step)) - 1                               # f1 < k step < f2: the falling side
    if k3 >= k2:
        n = k3 - k2 + 1
        total += (n * f2 - n * (k2 + k3) / 2.0 * step) / (f2 - f1)
    return total * 2.0 / (f2 - f0)


def test_basis_against_its_closed_form():
    basis, band = W.fcpe_mel_basis()
    f = W.fcpe_mel_edges()
    assert basis.shape == (128, 513) and basis.dtype == np.float32 and band.shape == (128, 2)
    for m in range(128):
        want = _triangle_sum(f[m], f[m + 1], f[m + 2])
        assert abs(float(basis[m].astype(np.float64).sum()) - want) <= 1e-6 * want, m
        lo, hi = int(band[m, 0]), int(band[m, 1])
        assert 0 <= lo < hi <= 513 and hi - lo < 64 and np.all(basis[m, :lo] == 0) and np.all(basis[m, hi:] == 0) and basis[m, lo] > 0 and basis[m, hi - 1] > 0
    # the first filter spans 0 .. f[2] (about 47 Hz: the bins at 15.6 and 31.25 Hz); the last ends at 8000 Hz, whose bin carries weight 0
    assert band[0].tolist() == [1, 3] and band[127, 1] == 512 and basis[127, 512] == 0
    step = 8000.0 / 512
    assert abs(basis[0, 1] - (step / f[1]) * 2.0 / f[2]) < 1e-7 * basis[0, 1]
    assert int(np.argmax(basis[127])) == int(round(f[128] / step))


# ------------------------------------------------------------------------------------------------ the network against torch
def torch_network(t, mel):
    """torchfcpe's CFNaiveMelPE (conv_only) from torch.nn modules in float64: -> {"stack", "l0.dw", "l0" .., "prob"}"""
    import torch
    import torch.nn as nn
    tt = lambda k: torch.from_numpy(np.asarray(t[k], np.float64))
    H, I = t["fc.in1.w"].shape[0], t["fc.l0.dw.w"].shape[0]

    def load(mod, w, b):
        with torch.no_grad():
            mod.weight.copy_(w); mod.bias.copy_(b)
        return mod

    stack = nn.Sequential(load(nn.Conv1d(128, H, 3, 1, 1), tt("fc.in0.w"), tt("fc.in0.b")), load(nn.GroupNorm(4, H), tt("fc.gn.g"), tt("fc.gn.b")),
                          nn.LeakyReLU(), load(nn.Conv1d(H, H, 3, 1, 1), tt("fc.in1.w"), tt("fc.in1.b"))).double()
    out = {}
    with torch.no_grad():
        x = stack(torch.from_numpy(np.asarray(mel, np.float64))[None])
        out["stack"] = x[0].numpy()
        for l in range(R.n_layers(t)):
            p = "fc.l%d." % l
            ln = load(nn.LayerNorm(H), tt(p + "ln.g"), tt(p + "ln.b")).double()
            pw1 = load(nn.Conv1d(H, 2 * I, 1), tt(p + "pw1.w")[..., None], tt(p + "pw1.b")).double()
            dw = load(nn.Conv1d(I, I, 31, padding=15, groups=I), tt(p + "dw.w")[:, None, :], tt(p + "dw.b")).double()
            pw2 = load(nn.Conv1d(I, H, 1), tt(p + "pw2.w")[..., None], tt(p + "pw2.b")).double()
            d = nn.SiLU()(dw(nn.GLU(dim=1)(pw1(ln(x.transpose(1, 2)).transpose(1, 2)))))
            if l == 0:
                out["l0.dw"] = d[0].numpy()
            x = x + pw2(d)
            out["l%d" % l] = x[0].numpy()
        norm = load(nn.LayerNorm(H), tt("fc.norm.g"), tt("fc.norm.b")).double()
        proj = load(nn.Linear(H, 360), tt("fc.out.w"), tt("fc.out.b")).double()
        out["prob"] = torch.sigmoid(proj(norm(x.transpose(1, 2))))[0].numpy()
    return out


def test_network_against_torch_float64(micro):
    mel = R.logmel(micro, Y.composite_signal(), FRAME16K)
    assert mel.shape == (128, 32)
    ref, tor = R.network(micro, mel), torch_network(micro, mel)
    assert set(ref) == set(tor) == {"stack", "l0.dw", "l0", "l1", "prob"}
    for k in ref:
        rms = float(np.sqrt(np.mean(tor[k] ** 2)))
        err = float(np.max(np.abs(ref[k] - tor[k]))) / rms
        print("%s: max over rms %.3e" % (k, err))
        assert ref[k].shape == tor[k].shape and err <= 1e-12, k


def test_logmel_is_the_front_end_of_the_text(micro):
    """the frames against a loop: frame i is centred on sample 160 i of the reflect-padded window; Hann periodic; plain magnitudes"""
    x = Y.composite_signal()
    fr = Y.f0_frame(FRAME16K)
    sig = x[len(x) - fr:].astype(np.float64)
    mel = R.logmel(micro, x, FRAME16K)
    n = np.arange(1024)
    win = 0.5 - 0.5 * np.cos(2 * np.pi * n / 1024)
    for i in (0, 1, 17, 31):
        idx = 160 * i + n - 512
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= fr, 2 * fr - 2 - idx, idx)
        mag = np.abs(np.fft.rfft(sig[idx] * win))
        want = np.log(np.maximum(micro["fc.mel_basis"].astype(np.float64) @ mag, 1e-5))
        assert np.max(np.abs(mel[:, i] - want)) < 1e-9


# ------------------------------------------------------------------------------------------------ the decoder
def _brute_decode(p, threshold):
    out, bins, cents = [], [], []
    for row in np.asarray(p, np.float64):
        k = 0
        for i in range(360):
            if row[i] > row[k]:
                k = i
        num = den = 0.0
        for j in range(9):
            i = min(max(k - 4 + j, 0), 359)
            num += row[i] * R.CENTS[i]; den += row[i]
        f0 = 10.0 * 2.0 ** (num / den / 1200.0) if den > 0 else 0.0
        if row[k] <= threshold or f0 < 50.0:
            f0 = 0.0
        out.append(f0); bins.append(k); cents.append(num / den if den > 0 else np.nan)
    return np.array(out), np.array(bins), np.array(cents)


def edge_cases():
    """peaks at bins 0, 3, 356, 359 (the clamped indices repeat) and an interior one, on a floor of 0.01 with an asymmetric shoulder"""
    p = np.full((5, 360), 0.01, np.float32)
    for r, k in enumerate((0, 3, 356, 359, 200)):
        p[r, k] = 0.9
        p[r, min(k + 1, 359)] = max(p[r, min(k + 1, 359)], np.float32(0.4)) if k < 359 else p[r, 359]
        if k > 0:
            p[r, k - 1] = 0.2
    return p


def test_decoder_against_a_loop():
    rng = np.random.default_rng(3)
    cases = [edge_cases(), R.ridge_case(32, 7)[0], rng.random((16, 360)).astype(np.float32) * 0.5]
    ties = np.full((2, 360), 0.1, np.float32); ties[0, [100, 200]] = 0.9; ties[1] = 0.5
    cases.append(ties)
    for p in cases:
        for thr in (0.006, 0.45):
            got = R.decode(p, thr)
            f0, bins, cents = _brute_decode(p, thr)
            assert np.array_equal(got["bins"], bins) and np.max(np.abs(got["f0"] - f0)) <= 1e-9 * max(1.0, f0.max())
            assert np.max(np.abs(got["cents"] - cents)) <= 1e-9          # (the low edge decodes under the 50 Hz floor: its clamping shows here)
    e = R.decode(edge_cases())
    assert e["bins"].tolist() == [0, 3, 356, 359, 200]
    assert e["f0"][0] == 0.0 and e["f0"][1] == 0.0          # bins 0 and 3 lie below 50 Hz (bin 38 is the first above): the floor
    assert e["f0"][2] > 1900 and e["f0"][3] > e["f0"][2] and 315 < e["f0"][4] < 330
    t = R.decode(ties)
    assert t["bins"].tolist() == [100, 0] and t["f0"][1] == 0.0
    assert abs(R.CENTS[1] - R.CENTS[0] - (R.CENTS[-1] - R.CENTS[0]) / 359) < 1e-9 and abs(10 * 2 ** (R.CENTS[0] / 1200) - 32.70) < 1e-9


# ------------------------------------------------------------------------------------------------ the importer
def state_dict(t, spelling="weight_g", rng=None):
    """a torchfcpe-shaped state dict whose import gives t back: the classifier's rows split into a direction v of arbitrary length and the gain g = |w|"""
    rng = rng or np.random.default_rng(1)
    sd = {"input_stack.0.weight": t["fc.in0.w"], "input_stack.0.bias": t["fc.in0.b"], "input_stack.1.weight": t["fc.gn.g"], "input_stack.1.bias": t["fc.gn.b"],
          "input_stack.3.weight": t["fc.in1.w"], "input_stack.3.bias": t["fc.in1.b"], "norm.weight": t["fc.norm.g"], "norm.bias": t["fc.norm.b"],
          "output_proj.bias": t["fc.out.b"]}
    for l in range(R.n_layers(t)):
        q, p = "net.encoder_layers.%d.conformer.net." % l, "fc.l%d." % l
        sd[q + "0.weight"], sd[q + "0.bias"] = t[p + "ln.g"], t[p + "ln.b"]
        sd[q + "2.weight"], sd[q + "2.bias"] = t[p + "pw1.w"][..., None], t[p + "pw1.b"]
        sd[q + "4.conv.weight"], sd[q + "4.conv.bias"] = t[p + "dw.w"][:, None, :], t[p + "dw.b"]
        sd[q + "6.weight"], sd[q + "6.bias"] = t[p + "pw2.w"][..., None], t[p + "pw2.b"]
    w = t["fc.out.w"].astype(np.float64)
    g = np.sqrt(np.sum(w * w, axis=1, keepdims=True))
    v = w * rng.uniform(0.5, 2.0, size=(360, 1))
    names = ("output_proj.weight_g", "output_proj.weight_v") if spelling == "weight_g" else \
            ("output_proj.parametrizations.weight.original0", "output_proj.parametrizations.weight.original1")
    sd[names[0]], sd[names[1]] = g, v
    return sd


@pytest.mark.parametrize("spelling", ["weight_g", "parametrizations"])
def test_importer_round_trip(micro, spelling, tmp_path):
    cfg, t = IM.import_fcpe(state_dict(micro, spelling))
    assert cfg == dict(kind=5, hidden=64, inner=128, layers=2) and set(t) == set(micro)
    for k in micro:
        assert t[k].shape == micro[k].shape and np.allclose(t[k], micro[k], rtol=1e-6, atol=1e-9), k
    # through the file, as the command line goes
    import torch
    src, dst = str(tmp_path / "fcpe.pt"), str(tmp_path / "fcpe.rvcw")
    torch.save({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in state_dict(micro, spelling).items()}, src)
    IM.main(["fcpe", src, dst])
    cfg2, t2 = W.read_blob(dst)
    assert cfg2 == {"kind": 5.0, "hidden": 64.0, "inner": 128.0, "layers": 2.0}
    assert all(np.allclose(t2[k], micro[k], rtol=1e-6, atol=1e-9) for k in micro)


def test_importer_rejects_what_it_does_not_build(micro):
    sd = state_dict(micro)
    sd["net.encoder_layers.0.attn.to_q.weight"] = np.zeros((64, 64), np.float32)
    with pytest.raises(IM.ImportError_, match="attention"):
        IM.import_fcpe(sd)
    sd = state_dict(micro); del sd["norm.bias"]
    with pytest.raises(IM.ImportError_, match="norm.bias"):
        IM.import_fcpe(sd)
    sd = state_dict(micro); sd["net.encoder_layers.1.conformer.net.4.conv.weight"] = np.zeros((128, 1, 15), np.float32)
    with pytest.raises(IM.ImportError_, match="4.conv.weight"):
        IM.import_fcpe(sd)
    sd = state_dict(micro); sd["output_proj.weight_g"] = np.zeros((360,), np.float32)
    with pytest.raises(IM.ImportError_, match="weight_g"):
        IM.import_fcpe(sd)
    sd = state_dict(micro); sd["input_stack.0.weight"] = np.zeros((64, 80, 3), np.float32)
    with pytest.raises(IM.ImportError_, match="input_stack.0.weight"):
        IM.import_fcpe(sd)


# ------------------------------------------------------------------------------------------------ the zoo, the command line
@pytest.mark.parametrize("preset", ["micro", "full"])
def test_zoo_posteriors_are_peaky_and_unsaturated(preset):
    """on the composite input the top bin is at least twice the ninth-largest on at least three frames in four, and no posterior is pinned: the decoder's
    nine-bin window then holds a ridge, not a plateau"""
    t = W.make_fcpe(preset)[1]
    p = R.fcpe(t, Y.composite_signal(), FRAME16K)["prob"]
    s = np.sort(p, axis=1)
    peaky = int(np.sum(s[:, -1] >= 2.0 * s[:, -9]))
    print("%s: %d of 32 frames peaky, posteriors %.3g .. %.3g" % (preset, peaky, p.min(), p.max()))
    assert p.shape == (32, 360) and peaky >= 24 and p.max() < 0.95 and np.median(s[:, -1]) > 0.05
    cfg = W.make_fcpe(preset)[0]
    assert cfg == dict(kind=5, **W.FCPE_PRESETS[preset])
    assert W.FCPE_PRESETS["full"] == dict(hidden=512, inner=1024, layers=6) and W.FCPE_PRESETS["micro"] == dict(hidden=64, inner=128, layers=2)


def test_write_fcpe(tmp_path):
    import os
    path = W.write_fcpe(str(tmp_path), "micro")
    assert path == os.path.join(str(tmp_path), "f0", "fcpe.rvcw")
    cfg, t = W.read_blob(path)
    assert cfg["hidden"] == 64 and np.array_equal(t["fc.mel_basis"], W.fcpe_mel_basis()[0]) and t["fc.mel_band"].shape == (128, 2)
    with pytest.raises(ValueError):
        W.write_fcpe(str(tmp_path), "micro", as_preset="tiny")


def test_command_line_and_constants():
    from obs_rvc_amd import rvc_common as RC
    from obs_rvc_amd.convert import parse_args
    assert parse_args(["in.wav", "-o", "out.wav", "--model", "m.rvcw", "--f0", "fcpe"]).f0 == "fcpe"
    with pytest.raises(SystemExit):
        parse_args(["in.wav", "-o", "out.wav", "--model", "m.rvcw", "--f0", "crepe"])
    assert RC.F0_FCPE == 7 and (RC.F0_RMVPE, RC.F0_YIN, RC.F0_CREPE, RC.F0_CREPE_TINY) == (1, 2, 4, 5)


# ------------------------------------------------------------------------------------------------ what the GPU tests assume of their inputs
def test_assumptions_of_the_gpu_tests(micro):
    x = Y.composite_signal()
    assert len(x) >= Y.f0_frame(FRAME16K) == 4960 and Y.f0_frame(5120) == 10080
    r = R.fcpe(micro, x, FRAME16K)
    voiced = int(np.sum(r["f0"] > 0))
    assert 8 <= voiced and np.all(r["f0"][r["f0"] > 0] >= 50.0)          # the f0 comparison has frames to compare
    # the decoder cases: ridges follow their decoys, float32 and float64 agree bin for bin, every ridge frame is voiced
    for seed in (320, 321, 322):
        p, centre, decoy = R.ridge_case(32, seed)
        d64, d32 = R.decode(p), R.decode(p, dtype=np.float32)
        assert np.array_equal(d64["bins"], d32["bins"]) and all(d64["bins"][t] == k for t, k in decoy.items())
        rest = [t for t in range(32) if t not in decoy]
        assert np.max(np.abs(d64["bins"][rest] - centre[rest])) <= 1 and np.all(d64["f0"] > 0)
    # a value exactly at the threshold: the float next to 0.006 is not 0.006, so "exactly at" is stated on a threshold that is a float32
    thr = float(np.float32(0.25))
    assert thr == 0.25
    # a peak below 50 Hz: bin 10 is 36.7 Hz
    assert 35.0 < 10 * 2 ** (R.CENTS[10] / 1200) < 38.0
    # the depthwise cases: one past the time tile of 64, shorter than the filter, and an odd length
    assert 16 < R.DW_K < 65 < 101
