"""tests/crepe_ref.py, the float64 definition of the CREPE f0 method, checked on the CPU: the length bookkeeping, a torch restatement
of the network (F.conv1d / batch_norm / max_pool1d in float64, kept here and not in the definition), Viterbi against brute force, the importer's round
trip, and what the GPU tests (tests/test_gpu_crepe.py) assume of their inputs: float32 and float64 agree bin for bin on the constructed ridges, and the
composite input has no frame within 1e-4 of the voicing threshold."""
import itertools

import numpy as np
import pytest

import crepe_ref as R
import yin_ref as Y
from obs_rvc_amd import importers, weights as W


def torch_network(t, F):
    """crepe_ref.network in torch float64: t = the blob's tensors (BatchNorm as scale and shift: running_mean 0, running_var 1 - eps)"""
    import torch
    import torch.nn.functional as TF
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = f64(F)[:, None, :]
    out = {}
    for l in range(6):
        n = l + 1
        x = TF.pad(x, R.PADS[l])
        x = TF.conv1d(x, f64(t["cr.conv%d.w" % n]), f64(t["cr.conv%d.b" % n]), stride=R.STRIDES[l])
        x = torch.relu(x)
        co = x.shape[1]
        x = TF.batch_norm(x, torch.zeros(co, dtype=torch.float64), torch.full((co,), 1.0 - R.BN_EPS, dtype=torch.float64), f64(t["cr.bn%d.scale" % n]),
                          f64(t["cr.bn%d.shift" % n]), False, 0.0, R.BN_EPS)
        x = TF.max_pool1d(x, 2)
        out["p%d" % n] = x.numpy()
    feat = x.permute(0, 2, 1).reshape(x.shape[0], -1)
    out["prob"] = torch.sigmoid(TF.linear(feat, f64(t["cr.fc.w"]), f64(t["cr.fc.b"]))).numpy()
    return out


def test_constants_and_length_bookkeeping():
    assert (R.LO, R.HI) == (39, 308)
    assert abs(R.F0_OF_BIN[0] - 31.70) < 0.01 and 50.0 > R.F0_OF_BIN[R.LO] > 49.0 and R.F0_OF_BIN[R.HI - 1] < 1100.0 < R.F0_OF_BIN[R.HI]
    for preset, m in (("full", 32), ("tiny", 4), ("micro", 1)):
        assert W.CREPE_PRESETS[preset] == R.CAPACITY[preset] == m
        shapes = R.layer_shapes(preset)
        assert [s[0] for s in shapes] == [c * m for c in (32, 4, 4, 4, 8, 16)]
        assert [s[3] for s in shapes] == [1024, 128, 64, 32, 16, 8] and [s[4] for s in shapes] == [256, 128, 64, 32, 16, 8]          # in, conv out
        assert [s[5] for s in shapes] == [128, 64, 32, 16, 8, 4]                                                                       # pooled: 1024 -> ... -> 4
        cfg, t = W.make_crepe(preset) if preset != "full" else (dict(kind=4, cap=32), None)
        assert cfg["cap"] == m
        if t is not None:
            cin = 1
            for l, (co, ci, k, *_rest) in enumerate(shapes):
                assert ci == cin and t["cr.conv%d.w" % (l + 1)].shape == (co, ci, k) and t["cr.bn%d.scale" % (l + 1)].shape == (co,)
                assert np.any(t["cr.bn%d.scale" % (l + 1)] < 0) or co < 8          # negative BatchNorm scales are in the zoo
                cin = co
            assert t["cr.fc.w"].shape == (360, 64 * m)
            o = R.network(t, np.zeros((2, 1024)))
            assert [o["p%d" % (l + 1)].shape for l in range(6)] == [(2, s[0], s[5]) for s in shapes] and o["prob"].shape == (2, 360)
    assert Y.f0_frame(2560) == 4960 and R.frames(Y.composite_signal(), 2560).shape == (32, 1024)


def test_frames_are_centred_and_normalised():
    x = Y.composite_signal()
    F = R.frames(x, 2560)
    sig = x[-4960:].astype(np.float64)
    raw = np.concatenate([np.zeros(512), sig, np.zeros(512)])[160 * 5:160 * 5 + 1024]          # frame 5: centred on sample 800
    assert raw[512] == sig[800]
    want = (raw - raw.mean()) / max(1e-10, raw.std(ddof=1))
    assert np.max(np.abs(F[5] - want)) < 1e-12
    assert np.all(R.frames(np.zeros(6000, np.float32), 2560) == 0.0)          # silence: 0 / 1e-10


@pytest.mark.parametrize("preset", ["micro", "tiny"])
def test_torch_restatement_agrees(preset):
    t = W.make_crepe(preset)[1]
    F = R.frames(Y.composite_signal(), 2560)
    a, b = R.network(t, F), torch_network(t, F)
    for k in a:
        assert a[k].shape == b[k].shape and np.max(np.abs(a[k] - b[k])) <= 1e-12, k


def test_viterbi_against_brute_force():
    rng = np.random.default_rng(1)
    for width in (1, 2, 3, 12):
        lt = R.log_transition(5, width)
        for trial in range(20):
            p = rng.random((4, 5))
            if trial % 4 == 0:
                p = np.round(p * 4) / 4          # exact ties
            lo = R.log_observation(p, 0, 5)
            best, arg = -np.inf, None
            for path in itertools.product(range(5), repeat=4):          # ascending: the first maximum is the lexicographically lowest
                s = R.path_score(lo, lt, path, 0, 5)
                if s > best + 1e-13:
                    best, arg = s, path
            got = R.viterbi(lo, lt, 0, 5)
            assert abs(R.path_score(lo, lt, got, 0, 5) - best) <= 1e-12, (width, trial)
            if trial % 4:
                assert tuple(got) == arg
    # the range: bins outside [lo, hi) are never decoded
    p = rng.random((6, 9)); p[:, [0, 8]] = 5.0
    assert np.all((R.viterbi(R.log_observation(p, 1, 8), R.log_transition(9, 3), 1, 8) >= 1) & (R.viterbi(R.log_observation(p, 1, 8), None, 1, 8) <= 7))


def test_filters_and_threshold():
    x = np.array([1.0, 5.0, 2.0, 9.0, 3.0])
    assert np.array_equal(R.filter3(x, "median"), [3.0, 2.0, 5.0, 3.0, 6.0]) and np.allclose(R.filter3(x, "mean"), [3.0, 8 / 3, 16 / 3, 14 / 3, 6.0])
    p = np.zeros((5, 360)); p[:, 150] = [0.5, 0.05, 0.5, 0.05, 0.05]
    d = R.decode(p)
    assert np.all(d["bins"] == 150) and np.array_equal(d["f0"] > 0, [True, True, False, False, False])          # pd filtered: .275 .5 .05 .05 .05
    assert np.allclose(d["f0"][:2], R.F0_OF_BIN[150])


def _state_dict(m, seed=3):
    """a torchcrepe-shaped state dict with float32 values and real BatchNorm statistics"""
    rng = np.random.default_rng(seed)
    sd, cin = {}, 1
    for n in range(1, 7):
        co, k = R.CHANNELS[n - 1] * m, R.KERNELS[n - 1]
        sd["conv%d.weight" % n] = (rng.standard_normal((co, cin, k, 1)) * 1.6 / np.sqrt(cin * min(k, 2 * R.LENGTHS[n - 1]))).astype(np.float32)
        sd["conv%d.bias" % n] = (0.05 * rng.standard_normal(co)).astype(np.float32)
        sd["conv%d_BN.weight" % n] = (rng.choice([-1.0, 1.0], co) * (1 + 0.2 * rng.standard_normal(co))).astype(np.float32)
        sd["conv%d_BN.bias" % n] = (0.1 * rng.standard_normal(co)).astype(np.float32)
        sd["conv%d_BN.running_mean" % n] = (0.3 + 0.1 * rng.standard_normal(co)).astype(np.float32)
        sd["conv%d_BN.running_var" % n] = (0.5 + rng.random(co)).astype(np.float32)
        sd["conv%d_BN.num_batches_tracked" % n] = np.array(7, np.int64)
        cin = co
    sd["classifier.weight"] = (rng.standard_normal((360, 4 * cin)) * 2.0 / np.sqrt(4 * cin)).astype(np.float32)
    sd["classifier.bias"] = (rng.standard_normal(360) - 1.0).astype(np.float32)
    return sd


def _torch_upstream(sd, F):
    """the state dict run as upstream runs it: batch_norm with the running statistics, float64"""
    import torch
    import torch.nn.functional as TF
    f64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = f64(F)[:, None, :, None]          # torchcrepe keeps a trailing unit axis: conv2d with [k][1] kernels
    for l in range(6):
        n = l + 1
        x = TF.pad(x, (0, 0) + R.PADS[l])
        x = TF.conv2d(x, f64(sd["conv%d.weight" % n]), f64(sd["conv%d.bias" % n]), stride=(R.STRIDES[l], 1))
        x = torch.relu(x)
        x = TF.batch_norm(x, f64(sd["conv%d_BN.running_mean" % n]), f64(sd["conv%d_BN.running_var" % n]), f64(sd["conv%d_BN.weight" % n]),
                          f64(sd["conv%d_BN.bias" % n]), False, 0.0, R.BN_EPS)
        x = TF.max_pool2d(x, (2, 1))
    feat = x.permute(0, 2, 1, 3).reshape(x.shape[0], -1)
    return torch.sigmoid(TF.linear(feat, f64(sd["classifier.weight"]), f64(sd["classifier.bias"]))).numpy()


def test_importer_round_trip(tmp_path):
    import torch
    sd = _state_dict(4)
    src, dst = str(tmp_path / "tiny.pth"), str(tmp_path / "crepe-tiny.rvcw")
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, src)
    importers.main(["crepe", src, dst])
    cfg, t = W.read_blob(dst)
    assert cfg == {"kind": 4.0, "cap": 4.0} and t["cr.conv2.w"].shape == (16, 128, 64) and t["cr.fc.w"].shape == (360, 256)
    F = R.frames(Y.composite_signal(), 2560)
    got, want = R.network(t, F)["prob"], _torch_upstream(sd, F)
    # the blob holds scale and shift rounded to float32 (2^-24 relative each), six layers deep, in front of a sigmoid whose slope is at most 1/4: 1e-5 is two
    # orders above what that rounding can do and four below a wrong axis order or a mis-folded BatchNorm
    err = float(np.max(np.abs(got - want)))
    print("importer round trip: largest posterior difference %.3e, posteriors %.3g .. %.3g" % (err, want.min(), want.max()))
    assert err <= 1e-5 and want.max() - want.min() > 0.2
    # anything that is not full or tiny is refused by name, and so is a dict with holes
    bad = _state_dict(2)
    with pytest.raises(importers.ImportError_, match="neither full"):
        importers.import_crepe(bad)
    del sd["conv3_BN.running_var"]
    with pytest.raises(importers.ImportError_, match="conv3_BN.running_var"):
        importers.import_crepe(sd)


def test_write_crepe_is_idempotent_and_the_zoo_is_unchanged(tmp_path):
    p = W.write_crepe(str(tmp_path), "micro")
    assert p.endswith("f0/crepe-micro.rvcw")
    before = open(p, "rb").read()
    assert W.write_crepe(str(tmp_path), "micro") == p and open(p, "rb").read() == before
    a, b = W.make_crepe("micro", 5)[1], W.make_crepe("micro", 5)[1]
    assert all(np.array_equal(a[k], b[k]) for k in a)
    z = W.build_model_zoo(str(tmp_path / "zoo"), "tiny")
    import os
    assert sorted(os.listdir(os.path.join(z["data"], "f0"))) == ["rmvpe.rvcw"]


def test_what_the_gpu_tests_assume_of_their_inputs():
    # the constructed ridges: float32 and float64 decode the same bins, the path stays on the ridge, the decoys are more than 40 bins away and win the arg-max
    for Tm, seed in ((32, 320), (32, 321), (32, 322), (1024, 10240), (32, 99)):
        p, centre, decoy = R.ridge_case(Tm, seed)
        a, b = R.decode(p, "viterbi"), R.decode(p, "viterbi", np.float32)
        assert np.array_equal(a["bins"], b["bins"]) and np.max(np.abs(a["bins"] - centre)) <= 2
        am = R.decode(p, "argmax")["bins"]
        assert decoy and all(am[t] == d and abs(d - centre[t]) > 40 for t, d in decoy.items())
    # the composite input: no frame within 1e-4 of the threshold, both decoders, both test presets; posteriors not saturated
    x = Y.composite_signal()
    for preset in ("tiny", "micro"):
        t = W.make_crepe(preset)[1]
        for dec in ("viterbi", "argmax"):
            o = R.crepe(t, x, 2560, dec)
            assert np.min(o["margin"]) >= 1e-4, (preset, dec, np.min(o["margin"]))
        assert 0.0 < o["prob"].min() < 0.05 and 0.5 < o["prob"].max() < 0.99
    # the whole-window input (n == frame: the f0 window is the whole buffer, frames 0..3 and Tm - 4.. are zero-extended past its ends): inside the 10 % cap,
    # an end frame voiced (else the edge is not tested), float32 decodes the same bins, posteriors not saturated
    x = Y.whole_window_signal(5120)
    assert len(x) == Y.f0_frame(5120) == 10080
    for preset in ("tiny", "micro"):
        t = W.make_crepe(preset)[1]
        o, o32 = R.crepe(t, x, 5120, "viterbi"), R.crepe(t, x, 5120, "viterbi", np.float32)
        assert o["f0"].shape == (64,) and np.sum(o["margin"] < 1e-4) <= 6
        assert np.any(o["f0"][:4] > 0) or np.any(o["f0"][-4:] > 0)
        assert np.array_equal(o["bins"], o32["bins"])
        assert 0.0 < o["prob"].min() < 0.05 and 0.5 < o["prob"].max() < 0.99
        # frame 0: 512 zeros in front of the buffer's first 512 samples, then normalised -- its first half is one constant, its second is not
        assert np.ptp(o["frames"][0][:512]) == 0.0 and np.ptp(o["frames"][0][512:]) > 0.1 and np.ptp(o["frames"][63][-511:]) == 0.0


def test_cli_names_the_presets_by_their_files():
    # --f0 takes the CREPE presets under the names of their weight files; the bare word "crepe" stays the unknown choice it was (tests/test_convert_ref.py)
    from obs_rvc_amd.convert import parse_args
    for name in ("crepe-full", "crepe-tiny"):
        assert parse_args(["in.wav", "-o", "o.wav", "--model", "m", "--f0", name]).f0 == name
    with pytest.raises(SystemExit):
        parse_args(["in.wav", "-o", "o.wav", "--model", "m", "--f0", "crepe"])
