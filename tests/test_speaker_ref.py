"""Run-time speaker selection, the part that needs no GPU: the blob (make_synth n_spk, import_synth speakers), the float64
reference of the fold and of the mix rule (tests/speaker_ref.py), the CLI's mix parser, and the four calls on every public surface."""
import os
import re

import numpy as np
import pytest

import nof0_ref as NR
import speaker_ref as SP
from common import ROOT
from obs_rvc_amd import _native, convert as CV, importers as IM, weights as W
from test_nof0_ref import PARENT_DIGEST


@pytest.mark.parametrize("preset,phone_dim", sorted(PARENT_DIGEST))
def test_make_synth_with_one_speaker_is_what_it_was(preset, phone_dim):
    cfg, tens = W.make_synth(preset, phone_dim, n_spk=1)
    assert "sy.emb_g" not in tens and "n_spk" not in cfg
    assert NR.blob_digest(cfg, tens) == PARENT_DIGEST[(preset, phone_dim)]


@pytest.mark.parametrize("f0", [True, False])
def test_make_synth_with_a_table_keeps_every_other_tensor(f0, tmp_path):
    cfg1, t1 = W.make_synth("tiny", 48, seed=5, f0=f0)
    cfg3, t3 = W.make_synth("tiny", 48, seed=5, f0=f0, n_spk=3)
    assert list(t3)[:-1] == list(t1) and list(t3)[-1] == "sy.emb_g" and list(cfg3)[:-1] == list(cfg1) and cfg3["n_spk"] == 3
    for k in t1:
        assert t1[k].dtype == t3[k].dtype and np.array_equal(t1[k].view(np.uint32), t3[k].view(np.uint32)), k
    emb = t3["sy.emb_g"]
    assert emb.shape == (3, int(cfg1["gin"])) and emb.dtype == np.float32 and np.array_equal(emb[0], t3["sy.g"])
    assert not np.array_equal(emb[1], emb[0]) and not np.array_equal(emb[2], emb[1]) and 0.5 < emb[1:].std() < 1.5
    # the other rows are a function of (seed, n_spk) alone and a prefix of a longer table's
    assert np.array_equal(W.make_synth("tiny", 48, seed=5, n_spk=9)[1]["sy.emb_g"][:3], emb)
    assert not np.array_equal(W.make_synth("tiny", 48, seed=6, n_spk=3)[1]["sy.emb_g"][1:], emb[1:])
    with pytest.raises(ValueError):
        W.make_synth("tiny", 48, n_spk=0)
    # the blob round trip and the zoo's file name
    p = str(tmp_path / "m.rvcw")
    W.write_blob(p, cfg3, t3)
    c, t = W.read_blob(p)
    assert c["n_spk"] == 3 and np.array_equal(t["sy.emb_g"], emb)
    z1 = W.build_model_zoo(str(tmp_path / "zoo"), "tiny")
    z3 = W.build_model_zoo(str(tmp_path / "zoo"), "tiny", n_spk=3)
    assert z1["model"] != z3["model"] and z1["data"] == z3["data"]
    assert "sy.emb_g" not in W.read_blob(z1["model"])[1] and W.read_blob(z3["model"])[1]["sy.emb_g"].shape[0] == 3


def test_import_synth_keeps_the_table_on_request(tmp_path):
    from test_importers import _upstream_synth
    m = _upstream_synth()
    sd = {k: v.detach().numpy() for k, v in m.state_dict().items()}
    emb = sd["emb_g.weight"]
    kw = dict(sr=4800, up_rates=[4, 3, 2, 2], heads=2)
    c0, t0 = IM.import_synth(sd, sid=1, **kw)
    assert "sy.emb_g" not in t0 and "n_spk" not in c0 and np.array_equal(t0["sy.g"], emb[1])
    ca, ta = IM.import_synth(sd, sid=1, speakers="all", **kw)
    assert ca["n_spk"] == 3 and np.array_equal(ta["sy.emb_g"], emb) and np.array_equal(ta["sy.g"], emb[1])
    assert {k: v for k, v in ca.items() if k != "n_spk"} == c0 and set(ta) == set(t0) | {"sy.emb_g"}
    for k in t0:
        assert np.array_equal(np.asarray(t0[k]), np.asarray(ta[k])), k
    c2, t2 = IM.import_synth(sd, sid=0, speakers=2, **kw)
    assert c2["n_spk"] == 2 and np.array_equal(t2["sy.emb_g"], emb[:2]) and np.array_equal(t2["sy.g"], emb[0])
    for bad in (dict(sid=2, speakers=2), dict(sid=0, speakers=4), dict(sid=0, speakers=0), dict(sid=0, speakers="some")):
        with pytest.raises(IM.ImportError_):
            IM.import_synth(sd, **bad, **kw)
    # the CLI: --speakers all writes the table, without it the file is what it was
    import torch
    src = str(tmp_path / "m.pth")
    torch.save({"weight": m.state_dict()}, src)
    IM.main(["synth", src, str(tmp_path / "a.rvcw"), "--sid", "1", "--sr", "4800", "--up-rates", "4,3,2,2"])
    IM.main(["synth", src, str(tmp_path / "b.rvcw"), "--sid", "1", "--sr", "4800", "--up-rates", "4,3,2,2", "--speakers", "all"])
    (cA, tA), (cB, tB) = W.read_blob(str(tmp_path / "a.rvcw")), W.read_blob(str(tmp_path / "b.rvcw"))
    assert "sy.emb_g" not in tA and cB["n_spk"] == 3 and np.array_equal(tB["sy.emb_g"], emb)
    assert NR.blob_digest(cA, tA) == NR.blob_digest({k: v for k, v in cB.items() if k != "n_spk"}, {k: v for k, v in tB.items() if k != "sy.emb_g"})


def test_fold_reference_is_the_loaders_fold_and_the_mix_rule():
    cfg, t = W.make_synth("tiny", 48, n_spk=9)
    H, G, nl, fn, C0 = int(cfg["hidden"]), int(cfg["gin"]), int(cfg["wn_layers"]), int(cfg["flow_n"]), int(cfg["up_init"])
    emb = t["sy.emb_g"]
    bias, mag = SP.fold(cfg, t, emb[4])
    assert bias.shape == mag.shape == (fn * nl * 2 * H + C0,) and np.all(mag >= np.abs(bias) - 1e-12)
    # spelled out for one row of one in-layer and one of dec_pre
    r = 2 * H * (1 * nl + 1) + 5
    want = float(t["sy.flow1.in1.b"][5]) + float(t["sy.flow1.cond.b"][2 * H + 5]) + float(np.dot(t["sy.flow1.cond.w"][2 * H + 5].astype(np.float64), emb[4].astype(np.float64)))
    assert abs(bias[r] - want) < 1e-12
    want = float(t["sy.dec.pre.b"][7]) + float(t["sy.dec.cond.b"][7]) + float(np.dot(t["sy.dec.cond.w"][7].astype(np.float64), emb[4].astype(np.float64)))
    assert abs(bias[fn * nl * 2 * H + 7] - want) < 1e-12
    # the loader's fp32 fold (cond_b + sum over q ascending, then + base_b) sits inside the bound
    j32 = []
    for bb, cw, cb in SP.layers(cfg, t):
        a = cb.astype(np.float32).copy()
        for q in range(G):
            a = a + cw[:, q] * emb[4][q]
        j32.append(bb + a)
    assert np.all(np.abs(np.concatenate(j32) - bias) <= SP.fold_bound(cfg, mag))
    # the mix rule
    ids, w = SP.normalise_mix({0: 3.0, 2: 1.0}, 3)
    assert ids == [0, 2] and w.tolist() == [0.75, 0.25]
    assert np.allclose(SP.mix_g(emb, ids, w), 0.75 * emb[0].astype(np.float64) + 0.25 * emb[2].astype(np.float64), rtol=0, atol=1e-15)
    ids, w = SP.normalise_mix([(i, 1.0 + i) for i in range(8)], 9)
    assert abs(w.sum() - 1.0) < 1e-15 and len(ids) == 8
    for bad in ({}, {i: 1.0 for i in range(9)}, {3: 1.0}, {-1: 1.0}, [(0, 1.0), (0, 1.0)], {0: -1.0}, {0: float("nan")}, {0: float("inf")}, {0: 0.0, 1: 0.0}):
        with pytest.raises(ValueError):
            SP.normalise_mix(bad, 3)
    # a blob baked for a speaker: no table, sy.g = that g in f32, the rest untouched
    cb_, tb_ = SP.baked(cfg, t, SP.mix_g(emb, [1, 2], [0.25, 0.75]))
    assert "n_spk" not in cb_ and "sy.emb_g" not in tb_ and tb_["sy.g"].dtype == np.float32 and set(tb_) == set(t) - {"sy.emb_g"}
    assert np.array_equal(SP.baked(cfg, t, emb[2])[1]["sy.g"], emb[2])


def test_glu_row_map_is_written_once_and_is_its_own_inverse():
    # engine_int.h: glu_model_row (what glu_pack_rows walks) and glu_packed_row (where the fold stores); restated here and composed
    src = open(os.path.join(_native.CSRC, "engine_int.h")).read()
    assert "glu_model_row(int p, int H)" in src and "glu_packed_row(int m, int H)" in src
    assert "glu_model_row(r, H)" in open(os.path.join(_native.CSRC, "model_synth.hip")).read()
    assert "glu_packed_row(m, L.glu_h)" in open(os.path.join(_native.CSRC, "speaker.hip.h")).read()

    def model_row(p, H):
        f, kq, rr = p >> 4, (p & 15) >> 2, p & 3
        return f * 8 + kq * 2 + (rr & 1) + (H if rr >= 2 else 0)

    def packed_row(m, H):
        hi = 1 if m >= H else 0
        q = m - hi * H
        return (q >> 3) * 16 + ((q & 7) >> 1) * 4 + (q & 1) + 2 * hi
    for H in (8, 16, 192):
        assert [packed_row(model_row(p, H), H) for p in range(2 * H)] == list(range(2 * H))
        assert sorted(model_row(p, H) for p in range(2 * H)) == list(range(2 * H))


def test_convert_cli_speaker_options():
    base = ["in.wav", "-o", "out.wav", "--model", "m.rvcw"]
    a = CV.parse_args(base)
    assert a.sid is None and a.sid_mix is None
    assert CV.parse_args(base + ["--sid", "2"]).sid == 2
    assert CV.parse_args(base + ["--sid-mix", "0:0.3,2:0.7"]).sid_mix == {0: 0.3, 2: 0.7}
    for bad in (["--sid", "-1"], ["--sid", "1", "--sid-mix", "0:1"], ["--sid-mix", "0"], ["--sid-mix", "0:1,0:2"], ["--sid-mix", "0:-1"], ["--sid-mix", "0:0"],
                ["--sid-mix", ",".join("%d:1" % i for i in range(9))], ["--sid-mix", "a:1"]):
        with pytest.raises(SystemExit):
            CV.parse_args(base + bad)


def test_the_four_calls_are_on_every_surface():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvc_mi355x.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "ffi.rs")).read()
    shim = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "rvc.rs")).read()
    for name in ("rvc_model_speakers", "rvc_set_speaker", "rvc_set_speaker_mix", "rvc_speaker_mix"):
        assert name in _native.SYMBOLS and re.search(r"\b%s\s*\(" % name, hdr) and re.search(r"pub fn %s\s*\(" % name, ffi) and "ffi::%s(" % name in shim, name
    dbg = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rvc_mi355x_debug.h")).read(), flags=re.S)
    assert "rvc_debug_speaker_biases(" in dbg and "rvc_debug_speaker_fold_ms(" in dbg
    from obs_rvc_amd.rvc import RvcInfer
    for m in ("speakers", "set_speaker", "set_speaker_mix", "speaker_mix"):
        assert callable(getattr(RvcInfer, m)), m
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "speaker_fold_kernel" in design and "rvc_set_speaker_mix" in design
