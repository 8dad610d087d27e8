"""front_stage_ref.py (ContentVec and RMVPE in float64, one function per tap interval) against the references the suite already trusts, and the check
that the GPU test built on it (tests/test_gpu_front_stages.py) would notice a wrong stage.  No GPU.

  * chain pin: the stages chained in fp32 give torch_ref.contentvec_hf / rmvpe_salience end to end, and every stage, teacher-forced from the C oracle's
    taps and evaluated in fp64, gives the oracle's next tap at the 1e-5 relative RMS of test_synth_ref.py;
  * raw-form algebra: LayerNorm of a raw stage's output is the plain stage's output, every layer, in fp64;
  * folded-GEMM algebra: the folded restatement equals the layer-by-layer form in fp64, and in fp32 stays where fp32 puts it;
  * the test bites: with the oracle's fp32 taps standing in for the engine, every planted reference-side mistake pushes e = max |got - ref| / rms(ref)
    above that stage's bound (2e-5, or max(2e-5, 4 delta32)) by at least 10 x.  The ratios are printed: they are what justifies the bounds."""
import functools

import numpy as np
import pytest

import front_stage_ref as FS
import torch_ref as TR
from common import BASELINE_160MS as g, rel_rms, voice_signal, zoo
from obs_rvc_amd import weights as W
from oracle import oracle as O

torch = pytest.importorskip("torch")

CASES = [("tiny", 2), ("tiny", 1), ("full", 2)]
BITE = 10.0
SINGLE = ("cv.conv0", "cv.out", "rm.mel", "rm.cnn", "rm.sal")      # the one-launch stages: the per-layer bound


@functools.lru_cache(maxsize=None)
def _case(preset, version):
    """one oracle chunk with taps -> (ContentVec cfg, tensors, RMVPE cfg, tensors, audio, taps by the ENGINE's names and layouts)"""
    z = zoo(preset, version)
    ccfg, ct = W.read_blob("%s/contentvec/%s" % (z["data"], W.cv_blob_name(version)))
    rcfg, rt = W.read_blob("%s/f0/rmvpe.rvcw" % z["data"])
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(version); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(3, 1)
    ora.enable_taps(True)
    audio = voice_signal(g.input_buffer_16k_size, seed=4)
    ora.infer(audio, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
    taps = {}
    for nm in ["cv.conv0", "cv.feat", "cv.proj", "cv.pos", "cv.out", "rm.mel", "rm.int"] + ["cv.l%d" % l for l in range(int(ccfg["run_layers"]))] + \
            ["rm.%s%d" % (k, lv) for k in ("enc", "dec") for lv in range(int(rcfg["levels"]))]:
        taps[nm] = ora.tap(nm)
    Tm = FS.mel_frame(g.sample_frame_16k)[1]
    for nm in ("cnn", "gru", "sal"):                    # the oracle keeps these [Tm][C], the engine [C][Tm]
        taps["rm.%s_ct" % nm] = np.ascontiguousarray(ora.tap("rm." + nm).reshape(Tm, -1).T)
    ora.close()
    return ccfg, ct, rcfg, rt, audio, taps


def _getter(taps):
    return (lambda name, shape: taps[name].reshape(shape)), (lambda name: name in taps)


@pytest.mark.parametrize("preset,version", CASES)
def test_stages_reproduce_torch_ref_and_the_oracle(preset, version):
    ccfg, ct, rcfg, rt, audio, taps = _case(preset, version)
    get, has = _getter(taps)
    f32 = torch.float32
    # ContentVec chained in fp32 from the audio against the HuggingFace class
    x = FS.cv_pos(ccfg, ct, FS.cv_proj(ccfg, ct, FS.cv_stem(ccfg, ct, FS.cv_conv0(ccfg, ct, audio, f32), f32), f32), f32)
    for l in range(int(ccfg["run_layers"])):
        x = FS.cv_layer(ccfg, ct, l, x, f32)
    if int(ccfg["out_dim"]) != int(ccfg["embed"]):
        x = FS.cv_final_proj(ccfg, ct, x, f32)
    hf = TR.contentvec_hf(ccfg, ct, audio)
    e = rel_rms(x, hf)
    print("%s v%d ContentVec chained fp32 vs contentvec_hf %.2e" % (preset, version, e))
    assert x.shape == hf.shape and e < 1e-5, e
    # RMVPE chained in fp32 from the oracle's mel against rmvpe_salience
    mel = get("rm.mel", (128, -1))
    levels = int(rcfg["levels"])
    enc = [FS.rm_enc0(rcfg, rt, mel, f32)]
    for lv in range(1, levels):
        enc.append(FS.rm_enc(rcfg, rt, lv, enc[-1], f32))
    y = FS.rm_int(rcfg, rt, enc[-1], f32)
    for lv in range(levels):
        y = FS.rm_dec(rcfg, rt, lv, y, enc[levels - 1 - lv], f32)
    sal = FS.rm_sal(rcfg, rt, FS.rm_gru(rcfg, rt, FS.rm_cnn(rcfg, rt, y, f32), f32), f32)
    ref = TR.rmvpe_salience(rcfg, rt, mel).T
    e = rel_rms(sal, ref)
    print("%s RMVPE chained fp32 vs rmvpe_salience %.2e" % (preset, e))
    assert sal.shape == ref.shape and e < 1e-5, e
    # every stage in fp64 from the oracle's own upstream tap against the oracle's tap
    bad = []
    for stage, kind, got, fn, args, _ in FS.cv_stages(ccfg, ct, audio, get, has) + FS.rm_stages(rcfg, rt, audio, g.sample_frame_16k, get):
        if kind == "bits":
            assert np.array_equal(got, args[0]), stage
            continue
        r = fn(*args)
        e = rel_rms(got, r)
        print("%s v%d oracle tap vs fp64 stage %-9s %.2e" % (preset, version, stage, e))
        if not (r.shape == got.shape and e < 1e-5):
            bad.append((stage, e))
    assert not bad, bad


def _raw_chain(ccfg, ct, taps, dtype):
    """the raw taps of a folded plan from the oracle's cv.proj: {name: array}, evaluated layer by layer in `dtype`"""
    E, n = int(ccfg["embed"]), int(ccfg["run_layers"])
    out = {"cv.pos.raw": FS.cv_pos_raw(ccfg, ct, taps["cv.proj"].reshape(E, -1), dtype)}
    x = out["cv.pos.raw"]
    for l in range(n):
        last = l == n - 1
        x = FS.cv_layer_raw(ccfg, ct, l, x, dtype, norm=last)
        out["cv.l%d" % l if last else "cv.l%d.raw" % l] = x
    return out


@pytest.mark.parametrize("preset,version", CASES)
def test_raw_form_is_the_plain_stage_before_its_layernorm(preset, version):
    ccfg, ct, _, _, _, taps = _case(preset, version)
    E, n = int(ccfg["embed"]), int(ccfg["run_layers"])
    proj = taps["cv.proj"].reshape(E, -1)
    raw = FS.cv_pos_raw(ccfg, ct, proj)
    x = FS.cv_pos(ccfg, ct, proj)
    assert np.abs(FS.layer_norm_ct(raw, ct["cv.enc_ln.g"], ct["cv.enc_ln.b"]) - x).max() <= 1e-12 * np.abs(x).max()
    for l in range(n):
        y = FS.cv_layer(ccfg, ct, l, x)
        yraw = FS.cv_layer_raw(ccfg, ct, l, raw)
        d = np.abs(FS.layer_norm_ct(yraw, ct["cv.l%d.ln2.g" % l], ct["cv.l%d.ln2.b" % l]) - y).max() / np.abs(y).max()
        d2 = np.abs(FS.cv_layer_raw_last(ccfg, ct, l, raw) - y).max() / np.abs(y).max()
        print("%s v%d layer %d: LN(raw) vs plain %.1e, raw -> normalised vs plain %.1e" % (preset, version, l, d, d2))
        assert d <= 1e-11 and d2 <= 1e-11, (l, d, d2)
        x, raw = y, yraw
    # ... and the fp32 raw chain, the engine's stand-in below, ends on the oracle's last layer
    r32 = _raw_chain(ccfg, ct, taps, torch.float32)
    assert rel_rms(r32["cv.l%d" % (n - 1)], taps["cv.l%d" % (n - 1)].reshape(E, -1)) < 1e-5


@pytest.mark.parametrize("preset,version", CASES)
def test_folded_algebra(preset, version):
    """folded == layer by layer in fp64 (the algebra), and in fp32 the folded form stays within 1e-5 (max / rms) of fp64: the second yardstick of the
    folded plans' stages is of the size of the first"""
    ccfg, ct, _, _, _, taps = _case(preset, version)
    C, n = int(ccfg["conv_dim"]), int(ccfg["run_layers"])
    feat = taps["cv.feat"].reshape(C, -1)
    checks = [("cv.proj", FS.cv_proj, FS.cv_proj_folded, (ccfg, ct, feat))]
    raws = _raw_chain(ccfg, ct, taps, torch.float64)
    x = raws["cv.pos.raw"]
    for l in range(n):
        last = l == n - 1
        checks.append(("cv.l%d" % l, FS.cv_layer_raw_last if last else FS.cv_layer_raw, FS.cv_layer_folded_last if last else FS.cv_layer_folded, (ccfg, ct, l, x)))
        x = raws["cv.l%d" % l if last else "cv.l%d.raw" % l]
    for name, plain, fold, args in checks:
        r64, d_plain = FS.stage_delta32(plain, *args)
        a64 = FS.max_over_rms(fold(*args), r64)
        a32 = FS.max_over_rms(fold(*args, dtype=torch.float32), r64)
        print("%s v%d %-7s folded vs plain fp64 %.1e; fp32 plain %.2e, fp32 folded %.2e" % (preset, version, name, a64, d_plain, a32))
        assert a64 <= 1e-11 and a32 <= 1e-5 and d_plain <= 1e-5, (name, a64, a32, d_plain)
        assert FS.folded_delta32(plain, fold, *args)[1] == max(d_plain, a32)


def _neighbour(a):
    """one output column of one channel replaced by its neighbour: the middle channel, the middle column (images: the middle row as well)"""
    b = np.array(a, np.float32)
    idx = tuple(n // 2 for n in b.shape)
    nxt = idx[:-1] + (idx[-1] + 1,)
    b[idx] = b[nxt]
    return b


@pytest.mark.parametrize("preset,version", CASES)
def test_planted_mistakes_are_caught(preset, version):
    ccfg, ct, rcfg, rt, audio, taps = _case(preset, version)
    get, has = _getter(taps)
    E, n, levels = int(ccfg["embed"]), int(ccfg["run_layers"]), int(rcfg["levels"])
    tag = "%s v%d" % (preset, version)
    weak = []

    def bite(what, stage, got, fn, args, fold=None, wrong=None, **flaw):
        """got against the right reference (must pass) and against the mistaken one / with a corrupted `got` (must miss by >= BITE x)"""
        e0, bound, _ = FS.judge("multi" if fold or stage not in SINGLE else "single", got, fn, args, fold)
        e1 = FS.max_over_rms(got if wrong is None else wrong, fn(*args, **flaw))
        print("%s %-24s %-10s clean e %.2e  bound %.1e  planted e %.2e  = %8.1f x bound" % (tag, what, stage, e0, bound, e1, e1 / bound))
        assert e0 <= bound, (what, stage, e0, bound)
        if not e1 >= BITE * bound:
            weak.append((what, stage, e1 / bound))

    # ---- the plain plan: the oracle's taps
    cv = {s[0]: s for s in FS.cv_stages(ccfg, ct, audio, get, has)}
    rm = {s[0]: s for s in FS.rm_stages(rcfg, rt, audio, g.sample_frame_16k, get)}
    _, _, got, fn, args, _ = cv["cv.pos"]
    bite("pos pad k/2 - 1", "cv.pos", got, fn, args, pad=int(ccfg["pos_k"]) // 2 - 1)
    bite("pos column dropped in front", "cv.pos", got, fn, args, drop="front")
    for lv in range(levels):
        _, _, got, fn, args, _ = rm["rm.dec%d" % lv]
        bite("concat skip first", "rm.dec%d" % lv, got, fn, args, swap=True)
    for st in ["rm.enc%d" % lv for lv in range(1, levels)] + ["rm.int"]:
        _, _, got, fn, args, _ = rm[st]
        bite("stride-2 pick for AvgPool", st, got, fn, args, pick=True)
    for st, (_, kind, got, fn, args, fold) in list(cv.items()) + list(rm.items()):
        if kind != "bits":
            bite("column <- its neighbour", st, got, fn, args, fold, wrong=_neighbour(got))
    # ---- the folded plan: its raw taps, evaluated in fp32 from the oracle's cv.proj
    raws = _raw_chain(ccfg, ct, taps, torch.float32)
    rtaps = dict(taps); rtaps.pop("cv.pos"); rtaps.update(raws)
    for l in range(n - 1):
        rtaps.pop("cv.l%d" % l)
    get2, has2 = _getter({k: np.asarray(v, np.float32) for k, v in rtaps.items()})
    cvr = {s[0]: s for s in FS.cv_stages(ccfg, ct, audio, get2, has2)}
    assert "cv.pos.raw" in cvr and all("cv.l%d.raw" % l in cvr for l in range(n - 1)) and "cv.l%d" % (n - 1) in cvr
    _, _, got, fn, args, _ = cvr["cv.pos.raw"]
    bite("pos pad k/2 - 1", "cv.pos.raw", got, fn, args, pad=int(ccfg["pos_k"]) // 2 - 1)
    bite("pos column dropped in front", "cv.pos.raw", got, fn, args, drop="front")
    for st, (_, kind, got, fn, args, fold) in cvr.items():
        if st.startswith("cv.l"):
            e0, bound, _ = FS.judge("multi", got, fn, args, fold)
            e1 = FS.max_over_rms(got, FS.cv_layer_raw(*args, norm=not st.endswith(".raw"), skip_pending=True))
            print("%s %-24s %-10s clean e %.2e  bound %.1e  planted e %.2e  = %8.1f x bound" % (tag, "pending LN left out", st, e0, bound, e1, e1 / bound))
            assert e0 <= bound, (st, e0, bound)
            if not e1 >= BITE * bound:
                weak.append(("pending LN left out", st, e1 / bound))
            bite("column <- its neighbour", st, got, fn, args, fold, wrong=_neighbour(got))
    assert not weak, weak

