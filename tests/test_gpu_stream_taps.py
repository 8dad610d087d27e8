"""Every stream of a batched plan, stage by stage, against float64.

A tap used to show stream 0 only; streams 1..S-1 of a batched plan were checked through their PCM alone, at 1e-3 absolute RMS.  Here every stream of every
plan has its own input, pitch shift and stream id, two chunks are run (the Philox key's chunk counter and the pitch cache have moved), and every tapped
interval of the synthesizer is TEACHER-FORCED: the stage's float64 value (tests/synth_ref.py) is computed from the GPU's own upstream tap of the same stream,
so an error is charged to the stage that made it.  Metric: e = max |gpu - ref64| / rms(ref64), the per-layer metric of the suite.

  * one launch / one elementwise kernel (embed, stats, prior, latent stretch, decoder pre, each up, post): e <= TOL = 2e-5 (tests/test_gpu_tiles.py)
  * pure gathers (phone gather, the final flip): bitwise
  * multi-layer stages (encoder, encoder + stats, each flow, each ResBlock stage): e <= max(TOL, 4 delta32), delta32 = torch's own fp32 evaluation of the
    stage on the same inputs against the fp64 one -- the reference's error, never the engine's; 4 = two summation reorderings (kernel vs torch, composed vs
    layer by layer), each of the order of delta32.  A wrong element costs >= 1e-3 of rms at these weights.
  * ContentVec / RMVPE taps and f0 of every stream against that stream's own oracle at test_stage_by_stage's 1e-4 relative RMS.

Cases sit on the planner's thresholds (composed WaveNets and gru_multi up to 8 streams, CU partition up to 4, LayerNorm strips / LDS GEMMs from 16,
ResBlock chains unfused from 16), not at workload size.  Upstream's other decoder layouts (v1 48k, v1 32k: five stages down to 16 channels; v2 32k) run
at toy width on both plans, at full width on the production plan and at 20 streams, where the profile shows which kernel ran which stage.  Every (stage, e, delta32, e / delta32) is printed; DESIGN.md "Synthesizer stages: what is tested"
records the worst per stage and plan."""
import functools

import numpy as np
import pytest

import debug_abi as D
import synth_ref as SR
from common import BASELINE_160MS as g, TAP_MAP, rel_rms, rms, set_opt, synth_zoo, voice_signal
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import RvcInferError

pytestmark = pytest.mark.gpu
TOL = 2e-5                 # the per-layer bound of tests/test_gpu_tiles.py
PCM_TOL = 1e-3
SEED, ID0 = 11, 40
SHIFTS = [12, 0, -12, 5, 7, -7, 12, 3, -3, 0, 12, -12, 1, 2, 9, -9, 4, 6, 8, -5]
HINTS = {"rm.cnn": 32, "rm.gru": 32, "rm.sal": 32}
PARENT_OPS_1, PARENT_OPS_5 = 121, 132      # launches of the taps-off plans of 1 / 5 streams on `tiny`, measured on the parent commit's library


@functools.lru_cache(maxsize=None)
def _model(preset):
    z, _ = synth_zoo(preset)
    cfg, tens = W.read_blob(z["model"])
    return z, cfg, tens


def _version(preset):
    """the ContentVec version a preset's model takes (the v1 layouts: 1)"""
    return synth_zoo(preset)[1]


@functools.lru_cache(maxsize=None)
def _inputs(S):
    """two chunks, every stream its own signal: [chunk][stream][n]"""
    return [np.stack([voice_signal(g.input_buffer_16k_size, seed=1 + s + 20 * c) for s in range(S)]) for c in range(2)]


@functools.lru_cache(maxsize=None)
def _oracles(preset, S, R, streams):
    """per checked stream: (the oracle's taps of ContentVec / RMVPE / f0 after the second chunk, its PCM): computed once, shared by the plans' tests"""
    from oracle import oracle as O
    z, _, _ = _model(preset)
    xs = _inputs(S)
    out = {}
    for s in streams:
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(_version(preset)); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(SEED, ID0 + s)
        o.enable_taps(True)
        for c in range(2):
            y = o.infer(xs[c][s], g.sample_frame_16k, SHIFTS[s], g.skip_head, R)
        taps = {}
        for oname, _, _ in TAP_MAP:
            if oname.startswith(("cv.", "rm.")) or oname == "f0":
                try:
                    taps[oname] = o.tap(oname)
                except KeyError:                 # (a level the small RMVPE does not have)
                    pass
        o.close()
        out[s] = (taps, y)
    return out


def _engine(preset, S, level, formant=None):
    from obs_rvc_amd.rvc import RvcInfer
    z, _, _ = _model(preset)
    eng = RvcInfer(z["data"]); eng.load_contentvec(_version(preset)); eng.load_f0(); eng.load_model(z["model"])
    if S > 1:
        eng.set_streams(S)
    eng.set_noise_seed(SEED, ID0)
    for s, phi in (formant or {}).items():
        eng.set_formant_shift(phi, stream=s)
    eng.enable_taps(level)
    return eng


def _run(eng, S, R):
    xs = _inputs(S)
    for c in range(2):
        y = eng.infer_batch(xs[c], g.sample_frame_16k, np.array(SHIFTS[:S], np.int32), g.skip_head, R)
    return y


def _has(eng, name, p=0):
    try:
        eng.tap(name, p)
        return True
    except RvcInferError:
        return False


class Report:
    """collects (stage, e, delta32, bound) of one case, prints every figure, fails at the end with everything that missed"""

    def __init__(self, tag):
        self.tag, self.bad, self.worst = tag, [], {}

    def add(self, s, stage, e, bound, d32=None):
        ratio = e / d32 if d32 else float("nan")
        print("%s stream %2d %-10s e %.2e  delta32 %s  e/delta32 %6.2f  bound %.1e%s" % (self.tag, s, stage, e, "%.2e" % d32 if d32 is not None else "   -    ", ratio, bound,
                                                                                  "" if e <= bound else "   <-- MISSED"))
        w = self.worst.get(stage, (0.0, 0.0))
        self.worst[stage] = (max(w[0], e), max(w[1], ratio if d32 else 0.0))
        if not e <= bound:
            self.bad.append((s, stage, e, bound))

    def bits(self, s, stage, got, ref):
        ok = got.shape == ref.shape and D.same_bits(np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32))
        print("%s stream %2d %-10s %s" % (self.tag, s, stage, "bitwise" if ok else "DIFFERS   <-- MISSED"))
        if not ok:
            self.bad.append((s, stage, "bits", 0))

    def done(self):
        for st, (e, r) in self.worst.items():
            print("%s WORST %-10s e %.2e  e/delta32 %.2f" % (self.tag, st, e, r))
        assert not self.bad, (self.tag, self.bad)


def _front_taps(rep, eng, p, gs, otaps, phi=0.0, hints=HINTS):
    """ContentVec, RMVPE and f0 of plan stream p (engine stream gs) against that stream's oracle.  phi: the stream's formant shift -- by definition
     its f0 multiplier carries (float)2^(-phi/12); the oracle has no formant shift.  hints: the f0 frames Tm of the
    window, per transposed tap"""
    raw = _has(eng, "cv.pos.raw", p)             # plans with folded LayerNorms hold these two not yet normalised
    n = 0
    for oname, ename, tr in TAP_MAP:
        if oname not in otaps or (raw and oname in ("cv.pos", "cv.l0")):
            continue
        a, b = otaps[oname], eng.tap(ename, p)
        assert a.size == b.size, (oname, a.size, b.size)
        if oname == "f0" and phi:
            a = a * np.float32(2.0 ** (-phi / 12.0))
        if tr == "T":
            b = b.reshape(-1, hints[oname]).T.reshape(-1)
        rep.add(gs, oname, rel_rms(b, a), 1e-4)
        n += 1
    assert n >= 12, n


def _synth_stages(rep, cfg, tens, eng, p, gs, R, pcm, only=None, skip_head=g.skip_head, chunk=1):
    """every tapped interval of the synthesizer of plan stream p (engine stream gs: its Philox stream id is ID0 + gs), teacher-forced.  skip_head and
    chunk (the Philox chunk counter of the call that was tapped) default to this file's: the streaming window, second chunk"""
    from oracle import oracle as O
    C, H, I, fn, n_ups = (int(cfg[k]) for k in ("phone_dim", "hidden", "inter", "flow_n", "n_ups"))

    def tap(name, rows):
        return eng.tap(name, p).reshape(rows, -1)

    def single(stage, got, fnc, *args):
        if only is None or stage.rstrip("0123456789") in only:
            rep.add(gs, stage, SR.max_over_rms(got, fnc(*args)), TOL)

    def multi(stage, got, fnc, *args):
        if only is None or stage.rstrip("0123456789") in only:
            ref, d32 = SR.stage_delta32(fnc, *args)
            rep.add(gs, stage, SR.max_over_rms(got, ref), max(TOL, 4 * d32), d32)

    phone = tap("phone_ct", C)
    assert phone.shape == (C, R)
    if only is None:
        rep.bits(gs, "gather", phone, SR.phone_gather(tap("cv.out", C), skip_head, R))
    pitchf = eng.tap("pitchf").reshape(-1, R)[p]
    emb = tap("sy.emb", H)
    single("embed", emb, SR.embed, cfg, tens, phone, pitchf)
    stats = tap("sy.stats", 2 * I)
    if _has(eng, "sy.enc", p):
        enc = tap("sy.enc", H)
        multi("encoder", enc, SR.encoder, cfg, tens, emb)
        single("stats", stats, SR.stats, cfg, tens, enc)
    else:
        assert _has(eng, "sy.enc.raw", p)
        multi("enc+stats", stats, SR.encoder_stats, cfg, tens, emb)
    zp = tap("sy.zp", I)
    eps = O.philox_normal(SEED, ID0 + gs, chunk, 0, I * R).reshape(I, R)      # (this file: second chunk, chunk counter 1)
    single("prior", zp, SR.prior, cfg, stats, eps)
    zin = zp
    for fi in reversed(range(fn)):
        zf = tap("sy.flow%d" % fi, I)
        multi("flow%d" % fi, zf, SR.flow, cfg, tens, fi, zin)
        zin = zf
    z = tap("sy.z", I)
    if only is None:
        rep.bits(gs, "flip", z, SR.final_flip(cfg, zin))
    src = eng.tap("sy.src", p)
    if _has(eng, "sy.zi", p):
        zi = tap("sy.zi", I)
        single("stretch", zi, SR.latent_stretch, z, zi.shape[1])
        z, src = zi, eng.tap("sy.srci", p)
    x = tap("sy.pre", int(cfg["up_init"]))
    single("pre", x, SR.dec_pre, cfg, tens, z)
    for i in range(n_ups):
        u = tap("sy.up%d" % i, int(cfg["up_init"]) >> (i + 1))
        single("up%d" % i, u, SR.dec_up, cfg, tens, i, x, src)
        x = tap("sy.rb%d" % i, int(cfg["up_init"]) >> (i + 1))
        multi("rb%d" % i, x, SR.dec_rb, cfg, tens, i, u)
    out = tap("sy.dec", 1) if _has(eng, "sy.dec", p) else np.asarray(pcm).reshape(1, -1)
    single("post", out, SR.dec_post, cfg, tens, x)


def _case(preset, S, level, R=g.model_return_length, check=None, formant=None, plan_streams=None):
    """one plan: run two chunks, then check `check` (default: every stream).  plan_streams: the engine streams the LAST plan of the call holds, in plan
    order (default: all of them, one plan)"""
    z, cfg, tens = _model(preset)
    eng = _engine(preset, S, level, formant)
    y = _run(eng, S, R)
    plan_streams = list(range(S)) if plan_streams is None else plan_streams
    check = plan_streams if check is None else check
    rep = Report("%s S=%d R=%d taps=%d%s" % (preset, S, R, level, " formant" if formant else ""))
    ora = _oracles(preset, S, R, tuple(check))
    for gs in check:
        p = plan_streams.index(gs)
        _front_taps(rep, eng, p, gs, ora[gs][0], (formant or {}).get(gs, 0.0))
        _synth_stages(rep, cfg, tens, eng, p, gs, R, y[gs])
        if not formant:
            assert y[gs].shape == ora[gs][1].shape == (R * int(cfg["sr"]) // 100,) and rms(y[gs] - ora[gs][1]) < PCM_TOL, gs
    # the hook's stream 0 is rvc_get_tap's, bit for bit; a stream the plan did not have is refused
    for name in ("cv.out", "rm.enc0", "rm.sal_ct", "phone_ct", "sy.stats", "sy.flow0", "sy.z", "sy.rb0"):
        rc, a = D.debug_tap(eng, name, 0)
        assert rc == 0 and D.same_bits(a, eng.tap(name)), name
    assert D.debug_tap(eng, "sy.z", len(plan_streams))[0] == D.RVC_SHAPE and D.debug_tap(eng, "sy.z", -1)[0] == D.RVC_SHAPE
    with pytest.raises(RvcInferError):
        eng.tap("f0", len(plan_streams))
    ops = eng.plan_ops()
    eng.close()
    rep.done()
    return ops, rep


# ---- tiny: flow_n 2, H = I = 16.  8 | 9: composed WaveNets and gru_multi end; 5: past the CU partition; 17: past the 16-stream LayerNorm / LDS-GEMM / fused-ResBlock rules
@pytest.mark.parametrize("S", [1, 2, 5, 8, 9, 17])
def test_tiny_every_stream_both_plans(S):
    ops1, _ = _case("tiny", S, 1)
    ops2, _ = _case("tiny", S, 2)
    _composed_or_not(_model("tiny")[1], S, ops1, ops2)


def _composed_or_not(cfg, S, ops1, ops2):
    """Did the production plan (ops2 launches) take the path it is meant to, against the explicit plan of the same streams (ops1)?  Up to 8 streams it
    composes the WaveNets: a flow is wn_layers in-layers + one merged post / next-pre launch (+ one pre in front of the first) instead of pre, wn_layers x
    (in-layer, res_skip), post.  From 9 streams it runs them layer by layer and -- LayerNorm folds are for one stream -- is the explicit plan launch for launch."""
    fn, wl = int(cfg["flow_n"]), int(cfg["wn_layers"])
    saved = fn * (2 + 2 * wl) - (fn * (wl + 1) + 1)
    if S == 1:
        assert ops2 <= ops1 - saved, (ops1, ops2)            # (and the LayerNorm folds of the wide models)
    elif S <= 8:
        assert ops2 == ops1 - saved, (ops1, ops2)
    else:
        assert ops2 == ops1, (ops1, ops2)


@pytest.mark.parametrize("S", [2, 9])
@pytest.mark.parametrize("R", [1, 3])       # the shortest window the engine accepts; 3 < the WaveNet's 5 taps: both paddings overlap
def test_tiny_shortest_windows(S, R):
    for level in (1, 2):
        _case("tiny", S, level, R=R)


def test_tiny_many_streams_resblock_mean_as_a_launch():
    # 17 streams: the chains run one after the other and the last convolutions average in their epilogues (checked above); hook RVC_MEAN3: mean3_kernel instead
    try:
        set_opt("RVC_MEAN3", "1")
        z, cfg, tens = _model("tiny")
        eng = _engine("tiny", 17, 1)
        y = _run(eng, 17, g.model_return_length)
        rep = Report("tiny S=17 RVC_MEAN3")
        for s in range(17):
            _synth_stages(rep, cfg, tens, eng, s, s, g.model_return_length, y[s], only=("rb",))
        ops = eng.plan_ops()
        eng.close()
    finally:
        set_opt("RVC_MEAN3", None)
    ops_epi, _ = _case("tiny", 17, 1, check=[16])
    assert ops == ops_epi + int(cfg["n_ups"]), (ops, ops_epi)       # one averaging launch per stage
    rep.done()


# ---- tiny5: odd flow_n (one materialised flip), five upsampling stages, ResBlock kernels 3 / 7 / 11 on conv_tile
@pytest.mark.parametrize("S", [1, 3, 9])
def test_tiny5_every_stream_both_plans(S):
    ops1, _ = _case("tiny5", S, 1)
    ops2, _ = _case("tiny5", S, 2)
    _composed_or_not(_model("tiny5")[1], S, ops1, ops2)


def test_tiny5_formant_shift_on_one_stream_of_three():
    # Streams whose shifts give different decoder lengths run as one plan per length, shortest first (infer_r2_buckets): the call's LAST plan is stream 1's,
    # alone, on its gathered state -- its latent and source are stretched (sy.zi, sy.srci), its Philox stream is still ID0 + 1
    for level in (1, 2):
        _, rep = _case("tiny5", 3, level, formant={1: 3.0}, plan_streams=[1])
        assert "stretch" in rep.worst


def test_tiny5_formant_shift_on_every_stream_of_three():
    # ... and with the same shift on all three they share one plan: sy.zi and sy.srci of three different streams inside it
    for level in (1, 2):
        _, rep = _case("tiny5", 3, level, formant={0: 3.0, 1: 3.0, 2: 3.0})
        assert "stretch" in rep.worst


# ---- full: the production plan (folded LayerNorms at one stream, composed flows, fused decoder launches); streams 0 and S - 1
@pytest.mark.parametrize("S", [1, 2])
def test_full_production_plan(S):
    ops2, rep = _case("full", S, 2, check=sorted({0, S - 1}))
    assert ("enc+stats" in rep.worst) == (S == 1)               # LayerNorm fold: one stream only
    z, cfg, tens = _model("full")
    eng = _engine("full", S, 1)
    _run(eng, S, g.model_return_length)
    ops1 = eng.plan_ops()
    eng.close()
    _composed_or_not(cfg, S, ops1, ops2)
    if S == 1:
        assert ops2 < ops1 - 40                                  # as test_stage_by_stage: the folds took their launches out


# ---- upstream's other decoder layouts (weights.py SYNTH_PRESETS): v1 48k 10*6*2*2*2, v1 32k 10*4*2*2*2 (five stages: 512 channels down to 16; transposed convs of
# three / four taps per phase; noise convs of stride 48 / 32 / 8 / 2 and a one-tap one onto 16 channels; 256-d phone, ContentVec v1), v2 32k 10*8*2*2
LAYOUTS_TOY = ["tiny_v1_48k", "tiny_v1_32k", "tiny32k"]
LAYOUTS_FULL = ["full_v1_48k", "full_v1_32k", "full32k"]


@pytest.mark.parametrize("S", [1, 3, 9])
@pytest.mark.parametrize("preset", LAYOUTS_TOY)
def test_layout_toy_every_stream_both_plans(preset, S):
    ops1, _ = _case(preset, S, 1)
    ops2, _ = _case(preset, S, 2)
    _composed_or_not(_model(preset)[1], S, ops1, ops2)


@pytest.mark.parametrize("S", [1, 2])
@pytest.mark.parametrize("preset", LAYOUTS_FULL)
def test_layout_full_production_plan(preset, S):
    _, rep = _case(preset, S, 2, check=sorted({0, S - 1}))
    assert ("enc+stats" in rep.worst) == (S == 1)
    assert all("rb%d" % i in rep.worst and "up%d" % i in rep.worst for i in range(int(_model(preset)[1]["n_ups"])))


def _profile(eng):
    """the launches of the last (profiled) call that have a planner description: [(family, {M, N, K, B, nph})]"""
    import ctypes
    lib = eng._L
    lib.rvc_debug_profile_dump.restype = ctypes.c_int
    lib.rvc_debug_profile_dump.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(1 << 21)
    assert lib.rvc_debug_profile_dump(eng._h, buf, len(buf)) > 0
    out = []
    for ln in buf.value.decode().splitlines():
        w = ln.split(" ", 2)[2].split()
        kv = dict(x.split("=", 1) for x in w[1:] if "=" in x)
        if all(k in kv for k in ("M", "N", "K", "B", "nph")):
            out.append((w[0], {k: int(kv[k]) for k in ("M", "N", "K", "B", "nph")}))
    return out


MANY_STREAM_FAMILIES = {"c32s", "g32", "g32t", "g32l", "lds"}        # the workgroup-tiled / staged kernels of the many-stream plans (plan.hip queue_conv32s, queue_tiled)


@pytest.mark.parametrize("preset", LAYOUTS_FULL)
def test_layout_full_twenty_streams(preset):
    """20 streams: past the 16-stream rules (ResBlock chains one after the other, each conv a launch of its own; the plan-time tuner on).  One chunk; the ResBlock
    stages and the last layer of streams 0, 10 and 19 teacher-forced against fp64, their PCM against their own oracles, and from the profile which kernel
    ran which decoder stage.  What the planner's rules fix, and is asserted:
      * a 16-channel ResBlock convolution (the fifth stage of the v1 layouts) and the last layer behind it (1 x 16 x 7) can only run on reg: conv32s wants input
        channels in 32s, conv_tile two K shares of 16 channels each, the workgroup-tiled kernels more than 16 rows (tests/test_gpu_layers.py, EXPECTED);
      * so no c32s launch has a 16-channel input.
    What they do not fix: at 20 streams and 21 frames the v1 layouts' wider stages have 400 conv32s workgroups, fewer than the two per CU its size rule wants
    (plan.hip queue_conv32s), so the rules send them to reg / lds and the tuner decides by timing between that and conv32s / igemm32.  Asserted is therefore
    that the decoder as a whole did not fall back -- some ResBlock convolution of 32 channels or more ran on a many-stream kernel; the launches per stage and
    family are printed (DESIGN.md "Synthesizer stages: what is tested" has them from one run)."""
    from oracle import oracle as O
    S, R, check = 20, g.model_return_length, (0, 10, 19)
    z, cfg, tens = _model(preset)
    n_ups, c0 = int(cfg["n_ups"]), int(cfg["up_init"])
    eng = _engine(preset, S, 2)
    eng.set_profile(True)
    xs = _inputs(S)[0]
    y = eng.infer_batch(xs, g.sample_frame_16k, np.array(SHIFTS[:S], np.int32), g.skip_head, R)
    assert y.shape == (S, R * int(cfg["sr"]) // 100)
    prof = _profile(eng)
    rep = Report("%s S=%d one chunk" % (preset, S))
    for s in check:
        _synth_stages(rep, cfg, tens, eng, s, s, R, y[s], only=("rb", "post"), chunk=0)
    eng.close()
    # which kernel ran which stage: ResBlock convolutions are the launches with M = the stage's channels, K = M x 3 / 7 / 11 and the stage's columns (a description
    # has them per stream, or -- streams folded into N -- in all)
    widths = [c0 >> (i + 1) for i in range(n_ups)]
    cols = {m: S * R * int(np.prod([int(cfg["up_rate%d" % q]) for q in range(i + 1)])) for i, m in enumerate(widths)}
    by_stage = {}
    for fam, d in prof:
        if d["M"] in widths and d["K"] in (3 * d["M"], 7 * d["M"], 11 * d["M"]) and d["N"] * d["B"] == cols[d["M"]]:
            by_stage.setdefault(d["M"], {}).setdefault(fam, 0)
            by_stage[d["M"]][fam] += 1
    for m in widths:
        print("%s S=%d ResBlock convolutions of the %3d-channel stage: %s" % (preset, S, m, by_stage.get(m)))
        assert sum(by_stage.get(m, {}).values()) == 18, (m, by_stage.get(m))          # 3 kernels x 3 dilations x (c1, c2), one launch each
    post = [(fam, d) for fam, d in prof if d["M"] == 1 and d["K"] == 7 * widths[-1] and d["N"] * d["B"] == cols[widths[-1]]]
    print("%s S=%d last layer: %s" % (preset, S, post))
    assert len(post) == 1
    for fam, d in prof:
        if fam == "c32s":
            assert d["M"] >= 32 and d["K"] % 32 == 0 and not (d["M"] == 1 and d["K"] == 7 * 16), (fam, d)
    if 16 in widths:
        assert by_stage[16] == {"reg": 18} and post[0][0] == "reg", (by_stage[16], post)
    many = sum(n for m in widths if m >= 32 for fam, n in by_stage[m].items() if fam in MANY_STREAM_FAMILIES)
    assert many > 0, by_stage
    for s in check:
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(_version(preset)); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(SEED, ID0 + s)
        yo = o.infer(xs[s], g.sample_frame_16k, SHIFTS[s], g.skip_head, R)
        o.close()
        e = rms(y[s] - yo)
        print("%s S=%d stream %2d PCM rms error %.2e (bound %.0e)" % (preset, S, s, e, PCM_TOL))
        if not (y[s].shape == yo.shape and e < PCM_TOL):
            rep.bad.append((s, "pcm", e, PCM_TOL))
    rep.done()


def test_plans_without_taps_are_unchanged():
    # add_tap does nothing on a plan without taps: the launches of a taps-off plan are the parent commit's (measured there: 1 and 5 streams on tiny)
    from obs_rvc_amd.rvc import RvcInfer
    z, _, _ = _model("tiny")
    for S, parent_ops in ((1, PARENT_OPS_1), (5, PARENT_OPS_5)):
        eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
        if S > 1:
            eng.set_streams(S)
        eng.infer_batch(_inputs(S)[0], g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
        assert eng.plan_ops() == parent_ops, (S, eng.plan_ops())
        with pytest.raises(RvcInferError):
            eng.tap("sy.z")                                      # no taps on this plan
        eng.close()

