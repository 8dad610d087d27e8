"""Parity tests proper: the HIP path, called through the C ABI, against the CPU oracle and the committed
golden vectors.  Tolerance (BASELINE.json north_star): +-1e-3 RMS on the float PCM output, bit-exact kNN hits.
Per-stage relative RMS tolerances are tighter (1e-4) so that a wrong sub-stage cannot hide in the total."""
import os

import numpy as np
import pytest

from common import BASELINE_160MS as g, GOLDEN, chunk_stream, compare_taps, derive, rel_rms, rms, set_opt, voice_signal, zoo
from obs_rvc_amd import weights as W
from obs_rvc_amd.rvc_common import RvcInferError, RvcModelVersion

pytestmark = pytest.mark.gpu
PCM_TOL = 1e-3


def _pair(preset="tiny", version=2, seed=(1234, 0), taps=False):
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo(preset, version)
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(version); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(*seed)
    eng = RvcInfer(z["data"]); eng.load_contentvec(RvcModelVersion.from_value(version)); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(*seed)
    if taps:
        ora.enable_taps(True); eng.enable_taps(True)
    return z, ora, eng


def _flow_taps(ora, eng, n_flows, I):
    """(name, rel rms) of the latent behind every coupling layer.  The oracle holds it with flow_n - fi flips applied (rvc_oracle.c, the
    reference's Flip modules); the engine keeps the physical channel order and folds the flips into its weights."""
    out = []
    for fi in range(n_flows):
        a = ora.tap("sy.flow%d" % fi).reshape(I, -1)
        b = eng.tap("sy.flow%d" % fi).reshape(I, -1)
        if (n_flows - fi) % 2:
            b = b[::-1]
        out.append(("sy.flow%d" % fi, rel_rms(b, a)))
    return out


@pytest.mark.parametrize("preset", ["tiny", "full"])
def test_stage_by_stage(preset):
    z, ora, eng = _pair(preset, taps=True)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    yo = ora.infer(x, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
    ye = eng.infer(x, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
    hints = {"rm.cnn": 32, "rm.gru": 32, "rm.sal": 32, "phone": g.model_return_length}
    worst = {}
    for name, e, n in compare_taps(ora, eng, hints):
        worst[name] = e
        assert e < (5e-4 if name.startswith("sy.") else 1e-4), (name, e)
    assert len(worst) >= 25
    assert ye.shape == yo.shape == ((g.model_return_size,) if preset == "full" else (g.model_return_length * 48,))
    assert rms(ye - yo) < PCM_TOL
    cfg = W.read_blob(z["model"])[0]
    n_flows, inter = int(cfg["flow_n"]), int(cfg["inter"])
    for name, e in _flow_taps(ora, eng, n_flows, inter):
        assert e < 5e-4, (name, e)
    # The PRODUCTION plan of one stream (taps level 2): LayerNorms folded into the neighbouring GEMMs, every flow's WaveNet composed
    # (res_skip layers multiplied into the in-layers, post + next pre as one two-output launch), decoder on conv_tile_kernel.  Plans with
    # level-1 taps keep the explicit layers, so the algebraic rewrites were only ever checked through the final PCM:
    # here the latent behind EVERY flow, the prior statistics, the ContentVec output and every decoder stage are compared on that plan.
    from obs_rvc_amd.rvc import RvcInfer
    prod = RvcInfer(z["data"]); prod.load_contentvec(RvcModelVersion.V2); prod.load_f0(); prod.load_model(z["model"]); prod.set_noise_seed(1234, 0)
    prod.enable_taps(2)
    yp = prod.infer(x, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
    assert rms(yp - yo) < PCM_TOL
    seen = {}
    for name, e, n in compare_taps(ora, prod, hints, skip=("cv.pos", "cv.l0", "sy.enc")):     # not yet normalised on this plan (".raw" taps)
        seen[name] = e
        assert e < (5e-4 if name.startswith("sy.") else 1e-4), ("production plan", name, e)
    assert {"cv.out", "sy.stats", "sy.zp", "sy.z", "sy.pre", "sy.rb0", "sy.rb3", "rm.sal"} <= set(seen)
    for name, e in _flow_taps(ora, prod, n_flows, inter):
        assert e < 5e-4, ("production plan", name, e)
    if preset == "full":
        # the production plan did take the other code paths: folded LayerNorm (a ".raw" tap exists) and fewer launches than the explicit plan
        assert prod.tap("cv.pos.raw").size == eng.tap("cv.pos").size and not np.allclose(prod.tap("cv.pos.raw"), eng.tap("cv.pos"))
        assert prod.plan_ops() < eng.plan_ops() - 40


@pytest.mark.parametrize("preset,version", [("tiny", 2), ("tiny", 1), ("full", 2), ("full", 1)])      # (full, 1): v1 = ContentVec-256 (layer 9 + final_proj) + the v1 synthesizer, the literal reading of BASELINE configs[1] that the bench times
def test_stream_of_chunks(preset, version):
    # BASELINE configs[0]/[1]: a 16 kHz stream fed as 160 ms chunks through the 35 840-sample ring; state (pitch cache,
    # noise counters) carries across calls
    z, ora, eng = _pair(preset, version)
    n_chunks = 12 if preset == "tiny" else 5
    audio = voice_signal(g.sample_frame_16k * (n_chunks + 14), seed=1)
    rings = list(chunk_stream(audio, g.input_buffer_16k_size, g.sample_frame_16k))[-n_chunks:]
    for i, r in enumerate(rings):
        shift = [12, 0, -12, 7, 13][i % 5]
        yo = ora.infer(r, g.sample_frame_16k, shift, g.skip_head, g.model_return_length)
        ye = eng.infer(r, g.sample_frame_16k, shift, g.skip_head, g.model_return_length)
        assert rms(ye - yo) < PCM_TOL, (i, rms(ye - yo))
        assert np.abs(ye).max() <= 1.0
    assert np.allclose(eng.pitch_cache(), ora.pitch_cache(), rtol=1e-5, atol=1e-3)


def test_committed_golden_chain():
    d = np.load(os.path.join(GOLDEN, "tiny_chain.npz"))
    z, ora, eng = _pair("tiny", seed=(99, 5))
    rings = list(chunk_stream(d["audio"], g.input_buffer_16k_size, g.sample_frame_16k))[-4:]
    assert rel_rms(eng.extract_feature(rings[0]), d["feat"]) < 1e-4
    assert np.allclose(eng.pitch(rings[0], 12, g.sample_frame_16k), d["f0"], rtol=1e-5)
    for i, r in enumerate(rings):
        y = eng.infer(r, g.sample_frame_16k, 7 if i % 2 else -12, g.skip_head, g.model_return_length)
        assert rms(y - d["outs"][i]) < PCM_TOL
    assert np.allclose(eng.pitch_cache(), d["cache"], rtol=1e-5, atol=1e-3)


def test_api_surface_matches_rvcinfer():
    z, ora, eng = _pair("tiny")
    wav = np.load(os.path.join(GOLDEN, "ref_input_wav2.npy"))          # rvc/src/tests/input_wav2.npy (38240 samples)
    h = eng.hubert(wav)
    assert h.shape == (1, 48, 119) and rel_rms(h, ora.hubert(wav)) < 1e-4
    f = eng.extract_feature(wav)
    assert f.shape == (1, 239, 48)                                     # 2T+1 frames (Q2), as rvc/src/tests/feats.npy (1,239,768)
    assert np.array_equal(f[0, 0:238:2], f[0, 1:238:2]) and np.array_equal(f[0, 238], f[0, 236])
    assert rel_rms(f, ora.extract_feature(wav)) < 1e-4
    # rvc/src/tests/pitch.rs:19-30: pitch(input_wav2, 13, 4800); pitch() must not touch the cache
    p = eng.pitch(wav, 13, 4800)
    po = ora.pitch(wav, 13, 4800)
    assert p.shape == po.shape == (64,) and np.allclose(p, po, rtol=1e-5)
    assert not eng.pitch_cache().any()
    # Option::None pitch shift (rvc.rs:163)
    x = voice_signal(g.input_buffer_16k_size, seed=9)
    assert rms(eng.infer(x, 2560, None, 200, 21) - ora.infer(x, 2560, None, 200, 21)) < PCM_TOL


def test_error_behaviour_matches_reference():
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    eng = RvcInfer(z["data"])
    x = np.zeros(g.input_buffer_16k_size, np.float32)
    with pytest.raises(RvcInferError) as e:
        eng.infer(x, 2560, 12, 200, 21)
    assert e.value.kind == "ModelNotLoaded"                          # rvc.rs:141-143
    eng.load_model(z["model"])
    with pytest.raises(RvcInferError) as e:
        eng.infer(x, 2560, 12, 200, 21)
    assert e.value.kind == "ContentvecNotLoaded"                     # rvc.rs:85-88
    with pytest.raises(RvcInferError) as e:
        eng.hubert(x)
    assert e.value.kind == "ContentvecNotLoaded"
    eng.load_contentvec(RvcModelVersion.V2)
    with pytest.raises(RvcInferError) as e:
        eng.infer(x, 2560, 12, 200, 21)
    assert e.value.kind == "F0NotLoaded"
    eng.load_f0()
    assert eng.infer(x, 2560, 12, 200, 21).shape == (1008,)
    eng.unload_model()
    with pytest.raises(RvcInferError) as e:
        eng.infer(x, 2560, 12, 200, 21)
    assert e.value.kind == "ModelNotLoaded"
    with pytest.raises(RvcInferError) as e:
        eng.load_model("/nonexistent/model.onnx")
    assert e.value.kind == "Backend"
    eng.load_model(z["model"])
    with pytest.raises(RvcInferError) as e:                          # slice past the 2T+1 frames -> the reference panics
        eng.infer(x, 2560, 12, 220, 21)
    assert e.value.kind == "Panic"
    with pytest.raises(RvcInferError):                               # ragged / too-short input
        eng.infer(x[:300], 2560, 12, 0, 1)
    with pytest.raises(RvcInferError):                               # empty input
        eng.infer(x[:0], 2560, 12, 0, 1)
    with pytest.raises(RvcInferError):
        eng.hubert(x[:5])
    with pytest.raises(RvcInferError):                               # shorter than f0_extractor_frame: the reference's slice panics
        eng.pitch(x[:3000], 0, 2560)
    assert eng.infer(x, 2560, 12, 200, 21).shape == (1008,)          # the engine survives errors
    for n_geo in range(8):                                            # plan cache is bounded: many geometries in a row
        assert eng.infer(x, 2560, 12, 200 - n_geo, 21).shape == (1008,)


def test_other_geometries():
    # plugin default 0.30 s chunks (R=35, Tm=64), a short-context geometry and the minimum return length
    for gg in (derive(48000, 0.30, 0.07, 2.0, 48000), derive(48000, 0.10, 0.05, 0.5, 48000)):
        z, ora, eng = _pair("tiny")
        x = voice_signal(gg.input_buffer_16k_size, seed=4)
        for _ in range(2):
            yo = ora.infer(x, gg.sample_frame_16k, 12, gg.skip_head, gg.model_return_length)
            ye = eng.infer(x, gg.sample_frame_16k, 12, gg.skip_head, gg.model_return_length)
            assert ye.shape == yo.shape and rms(ye - yo) < PCM_TOL
    z, ora, eng = _pair("tiny")
    x = voice_signal(g.input_buffer_16k_size, seed=4)
    assert rms(eng.infer(x, 2560, 0, 222, 1) - ora.infer(x, 2560, 0, 222, 1)) < PCM_TOL   # last frame of the 2T+1 (Q2 clamp)


def test_hubert_window_lengths_full_preset():
    # ContentVec attention has three code paths by window length: T <= 128 and T <= 256 (matrix-core kernel with 2 / 4 key
    # fragments per wave) and the LDS-resident VALU kernel beyond; hubert() on 0.8 s .. 5.5 s windows crosses all of them
    z, ora, eng = _pair("full")
    for L in (12800, 38080, 60000, 88000):
        x = voice_signal(L, seed=11)
        ho, he = ora.hubert(x), eng.hubert(x)
        assert he.shape == ho.shape and he.shape[1] == 768
        assert rel_rms(he, ho) < 1e-4, (L, rel_rms(he, ho))
    fo, fe = ora.extract_feature(voice_signal(60000, seed=12)), eng.extract_feature(voice_signal(60000, seed=12))
    assert fe.shape == fo.shape and rel_rms(fe, fo) < 1e-4


def test_plugin_default_configuration_full_size():
    # the plugin's own defaults (obs-rvc/src/lib.rs:200-227): 0.30 s chunks, 40 kHz v2 synthesizer (rates 10*10*2*2), 48 kHz host
    # -> L = 38080, R = 35, Tm = 64, N = 14000; and the v1 family (256-d ContentVec layer 9 + final_proj) at full size
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    gg = derive(48000, 0.30, 0.07, 2.0, 40000)
    assert (gg.sample_frame_16k, gg.input_buffer_16k_size, gg.model_return_length, gg.model_return_size) == (4800, 38080, 35, 14000)
    for version in (2, 1):
        z = zoo("full", version, "full40k")
        ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(version); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(9, 2)
        eng = RvcInfer(z["data"]); eng.load_contentvec(RvcModelVersion.from_value(version)); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(9, 2)
        audio = voice_signal(gg.sample_frame_16k * 12, seed=21)
        rings = list(chunk_stream(audio, gg.input_buffer_16k_size, gg.sample_frame_16k))[-2:]
        for r in rings:
            yo = ora.infer(r, gg.sample_frame_16k, 5, gg.skip_head, gg.model_return_length)
            ye = eng.infer(r, gg.sample_frame_16k, 5, gg.skip_head, gg.model_return_length)
            assert ye.shape == yo.shape == (gg.model_return_size,)
            assert rms(ye - yo) < PCM_TOL, (version, rms(ye - yo))
        assert np.allclose(eng.pitch_cache(), ora.pitch_cache(), rtol=1e-5, atol=1e-3)


def test_silence_and_loud_inputs():
    z, ora, eng = _pair("tiny")
    for x in (np.zeros(g.input_buffer_16k_size, np.float32), np.load(os.path.join(GOLDEN, "ref_input_wav.npy"))[:g.input_buffer_16k_size],
              np.clip(voice_signal(g.input_buffer_16k_size, seed=6) * 20, -1, 1)):
        yo = ora.infer(x, 2560, 12, 200, 21)
        ye = eng.infer(x, 2560, 12, 200, 21)
        assert np.isfinite(ye).all() and rms(ye - yo) < PCM_TOL


@pytest.mark.parametrize("preset", ["tiny", "full"])
def test_retrieval_hits_bit_exact(preset):
    # BASELINE configs[2]: flat-L2, k=4, index_rate 0.75 (100k x 768 at full size)
    z, ora, eng = _pair(preset, taps=True)
    dim = 48 if preset == "tiny" else 768
    index = W.make_index(5000 if preset == "tiny" else 100000, dim, seed=7)
    ora.load_index(index); ora.set_index_rate(0.75)
    eng.load_index(index); eng.set_index_rate(0.75)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    for _ in range(2):
        yo = ora.infer(x, 2560, 12, 200, 21)
        ye = eng.infer(x, 2560, 12, 200, 21)
        io, do = ora.knn()
        ie, de = eng.knn()
        assert ie.shape == io.shape == (21, 4)
        # the queries come out of the ContentVec stack at ~1e-6 relative, so a hit could only flip on a ~1e-6 tie;
        # demand identical index arrays and distances to fp32 round-off of the query
        assert np.array_equal(ie, io)
        assert np.allclose(de, do, rtol=1e-4)
        assert rel_rms(eng.tap("phone_ct").reshape(dim, 21).T, ora.tap("phone").reshape(21, dim)) < 1e-4
        assert rms(ye - yo) < PCM_TOL


def test_folded_layernorm_every_tile_and_split():
    # the folded LayerNorm lives in the K-split epilogue of the table-free 1x1 GEMM: the models only ever reach two of its 15 instantiations
    # (5 tile shapes x K split 4 / 8 / 16).  All of them, on small layers, against a double-precision host LayerNorm + GEMM: the consumer
    # on the raw tensor (folded weights, statistics from the operand stream, published), then a layer whose residual is the normalised tensor
    import ctypes as C
    from obs_rvc_amd import _native
    L = _native.lib()
    L.rvc_debug_ln_fold_check.restype = C.c_double
    L.rvc_debug_ln_fold_check.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float]
    h = C.c_void_p()
    assert L.rvc_create(b"/tmp", 0, C.byref(h)) == 0
    try:
        for (M, K, N) in ((96, 256, 37), (64, 512, 111), (144, 768, 21)):
            e0 = L.rvc_debug_ln_fold_check(h, M, K, N, 0.3)             # the planner's own choice
            assert 0 <= e0 < 2e-5, (M, K, N, e0)
            # a tensor whose mean is 100x its spread: the statistics are taken relative to the column's first element, so the variance
            # survives; what remains is the cancellation acc - mean * wsum of the folded form (~1e-7 * mean / spread)
            e9 = L.rvc_debug_ln_fold_check(h, M, K, N, 100.0)
            assert 0 <= e9 < 2e-3, (M, K, N, e9)
            for cfg in range(5):
                for ks in (4, 8, 16):
                    if (K // 16) // ks < 1:
                        continue
                    set_opt("RVC_FORCE_CFG", "%d,%d" % (cfg, ks))
                    e1 = L.rvc_debug_ln_fold_check(h, M, K, N, 0.3)
                    assert 0 <= e1 < 2e-5, (cfg, ks, M, K, N, e1)
            set_opt("RVC_FORCE_CFG", None)
            # round 6: igemm2w_kernel's LayerNorm-consumer variant (32 x 32 wave tile, four / eight waves splitting K) for the consuming layer
            for ks in (4, 8):
                if (K // 16) < ks:
                    continue
                set_opt("RVC_FORCE_G2W", "0,%d" % ks)
                e2 = L.rvc_debug_ln_fold_check(h, M, K, N, 0.3)
                assert 0 <= e2 < 2e-5, ("g2w", ks, M, K, N, e2)
                e3 = L.rvc_debug_ln_fold_check(h, M, K, N, 100.0)
                assert 0 <= e3 < 2e-3, ("g2w", ks, M, K, N, e3)
            set_opt("RVC_FORCE_G2W", None)
    finally:
        set_opt("RVC_FORCE_CFG", None); set_opt("RVC_FORCE_G2W", None)
        L.rvc_destroy(h)


def test_folded_layernorm_one_stream_full_size():
    # One-stream plans of the full-size ContentVec fold the two LayerNorm launches of a layer into the GEMMs around them (column
    # statistics from the operand stream of the consuming projection, normalised residual computed in the epilogue).  Plans with taps
    # keep the explicit LayerNorm, so the stage tests above never see the folded path: here it runs (a) against the explicit path of
    # the same library, (b) against the oracle end to end, with retrieval hits bit-exact.
    from obs_rvc_amd.rvc import RvcInfer
    z, ora, eng = _pair("full")                      # no taps -> folded
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    h_fold = eng.hubert(x)
    set_opt("RVC_NO_LN_FUSE", "1")
    ref = RvcInfer(z["data"]); ref.load_contentvec(2); ref.load_f0(); ref.load_model(z["model"]); ref.set_noise_seed(1234, 0)
    h_expl = ref.hubert(x)
    set_opt("RVC_NO_LN_FUSE", None)
    assert h_fold.shape == h_expl.shape and not np.array_equal(h_fold, h_expl)        # two different code paths did run
    assert np.abs(h_fold - h_expl).max() < 1e-5 * np.abs(h_expl).max()
    assert rel_rms(h_fold, ora.hubert(x)) < 1e-4
    index = W.make_index(100000, 768, seed=7)
    for e in (ora, eng, ref):
        e.load_index(index); e.set_index_rate(0.75)
    for _ in range(2):
        yo = ora.infer(x, 2560, 12, 200, 21)
        ye = eng.infer(x, 2560, 12, 200, 21)
        yr = ref.infer(x, 2560, 12, 200, 21)
        io, do = ora.knn(); ie, de = eng.knn(); ir, dr = ref.knn()
        assert np.array_equal(ie, io) and np.array_equal(ir, io)
        assert np.allclose(de, do, rtol=1e-4)
        assert rms(ye - yo) < PCM_TOL and rms(ye - yr) < 1e-5
    ref.close()


def test_retrieval_scan_exact_on_identical_queries():
    # feed the GPU's own queries to the oracle's search: indices AND distances must be bit-identical
    # (same sequential-fmaf distance, same (distance, index) ordering)
    from oracle import oracle as O
    z, ora, eng = _pair("tiny", taps=True)
    index = W.make_index(7777, 48, seed=9)
    index[100] = index[50]; index[2000] = index[50]                   # exact ties
    eng.load_index(index); eng.set_index_rate(0.5)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    eng.set_index_rate(0.0)
    eng.infer(x, 2560, 12, 200, 21)
    q = eng.tap("phone_ct").reshape(48, 21).T.copy()                  # un-blended queries
    eng.reset_state(); eng.set_index_rate(0.5)
    eng.infer(x, 2560, 12, 200, 21)
    ie, de = eng.knn()
    io, do = O.knn_search(index, q, 4)
    assert np.array_equal(ie, io) and np.array_equal(de, do)
    # query equal to an index row: distance 0 hits, ties by ascending index
    io2, do2 = O.knn_search(index, index[50:51], 4)
    assert io2[0, :3].tolist() == [50, 100, 2000]


def test_retrieval_degenerate_index_reranks_flagged_workgroups():
    # thousands of exact duplicates: sixty copies of the nearest vector tie inside the error margin.  One stream runs the one-launch form, where nothing
    # can overflow: every workgroup whose list the copies saturate is flagged and all of its vectors are re-ranked exactly; the hits must be the
    # definition's (ties broken by ascending index).  The many-stream twin below is the one whose candidate set overflows
    from oracle import oracle as O
    z, ora, eng = _pair("tiny", taps=True)
    base = W.make_index(40, 48, seed=3)
    index = np.tile(base, (60, 1))                         # 2400 vectors, each repeated 60 times
    ora.load_index(index); ora.set_index_rate(0.5)
    eng.load_index(index); eng.set_index_rate(0.5)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    yo = ora.infer(x, 2560, 12, 200, 21)
    ye = eng.infer(x, 2560, 12, 200, 21)
    io, do = ora.knn(); ie, de = eng.knn()
    assert np.array_equal(ie, io) and np.allclose(de, do, rtol=1e-4)
    assert (np.diff(ie, axis=1) == 40).all()               # the four smallest indices of one duplicated vector
    assert rms(ye - yo) < PCM_TOL


def test_retrieval_degenerate_index_many_streams_take_the_overflow_fallback():
    # the many-stream twin: 12 streams x 11 queries = 132 >= 128 go through the query GEMM and knn_select_blend_kernel, which holds at most KNN_CAND = 512
    # candidates.  The same 40 vectors, each repeated 600 times: the copies of a query's nearest vector alone are 600 candidates with one approximate
    # distance, so every stream overflows and knn_scan_kernel + knn_merge_blend_kernel recompute it inside a real plan (60 copies, as above, stay below 512).
    # Hits of three streams against their own oracles, bit-exact; the four smallest indices of one duplicated vector
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    S = 12
    base = W.make_index(40, 48, seed=3)
    index = np.tile(base, (600, 1))
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    eng.set_streams(S); eng.set_noise_seed(1234, 0); eng.load_index(index); eng.set_index_rate(0.5)
    xin = np.stack([voice_signal(g.input_buffer_16k_size, seed=30 + s) for s in range(S)])
    ye = eng.infer_batch(xin, 2560, 12, 200, 21)
    ie, de = eng.knn(rows_cap=S * 64)
    assert ie.shape == (S * 21, 4)
    assert (np.diff(ie, axis=1) == 40).all()
    for s in (0, 5, 11):
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(1234, s)
        o.load_index(index); o.set_index_rate(0.5)
        yo = o.infer(xin[s], 2560, 12, 200, 21)
        io, do = o.knn()
        assert np.array_equal(ie[s * 21:(s + 1) * 21], io) and np.allclose(de[s * 21:(s + 1) * 21], do, rtol=1e-4), s
        assert rms(ye[s] - yo) < PCM_TOL, s
    eng.close()


def test_retrieval_runs_of_duplicates_expand_the_workgroups_that_hide_them():
    # one-launch retrieval (knn_scan_select_kernel): a workgroup publishes only its 4 best per query.  A run of near-identical vectors
    # next to each other in the index (silence frames of a training set) puts more than four candidates inside ONE workgroup's slice: its
    # list is saturated ("flagged") and the selector must re-rank every vector that workgroup scanned.  300 copies of the stream's own
    # query rows (exact duplicates: ties by ascending index) in three runs, one of them across a workgroup boundary; the GPU's own
    # un-blended queries go through the oracle's search: indices and distances bit-identical.
    from oracle import oracle as O
    z, ora, eng = _pair("tiny", taps=True)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    index = W.make_index(9000, 48, seed=11)
    eng.load_index(index); eng.set_index_rate(0.0)
    eng.infer(x, 2560, 12, 200, 21)
    q = eng.tap("phone_ct").reshape(48, 21).T.copy()                  # un-blended queries
    index[1000:1100] = q[4]                                           # a run inside one wave's tiles
    index[4090:4190] = q[10] + np.float32(1e-4) * index[4090:4190]     # near-duplicates, not exact
    index[8950:9000] = q[16]                                          # a run that ends with the index
    eng.load_index(index); eng.reset_state(); eng.set_index_rate(0.5)
    eng.infer(x, 2560, 12, 200, 21)
    ie, de = eng.knn()
    io, do = O.knn_search(index, q, 4)
    assert np.array_equal(ie, io) and np.array_equal(de, do)
    assert ie[4].tolist() == [1000, 1001, 1002, 1003] and ie[16].tolist() == [8950, 8951, 8952, 8953]
    assert 4090 <= ie[10].min() and ie[10].max() < 4190


@pytest.mark.parametrize("n", [4, 5, 17, 130])
def test_retrieval_index_smaller_than_the_grid(n):
    # the one-launch retrieval sizes its grid by the index: fewer 16-vector tiles than queries means fewer selectors than queries (each
    # takes several in turn), one tile means ONE workgroup that scans, publishes, waits for itself and selects all eleven queries
    from oracle import oracle as O
    z, ora, eng = _pair("tiny", taps=True)
    index = W.make_index(n, 48, seed=21 + n)
    ora.load_index(index); ora.set_index_rate(0.5)
    eng.load_index(index); eng.set_index_rate(0.5)
    x = voice_signal(g.input_buffer_16k_size, seed=3)
    for _ in range(2):
        yo = ora.infer(x, 2560, 12, 200, 21)
        ye = eng.infer(x, 2560, 12, 200, 21)
        io, do = ora.knn(); ie, de = eng.knn()
        assert np.array_equal(ie, io) and np.allclose(de, do, rtol=1e-4)
        assert rms(ye - yo) < PCM_TOL


def test_retrieval_two_query_groups_and_three_streams_in_one_launch_each():
    # knn_scan_select_kernel takes 16 queries per launch and one grid row per stream.  The plugin's default 300 ms chunk slices 35 frames =
    # 18 unique queries: two launches (16 + 2 queries, the second with fewer selectors than a full group); three streams with their own inputs
    # share the launches (grid.y = 3, a third of the workgroups each).  Hits of every stream against its own oracle, bit-exact.
    from common import derive
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    q = derive(48000, 0.30, 0.07, 2.0, 48000)
    assert (q.skip_head + q.model_return_length - 1) // 2 - q.skip_head // 2 + 1 > 16          # really two groups
    S = 3
    index = W.make_index(6000, 48, seed=13)
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    eng.set_streams(S); eng.set_noise_seed(77, 5); eng.load_index(index); eng.set_index_rate(0.6)
    oras = []
    for s in range(S):
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(77, 5 + s)
        o.load_index(index); o.set_index_rate(0.6)
        oras.append(o)
    for tick in range(2):
        xin = np.stack([voice_signal(q.input_buffer_16k_size, seed=400 + 10 * tick + s) for s in range(S)])
        ye = eng.infer_batch(xin, q.sample_frame_16k, [12, 0, -5], q.skip_head, q.model_return_length)
        ie, de = eng.knn(rows_cap=S * 64)
        R = q.model_return_length
        assert ie.shape == (S * R, 4)
        for s in range(S):
            yo = oras[s].infer(xin[s], q.sample_frame_16k, [12, 0, -5][s], q.skip_head, q.model_return_length)
            io, do = oras[s].knn()
            assert np.array_equal(ie[s * R:(s + 1) * R], io), (tick, s)
            assert np.allclose(de[s * R:(s + 1) * R], do, rtol=1e-4)
            assert rms(ye[s] - yo) < PCM_TOL, (tick, s)
    eng.close()


def test_batched_streams_match_single_stream_oracles():
    # BASELINE config 4 in miniature: S concurrent streams batched per stage, each with its own state
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    S = 5
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    eng.set_streams(S); eng.set_noise_seed(42, 10)
    oras = []
    for s in range(S):
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(42, 10 + s)
        oras.append(o)
    streams = [list(chunk_stream(voice_signal(g.sample_frame_16k * 17, seed=30 + s), g.input_buffer_16k_size, g.sample_frame_16k))[-3:] for s in range(S)]
    for c in range(3):
        xin = np.stack([streams[s][c] for s in range(S)])
        ye = eng.infer_batch(xin, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
        for s in range(S):
            yo = oras[s].infer(xin[s], g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
            assert rms(ye[s] - yo) < PCM_TOL, (c, s)
    for s in range(S):
        assert np.allclose(eng.pitch_cache(s), oras[s].pitch_cache(), rtol=1e-5, atol=1e-3)


def test_batched_streams_full_size_throughput_kernels():
    # full-size models, several streams: exercises the workgroup-tiled (LDS) implicit-GEMM path used in throughput mode
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    S = 6
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    eng.set_streams(S); eng.set_noise_seed(5, 100)
    xin = np.stack([voice_signal(g.input_buffer_16k_size, seed=50 + s) for s in range(S)])
    for c in range(2):
        ye = eng.infer_batch(xin, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
        if c == 0:
            oras = []
            for s in range(S):
                o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(5, 100 + s)
                oras.append(o)
        for s in (0, 3, 5):
            yo = oras[s].infer(xin[s], g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
            assert rms(ye[s] - yo) < PCM_TOL, (c, s, rms(ye[s] - yo))


def test_many_streams_full_size_take_the_throughput_paths():
    # 18 streams: past every small-batch special case (no CU partition above 4 streams, generic GRU above 8, unfused ResBlock chains,
    # tile LayerNorm and LDS-tiled GEMMs from 16) -- BASELINE config 4's code paths at a size the oracle can still check
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    S = 18
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    eng.set_streams(S); eng.set_noise_seed(6, 200)
    xin = np.stack([voice_signal(g.input_buffer_16k_size, seed=70 + s) for s in range(S)])
    ye = eng.infer_batch(xin, g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
    assert ye.shape == (S, g.model_return_size) and np.isfinite(ye).all()
    for s in (0, 9, 17):
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(6, 200 + s)
        yo = o.infer(xin[s], g.sample_frame_16k, 12, g.skip_head, g.model_return_length)
        assert rms(ye[s] - yo) < PCM_TOL, (s, rms(ye[s] - yo))


def test_graph_replay_equals_eager_and_device_api():
    import torch
    z, ora, eng = _pair("tiny")
    z2, ora2, eng2 = _pair("tiny")
    eng2.set_use_graph(True)
    x = voice_signal(g.input_buffer_16k_size, seed=8)
    d_in = torch.from_numpy(x).cuda()
    d_out = torch.zeros(g.model_return_length * 48, device="cuda")
    torch.cuda.synchronize()         # (the fill runs on torch's stream, the engine on its own)
    for i in range(4):
        ya = eng.infer(x, 2560, 12 if i < 2 else -12, 200, 21)
        n = eng2.infer_device(d_in.data_ptr(), len(x), 2560, 12 if i < 2 else -12, 200, 21, d_out.data_ptr(), d_out.numel(), sync=True)
        assert n == len(ya)
        assert np.array_equal(d_out.cpu().numpy(), ya)                 # same kernels, same order -> bitwise equal
    assert eng2.last_gpu_ms() > 0
    # ... and with retrieval: the one-launch kernel re-arms its own ticket counters, so a replayed graph finds them as the capture did
    index = W.make_index(4000, 48, seed=17)
    for e in (eng, eng2):
        e.load_index(index); e.set_index_rate(0.5)
    for i in range(4):
        ya = eng.infer(x, 2560, 12, 200, 21)
        n = eng2.infer_device(d_in.data_ptr(), len(x), 2560, 12, 200, 21, d_out.data_ptr(), d_out.numel(), sync=True)
        assert n == len(ya) and np.array_equal(d_out.cpu().numpy(), ya)
        ia, da = eng.knn(); ib, db = eng2.knn()
        assert np.array_equal(ia, ib) and np.array_equal(da, db) and ia.shape == (21, 4)


def test_linearity_of_retrieval_free_feature_path_properties():
    # size-independent properties at BASELINE's full size: determinism across engines and chunk-counter dependence
    z, ora, eng = _pair("full")
    z2, ora2, eng2 = _pair("full")
    x = voice_signal(g.input_buffer_16k_size, seed=12)
    a1 = eng.infer(x, 2560, 12, 200, 21); a2 = eng.infer(x, 2560, 12, 200, 21)
    b1 = eng2.infer(x, 2560, 12, 200, 21)
    assert a1.shape == (10080,) and np.array_equal(a1, b1) and not np.array_equal(a1, a2)
    assert np.abs(a1).max() <= 1.0 and np.isfinite(a1).all()


def test_five_stage_synthesizer_with_odd_flow_count():
    # a synthesizer family the zoo does not otherwise cover: 5 upsampling stages (upstream's 32 kHz v1 layout), 3 ResBlock kernels at
    # toy width, an ODD number of flows (the folded channel flips then need one materialised flip at the end)
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny", 2, "tiny5")
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(4, 1)
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(4, 1)
    x = voice_signal(g.input_buffer_16k_size, seed=17)
    for _ in range(2):
        yo, ye = ora.infer(x, 2560, 3, 200, 21), eng.infer(x, 2560, 3, 200, 21)
        assert ye.shape == yo.shape == (21 * 64,) and rms(ye - yo) < PCM_TOL, rms(ye - yo)
    # ... and with three streams (round 5: the materialised flip of an odd flow count read and wrote with ONE batch stride; with composed WaveNets the
    # latent is a row range of a wider tensor, so every stream but the first came out wrong -- 0.19 RMS -- and no test ran this family with streams)
    eng3 = RvcInfer(z["data"]); eng3.load_contentvec(2); eng3.load_f0(); eng3.load_model(z["model"]); eng3.set_streams(3); eng3.set_noise_seed(4, 30)
    xin = np.stack([voice_signal(g.input_buffer_16k_size, seed=40 + s) for s in range(3)])
    y3 = eng3.infer_batch(xin, 2560, 3, 200, 21)
    for s in range(3):
        o = O.OracleRvcInfer(z["data"]); o.load_contentvec(2); o.load_f0(1); o.load_model(z["model"]); o.set_noise_seed(4, 30 + s)
        assert rms(y3[s] - o.infer(xin[s], 2560, 3, 200, 21)) < PCM_TOL, s
    eng3.close()


def test_plain_c_client_links_and_runs(tmp_path):
    # examples/c_smoke.c is compiled with gcc as C99 against include/rvc_mi355x.h and linked to the shared library: the boundary is a
    # C ABI, not a Python extension.  Its infer output must equal the ctypes path's (same seed, same input).
    import shutil, subprocess
    from obs_rvc_amd import _native
    from obs_rvc_amd.rvc import RvcInfer
    if not shutil.which("gcc"):
        pytest.skip("gcc not found")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "c_smoke")
    libdir = os.path.dirname(_native.SO_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "c_smoke.c"),
                           "-L", libdir, "-lrvc_mi355x", "-Wl,-rpath," + libdir, "-lm", "-o", exe])
    z = zoo("tiny")
    out = subprocess.run([exe, z["data"], z["model"]], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().splitlines()
    assert lines[-1].startswith("ok ") and "gfx950" in lines[-1]
    n, r = int(lines[0].split()[1]), float(lines[0].split("rms")[1].split(",")[0])
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(1234, 0)
    i = np.arange(35840)
    x = (np.float32(0.1) * np.sin(2.0 * 3.14159265358979 * 180.0 * i / 16000.0).astype(np.float32) + np.float32(0.05) * np.sin(2.0 * 3.14159265358979 * 360.0 * i / 16000.0).astype(np.float32)).astype(np.float32)
    y = eng.infer(x, 2560, 12, 200, 21)
    assert n == y.size == 1008 and abs(rms(y) - r) < 1e-5 * max(r, 1e-3) + 2e-6
    assert "small buffer: status 5 (expected 5), required 1008" in out.stdout
    assert "session: frame 768 samples" in out.stdout


def test_non_finite_input_is_contained():
    # NaN / Inf samples (a glitching capture device) must not fault the GPU or poison later chunks: with retrieval on, a non-finite
    # query has no nearest neighbour (hits report index -1) and the chunk's output is NaN; the next clean chunk is clean again
    z = zoo("tiny")
    from obs_rvc_amd.rvc import RvcInfer
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    eng.load_index(W.make_index(2000, 48, seed=1)); eng.set_index_rate(0.5)
    x = voice_signal(g.input_buffer_16k_size, seed=1)
    for bad in (np.where(np.arange(x.size) % 1000 == 0, np.nan, x), np.where(np.arange(x.size) % 777 == 0, np.inf, x)):
        y = eng.infer(bad.astype(np.float32), 2560, 12, 200, 21)
        assert y.shape == (1008,) and not np.isfinite(y).all()
        idx, dist = eng.knn()
        assert (idx == -1).all()
    y = eng.infer((x * 1e30).astype(np.float32), 2560, 12, 200, 21)
    assert y.shape == (1008,)
    y = eng.infer(x, 2560, 12, 200, 21)
    assert np.isfinite(y).all() and (eng.knn()[0] >= 0).all()


def test_edge_case_sweep_leaves_the_engine_usable():
    # sizes at and past the edges (see tests/tools/fuzz_probe.py, which runs each case in its own process to catch GPU faults):
    # every call either returns a finite result of the expected size or raises the mapped error, and the engine keeps working
    z = zoo("tiny")
    from obs_rvc_amd.rvc import RvcInfer
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"])
    x = voice_signal(g.input_buffer_16k_size, seed=1)
    ok = [(lambda: eng.infer(x[:5120], 2560, 12, 0, 1), (48,)), (lambda: eng.infer(x[:35001], 2560, 12, 200, 17), (816,)),
          (lambda: eng.infer(x, 2560, 12, 0, 223), (10704,)), (lambda: eng.infer(x, 0, 12, 200, 21), (1008,)),
          (lambda: eng.infer(x, 2560, 1200, 200, 21), (1008,)), (lambda: eng.infer(x, 2560, -1200, 200, 21), (1008,)),
          (lambda: eng.pitch(x, 12, 30000), (224,)), (lambda: eng.hubert(x[:400]), (1, 48, 1))]
    for fn, shape in ok:
        y = fn()
        assert y.shape == shape and np.isfinite(y).all()
    bad = [(lambda: eng.infer(x[:400], 2560, 12, 0, 1), "Panic"), (lambda: eng.infer(x, 2560, 12, 200, 100), "Panic"),
           (lambda: eng.infer(x, 2560, 12, 200, 0), "NdarrayShapeError"), (lambda: eng.infer(x, 10 ** 6, 12, 200, 21), "Panic"),
           (lambda: eng.load_index(W.make_index(3, 48, seed=1)), "NdarrayShapeError"), (lambda: eng.set_streams(0), "NdarrayShapeError"),
           (lambda: eng.infer(np.concatenate([x] * 6), 2560, 12, 200, 21), "Panic")]
    for fn, kind in bad:
        with pytest.raises(RvcInferError) as ei:
            fn()
        assert ei.value.kind == kind
        assert np.isfinite(eng.infer(x, 2560, 12, 200, 21)).all()
    eng.set_streams(300)                                   # far more streams than CUs' worth of workgroups in the small kernels
    yb = eng.infer_batch(np.stack([x] * 300), 2560, 12, 200, 21)
    assert yb.shape == (300, 1008) and np.isfinite(yb).all()


def test_plugin_maximum_settings():
    # the plugin's sliders at their upper ends (obs-rvc/src/lib.rs:396-413): 1.5 s chunks, 0.15 s crossfade, 5 s of extra context at a
    # 48 kHz host -> a 6.66 s window (L = 106 560, ContentVec T = 332: the attention falls back to the one-buffer LDS kernel),
    # R = 155 frames (text-encoder attention past the small-T kernel), Tm = 160 mel frames
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    gg = derive(48000, 1.5, 0.15, 5.0, 48000)
    assert (gg.input_buffer_16k_size, gg.sample_frame_16k, gg.model_return_length, gg.skip_head) == (106560, 24000, 155, 500)
    # full-size ContentVec on the long window
    z = zoo("full")
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(8, 0)
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(8, 0)
    x = voice_signal(gg.input_buffer_16k_size, seed=23)
    ho, he = ora.hubert(x), eng.hubert(x)
    assert he.shape == ho.shape == (1, 768, 332) and rel_rms(he, ho) < 1e-4
    # the whole chunk at full size (zoo revision 2: the RMVPE head's edge bins are switched off, so the 160 frames decode inside the table).
    # 160 frames of the synthetic head's flat salience hold near-ties: the arg-max of one frame can resolve differently under two fp32
    # summation orders ("discrete decisions": measured here, frame 97, 183.4 vs 181.3 Hz with the saliences equal to
    # 4e-7).  So: every arithmetic stage must agree, the decisions are compared as decisions, and the audio is compared when they agree.
    ora.enable_taps(True); eng.enable_taps(2)
    yo = ora.infer(x, gg.sample_frame_16k, 7, gg.skip_head, gg.model_return_length)
    ye = eng.infer(x, gg.sample_frame_16k, 7, gg.skip_head, gg.model_return_length)
    assert ye.shape == yo.shape == (155 * 480,) and np.isfinite(ye).all()
    assert rel_rms(eng.tap("rm.sal_ct").reshape(-1, 160).T.reshape(-1), ora.tap("rm.sal")) < 1e-5
    assert rel_rms(eng.tap("cv.out"), ora.tap("cv.out")) < 1e-4
    fo, fe = ora.tap("f0"), eng.tap("f0")
    flips = np.abs(fe - fo) > 1e-3 * np.abs(fo) + 1e-3
    assert flips.sum() <= 2 and np.all(np.abs(fe - fo)[flips] <= 0.03 * np.abs(fo)[flips] + 1e-3), (int(flips.sum()), fo[flips], fe[flips])      # at most two frames, one or two 20-cent bins
    if not flips.any():
        assert rms(ye - yo) < PCM_TOL, rms(ye - yo)
    ora.enable_taps(False); eng.enable_taps(False)
    # the whole chunk at these sizes on the small model (same code paths, well-behaved salience)
    z = zoo("tiny")
    ora = O.OracleRvcInfer(z["data"]); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(8, 0)
    eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(8, 0)
    for _ in range(2):
        yo = ora.infer(x, gg.sample_frame_16k, 7, gg.skip_head, gg.model_return_length)
        ye = eng.infer(x, gg.sample_frame_16k, 7, gg.skip_head, gg.model_return_length)
        assert ye.shape == yo.shape == (155 * 48,) and rms(ye - yo) < PCM_TOL, rms(ye - yo)
    assert np.allclose(eng.pitch_cache(), ora.pitch_cache(), rtol=1e-5, atol=1e-3)


def test_salience_peak_at_the_table_edge_panics_like_the_reference(tmp_path):
    # rmvpe.rs:124: a frame whose arg-max bin is >= 348 makes the reference index out of bounds (it slices the UNPADDED salience with a
    # centre found on the padded one) and panic.  A model whose head puts its bump at bin 354 must produce exactly that on both sides
    # (the zoo's own heads keep away from the edge: trained heads do, and the bench's plugin chain should not count panic chunks).
    import shutil
    from oracle import oracle as O
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("tiny")
    data = str(tmp_path / "data")
    shutil.copytree(z["data"], data)
    cfg, t = W.read_blob(os.path.join(data, "f0", "rmvpe.rvcw"))
    bins = np.arange(t["rm.fc.b"].shape[0], dtype=np.float64)
    t["rm.fc.b"] = (12.0 * np.exp(-0.5 * ((bins - 354.0) / 3.0) ** 2) - 6.0).astype(np.float32)
    W.write_blob(os.path.join(data, "f0", "rmvpe.rvcw"), cfg, t)
    ora = O.OracleRvcInfer(data); ora.load_contentvec(2); ora.load_f0(1); ora.load_model(z["model"]); ora.set_noise_seed(8, 0)
    eng = RvcInfer(data); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(8, 0)
    x = voice_signal(g.input_buffer_16k_size, seed=23)
    with pytest.raises(Exception) as eo:
        ora.infer(x, g.sample_frame_16k, 7, g.skip_head, g.model_return_length)
    with pytest.raises(RvcInferError) as ee:
        eng.infer(x, g.sample_frame_16k, 7, g.skip_head, g.model_return_length)
    assert "Panic" in str(eo.value) and ee.value.kind == "Panic"
    # the engine is usable afterwards (the status word was cleared): a well-behaved model on the same engine object's sibling
    ok = RvcInfer(z["data"]); ok.load_contentvec(2); ok.load_f0(); ok.load_model(z["model"]); ok.set_noise_seed(8, 0)
    assert np.isfinite(ok.infer(x, g.sample_frame_16k, 7, g.skip_head, g.model_return_length)).all()


def test_pipelined_chunks_equal_serial_chunks():
    # offline throughput mode: unsynchronised infer_device calls overlap chunk i+1's front branches with chunk i's synthesizer
    # (two plan slots); per-stream state (pitch cache, noise counters) must evolve exactly as in the serial order
    import torch
    from obs_rvc_amd.rvc import RvcInfer
    z = zoo("full")
    L, chunk, N = g.input_buffer_16k_size, g.sample_frame_16k, g.model_return_size
    audio = voice_signal(chunk * 24, seed=31)
    rings = torch.from_numpy(np.stack(list(chunk_stream(audio, L, chunk))[-8:])).cuda()

    def run(pipelined):
        eng = RvcInfer(z["data"]); eng.load_contentvec(2); eng.load_f0(); eng.load_model(z["model"]); eng.set_noise_seed(11, 0)
        eng.set_pipeline(pipelined)
        outs = torch.zeros((8, N), device="cuda")
        torch.cuda.synchronize()     # (the fill runs on torch's stream, the engine on its own)
        for i in range(8):
            eng.infer_device(rings[i].data_ptr(), L, chunk, 12, g.skip_head, g.model_return_length, outs[i].data_ptr(), N, sync=not pipelined)
        eng.synchronize()
        return outs.cpu().numpy(), eng.pitch_cache()
    ys, cs = run(False)
    yp, cp = run(True)
    assert np.isfinite(ys).all() and np.array_equal(ys, yp) and np.array_equal(cs, cp)


