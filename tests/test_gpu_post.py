"""The chain every output sample leaves through -- RMS envelope mixing, the SOLA search and blend, the two converters, the session's rings -- kernel by kernel
against the float64 definitions of tests/post_ref.py (DESIGN.md "Post-processing and resamplers: what is tested"): through the public one-stream calls and
through rvc_debug_post with 1 and 3 streams, padded strides and different data per stream.

Tolerance (the rule of tests/test_gpu_crossfade.py): delta32 = what the reference's own fp32 evaluation of a case deviates from its fp64 evaluation; the kernel
gets 2 * delta32; the case asserts delta32 <= 1e-4 * peak (tests/test_post_ref.py asserts the same without a GPU).  A case is one launch: delta32 is taken
over all of its streams.  For the converters delta32 includes tap32 (post_ref.resample_bound).  Copies, offsets, untouched samples and padding are exact."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import debug_abi as D
import post_ref as R
from common import zoo
from obs_rvc_amd.rvc_common import RvcInferError
from oracle import resample_oracle as RO

pytestmark = pytest.mark.gpu
PAD = np.float32(-7.5)            # the padding of every buffer: finite, recognisable, and it must come back bit for bit
WORST = {}


@pytest.fixture(scope="module")
def eng():
    from obs_rvc_amd.rvc import RvcInfer
    D.lib()
    return RvcInfer(zoo("tiny")["data"])


def padded(rows, bs):
    a = np.full((len(rows), bs), PAD, np.float32)
    for s, r in enumerate(rows):
        a[s, :len(r)] = r
    return a


def pad_intact(a, n):
    return (a[:, n:].view(np.uint32) == PAD.view(np.uint32)).all()


def post(eng, bufs, mix_power=None, offsets=None, **kw):
    """rvc_debug_post -> status"""
    spec = D.PostSpec(**kw)
    arr = (C.c_void_p * 4)(*[None if b is None else b.ctypes.data for b in list(bufs) + [None] * (4 - len(bufs))])
    return D.lib().rvc_debug_post(eng._h, C.byref(spec), arr, D.ptr(mix_power), D.ptr(offsets))


def within(family, tag, got, ref, d32, peak):
    err = float(np.abs(np.asarray(got, np.float64) - ref).max()) if np.size(ref) else 0.0
    ratio = err / d32 if d32 > 0 else (0.0 if err == 0 else np.inf)
    WORST[family] = max(WORST.get(family, 0.0), ratio)
    print("%s %s delta32=%.3e kernel=%.3e (%.2f x delta32) peak=%.3e" % (family, tag, d32, err, ratio, peak))
    assert d32 <= 1e-4 * peak or peak == 0, (family, tag, d32, peak)      # an ill-conditioned input must not widen its own tolerance
    assert np.isfinite(got).all() and err <= 2.0 * d32, (family, tag, err, d32)


# ------------------------------------------------------------------------------------------------------------------------------
# envelope mixing
# ------------------------------------------------------------------------------------------------------------------------------
ENV_KINDS = ("plain", "silent_out", "quiet_out", "silent_in", "loud_quiet")


@pytest.mark.parametrize("zc,n", [(zc, n) for zc in R.ENV_ZC for n in R.env_lengths(zc)])
def test_envelope_public_call(eng, zc, n):
    if True:
        for kind in ENV_KINDS:
            xs, ys = R.env_case(zc, n, kind)
            for rate in (0.0, 0.5, 1.0):
                ex = float(np.float32(1.0 - rate))
                m64, _, _, d32, _, peak = R.env_bound(xs[0], ys[0], zc, ex)
                got = eng.envelop_mixing(xs[0], ys[0], 100 * zc, rate)
                within("mix", "public zc=%d n=%d %s rate=%.1f" % (zc, n, kind, rate), got, m64, d32, peak)
                if rate == 1.0:
                    assert D.same_bits(got, ys[0])


@pytest.mark.parametrize("zc,n", [(zc, n) for zc in R.ENV_ZC for n in R.env_lengths(zc)])
@pytest.mark.parametrize("S", [1, 3])
def test_envelope_hook(eng, zc, n, S):
    exps = np.array([0.0, 0.3, 1.0] if S == 3 else [0.3], np.float32)
    if True:
        nf = (n + 2 * (2 * zc) - 4 * zc) // zc + 1
        for kind in ENV_KINDS:
            xs, ys = R.env_case(zc, n, kind, S)
            bx, by, br = padded(xs, n + 5), padded(ys, n + 7), np.full((S, 2 * nf + 3), PAD, np.float32)
            bx0 = bx.copy()
            assert post(eng, [bx, by, br], exps, op=0, streams=S, n=n, frame=4 * zc, hop=zc, in_bs=n + 5, out_bs=n + 7, r_bs=2 * nf + 3) == 0, eng._L.rvc_last_error_message(eng._h)
            b = [R.env_bound(xs[s], ys[s], zc, float(exps[s])) for s in range(S)]
            tag = "hook zc=%d n=%d S=%d %s" % (zc, n, S, kind)
            assert len(b[0][1]) == nf
            within("rms", tag, br[:, :2 * nf], np.stack([np.concatenate([v[1], v[2]]) for v in b]), max(v[4] for v in b), max(max(v[1].max(), v[2].max()) for v in b))
            within("mix", tag, by[:, :n], np.stack([v[0] for v in b]), max(v[3] for v in b), max(v[5] for v in b))
            assert D.same_bits(bx, bx0) and pad_intact(by, n) and pad_intact(br, 2 * nf)
            for s in range(S):
                if exps[s] == 0:
                    assert D.same_bits(by[s, :n], ys[s]), (tag, s)          # exponent 0 beside non-zero exponents: untouched
            if kind == "silent_in":
                assert all((by[s, :n] == 0).all() for s in range(S) if exps[s] != 0)


# ------------------------------------------------------------------------------------------------------------------------------
# SOLA
# ------------------------------------------------------------------------------------------------------------------------------
def check_sola(tag, b, n, frame, output, off, out, fr, tail):
    """one stream's results against the definition b (post_ref.sola_bound): exact wherever the kernel copies"""
    assert off == b["off"], (tag, off, b["off"])
    assert D.same_bits(out[:off], output[:off]) and D.same_bits(out[off + n:], output[off + n:]), tag        # output outside the seam
    assert D.same_bits(fr, out[off:off + frame]) and D.same_bits(tail, out[off + frame:off + frame + n]), tag       # frame and tail are copies of the blended output
    assert D.same_bits(fr[n:], output[off + n:off + frame]), tag
    return out[off:off + n]


@pytest.mark.parametrize("n,search,frame", R.SOLA_CASES)
def test_sola_public_call(eng, n, search, frame):
    output, sola, lead = R.sola_case(n, search, frame)
    b = R.sola_bound(output, sola, search, frame)
    off, fr, tail, out = eng.sola_step_full(output, sola, search, frame)
    tag = "public n=%d search=%d frame=%d" % (n, search, frame)
    seam = check_sola(tag, b, n, frame, output, off, out, fr, tail)
    within("sola_blend", tag, seam, b["out"][off:off + n], b["d_seam"], b["p_seam"])
    within("sola_blend", tag + " tail", tail, b["tail"], b["d_seam"], b["p_seam"])          # frame < sola_len: the tail overlaps the blended seam


def run_sola_hook(eng, outputs, solas, search, frame, graph=0):
    S, n, total = len(outputs), len(solas[0]), len(outputs[0])
    bo, bs, bf, bc = padded(outputs, total + 5), padded(solas, n + 3), np.full((S, frame + 2), PAD, np.float32), np.full((S, search + 1 + 4), PAD, np.float32)
    offs = np.full(S, -1, np.int32)
    rc = post(eng, [bo, bs, bf, bc], None, offs, op=1, streams=S, graph=graph, sola_len=n, search=search, frame=frame, out_bs=total + 5, sola_bs=n + 3, frame_bs=frame + 2,
              cor_bs=search + 5)
    assert rc == 0, eng._L.rvc_last_error_message(eng._h)
    assert pad_intact(bo, total) and pad_intact(bs, n) and pad_intact(bf, frame) and pad_intact(bc, search + 1)
    return offs, bo[:, :total], bs[:, :n], bf[:, :frame], bc[:, :search + 1]


@pytest.mark.parametrize("n,search,frame", R.SOLA_CASES)
@pytest.mark.parametrize("S", [1, 3])
def test_sola_hook(eng, n, search, frame, S):
    cases = [R.sola_case(n, search, frame, s) for s in range(S)]
    bounds = [R.sola_bound(c[0], c[1], search, frame) for c in cases]
    offs, out, tail, fr, cor = run_sola_hook(eng, [c[0] for c in cases], [c[1] for c in cases], search, frame)
    tag = "hook n=%d search=%d frame=%d S=%d" % (n, search, frame, S)
    within("sola_cor", tag, cor, np.stack([b["cor"] for b in bounds]), max(b["d_cor"] for b in bounds), max(b["p_cor"] for b in bounds))
    seams = [check_sola(tag, bounds[s], n, frame, cases[s][0], int(offs[s]), out[s], fr[s], tail[s]) for s in range(S)]
    assert len({int(o) for o in offs}) == len({c[2] for c in cases})                               # (the streams' offsets differ wherever the search has room)
    d, p = max(b["d_seam"] for b in bounds), max(b["p_seam"] for b in bounds)
    within("sola_blend", tag, np.stack(seams), np.stack([b["out"][b["off"]:b["off"] + n] for b in bounds]), d, p)
    within("sola_blend", tag + " tail", tail, np.stack([b["tail"] for b in bounds]), d, p)
    # the one-stream public call computes the same bits as the batched launch
    off1, fr1, tail1, out1 = eng.sola_step_full(cases[0][0], cases[0][1], search, frame)
    assert off1 == offs[0] and D.same_bits(out1, out[0]) and D.same_bits(fr1, fr[0]) and D.same_bits(tail1, tail[0])


def test_sola_ties_and_the_zero_window(eng):
    # exact ties: an output of period 16 puts the same floats at lags 5, 21, 37 -> the same correlation bits, and the LAST of them wins
    output, sola, search, frame, tied = R.sola_periodic()
    assert eng.sola_step_full(output, sola, search, frame)[0] == tied[-1]
    zeros = np.zeros_like(output)
    offs, out, tail, fr, cor = run_sola_hook(eng, [output, zeros, output], [sola, np.zeros_like(sola), sola], search, frame)
    assert list(offs) == [tied[-1], search, tied[-1]]                                        # all zeros: every lag ties, the last lag wins
    assert len({cor[0, t].tobytes() for t in tied}) == 1 and (cor[0] <= cor[0, tied[0]]).all() and (cor[1] == 0).all()
    assert (out[1] == 0).all() and (tail[1] == 0).all() and (fr[1] == 0).all()
    assert eng.sola_step_full(zeros, np.zeros_like(sola), search, frame)[0] == search
    # the den + 1e-8 guard: all-zero windows at the first lags give 0 (not NaN), the maximum sits behind them
    output, sola, search, frame, dead = R.sola_zero_window()
    b = R.sola_bound(output, sola, search, frame)
    offs, out, tail, fr, cor = run_sola_hook(eng, [output], [sola], search, frame)
    assert (cor[0, :dead] == 0).all() and offs[0] == b["off"] == dead + 5
    within("sola_cor", "zero-window", cor[0], b["cor"], b["d_cor"], b["p_cor"])
    assert eng.sola_step_full(output, sola, search, frame)[0] == dead + 5


def test_sola_errors_leave_the_engine_working(eng):
    n, search, frame = 64, 1023, 64
    output, sola, lead = R.sola_case(n, search, frame)
    long_out = np.concatenate([output, np.zeros(8, np.float32)])
    with pytest.raises(RvcInferError) as ei:
        eng.sola_step_full(long_out, sola, 1024, frame)                                       # one lag more than post_sola_kernel's cor[1024] holds
    assert ei.value.code == D.RVC_SHAPE
    assert eng.sola_step_full(output, sola, search, frame)[0] == lead
    with pytest.raises(RvcInferError) as ei:
        eng.sola_step_full(output[:-1], sola, search, frame)                                  # one sample short: the reference slices out of range
    assert ei.value.code == 6
    assert eng.sola_step_full(output, sola, search, frame)[0] == lead
    # the hook: the same limits, and every stride at least its row
    good = dict(op=1, streams=1, sola_len=n, search=search, frame=frame, out_bs=len(output), sola_bs=n, frame_bs=frame, cor_bs=search + 1)
    bufs = lambda: [output.copy()[None], sola.copy()[None], np.zeros((1, frame), np.float32), np.zeros((1, search + 1), np.float32)]
    offs = np.zeros(1, np.int32)
    for bad in (dict(search=1024, cor_bs=1025, out_bs=len(output) + 1), dict(out_bs=len(output) - 1), dict(sola_bs=n - 1), dict(frame_bs=frame - 1), dict(cor_bs=search),
                dict(sola_len=0), dict(streams=0), dict(op=5)):
        assert post(eng, bufs(), None, offs, **{**good, **bad}) == D.RVC_SHAPE, bad
    bb = bufs()
    assert post(eng, bb, None, offs, **good) == 0 and offs[0] == lead
    z = np.zeros((1, 64), np.float32)
    for bad in (dict(op=0, streams=1, n=10, frame=4, hop=1, in_bs=9, out_bs=10, r_bs=22), dict(op=0, streams=1, n=10, frame=4, hop=1, in_bs=10, out_bs=10, r_bs=21),
                dict(op=3, streams=1, n=10, f=3, skip=2, copy_begin=5, x_bs=6), dict(op=3, streams=1, n=10, f=3, skip=0, copy_begin=8, x_bs=10),
                dict(op=2, streams=1, n=10, f=11), dict(op=4, streams=1, rate_in=300, rate_out=100, chunk=30, chunks=1, x_bs=29, out_bs=10),
                dict(op=4, streams=1, rate_in=300, rate_out=100, chunk=30, chunks=1, x_bs=30, out_bs=9)):
        assert post(eng, [z.copy(), z.copy(), z.copy()], np.zeros(1, np.float32), offs, **bad) == D.RVC_SHAPE, bad
    assert eng.sola_step_full(output, sola, search, frame)[0] == lead


# ------------------------------------------------------------------------------------------------------------------------------
# converters
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ri,ro,ch", R.RESAMPLE_CASES + R.RESAMPLE_MINIMAL)
def test_converter_public_calls(eng, ri, ro, ch):
    from obs_rvc_amd.resample import FftFixedInOut
    gpu = FftFixedInOut(eng, ri, ro, ch)
    fi, fo = RO.fft_sizes(ri, ro, ch)
    assert (gpu.input_frames_next(), gpu.output_frames_max()) == (fi, fo)
    x = R.resample_signal(fi, 4)
    r64, bound, peak = R.resample_bound(x, ri, ro, ch, 4, 1)
    got = [gpu.process(x[c * fi:(c + 1) * fi]) for c in range(4)]          # the overlap ping-pong over more than two chunks
    gpu.reset()
    got.append(gpu.process(x[:fi]))
    within("converter", "public %d->%d chunk %d" % (ri, ro, ch), np.stack(got), r64, bound, peak)
    assert D.same_bits(got[4], got[0])                                        # after the reset: the first chunk's bits again


def run_converter_hook(eng, ri, ro, ch, S, chunks, graph=0):
    fi, fo = RO.fft_sizes(ri, ro, ch)
    xs = [R.resample_signal(fi, chunks, seed=5 + s) * np.float32(1 + 0.5 * s) for s in range(S)]
    bx = np.full((chunks, S, fi + 5), PAD, np.float32)
    for s in range(S):
        bx[:, s, :fi] = xs[s].reshape(chunks, fi)
    by = np.full((chunks, S, fo + 3), PAD, np.float32)
    bx0 = bx.copy()
    rc = post(eng, [bx, by], op=4, streams=S, graph=graph, rate_in=ri, rate_out=ro, chunk=ch, chunks=chunks, x_bs=fi + 5, out_bs=fo + 3)
    assert rc == 0, eng._L.rvc_last_error_message(eng._h)
    assert D.same_bits(bx, bx0) and (by[:, :, fo:].view(np.uint32) == PAD.view(np.uint32)).all()
    return xs, by[:, :, :fo]


@pytest.mark.parametrize("ri,ro,ch", R.RESAMPLE_CASES + R.RESAMPLE_MINIMAL)
def test_converter_hook_three_streams(eng, ri, ro, ch):
    xs, got = run_converter_hook(eng, ri, ro, ch, 3, 3)
    b = [R.resample_bound(x, ri, ro, ch, 3) for x in xs]
    within("converter", "hook %d->%d chunk %d S=3" % (ri, ro, ch), got.transpose(1, 0, 2), np.stack([v[0] for v in b]), max(v[1] for v in b), max(v[2] for v in b))


# ------------------------------------------------------------------------------------------------------------------------------
# rings
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,f", [(2, 1), (257, 256), (1000, 1), (1000, 300)])
def test_rings(eng, n, f):
    S = 3
    rng = np.random.default_rng(n + f)
    ring, chunk = rng.standard_normal((S, n)).astype(np.float32), rng.standard_normal((S, f)).astype(np.float32)
    out = np.full((S, n), PAD, np.float32)
    r0, c0 = ring.copy(), chunk.copy()
    assert post(eng, [ring, out, chunk], op=2, streams=S, n=n, f=f) == 0
    assert D.same_bits(ring, r0) and D.same_bits(chunk, c0)
    assert all(D.same_bits(out[s], R.ring_shift_append(r0[s], c0[s])) for s in range(S))
    for skip in (0, 5):
        cb = n - f - skip
        if cb < 0:
            continue
        bs = skip + f + skip + 4                                            # the row the kernel reads is res[skip .. skip + n - copy_begin)
        res = np.full((S, bs), PAD, np.float32)
        res[:, :skip + n - cb] = rng.standard_normal((S, skip + n - cb)).astype(np.float32)
        out = np.full((S, n), PAD, np.float32)
        res0 = res.copy()
        assert post(eng, [ring, out, res], op=3, streams=S, n=n, f=f, skip=skip, copy_begin=cb, x_bs=bs) == 0, eng._L.rvc_last_error_message(eng._h)
        assert D.same_bits(ring, r0) and D.same_bits(res, res0)
        assert all(D.same_bits(out[s], R.ring16_update(r0[s], res0[s], f, skip, cb)) for s in range(S)), (n, f, skip)


# ------------------------------------------------------------------------------------------------------------------------------
# graph replay
# ------------------------------------------------------------------------------------------------------------------------------
def test_graph_replay_gives_the_eager_bits(eng):
    zc, n, S = 7, 38, 3
    nf = n // zc + 1
    xs, ys = R.env_case(zc, n, "plain", S)
    exps = np.array([0.0, 0.3, 1.0], np.float32)
    res = []
    for graph in (0, 1):
        bx, by, br = padded(xs, n + 5), padded(ys, n + 7), np.full((S, 2 * nf + 3), PAD, np.float32)
        assert post(eng, [bx, by, br], exps, op=0, streams=S, graph=graph, n=n, frame=4 * zc, hop=zc, in_bs=n + 5, out_bs=n + 7, r_bs=2 * nf + 3) == 0
        res.append((by, br))
    assert D.same_bits(res[0][0], res[1][0]) and D.same_bits(res[0][1], res[1][1]) and not D.same_bits(res[0][0][1, :n], ys[1])
    n, search, frame = 200, 481, 77
    cases = [R.sola_case(n, search, frame, s) for s in range(S)]
    a = run_sola_hook(eng, [c[0] for c in cases], [c[1] for c in cases], search, frame, 0)
    b = run_sola_hook(eng, [c[0] for c in cases], [c[1] for c in cases], search, frame, 1)
    assert all(D.same_bits(np.ascontiguousarray(u), np.ascontiguousarray(v)) for u, v in zip(a[1:], b[1:])) and list(a[0]) == list(b[0])
    for ri, ro, ch in ((700, 300, 21), (100, 100, 200)):
        ya, yb = run_converter_hook(eng, ri, ro, ch, S, 3, 0)[1], run_converter_hook(eng, ri, ro, ch, S, 3, 1)[1]
        assert D.same_bits(np.ascontiguousarray(ya), np.ascontiguousarray(yb)) and np.abs(ya).max() > 0.01


def test_report_the_largest_ratios():
    # (runs last in the file: the largest kernel / delta32 seen per family, the figures DESIGN.md quotes)
    print("largest kernel / delta32 per family:", {k: round(v, 3) for k, v in sorted(WORST.items())})
    assert set(WORST) == {"converter", "mix", "rms", "sola_blend", "sola_cor"}          # (each case asserts its own bound)
