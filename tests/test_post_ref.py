"""tests/post_ref.py -- the float64 reference of the post-processing chain and the converters -- pinned on what the project already holds (the reference's golden
vectors and known answers, the C oracle, the fp32 restatement of the converters), and the conditions on the inputs of tests/test_gpu_post.py: delta32 <= 1e-4
peak, the lead of the best SOLA lag, the margin from the 1e-3 floor, the converter geometry each case reaches.  No GPU."""
import os
import re

import numpy as np
import pytest

import post_ref as R
from common import GOLDEN, voice_signal
from oracle import oracle as O
from oracle import resample_oracle as RO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _g(name):
    return np.load(os.path.join(GOLDEN, "ref_post_%s.npy" % name))


# ------------------------------------------------------------------------------------------------------------------------------
# the reference against what is already pinned
# ------------------------------------------------------------------------------------------------------------------------------
def test_rms_and_lerp_known_answers():
    # rt_utils.rs:139-159 (the values tests/test_postprocess.py holds the C oracle to)
    want = np.array([1.118034, 2.738613, 4.6368093, 6.595453, 8.573215, 6.726812])
    for dt in (np.float64, np.float32):
        assert np.abs(R.rms(np.arange(1, 11), 4, 2, dt) - want).max() < 1e-6
    inp = np.array([0.2353, 0.9068, 0.7870, 0.5878, 0.0097, 0.7160, 0.5812, 0.8901, 0.8822, 0.8547], np.float32)
    exp15 = [0.2353, 0.66697854, 0.8725714, 0.79555714, 0.6731714, 0.4639215, 0.09228568, 0.36285, 0.6967429, 0.6100857,
             0.7135856, 0.8895357, 0.8844571, 0.8723786, 0.8547]
    for dt in (np.float64, np.float32):
        assert np.abs(R.lerp_align_corners(inp, 3, dt) - [0.2353, 0.36285, 0.8547]).max() < 1e-6
        assert np.abs(R.lerp_align_corners(inp, 15, dt) - exp15).max() < 1e-6
    # n_in = 2 (the shortest track) and the last index, where ceil reaches n_in - 1 (or, rounded up, n_in: clamped)
    assert np.abs(R.lerp_align_corners([1.0, 3.0], 5) - [1.0, 1.5, 2.0, 2.5, 3.0]).max() < 1e-15
    for dt in (np.float64, np.float32):
        for n_in, size in ((2, 8), (7, 30), (44, 2601)):
            v = np.arange(n_in) * 0.25 + 1
            assert abs(float(R.lerp_align_corners(v, size, dt)[-1]) - v[-1]) < 1e-5
    # against the C oracle on a test input
    y = voice_signal(1000, seed=3)
    assert np.abs(R.rms(y, 64, 16) - O.rms(y, 64, 16)).max() < 1e-6
    assert np.abs(R.lerp_align_corners(O.rms(y, 64, 16), 1001) - O.lerp_align_corners(O.rms(y, 64, 16), 1001)).max() < 1e-6


def test_golden_vectors():
    # obs-rvc/src/tests/envelop_mixing.rs:9-36 (zc = 480, mix rate 0.8, the reference's own eps 1e-6), sola.rs:11-16
    iw, ow = _g("envelop_input_wav"), _g("envelop_infer_wav")
    n = len(ow)
    mixed, r1, r2 = R.envelop_mix(iw, ow, 480, 1.0 - 0.8)
    assert np.abs(R.lerp_align_corners(r1, n + 1)[:n] - _g("envelop_rms1")).max() < 1e-6
    assert np.abs(np.maximum(R.lerp_align_corners(r2, n + 1), R.FLOOR)[:n] - _g("envelop_rms2")).max() < 1e-6
    assert np.abs(mixed - _g("envelop_infer_wav2")).max() < 1e-6
    cor, off = R.sola_cor(_g("infer_wav"), _g("sola_buffer"), 480)
    assert off == 321 and len(cor) == 481
    assert R.sola_cor(_g("infer_wav"), _g("sola_buffer"), 480, np.float32)[1] == 321


def test_sola_step_agrees_with_the_oracle():
    for n, search, frame in R.SOLA_CASES:
        out, sola, lead = R.sola_case(n, search, frame)
        off, o, fr, tail = R.sola_step(out, sola, search, frame)
        o_off, o_fr, o_tail = O.sola_step(out, sola, search, frame)
        assert off == o_off == lead, (n, search, frame, off, o_off, lead)
        assert np.abs(fr - o_fr).max() < 1e-6 and np.abs(tail - o_tail).max() < 1e-6
        # everything outside the seam is a copy
        assert (o[:off] == out[:off]).all() and (o[off + n:] == out[off + n:]).all()
        assert (fr == o[off:off + frame]).all() and (tail == o[off + frame:off + frame + n]).all()
    z = np.zeros(100, np.float32)
    assert R.sola_cor(z, z[:20], 30)[1] == O.sola_step(z, z[:20], 30, 50)[0] == 30           # all ties: the last lag
    assert np.array_equal(R.fade_in(1), [0.0]) and R.fade_in(5)[0] == 0 and abs(R.fade_in(5)[-1] - 1) < 1e-15


@pytest.mark.parametrize("ri,ro,ch", R.RESAMPLE_CASES + R.RESAMPLE_MINIMAL + [(48000, 16000, 8640)])
def test_converter_agrees_with_the_fp32_restatement(ri, ro, ch):
    fi, fo = RO.fft_sizes(ri, ro, ch)
    x = R.resample_signal(fi, 3)
    a, b = R.Resampler(ri, ro, ch), RO.FftFixedInOut(ri, ro, ch)
    assert (a.fft_in, a.fft_out) == (b.input_frames_next(), b.output_frames_max()) == (fi, fo)
    for c in range(3):
        assert np.abs(a.process(x[c * fi:(c + 1) * fi]) - b.process(x[c * fi:(c + 1) * fi])).max() < 2e-6
    a.reset(); b.reset()
    assert np.abs(a.process(x[:fi]) - b.process(x[:fi])).max() < 2e-6
    a.reset()
    assert (a.process(np.zeros(fi)) == 0).all()                                              # nothing left after a reset
    assert np.abs(R.taps64(fi, fo) - R.taps32(fi, fo)).max() < 1e-6 * np.abs(R.taps32(fi, fo)).max() + 1e-9


def test_converter_chunk_against_the_brute_force_sums():
    for ri, ro, ch in ((300, 100, 30), (100, 300, 10), (700, 300, 7), (100, 100, 33)):
        fi, fo = RO.fft_sizes(ri, ro, ch)
        x, h = R.resample_signal(fi, 2)[fi:], R.taps32(fi, fo)
        y = R.resample_chunk(x, h, fi, fo)
        assert y.shape == (2 * fo,) and np.abs(y - R.resample_chunk_brute(x, h, fi, fo)).max() < 1e-13


def test_rings():
    ring, chunk = np.arange(10.0), np.arange(100.0, 103.0)
    assert np.array_equal(R.ring_shift_append(ring, chunk), [3, 4, 5, 6, 7, 8, 9, 100, 101, 102])
    res = np.arange(200.0, 210.0)
    # lib.rs:669-679 with f = 3, skip = 2: the converter's output re-writes the 2 samples before the new chunk as well
    assert np.array_equal(R.ring16_update(ring, res, 3, 2, 10 - 3 - 2), [3, 4, 5, 6, 7, 202, 203, 204, 205, 206])
    assert np.array_equal(R.ring16_update(ring, res, 3, 0, 7), [3, 4, 5, 6, 7, 8, 9, 200, 201, 202])


# ------------------------------------------------------------------------------------------------------------------------------
# the conditions on the inputs of tests/test_gpu_post.py
# ------------------------------------------------------------------------------------------------------------------------------
ENV_KINDS = ("plain", "silent_out", "quiet_out", "silent_in", "loud_quiet")


def test_envelope_inputs_are_well_conditioned():
    for zc in R.ENV_ZC:
        for n in R.env_lengths(zc):
            for kind in ENV_KINDS:
                xs, ys = R.env_case(zc, n, kind, 3)
                for s, e in enumerate((0.0, 0.3, 1.0)):
                    for ex in {e, 0.5, 1.0}:
                        m64, r1, r2, d32, dtr, peak = R.env_bound(xs[s], ys[s], zc, ex)
                        assert d32 <= 1e-4 * peak, (zc, n, kind, s, ex, d32, peak)
                        assert dtr <= 1e-4 * max(r1.max(), r2.max()) or r1.max() == r2.max() == 0
                        # max(r, 1e-3) has a kink: the fp32 and fp64 evaluations must be on the same side of it, with room
                        assert R.floor_margin(ys[s], zc) > 10 * max(d32, dtr), (zc, n, kind, s, R.floor_margin(ys[s], zc), d32, dtr)
                        if ex == 0.0:
                            assert (m64 == ys[s]).all()
                r2 = R.rms(ys[0], 4 * zc, zc)
                if kind in ("silent_out", "quiet_out"):
                    assert r2.max() < 0.1 * R.FLOOR                     # the floor is active everywhere
                else:
                    assert r2.min() > 10 * R.FLOOR
                if kind == "silent_in":
                    assert (R.envelop_mix(xs[0], ys[0], zc, 0.5)[0] == 0).all()
            # the edges the shapes are there for: frames of 4, 28, 64, 260; n not a multiple of the hop; the shortest track
            assert len(R.rms(np.zeros(zc), 4 * zc, zc)) == 2


def test_sola_inputs_have_a_clear_best_lag():
    for n, search, frame in R.SOLA_CASES:
        for s in range(3):
            out, sola, lead = R.sola_case(n, search, frame, s)
            assert len(out) == search + frame + n
            b = R.sola_bound(out, sola, search, frame)
            assert b["off"] == lead and 0 <= lead <= search
            assert b["d_cor"] <= 1e-4 * b["p_cor"] and b["d_seam"] <= 1e-4 * b["p_seam"], (n, search, frame, s, b["d_cor"], b["p_cor"], b["d_seam"], b["p_seam"])
            assert b["lead"] >= 100 * b["d_cor"], (n, search, frame, s, b["lead"], b["d_cor"])          # no case is "too close"
    assert sum(frame < n for n, _, frame in R.SOLA_CASES) >= 2
    # the deliberate ties
    out, sola, search, frame, tied = R.sola_periodic()
    cor, off = R.sola_cor(out, sola, search)
    assert off == tied[-1] and len({cor[t] for t in tied}) == 1 and all(cor[l] < cor[off] for l in range(search + 1) if l not in tied)
    assert all((out[t:t + len(sola)] == out[tied[0]:tied[0] + len(sola)]).all() for t in tied)
    cor32, off32 = R.sola_cor(out, sola, search, np.float32)
    assert off32 == tied[-1] and len({cor32[t] for t in tied}) == 1
    # the zero-window guard
    out, sola, search, frame, dead = R.sola_zero_window()
    b = R.sola_bound(out, sola, search, frame)
    assert (b["cor"][:dead] == 0).all() and (out[:len(sola) + dead - 1] == 0).all() and b["cor"][dead] != 0 and b["off"] == dead + 5
    assert b["lead"] >= 100 * b["d_cor"] and b["d_cor"] <= 1e-4 * b["p_cor"]


def test_converter_cases_reach_the_edges_they_are_there_for():
    geo = {c: R.resampler_geometry(*c) for c in R.RESAMPLE_CASES + R.RESAMPLE_MINIMAL}
    first6 = [geo[c] for c in R.RESAMPLE_CASES[:6]]
    assert sum(g["fft_in"] < 64 for g in first6) == 5 and sum(g["fft_in"] % 2 == 1 for g in first6) == 3
    assert {(g["P"] > g["Q"], g["P"] < g["Q"], g["P"] == 1, g["Q"] == 1) for g in geo.values()} >= {(True, False, False, True), (False, True, True, False),
                                                                                                   (False, False, True, True), (True, False, False, False), (False, True, False, False)}
    # a group of 4 outputs that is cut short (the t1 - 1 clamp): outputs per split not a multiple of 4
    assert sum(any((t - (g["splits"] - 1) * p) % 4 for t, p in zip(g["n_t"], g["per"])) for g in geo.values()) >= 5
    assert all(set(geo[c]["n_t"]) == {2} for c in R.RESAMPLE_MINIMAL)                     # residue classes with fewer than 4 outputs
    for c in R.RESAMPLE_CASES[6:]:                                                          # splits > 1 with an uneven last split
        g = geo[c]
        last = [t - (g["splits"] - 1) * p for t, p in zip(g["n_t"], g["per"])]
        assert g["splits"] == 13 and all(0 < l < p for l, p in zip(last, g["per"])), (c, g["splits"], last)
    assert (geo[(100, 100, 200)]["per"], geo[(1600, 4800, 400)]["per"]) == ([31], [62] * 3)
    # what no converter can reach: 2 fft_out is a multiple of Q, so every class has the same count, and the split rule never leaves a split empty
    for ri, ro in ((100, 100), (300, 100), (100, 300), (700, 300), (300, 700), (44100, 16000), (48000, 44100)):
        for ch in list(range(1, 400)) + [8640, 10080, 72960]:
            g = R.resampler_geometry(ri, ro, ch)
            assert len(set(g["n_t"])) == 1 and all(t - (g["splits"] - 1) * p > 0 for t, p in zip(g["n_t"], g["per"]))


@pytest.mark.parametrize("ri,ro,ch", R.RESAMPLE_CASES + R.RESAMPLE_MINIMAL)
def test_converter_inputs_are_well_conditioned(ri, ro, ch):
    fi, fo = RO.fft_sizes(ri, ro, ch)
    r64, bound, peak = R.resample_bound(R.resample_signal(fi, 4), ri, ro, ch, 4, 1)
    assert r64.shape == (5, fo) and bound <= 1e-4 * peak, (bound, peak)
    assert np.abs(r64[4] - r64[0]).max() == 0                                              # after the reset the first chunk comes out again


def test_hook_is_declared_where_the_tests_look_for_it():
    hdr = open(os.path.join(ROOT, "include", "rvc_mi355x_debug.h")).read()
    dbg = open(os.path.join(ROOT, "obs_rvc_amd", "csrc", "debug.hip")).read()
    assert re.search(r"\brvc_debug_post\s*\(", hdr) and re.search(r"\brvc_debug_post\s*\(", dbg)
    # the correlations of a 1023-lag search fill post_sola_kernel's shared array exactly; one more lag must be refused on the host
    chunk = open(os.path.join(ROOT, "obs_rvc_amd", "csrc", "chunk.hip.h")).read()
    assert re.search(r"__shared__ float cor\[1024\]", chunk)
