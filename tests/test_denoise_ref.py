"""Spectral-gate noise reduction (DESIGN.md "Spectral-gate noise reduction"): the properties of the numpy definition in tests/denoise_ref.py, the
conditioning of the GPU tests' inputs, and the layers that exist without a GPU (declared entry points)."""
from __future__ import annotations

import fnmatch
import os
import re

import numpy as np
import pytest

from denoise_ref import CASES, SESSION_INPUTS, SHAPES, RefDenoiser, bound, case_batch, denoise, voiced
from obs_rvc_amd import _native
from obs_rvc_amd.rvc_common import DENOISE_INPUT, DENOISE_OUTPUT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["rvc_denoiser_create", "rvc_denoiser_destroy", "rvc_denoiser_reset", "rvc_denoiser_set", "rvc_denoiser_latency", "rvc_denoiser_process",
                    "rvc_denoiser_process_device", "rvc_session_set_noise_reduction", "rvc_session_set_noise_reduction_stream"]


@pytest.mark.parametrize("rate", [8000, 16000, 44100, 48000])
def test_all_ones_mask_reconstructs_the_input_delayed_by_one_hop(rate):
    zc = rate // 100
    x = voiced(9 * zc, rate, 1)
    for strength in (1.0, 0.6):
        y = RefDenoiser(rate, strength, 2.0, mask_override=1.0).process(x)
        assert np.abs(y[zc:] - x[:-zc].astype(np.float64)).max() <= 1e-12 and np.abs(y[:zc]).max() <= 1e-12
    w = RefDenoiser(rate).w
    assert np.abs(w[:zc] ** 2 + w[zc:] ** 2 - 1.0).max() < 1e-15


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_cutting_the_signal_into_calls_changes_nothing(dt):
    rate, zc = 8000, 80
    x = voiced(12 * zc, rate, 2)
    one = RefDenoiser(rate, 0.8, 1.0, dt).process(x)
    d = RefDenoiser(rate, 0.8, 1.0, dt)
    cut = np.concatenate([d.process(x[:3 * zc]), d.process(x[3 * zc:7 * zc]), d.process(x[7 * zc:])])
    assert (cut == one).all()
    d.reset()
    assert (d.process(x) == one).all()
    # strength 0: the input itself, undelayed, and the state is left alone
    d.set(0.0)
    S = d.S.copy()
    assert (d.process(x) == x).all() and (d.S == S).all()


def test_stationary_noise_is_attenuated():
    rate, zc = 16000, 160
    x = (0.05 * np.random.default_rng(11).standard_normal(120 * zc)).astype(np.float32)
    y = denoise(x, rate, 1.0, 2.0)
    p_in, p_out = float(np.mean(x[40 * zc:-zc].astype(np.float64) ** 2)), float(np.mean(y[41 * zc:] ** 2))
    print("stationary white noise, strength 1, threshold 2: output / input power after 40 frames = %.4f (%.1f dB)" % (p_out / p_in, 10 * np.log10(p_out / p_in)))
    assert p_out < p_in


def test_attack_of_a_sine_30_db_above_the_floor_passes():
    rate, zc = 16000, 160
    rng = np.random.default_rng(12)
    sigma = 0.01
    x = sigma * rng.standard_normal(100 * zc)
    on = 60 * zc                                            # the floor has settled (60 frames = 3 time constants)
    amp = np.sqrt(2.0) * sigma * 10.0 ** (30.0 / 20.0)      # rms 30 dB above the noise's
    t = np.arange(len(x) - on) / float(rate)
    x[on:] += amp * np.sin(2 * np.pi * 1000.0 * t)          # 1 kHz = bin 20
    d = RefDenoiser(rate, 1.0, 2.0)
    d.process(x.astype(np.float32))
    G = np.array(d.gains)                                   # [frame][bin]; frame 60 is the first that holds the sine (its second half)
    print("attack: G at bin 20, frames 58 .. 63: %s" % np.round(G[58:64, 20], 4))
    assert G[60, 20] >= 0.9                                 # the attack frame (later frames of a steady sine are narrow-band: step 4 pulls them down again)
    assert np.median(G[50:60]) < 0.5                        # while the settled floor itself is held down


@pytest.mark.parametrize("rate,hops", SHAPES + [(8000, 12)])
def test_fp32_reference_is_well_conditioned_on_the_gpu_test_inputs(rate, hops):
    # the GPU tests' tolerance is 2 * delta32; an ill-conditioned input must not be able to widen it: delta32 <= 1e-4 * peak (asserted inside bound)
    x = case_batch(rate, hops)
    for (kind, strength, thr), xs in zip(CASES, x):
        r64, d32, peak = bound(xs, rate, strength, thr)
        print("%d Hz, %d hops, %s strength %.1f threshold %.1f: delta32 %.3e peak %.3f (%.2e of peak)" % (rate, hops, kind, strength, thr, d32, peak, d32 / peak))
        assert 0.2 < peak < 0.8


@pytest.mark.parametrize("rate,frame,chunks,seed", SESSION_INPUTS)
def test_fp32_reference_is_well_conditioned_on_the_session_inputs(rate, frame, chunks, seed):
    r64, d32, peak = bound(voiced(chunks * frame, rate, seed), rate, 1.0, 2.0)
    print("%d Hz, %d chunks of %d: delta32 %.3e peak %.3f (%.2e of peak)" % (rate, chunks, frame, d32, peak, d32 / peak))


def test_entry_points_are_declared_in_every_layer():
    hdr = open(os.path.join(ROOT, "include", "rvc_mi355x.h")).read()
    ffi = open(os.path.join(ROOT, "bindings", "rust", "rvc", "src", "ffi.rs")).read()
    emap = open(os.path.join(ROOT, "obs_rvc_amd", "csrc", "exports.map")).read()
    exported = re.findall(r"[\w*]+", re.search(r"global:(.*?)local:", re.sub(r"/\*.*?\*/", "", emap, flags=re.S), flags=re.S).group(1))
    for name in NEW_ENTRY_POINTS:
        assert name in _native.SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert re.search(r"pub fn %s\s*\(" % name, ffi), name
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), name
    assert re.search(r"RVC_DENOISE_INPUT\s*=\s*0\s*,\s*RVC_DENOISE_OUTPUT\s*=\s*1", hdr)
    assert (DENOISE_INPUT, DENOISE_OUTPUT) == (0, 1)
    assert "denoise.hip.h" in _native.SOURCES
    from obs_rvc_amd.denoise import Denoiser
    from obs_rvc_amd.streaming import NativeStreamingSession
    assert callable(Denoiser.process) and callable(NativeStreamingSession.set_noise_reduction)
