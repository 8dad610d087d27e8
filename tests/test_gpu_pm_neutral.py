"""Adding the PM f0 method changed nothing under the methods that were there: rvc_pitch, a two-chunk PCM and the pitch cache under RMVPE and under YIN are
bit-identical to what a build of the commit before PM gave on an MI355X (tests/golden/f0_neutral_parent.npz, recorded once from that build with the
recipe below: the tiny zoo, noise seed 1234, the YIN test's composite input for rvc_pitch, two voice_signal chunks of which the second ends in it)."""
from __future__ import annotations

import os

import numpy as np
import pytest

import yin_ref as Y
from common import BASELINE_160MS as g, GOLDEN, voice_signal, zoo

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", ["rmvpe", "yin"])
def test_the_other_methods_compute_what_they_computed(method):
    from obs_rvc_amd.rvc import RvcInfer
    want = np.load(os.path.join(GOLDEN, "f0_neutral_parent.npz"))
    z = zoo("tiny")
    x = Y.composite_signal()
    L, FRAME16K, R = g.input_buffer_16k_size, g.sample_frame_16k, g.model_return_length
    chunks = [voice_signal(L, seed=3), voice_signal(L, seed=4)]
    chunks[1][-4960:] = x[-4960:]
    e = RvcInfer(z["data"]); e.load_contentvec(2); e.load_model(z["model"]); e.load_f0_method(method); e.set_noise_seed(1234, 0)
    pitch = e.pitch(x, 0, FRAME16K)
    pcm = np.stack([e.infer(c, FRAME16K, 12, g.skip_head, R) for c in chunks])
    cache = e.pitch_cache()
    e.close()
    assert np.array_equal(pitch, want["pitch_" + method])
    assert np.array_equal(cache, want["cache_" + method])
    assert pcm.shape == want["pcm_" + method].shape and np.array_equal(pcm, want["pcm_" + method])
