"""tests/layer_ref.py (the fp64 reference of tests/test_gpu_layers.py) pinned to torch.float64 on the CPU: convolutions with stride, dilation,
groups and padding, the transposed convolution (kernel not a multiple of the stride included), the 3x3 Conv2d and the activations -- so that the
GPU layers are checked against the operations' definitions, not against a restatement of the kernels' own indexing."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import layer_ref as R

TOL = 1e-12


def _rand(rng, *shape):
    return rng.uniform(-1.0, 1.0, shape)


@pytest.mark.parametrize("cin,cout,k,stride,pad,dil,groups,t", [
    (1, 8, 10, 5, 0, 1, 1, 57),          # ContentVec's strided stem
    (12, 8, 3, 2, 0, 1, 1, 40),          # ... its later strided layers
    (1, 6, 8, 4, 2, 1, 1, 64),           # noise conv: K = 2 sf, stride sf, pad sf / 2
    (1, 6, 24, 12, 6, 1, 1, 97),
    (32, 32, 16, 1, 8, 1, 16, 29),       # grouped positional conv (output one longer than the input)
    (16, 16, 11, 1, 25, 5, 1, 33),       # dilated ResBlock conv
    (16, 24, 5, 1, 2, 1, 1, 21),         # WaveNet in-layer
    (20, 10, 7, 1, 3, 1, 1, 13),
    (9, 6, 1, 1, 0, 1, 3, 7),
])
def test_conv1d_matches_torch(cin, cout, k, stride, pad, dil, groups, t):
    rng = np.random.default_rng(cin * 1000 + k)
    x, w, b = _rand(rng, 2, cin, t), _rand(rng, cout, cin // groups, k), _rand(rng, cout)
    ref = F.conv1d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=pad, dilation=dil, groups=groups).numpy()
    got = R.conv1d(x, w, b, stride, pad, dil, groups)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) < TOL


@pytest.mark.parametrize("k,s", [(24, 12), (20, 10), (16, 10), (16, 8), (8, 4), (7, 3), (4, 2), (5, 2)])
def test_conv_transpose1d_matches_torch(k, s):
    rng = np.random.default_rng(k * 31 + s)
    cin, cout, t, pad = 6, 5, 17, (k - s) // 2
    x, w, b = _rand(rng, 3, cin, t), _rand(rng, cin, cout, k), _rand(rng, cout)
    ref = F.conv_transpose1d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), stride=s, padding=pad).numpy()
    got = R.conv_transpose1d(x, w, b, s, pad)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) < TOL


def test_conv2d_matches_torch():
    rng = np.random.default_rng(5)
    x, w, b = _rand(rng, 2, 4, 7, 9), _rand(rng, 3, 4, 3, 3), _rand(rng, 3)
    ref = F.conv2d(torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b), padding=1).numpy()
    got = R.conv2d_3x3(x, w, b)
    assert np.max(np.abs(got - ref)) < TOL


def test_activations_match_torch():
    v = np.linspace(-9.0, 9.0, 2001)
    tv = torch.from_numpy(v)
    assert np.max(np.abs(R.act(v, R.ACT_GELU) - F.gelu(tv).numpy())) < TOL          # erf form
    assert np.max(np.abs(R.act(v, R.ACT_TANH) - torch.tanh(tv).numpy())) < TOL
    assert np.max(np.abs(R.act(v, R.ACT_SIGMOID) - torch.sigmoid(tv).numpy())) < TOL
    assert np.max(np.abs(R.act(v, R.ACT_RELU) - F.relu(tv).numpy())) < TOL
    assert np.max(np.abs(R.act(v, R.ACT_LRELU, 0.1) - F.leaky_relu(tv, 0.1).numpy())) < TOL
    a = np.linspace(-3.0, 3.0, 2 * 8 * 5).reshape(1, 16, 5)
    ta = torch.from_numpy(a)
    assert np.max(np.abs(R.glu_gate(a) - (torch.tanh(ta[:, :8]) * torch.sigmoid(ta[:, 8:])).numpy())) < TOL
