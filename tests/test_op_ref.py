"""tests/op_ref.py (the fp64 reference of tests/test_gpu_ops.py) pinned to torch.float64 on the CPU: F.layer_norm, nn.GRU(bidirectional) fed the
same gate pre-activations, a manual softmax attention, and the relative attention of tests/torch_ref.py (_rel_attn) run at double precision."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import op_ref as R
import torch_ref

TOL = 1e-12


def _rand(rng, *shape, scale=1.0):
    return rng.uniform(-scale, scale, shape)


@pytest.mark.parametrize("B,C,T,mean", [(1, 16, 5, 0.0), (2, 192, 7, 0.0), (3, 769, 3, 0.0), (1, 48, 9, 1e3)])
def test_layernorm_matches_torch(B, C, T, mean):
    rng = np.random.default_rng(C + T)
    x = mean + _rand(rng, B, C, T)
    g, b = _rand(rng, C), _rand(rng, C)
    want = F.layer_norm(torch.from_numpy(x).transpose(1, 2), (C,), torch.from_numpy(g), torch.from_numpy(b), eps=1e-5).transpose(1, 2).numpy()
    assert np.max(np.abs(R.layernorm(x, g, b) - want)) < TOL


@pytest.mark.parametrize("B,E,heads,T", [(1, 24, 2, 1), (2, 32, 4, 17), (3, 36, 3, 9)])
def test_mha_matches_manual_softmax_attention(B, E, heads, T):
    rng = np.random.default_rng(E * T)
    qkv = _rand(rng, B, 3 * E, T, scale=3.0)
    hd = E // heads
    t = torch.from_numpy(qkv)
    q, k, v = (t[:, i * E:(i + 1) * E].reshape(B, heads, hd, T).transpose(2, 3) for i in range(3))      # [B][h][T][hd]
    p = torch.softmax(q @ k.transpose(-2, -1) / math.sqrt(hd), dim=-1)
    want = (p @ v).transpose(2, 3).reshape(B, E, T).numpy()
    assert np.max(np.abs(R.mha(qkv, heads) - want)) < TOL


@pytest.mark.parametrize("B,E,heads,T,w", [(1, 16, 2, 1, 4), (2, 16, 2, 9, 4), (1, 24, 3, 23, 10), (2, 8, 1, 5, 10)])
def test_relpos_mha_matches_torch_ref(monkeypatch, B, E, heads, T, w):
    rng = np.random.default_rng(E * T + w)
    qkv = _rand(rng, B, 3 * E, T, scale=2.0)
    hd = E // heads
    rk, rv = _rand(rng, 2 * w + 1, hd), _rand(rng, 2 * w + 1, hd)
    # tests/torch_ref.py's _rel_attn with identity projections (x = qkv), in float64
    monkeypatch.setattr(torch_ref, "_t", lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)))
    eye, zero = np.eye(E), np.zeros((E, E))
    pre = "sy.enc.l0."
    wts = {pre + "q.w": np.hstack([eye, zero, zero]), pre + "k.w": np.hstack([zero, eye, zero]), pre + "v.w": np.hstack([zero, zero, eye]),
           pre + "o.w": eye, pre + "rel_k": rk, pre + "rel_v": rv}
    wts.update({pre + n + ".b": np.zeros(E) for n in "qkvo"})
    want = torch_ref._rel_attn(wts, 0, torch.from_numpy(qkv), heads, w).numpy()
    assert np.max(np.abs(R.relpos_mha(qkv, heads, rk, rv, w) - want)) < TOL


@pytest.mark.parametrize("B,H,T,gain", [(1, 4, 1, 1.0), (2, 8, 13, 1.0), (1, 16, 6, 8.0)])
def test_gru_matches_torch_bidirectional_gru(B, H, T, gain):
    rng = np.random.default_rng(H * T)
    I = 5
    gru = torch.nn.GRU(I, H, bidirectional=True, batch_first=True).double()
    with torch.no_grad():
        for p_ in gru.parameters():
            p_.copy_(torch.from_numpy(_rand(rng, *p_.shape, scale=gain / math.sqrt(H))))
    x = _rand(rng, B, T, I)
    with torch.no_grad():
        want = gru(torch.from_numpy(x))[0].transpose(1, 2).numpy()          # [B][2H][T]
    sd = {k: v.numpy() for k, v in gru.state_dict().items()}
    # gate pre-activations W_ih x + b_ih, forward then reverse: what the engine's input projection writes
    gi = np.concatenate([np.einsum("gi,bti->bgt", sd["weight_ih_l0" + s], x) + sd["bias_ih_l0" + s][None, :, None] for s in ("", "_reverse")], axis=1)
    whh = np.stack([sd["weight_hh_l0"], sd["weight_hh_l0_reverse"]])
    bhh = np.stack([sd["bias_hh_l0"], sd["bias_hh_l0_reverse"]])
    assert np.max(np.abs(R.gru_bidir(gi, whh, bhh) - want)) < TOL
