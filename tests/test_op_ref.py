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


# ---- the converter-length cases of tests/test_gpu_ops.py: what can be settled without a device
import test_gpu_ops as G  # noqa: E402


def test_attention_lds_arithmetic_at_the_converter_limit():
    """plan.hip's attn_valu_lds restated: return_length 351 (the default window, k = 14) is the last that fits 160 KB at head size 96"""
    assert G.attn_valu_lds(96, 351) == 163392 and G.attn_valu_lds(96, 350) == 163392          # 350 and 351 share the odd-padded row
    assert G.attn_valu_lds(96, 352) == 164288 and G.attn_valu_lds(96, 353) == 164288
    assert G.attn_valu_lds(96, 351) <= G.LDS_LIMIT == 163840 < G.attn_valu_lds(96, 352)
    assert G.attn_valu_lds(16, 1025) == 132224 <= G.LDS_LIMIT                                  # the 133 KB case
    assert G.attn_valu_lds(64, 499) <= G.LDS_LIMIT < G.attn_valu_lds(64, 500)                  # ContentVec's own limit (T <= 499)
    for c in G.long_cases():
        if c.op == G.OP_REL:
            assert G.attn_valu_lds(c.spec["E"] // 2, c.T) <= G.LDS_LIMIT and G.relpos_rule(c) == "valu", c.label
            assert not G.relpos_eligible(c, "mfma") and not G.relpos_eligible(c, "small"), c.label
        else:
            assert G.gru_rule(c) == "generic" and not G.gru_eligible(c, "multi"), c.label


def test_long_case_lists_are_the_converter_lengths():
    rel = {(c.spec["E"] // 2, c.T, c.B) for c in G.relpos_cases() if c.long}
    assert rel == {(96, T, B) for T in (156, 255, 256, 257, 350, 351) for B in (1, 3)} | {(16, 351, 1), (16, 1025, 1)}
    gru = {(c.spec["H"], c.T, c.B) for c in G.gru_cases() if c.long}
    assert gru == {(256, T, B) for T in (448, 1024) for B in (1, 3)} | {(32, 1024, 1)}
    assert all(c.spec["window"] == 10 for c in G.relpos_cases() if c.long)


@pytest.mark.parametrize("case", G.long_cases(), ids=repr)
def test_float32_restatement_sits_inside_a_quarter_of_the_tolerance(case):
    """TOL_ATTN and TOL_GRU were derived from the head size and the recurrence's contraction, not from T.  Before a device is held to them at the
    converter's lengths: the same definition in float32 numpy, on the case's own inputs, deviates from float64 by at most a quarter of the tolerance"""
    x, _, _, ref, _ = case.data()
    d32, tol = case.d32(), G.TOL[case.op]
    fits = d32 <= tol / 4
    print("%s: float32 numpy against float64 %.3e, tolerance %.1e (ratio %.3f)%s" % (case.label, d32, tol, d32 / tol, "" if fits else
          ": over a quarter, the case is held to 4 x this instead (%.2e)" % case.tol()))
    # a case over the quarter is not given a wider constant: its bound is 4 x its own float32 deviation (Case.tol).  Measured here: 0.02 .. 0.24 of the
    # tolerance, every case inside the quarter; the largest, 0.24, moves with numpy's summation order, so the quarter itself is not what fails the case.
    # Half the tolerance is: a restatement that far out would mean the tolerance's derivation does not hold at this length
    assert case.tol() == (tol if fits else 4.0 * d32) and d32 <= tol / 2, (case.label, d32)
    if case.op == G.OP_REL:
        # the recipe does its jobs at this length: logits of about +-40, a row of equal scores, dominant keys in column 0, T // 2 and T - 1, and a
        # query whose weight sits inside its relative window at the clamped end
        T, E, w = case.T, case.spec["E"], case.spec["window"]
        hd = E // 2
        q, k = x[:, :hd].astype(np.float64), x[:, E:E + hd].astype(np.float64)                  # head 0
        s = np.einsum("bdi,bdj->bij", q, k) / math.sqrt(hd)
        p = np.exp(s - s.max(axis=-1, keepdims=True))
        p /= p.sum(axis=-1, keepdims=True)
        assert 35 < np.abs(s).max() < 80 and np.all(s[:, 0] == 0)          # (the extremes of T^2 logits of standard deviation 13)
        qe = T - 1 - w // 2
        for qi, kj in ((1, T // 2), (2, T - 1), (3, 0), (qe, T - 1)):
            # (among several hundred random keys of standard deviation 13 one passes 40 now and then and takes most of the row: in every stream the
            # planted key keeps a weight above the tolerance)
            assert np.all(np.abs(s[:, qi, kj] - 40.0) < 1e-4), (qi, kj, s[:, qi, kj])
            print("  query %d -> key %d: weights %s" % (qi, kj, p[:, qi, kj]))
            assert np.all(p[:, qi, kj] > G.TOL_ATTN), (qi, kj, p[:, qi, kj])
            if qi != 1:                                      # the edge columns: in the best stream, losing one moves the output by a hundred tolerances
                assert np.max(p[:, qi, kj]) > 100 * G.TOL_ATTN, (qi, kj, p[:, qi, kj])
    else:
        H, T = case.spec["H"], case.T
        assert np.count_nonzero(np.abs(x[0, :, T // 2]) == 25.0) == 6 * H // 4                  # the saturated quarter of the gate rows
