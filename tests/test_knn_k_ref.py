"""CPU checks of tests/knn_k_ref.py: the K-parametric definition at K = 4 is knn_ref's, and every input of tests/test_gpu_knn_k8.py provokes at K = 8 what its
case claims (candidate counts far from KNN_CAND, the flagged workgroups of the one-launch form, duplicate runs longer than 8), so that no GPU assertion about
an overflow word rests on a count near a threshold."""
from __future__ import annotations

import numpy as np
import pytest

import knn_k_ref as R
import knn_ref as KR


@pytest.fixture(scope="module")
def cases():
    return R.shared_cases()


def test_k4_is_knn_ref():
    c = KR.make_case("near_runs", dim=48, n=1023, streams=3, nq=17, seed=100)
    q = c.used(0)
    d = KR.d64(c.index, q)
    for a, b in zip(R.topk(d, 4), KR.topk(d)):
        assert np.array_equal(a, b)
    assert np.array_equal(R.inside(c.index, q, 4), KR.inside(c.index, q))
    assert np.array_equal(R.inside(c.index, q, 4, 1e-3), KR.inside(c.index, q, 1e-3))
    assert np.array_equal(R.candidates(c.index, q, 4), KR.candidates(c.index, q))
    G = R.fused_grid(c.n, c.streams, 768)
    assert np.array_equal(R.per_workgroup(R.inside(c.index, q, 4), G), KR.per_workgroup(KR.inside(c.index, q), G))
    for dim in (16, 44, 48, 768):
        assert R.blend_bound(dim, 4) == KR.blend_bound(dim)
        assert R.blend_bound(dim, 8) == KR.blend_bound(dim) + 4 * R.U
    idx = R.topk(d, 8)[0][0]
    for a, b in zip(R.blend(c.index, q[0], idx, 0.75), KR.blend(c.index, q[0], idx, 0.75)):
        assert np.array_equal(a, b)


def test_top8_starts_with_top4():
    c = R.make_case("far_dups10_5", seed=1100, **R.FEW_SHAPE)
    d = KR.d64(c.index, c.used(0))
    assert np.array_equal(R.topk(d, 8)[0][:, :4], R.topk(d, 4)[0])


def counts(case, K=8, c=2e-3):
    return np.concatenate([R.candidates(case.index, case.used(b), K, c) for b in range(case.streams)])


def test_candidate_counts_far_from_knn_cand(cases):
    """the many-stream path's overflow words: every query of a class either collects fewer than KNN_CAND / 8 candidates or more than 1.9 KNN_CAND"""
    for name, (few, many) in cases.items():
        for case in (few, many):
            n = counts(case)
            if name == "offset_dim":
                assert n.min() == case.n and case.n > 1.9 * R.KNN_CAND, (name, n.min())       # every vector of the index is a candidate
            else:
                assert n.min() >= 8 and n.max() <= R.KNN_CAND // 8, (name, n.min(), n.max())
    t = R.truncated_case()
    assert counts(t).max() <= R.KNN_CAND // 8


def test_converter_window_case():
    """the file converter's default window as tests/test_gpu_knn_k8.py runs it: skip_head 48, 351 frames over T = 223 columns; frame r reads column
    (48 + r) / 2 -- 24 for r = 0, 199 for r = 350, no clamp -- which is 176 raw frames; the duplicate runs sit on the first and the last of them; the
    candidate counts are far from KNN_CAND at both stream counts"""
    assert KR.GEOMS[176] == (48, 351, 223) and KR.raw_range(48, 351, 223) == (24, 176)
    cols = KR.col_map(48, 351, 223)
    assert cols[0] == 24 and cols[350] == 199 and cols[349] == 198 and cols.max() < 222
    for streams in (1, 3):
        c = R.make_case("near_runs12", dim=48, n=1023, streams=streams, nq=176, seed=1400 + streams)
        assert (c.skip_head, c.R, c.T, c.first_raw) == (48, 351, 223, 24)
        assert {t for _, t, _, _ in c.meta["places"]} == {24, 199}
        n = counts(c)
        assert n.min() >= 8 and n.max() <= R.KNN_CAND // 8, (streams, n.min(), n.max())


def test_straddle_counts_at_k8():
    """knn_ref's `straddle` offset (scale 5.5, n = 4099) at K = 8: more than 2 KNN_CAND candidates for some query of every stream with the margin as it is, fewer
    than 0.6 KNN_CAND with half of it -- far from 512 either way, so the class is used as it is"""
    s = KR.make_case("straddle", dim=48, n=4099, streams=12, nq=11, seed=100)
    for b in range(s.streams):
        assert R.candidates(s.index, s.used(b), 8).max() > 2 * R.KNN_CAND
        assert R.candidates(s.index, s.used(b), 8, 1e-3).max() < 0.6 * R.KNN_CAND


def test_flagged_workgroups(cases):
    for few, _ in (cases["gaussian"], cases["far_dups10_5"], cases["norm_spread"]):
        G = R.fused_grid(few.n, few.streams, 768)
        for b in range(few.streams):
            assert not R.flagged(few.index, few.used(b), G, 8).any()
    few = cases["offset_dim"][0]
    G = R.fused_grid(few.n, few.streams, 768)
    assert G == 16
    for b in range(few.streams):
        assert R.flagged(few.index, few.used(b), G, 8).all()
    # near-duplicate runs of 12: the workgroup that owns a whole run inside one tile is flagged for that query, and only that one; a run split 7 | 5 over two
    # workgroups (the tile boundary 58..63 | 64..69 is also a workgroup boundary at one tile per step; the wrap 251..255 | 256..262) flags none
    few = cases["near_runs12"][0]
    for b, t, row, ln in few.meta["places"]:
        j = t - few.first_raw
        fl = R.flagged(few.index, few.used(b), G, 8)[j]
        wgs = sorted(set(((np.arange(row, row + ln) // 16) % G).tolist()))
        per = np.bincount((np.arange(row, row + ln) // 16) % G, minlength=G)
        assert fl.tolist() == (per >= 8).tolist(), (row, ln, wgs)
    assert any(ln >= 8 and len(set(((np.arange(row, row + ln) // 16) % G).tolist())) == 1 for _, _, row, ln in few.meta["places"])


def test_duplicate_runs_longer_than_k(cases):
    few = cases["near_runs12"][0]
    assert [ln for _, _, _, ln in few.meta["places"]] == [12, 12, 12, 15]
    for b, t, row, ln in few.meta["places"]:
        top = R.topk(KR.d64(few.index, few.q[b, t][None]), 8)[0][0]
        assert set(top.tolist()) <= set(range(row, row + ln))                   # the eight hits all come from the run: which eight is decided by (d, i)
    few = cases["far_dups10_5"][0]
    rows, rows2 = few.meta["rows"], few.meta["rows2"]
    f0, last = few.first_raw, few.first_raw + few.nq - 1
    assert R.topk(KR.d64(few.index, few.q[0, f0][None]), 8)[0][0].tolist() == rows[:8]            # ten bit-identical copies: the eight lowest row numbers
    top = R.topk(KR.d64(few.index, few.q[few.streams - 1, last][None]), 8)[0][0].tolist()
    assert top[:5] == rows2 and not set(top[5:]) & set(rows2)
    t = R.truncated_case()
    b, j = t.meta["where"]
    assert KR.per_thread(R.inside(t.index, t.used(b), 8))[j].max() == 8 and len(t.meta["rows"]) == 8      # exactly k in one thread's stride set


def test_oracle_top8_starts_with_top4(cases):
    from oracle import oracle as O
    for name, (few, _) in cases.items():
        q = few.used(0)
        i8, d8 = O.knn_search(few.index, q, 8)
        i4, d4 = O.knn_search(few.index, q, 4)
        assert np.array_equal(i8[:, :4], i4) and np.array_equal(d8[:, :4].view(np.uint32), d4.view(np.uint32)), name
        assert np.array_equal(i8, R.topk(KR.d64(few.index, q), 8)[0]) or name in ("near_runs12", "norm_spread")      # (near-ties may order differently in fp32)
