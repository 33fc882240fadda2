"""Nearest-neighbour retrieval on the GPU: actmi_op_knn_topk bit for bit against its numpy statement over both regimes, the tails
of the 4-way summation order and the tile edges; actmi_op_knn_predict / actmi_op_knn_ksweep against the float64 statements.

Bars.  Top-k: array_equal.  The distance is a fixed sequence of individually rounded fp32 operations in an order that is part
of the ABI (include/actmi.h), numpy's float32 subtract / multiply / add / sqrt are the same IEEE operations, and the selection
key (distance bits, index) has no ties, so there is exactly one right answer.
Predict / ksweep: |err| <= 2^-23 |ref| + 1e-12 max|target|.  The result is one float64 value rounded once to fp32 (half an ulp,
2^-24 relative; 2^-23 leaves room for a float64 difference that moves the rounding), and the second term covers at most 512
float64 terms at a few ulp each, 512 * 4 * 1.1e-16 = 2.3e-13 of the largest term, plus exp() differing in its last place.
Ns = K - 1 of the grid is taken as max(1, K - 1): K = 1 would name an empty support set, which every entry refuses."""
import functools
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from actmi import ops  # noqa: E402

DEV = "cuda"
DVS, SS, KS, NQS = (1, 3, 70, 512), (0, 3, 14), (1, 7, 512), (1, 33)


def ns_of(K):
    return sorted({1, max(1, K - 1), K, 257, 1000})


@functools.lru_cache(maxsize=None)
def pool(Dv, S):
    """33 queries and 1000 support rows of (Dv, S) dimensions, drawn once; smaller cases take leading rows"""
    rng = np.random.default_rng(1000 * Dv + S)
    qv, sv = rng.standard_normal((33, Dv)).astype(np.float32), rng.standard_normal((1000, Dv)).astype(np.float32)
    qs, ss = rng.standard_normal((33, S)).astype(np.float32), rng.standard_normal((1000, S)).astype(np.float32)
    sep = (np.arange(1000) // 37).astype(np.int32)
    return qv, qs, sv, ss, sep


def cu(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_topk(qv, qs, sv, ss, K, w, sep=None, exclude=None):
    out = ops.knn_topk(cu(qv), cu(qs) if qs is not None and qs.shape[1] else None, cu(sv),
                       cu(ss) if ss is not None and ss.shape[1] else None, K, w, cu(sep), cu(exclude))
    return tuple(t.cpu().numpy() for t in out)


def same(got, ref):
    for g, r, name in zip(got, ref, ("idx", "dist", "n")):
        assert g.dtype == r.dtype and np.array_equal(g.view(np.int32), r.view(np.int32)), name


@pytest.mark.parametrize("Dv,S", list(itertools.product(DVS, SS)))
def test_topk_matches_the_numpy_statement_bit_for_bit(Dv, S):
    qv, qs, sv, ss, _ = pool(Dv, S)
    for K in KS:
        for Ns in ns_of(K):
            ref33 = ops.knn_topk_ref(qv, qs, sv[:Ns], ss[:Ns], K, 0.75)
            for Nq in NQS:
                got = run_topk(qv[:Nq], qs[:Nq], sv[:Ns], ss[:Ns], K, 0.75)
                same(got, tuple(r[:Nq] for r in ref33))
                assert np.all(got[2] == min(K, Ns))


@pytest.mark.parametrize("Nq", NQS)
def test_exact_ties_take_the_lowest_index_and_a_stored_query_is_at_zero(Nq):
    qv, qs, sv, ss, _ = pool(70, 14)
    sv, ss = sv[:300].copy(), ss[:300].copy()
    sv[200:220], ss[200:220] = sv[10:30], ss[10:30]              # exact duplicates of rows 10..29
    qv, qs = qv[:Nq].copy(), qs[:Nq].copy()
    qv[0], qs[0] = sv[17], ss[17]                                # the query is support row 17 (and 207)
    got = run_topk(qv, qs, sv, ss, 300, 2.0)
    same(got, ops.knn_topk_ref(qv, qs, sv, ss, 300, 2.0))
    idx, dist, _ = got
    assert idx[0, 0] == 17 and idx[0, 1] == 207 and dist[0, 0] == 0.0 and dist[0, 1] == 0.0
    for q in range(Nq):
        pos = {int(s): i for i, s in enumerate(idx[q])}
        for s in range(10, 30):
            assert pos[s + 190] == pos[s] + 1 and dist[q, pos[s]] == dist[q, pos[s + 190]]


@pytest.mark.parametrize("Nq", NQS)
def test_exclude_nan_inf_and_zero_state_weight(Nq):
    qv, qs, sv, ss, sep = pool(70, 3)
    sv, ss, sep = sv[:257].copy(), ss[:257].copy(), sep[:257].copy()
    sv[5, 69], ss[6, 1], sv[7, 0] = np.nan, np.inf, -np.inf
    exclude = np.full(Nq, -1, dtype=np.int32)
    exclude[0] = 2                                               # episode 2 = rows 74..110
    if Nq > 1:
        exclude[1::2] = 3
    for w in (0.0, 1.5):
        got = run_topk(qv[:Nq], qs[:Nq], sv, ss, 257, w, sep, exclude)
        same(got, ops.knn_topk_ref(qv[:Nq], qs[:Nq], sv, ss, 257, w, sep, exclude))
        idx, dist, n = got
        # (row 6 is out at w = 0 too: 0 * inf is NaN)
        assert not (set(idx[0, :n[0]].tolist()) & ({5, 6, 7} | set(range(74, 111))))
        assert n[0] == 257 - 3 - 37 and np.all(idx[0, n[0]:] == -1) and np.all(np.isinf(dist[0, n[0]:]))
    # every row excluded: nothing is selected
    one = np.zeros(257, dtype=np.int32)
    got = run_topk(qv[:Nq], qs[:Nq], sv, ss, 7, 1.0, one, np.zeros(Nq, dtype=np.int32))
    assert np.all(got[2] == 0) and np.all(got[0] == -1) and np.all(np.isinf(got[1]))
    same(got, ops.knn_topk_ref(qv[:Nq], qs[:Nq], sv, ss, 7, 1.0, one, np.zeros(Nq, dtype=np.int32)))


def test_two_launches_and_both_regimes_give_the_same_bits():
    qv, qs, sv, ss, _ = pool(512, 14)
    a = run_topk(qv, qs, sv, ss, 512, 1.0)
    b = run_topk(qv, qs, sv, ss, 512, 1.0)
    same(a, b)
    one = run_topk(qv[:1], qs[:1], sv, ss, 512, 1.0)             # the single-query form against row 0 of the tiled form
    same(one, tuple(t[:1] for t in a))


def test_more_queries_than_one_workspace_tile():
    """1030 queries: two passes over the workspace (1024 + 6), the second a partial tile"""
    rng = np.random.default_rng(7)
    qv, sv = rng.standard_normal((1030, 3)).astype(np.float32), rng.standard_normal((130, 3)).astype(np.float32)
    same(run_topk(qv, None, sv, None, 7, 0.0), ops.knn_topk_ref(qv, None, sv, None, 7, 0.0))


def test_refusals():
    q, s = torch.zeros((2, 4), device=DEV), torch.zeros((5, 4), device=DEV)
    for K, w in ((0, 1.0), (513, 1.0), (3, -1.0), (3, float("nan")), (3, float("inf"))):
        with pytest.raises(ValueError):
            ops.knn_topk(q, None, s, None, K, w)
    with pytest.raises(ValueError):
        ops.knn_topk(q, None, torch.zeros((5, 3), device=DEV), None, 2)


# ---- predict and ksweep ----------------------------------------------------------------------------------------------------
Q, A = 6, 5


@functools.lru_cache(maxsize=None)
def rows():
    """a store of 4 episodes (11, 1, 7, 30 rows), a support row per stored row with its clamp, and neighbours of 9 queries"""
    rng = np.random.default_rng(21)
    T = [11, 1, 7, 30]
    R = sum(T)
    actions = (rng.standard_normal((R, A)) * 3 + 1).astype(np.float32)
    row0 = np.cumsum([0] + T[:-1])
    off = np.arange(R, dtype=np.int64)
    left = np.concatenate([np.arange(t, 0, -1) for t in T]).astype(np.int32)          # rows remaining from each row
    K = 8
    idx = np.stack([rng.permutation(R)[:K] for _ in range(9)]).astype(np.int32)
    # the clamps of the issue: left in {1, 2, Q, Q + 5} lead the first four queries
    idx[0, 0], idx[1, 0], idx[2, 0], idx[3, 0] = row0[0] + 10, row0[2] + 5, row0[3] + 30 - Q, row0[3] + 30 - Q - 5
    assert [int(left[i]) for i in idx[:4, 0]] == [1, 2, Q, Q + 5]
    dist = np.sort(rng.random((9, K)).astype(np.float32) * 3, axis=1)
    n = np.full(9, K, dtype=np.int32)
    n[4], n[5] = 3, 0                                           # k > n, and no neighbour at all
    idx[4, 3:], dist[4, 3:] = -1, np.inf
    idx[5], dist[5] = -1, np.inf
    dist[6, :2], dist[6, 2:] = (0.0, 80.0), 90.0                # peaked weights
    mean, std = rng.standard_normal(A), rng.random(A) + 0.5
    return actions, off, left, idx, dist, n, mean, std


def close(got, ref, scale):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = np.abs(got - ref)
    bound = 2.0 ** -23 * np.abs(ref) + 1e-12 * scale
    print("max err", err.max(), "max bound ratio", (err / bound).max())
    assert np.all(err <= bound)


@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("k", [1, 2, 8])
def test_predict_matches_float64(k, stats):
    actions, off, left, idx, dist, n, mean, std = rows()
    m, s = (mean, std) if stats else (None, None)
    ref, ref_empty = ops.knn_predict_ref(idx, dist, n, k, actions, off, left, Q, m, s)
    chunk, empty = ops.knn_predict(cu(idx), cu(dist), cu(n), k, cu(actions), cu(off), cu(left), Q, m, s)
    close(chunk.cpu().numpy(), ref, np.abs(ref).max())
    assert int(empty.item()) == ref_empty == 1
    assert np.all(chunk[5].cpu().numpy() == 0)
    if k == 1 and not stats:                                     # one neighbour: its own clamped rows, exactly
        got = chunk.cpu().numpy()
        for q in (0, 1, 2, 3):
            s0 = idx[q, 0]
            want = actions[off[s0] + np.minimum(np.arange(Q), left[s0] - 1)]
            assert np.array_equal(got[q], want)


@pytest.mark.parametrize("stats", [False, True])
def test_ksweep_matches_float64_and_repeats(stats):
    actions, off, left, idx, dist, n, mean, std = rows()
    m, s = (mean, std) if stats else (None, None)
    rng = np.random.default_rng(5)
    target = rng.standard_normal((9, A)).astype(np.float32)
    ref, ref_part = ops.knn_ksweep_ref(idx, dist, n, actions, off, target, m, s, want_partial=True)
    args = (cu(idx), cu(dist), cu(n), cu(actions), cu(off), cu(target), m, s)
    sse, part = ops.knn_ksweep(*args, want_partial=True)
    sse2, part2 = ops.knn_ksweep(*args, want_partial=True)
    assert torch.equal(sse, sse2) and torch.equal(part, part2)
    close(part.cpu().numpy(), ref_part, np.abs(ref_part).max())
    close(sse.cpu().numpy(), ref, np.abs(ref).max())
    # and it is the error of what predict writes at that k, query by query
    for k in (1, 3, 8):
        chunk, _ = ops.knn_predict(cu(idx), cu(dist), cu(n), k, cu(actions), cu(off), cu(left), Q, m, s)
        d = chunk[:, 0].double().cpu().numpy() - target.astype(np.float64)
        assert np.allclose(part[:, k - 1].cpu().numpy(), (d * d).sum(axis=1), rtol=1e-14, atol=0)
