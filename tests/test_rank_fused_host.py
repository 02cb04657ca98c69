"""Host side of the fused ranking evaluator (no GPU): the rule that picks the route, the workspace-size function of the C ABI (which asks
no device), and the `fused` argument of utils.misc.evaluate."""
import inspect

import pytest

from torch_rgcn import _native
from utils import misc


def test_default_route_is_fused_exactly_when_the_score_matrix_needs_a_second_chunk(monkeypatch):
    assert misc._SCORE_BYTES == 1 << 30
    Q = N = 1 << 14                                                      # Q * N * 4 == 2^30 exactly: one chunk still holds it
    assert misc.use_fused(Q, N) is False and misc.use_fused(Q, N, None) is False
    assert misc.use_fused(Q + 1, N) is True and misc.use_fused(Q, N + 1) is True
    size = Q * N * 4
    for budget, want in ((size - 1, True), (size, False), (size + 1, False)):        # one byte under / at / one byte over
        monkeypatch.setattr(misc, "_SCORE_BYTES", budget)
        assert misc.use_fused(Q, N) is want, budget
    monkeypatch.setattr(misc, "_SCORE_BYTES", 1 << 30)
    # the overrides win on both sides of the boundary
    for q, n in ((1, 1), (Q, N), (Q + 1, N), (10_000, 1_000_000)):
        assert misc.use_fused(q, n, True) is True and misc.use_fused(q, n, False) is False
    # the sizes on record: the largest evaluate() call of the suite, WN18 and FB15k-237 test sets, a million entities
    assert misc.use_fused(2_000, 40_943) is False and misc.use_fused(5_000, 40_943) is False
    assert misc.use_fused(20_466, 14_541) is True and misc.use_fused(10_000, 1_000_000) is True


def test_fused_batch_is_bounded_by_the_workspace_not_the_score_matrix(monkeypatch):
    assert misc._fused_batch(300, 4_099, 24) == 300
    monkeypatch.setattr(misc, "_SCORE_BYTES", 64 * 1024)                 # the score budget does not enter
    assert misc._fused_batch(300, 4_099, 24) == 300
    q = misc._fused_batch(10_000, 1_000_000, 200)                        # 268 queries per chunk on the materialised route
    assert q > 8_000
    for bf16 in (False, True):
        assert _native.rank_fused_workspace_bytes(q, 1_000_000, 200, 0, bf16) <= misc._FUSED_BYTES
    assert misc._fused_batch(10, 10 ** 9, 200) == 10 and misc._fused_batch(1_000, 10 ** 10, 200) == 64


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("strips", [0, 1, 3, 64])
def test_workspace_bytes_grow_with_q_and_n_and_hold_the_mask(bf16, strips):
    size = _native.rank_fused_workspace_bytes
    Qs = [1, 2, 127, 128, 129, 255, 256, 257, 1_000, 5_000, 20_466, 131_072, 1_000_000]
    Ns = [1, 31, 32, 33, 127, 128, 129, 700, 4_099, 40_943, 1_000_000]
    for d in (1, 24, 200):
        table = [[size(Q, N, d, strips, bf16) for N in Ns] for Q in Qs]
        for qi, Q in enumerate(Qs):
            for ni, N in enumerate(Ns):
                b = table[qi][ni]
                assert b % 16 == 0 and b >= 4 * Q * ((N + 31) // 32), (Q, N, d)
                assert qi == 0 or b >= table[qi - 1][ni], ("Q", Q, N, d)
                assert ni == 0 or b >= table[qi][ni - 1], ("N", Q, N, d)
    # the mask dominates at evaluation sizes: WN18's 5,000 queries stay near 26 MB (the score matrix: 819 MB)
    assert size(5_000, 40_943, 200, 0, bf16) < 40 * 2 ** 20
    assert size(0, 10, 8, 0, bf16) >= 0 and size(10, 0, 8, 0, bf16) == 0 and size(10, 10, 8, -1, bf16) == 0


def test_evaluate_accepts_fused():
    p = inspect.signature(misc.evaluate).parameters
    assert "fused" in p and p["fused"].default is None
    assert list(p)[:9] == ["model", "graph", "test_set", "true_triples", "num_nodes", "batch_size", "hits_at_k", "filter_candidates",
                           "verbose"]                                    # the reference's arguments, in its order, come first
