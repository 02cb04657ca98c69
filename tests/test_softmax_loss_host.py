"""Host side of the 1-N softmax loss (no GPU): the workspace-size functions of the C ABI (which ask no device), the chunk plan of the
backward, and the argument errors that are raised before anything touches a device."""
import os
import sys

import pytest
import torch
import yaml

from conftest import PKG
from torch_rgcn import _native, functional
from utils import misc


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("strips", [0, 1, 3, 64])
def test_lse_workspace_bytes(bf16, strips):
    size = _native.lse_workspace_bytes
    Qs = [1, 2, 127, 128, 129, 257, 1_000, 5_000, 20_466, 131_072, 1_000_000]
    Ns = [1, 31, 32, 33, 127, 128, 129, 700, 4_099, 40_943, 1_000_000]
    for d in (1, 24, 200):
        table = [[size(Q, N, d, strips, bf16) for N in Ns] for Q in Qs]
        for qi, Q in enumerate(Qs):
            for ni, N in enumerate(Ns):
                b = table[qi][ni]
                assert b > 0 and b % 16 == 0 and b >= 4 * Q * ((N + 31) // 32), (Q, N, d)
                assert qi == 0 or b >= table[qi - 1][ni], ("Q", Q, N, d)
                assert ni == 0 or b >= table[qi][ni - 1], ("N", Q, N, d)
                # the layout is the fused evaluator's: an (m, l) float pair where it keeps a (greater, equal) pair
                assert b == _native.rank_fused_workspace_bytes(Q, N, d, strips, bf16)
    # refused arguments
    assert size(-1, 10, 8, 0, bf16) == 0 and size(10, 0, 8, 0, bf16) == 0 and size(10, 10, 0, 0, bf16) == 0 and size(10, 10, 8, -1, bf16) == 0


def test_gradient_workspace_bytes():
    def size(Q, c_count, d):
        return _native.lib().rgcn_distmult_softmax_grad_workspace_bytes(Q, c_count, d, 0)

    assert size(-1, 128, 8) == 0 and size(10, 0, 8) == 0 and size(10, 128, 0) == 0
    prev = 0
    for c_count in (1, 32, 33, 128, 1_000, 40_943):
        b = size(5_000, c_count, 200)
        assert b % 16 == 0 and b >= 5_000 * 200 * 4 + 4 * 5_000 * ((c_count + 31) // 32) and b >= prev
        prev = b
    # the mask of a chunk, not of the whole table: a 128-column chunk of a million entities costs what it costs at 128 entities
    assert size(5_000, 128, 200) < 5 * 2 ** 20


def check_plan(Q, N, budget):
    plan = functional.softmax_chunk_plan(Q, N, budget)
    assert plan[0][0] == 0 and sum(c for _, c in plan) == N
    for (a, ca), (b, _) in zip(plan, plan[1:]):
        assert a + ca == b                                                  # no gap, no overlap
    for first, count in plan:
        assert first % 128 == 0 and count >= 1
    for first, count in plan[:-1]:
        assert count % 128 == 0 and count == plan[0][1]                     # only the last chunk is ragged
    assert plan[-1][1] <= plan[0][1]
    if len(plan) > 1:
        for first, count in plan:
            assert 4 * Q * count <= budget or count <= 128                  # the budget, down to one tile column
    return plan


def test_chunk_plan():
    assert functional.SOFTMAX_CHUNK_BYTES == misc._SCORE_BYTES
    for Q in (1, 3, 129, 130, 5_000, 30_000):
        for N in (1, 127, 128, 129, 700, 40_943, 1_000_000):
            for budget in (1, 4 * Q * 128, 4 * Q * 128 + 1, 4 * Q * 256 - 1, 4 * Q * N - 1, 4 * Q * N, 1 << 30):
                plan = check_plan(Q, N, budget)
                if 4 * Q * N <= budget:
                    assert plan == [(0, N)]                                 # the matrix fits: one chunk
    assert functional.softmax_chunk_plan(130, 700, 4 * 130 * 256) == [(0, 256), (256, 256), (512, 188)]
    assert [c for _, c in functional.softmax_chunk_plan(130, 700, 1)] == [128] * 5 + [60]
    # WN18 size, 5,000 queries: the 819 MB matrix fits the default budget; a million entities take 19 chunks of up to 53,632 columns
    assert functional.softmax_chunk_plan(5_000, 40_943, functional.SOFTMAX_CHUNK_BYTES) == [(0, 40_943)]
    big = functional.softmax_chunk_plan(5_000, 1_000_000, functional.SOFTMAX_CHUNK_BYTES)
    assert big[0] == (0, 53_632) and len(big) == 19 and 4 * 5_000 * 53_632 <= 1 << 30


def test_argument_errors_come_before_any_device_work():
    batch = torch.tensor([[0, 1, 2]])
    nodes, rel = torch.randn(4, 8), torch.randn(3, 8)
    for reduction in ("sum", "batchmean", None, ""):
        with pytest.raises(ValueError, match="reduction"):
            functional.distmult_softmax_loss(batch, False, nodes, rel, reduction=reduction)
    with pytest.raises(RuntimeError, match="no CPU fallback"):               # and a valid reduction gets as far as the device check
        functional.distmult_softmax_loss(batch, False, nodes, rel, reduction="none")
    from torch_rgcn.layers import DistMult
    assert callable(DistMult.softmax_loss)


def test_unknown_training_objective_is_refused():
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n.yaml")))
    assert cfg["training"]["objective"] == "1-n"
    plain = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18.yaml")))
    assert "objective" not in plain["training"]
    del cfg["training"]["objective"]
    assert cfg == plain                                                     # the WN18 configuration with that one key
    cfg["training"]["objective"] = "softmax"
    with pytest.raises(NotImplementedError, match="objective"):
        predict_links.run(cfg, epochs=1, quiet=True, synthetic=True)
