"""End-to-end: experiments/predict_links.py with training.objective = "1-n" and training.bf16 = true -- the model in bf16 and both terms of
the 1-N softmax loss on the native bf16 backward -- on the small synthetic graph of test_gpu_experiments_1n.py, captured by default and
eager."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import PKG
import torch_rgcn  # noqa: F401  (at collection, before the first HIP call: the captured step is the default only then, torch_rgcn/__init__.py)
from test_gpu_experiments_1n import _random_streams_left_as_found, small_wn18  # noqa: F401

pytestmark = pytest.mark.gpu


def small_wn18_bf16():
    c = small_wn18("1-n")
    c["training"]["bf16"] = True
    return c


@pytest.mark.parametrize("hipgraph", [None, False])
def test_predict_links_one_to_n_in_bf16_trains_and_ranks(hipgraph, monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    replays = []
    orig = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), orig(self))[1])
    torch.manual_seed(0)
    hist, metrics = predict_links.run(small_wn18_bf16(), epochs=30, quiet=True, max_test=100, synthetic=True, hipgraph=hipgraph)
    assert len(hist) == 30 and all(np.isfinite(hist)), hist
    assert hist[-1] < hist[0], hist
    assert 0.0 < metrics["mrr"] <= 1.0
    assert len(replays) == (30 if hipgraph is None else 0)                  # static shapes: the default captured step works in bf16 too


def test_an_eager_epoch_runs_the_bf16_gradient_cell_kernel(monkeypatch):
    """one eager epoch under the profiler: both loss terms take the native route (softmax_grad_bf16), none the fp32 gradient-cell kernel"""
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    from torch_rgcn import _native
    torch.manual_seed(0)
    _native.profile_start()
    try:
        hist, _ = predict_links.run(small_wn18_bf16(), epochs=1, quiet=True, max_test=10, synthetic=True, hipgraph=False)
    finally:
        tags = _native.profile_stop()
    assert len(hist) == 1 and np.isfinite(hist[0])
    assert len(tags.get("softmax_grad_bf16", ())) >= 2 and "lse_fused_bf16" in tags, sorted(tags)
    assert "softmax_grad" not in tags and "lse_fused" not in tags, sorted(tags)
