"""End-to-end: experiments/predict_links.py on configs/rgcn/lp-WN18-1n-bce.yaml -- the K-vs-All binary cross-entropy with label
smoothing 0.1, its positive labels looked up in a device-resident index of the training triples -- on the small synthetic graph of
test_gpu_experiments_1n.py: the step is captured by default like the 1-N softmax one, and it is another objective than that one.

The pattern and the sizes are those of test_gpu_experiments_1n_smoothed.py: whole-graph epochs with edge dropout off, so no run draws a
random number after the model is initialised, and what is left between a captured and an eager run are the unordered fp32 sums of the
step.  One bound separates "the same run" from "another loss": 100 fp32 ulps, 100 * 2^-23 = 1.2e-5 relative.  The captured and the eager
run must agree within it in every epoch; against the 1-N softmax run (lp-WN18-1n.yaml) the last epoch's loss must differ by more.
Recorded on an MI355X, epochs 1 to 6: captured against eager 0 / 0 / 8.5e-8 / 1.7e-7 / 3.5e-7 / 4.4e-7 (the bound is 1.2e-5); BCE
against softmax 0.875 / 0.875 / 0.876 / 0.876 / 0.878 / 0.881 -- the BCE loss starts at log 2 = 0.70 per cell (0.7035, falling to 0.6720),
the softmax loss at log N (5.645, falling to 5.628): two objectives, seventy thousand times the bound apart."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import PKG
import torch_rgcn  # noqa: F401  (at collection, before the first HIP call: the captured step is the default only then, torch_rgcn/__init__.py)

pytestmark = pytest.mark.gpu

BOUND = 100 * 2.0 ** -23
EPOCHS = 6


@pytest.fixture(autouse=True)
def _random_streams_left_as_found():
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])
    np.random.set_state(state[3])


def small(name, **training):
    c = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", name)))
    c["dataset"]["name"] = "fb-toy"
    c["encoder"].update(node_embedding=32, hidden1_size=32)
    c["encoder"]["edge_dropout"].update(general=0.0, self_loop=0.0)
    c["training"].update(graph_batch_size=None, **training)                   # the whole graph: nothing is sampled
    c["evaluation"].update(check_every=20, batch_size=32, verbose=False)
    return c


def losses(cfg, hipgraph, monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    replays = []
    orig = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), orig(self))[1])
    torch.manual_seed(0)
    random.seed(0)
    hist, metrics = predict_links.run(cfg, epochs=EPOCHS, quiet=True, max_test=20, synthetic=True, hipgraph=hipgraph)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", orig)
    assert len(hist) == EPOCHS and all(np.isfinite(hist)) and np.isfinite(metrics["mrr"]) and 0.0 < metrics["mrr"] <= 1.0
    return hist, len(replays)


def test_the_bce_step_is_captured_and_is_another_objective(monkeypatch):
    captured, replays = losses(small("lp-WN18-1n-bce.yaml"), None, monkeypatch)
    assert replays == EPOCHS                                                    # captured by default, exactly as the 1-N softmax step is
    eager, replays = losses(small("lp-WN18-1n-bce.yaml"), False, monkeypatch)
    assert replays == 0
    softmax, replays = losses(small("lp-WN18-1n.yaml"), None, monkeypatch)
    assert replays == EPOCHS
    print(f"[1-n bce] captured {captured}\n[1-n bce] eager    {eager}\n[1-n bce] softmax  {softmax}")
    for k in range(EPOCHS):
        print(f"[1-n bce] epoch {k + 1}: captured vs eager {abs(captured[k] - eager[k]) / abs(eager[k]):.3e}, "
              f"bce vs softmax {abs(captured[k] - softmax[k]) / abs(softmax[k]):.3e}")
    for k in range(EPOCHS):
        assert abs(captured[k] - eager[k]) <= BOUND * abs(eager[k]), (k, captured, eager)
    last = EPOCHS - 1
    assert abs(captured[last] - softmax[last]) > BOUND * abs(softmax[last]), (captured, softmax)


def test_bf16_and_the_bce_objective_together_are_captured(monkeypatch):
    both, replays = losses(small("lp-WN18-1n-bce.yaml", bf16=True), None, monkeypatch)
    assert replays == EPOCHS and all(np.isfinite(both))
    print(f"[1-n bce] bf16 {both}")
