"""End-to-end: experiments/predict_links.py on configs/rgcn/lp-WN18-1n-filtered.yaml -- the 1-N softmax loss with the other known
completions of every query (training triples only) left out, looked up in a device-resident FilterIndex -- on the small synthetic graph
of test_gpu_experiments_1n.py: the filtered step is captured like the unfiltered one, and the filter is really applied.

The runs compared here train on the whole graph every epoch with edge dropout off, so no run draws a random number after the model is
initialised (the captured run samples once more and runs warm-up steps before its first epoch: with sampling or dropout on, the two
loops would see different draws).  What is left between a captured and an eager run are the unordered fp32 sums of the step (the
atomics of the weight gradients), which move a loss in its last bits (test_gpu_experiments_1n.py records 1e-7 relative, one ulp, over 30
epochs).  One bound separates "the same run" from "another loss": 100 fp32 ulps, 100 * 2^-23 = 1.2e-5 relative -- two orders of
magnitude above any reordering of fp32 sums, and an order below what the filter must do on this graph: its 4,565 triples fall on 31,360
(s, p) cells, about one query in seven has another known completion, and taking one of 280 candidates out of such a denominator moves
the mean loss (5.6 = log 280 at the start) by about (1 / 7) (1 / 280) / 5.6 = 9e-5 relative.  The captured and the eager run must agree
within the bound in every epoch; the unfiltered run must be beyond it in every epoch, and above the filtered one in the first, where the
parameters are the same and the filtered denominators have fewer terms.  Recorded on an MI355X: captured against eager 0 / 8.4e-8 / 0,
filtered against unfiltered 9.79e-5 / 9.81e-5 / 9.82e-5."""
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
EPOCHS = 3


@pytest.fixture(autouse=True)
def _random_streams_left_as_found():
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])
    np.random.set_state(state[3])


def small(name):
    c = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", name)))
    c["dataset"]["name"] = "fb-toy"
    c["encoder"].update(node_embedding=32, hidden1_size=32)
    c["encoder"]["edge_dropout"].update(general=0.0, self_loop=0.0)
    c["training"].update(graph_batch_size=None)                               # the whole graph: nothing is sampled
    c["evaluation"].update(check_every=20, batch_size=32, verbose=False)
    return c


def losses(name, hipgraph, monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    replays = []
    orig = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), orig(self))[1])
    torch.manual_seed(0)
    random.seed(0)
    hist, metrics = predict_links.run(small(name), epochs=EPOCHS, quiet=True, max_test=20, synthetic=True, hipgraph=hipgraph)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", orig)
    assert len(hist) == EPOCHS and all(np.isfinite(hist)) and 0.0 < metrics["mrr"] <= 1.0
    return hist, len(replays)


def test_the_filtered_step_is_captured_and_the_filter_is_applied(monkeypatch):
    captured, replays = losses("lp-WN18-1n-filtered.yaml", None, monkeypatch)
    assert replays == EPOCHS                                                    # captured by default, exactly as the unfiltered step is
    eager, replays = losses("lp-WN18-1n-filtered.yaml", False, monkeypatch)
    assert replays == 0
    unfiltered, replays = losses("lp-WN18-1n.yaml", None, monkeypatch)
    assert replays == EPOCHS
    print(f"[1-n filtered] captured {captured}\n[1-n filtered] eager    {eager}\n[1-n filtered] unfiltered {unfiltered}")
    for k in range(EPOCHS):
        print(f"[1-n filtered] epoch {k + 1}: captured vs eager {abs(captured[k] - eager[k]) / abs(eager[k]):.3e}, "
              f"filtered vs unfiltered {abs(captured[k] - unfiltered[k]) / abs(unfiltered[k]):.3e}")
    for k in range(EPOCHS):
        assert abs(captured[k] - eager[k]) <= BOUND * abs(eager[k]), (k, captured, eager)
        if k == 0:                                                              # the same parameters, fewer terms in the denominators
            assert captured[k] < unfiltered[k], (k, captured, unfiltered)
        assert abs(captured[k] - unfiltered[k]) > BOUND * abs(unfiltered[k]), (k, captured, unfiltered)
