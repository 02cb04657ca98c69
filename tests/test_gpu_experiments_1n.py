"""End-to-end: experiments/predict_links.py with training.objective = "1-n" (the 1-N softmax loss, an extension) on the small synthetic graph
of test_gpu_experiments.py::test_predict_links_small_graph_trains_and_ranks, captured by default and eager; and the default objective,
which must stay the step it was."""
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


@pytest.fixture(autouse=True)
def _random_streams_left_as_found():
    """the tests of this file seed and draw from the global generators: put them back, so that the files that run after this one see the
    streams they saw before it existed"""
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])
    np.random.set_state(state[3])


def small_wn18(objective=None):
    c = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18.yaml")))
    c["dataset"]["name"] = "fb-toy"
    c["encoder"].update(node_embedding=32, hidden1_size=32)
    c["training"].update(graph_batch_size=2000)
    c["evaluation"].update(check_every=20, batch_size=32, verbose=False)
    if objective is not None:
        c["training"]["objective"] = objective
    return c


@pytest.mark.parametrize("hipgraph", [None, False])
def test_predict_links_one_to_n_trains_and_ranks(hipgraph, monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    replays = []
    orig = torch.cuda.CUDAGraph.replay
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", lambda self: (replays.append(1), orig(self))[1])
    torch.manual_seed(0)
    hist, metrics = predict_links.run(small_wn18("1-n"), epochs=30, quiet=True, max_test=100, synthetic=True, hipgraph=hipgraph)
    assert len(hist) == 30 and all(np.isfinite(hist)), hist
    assert hist[-1] < hist[0], hist
    assert 0.0 < metrics["mrr"] <= 1.0
    assert len(replays) == (30 if hipgraph is None else 0)                  # static shapes: the default captured step works


# The default objective before `training.objective` existed: the losses of small_wn18() (no key), 30 epochs, eager, from
# torch.manual_seed(0) and random.seed(0), recorded once on an MI355X from the commit before the key was added.  Three runs of that
# commit agreed to 1e-7 relative in every epoch (one fp32 ulp of the loss: the fp32 atomics of the weight gradients), so 1e-4 -- the
# suite's parity bound, a thousand times that drift -- separates "the same step" from another order of random draws, other labels or
# another penalty batch, which move the sampled batches and with them every epoch's loss in the third digit.
DEFAULT_OBJECTIVE_LOSSES = (
    0.7034487, 0.7032898, 0.7028595, 0.7023370, 0.7013342, 0.6999140,
    0.6957214, 0.6904432, 0.6821336, 0.6755365, 0.6771953, 0.6698494,
    0.6611282, 0.6445059, 0.6484658, 0.6367614, 0.6348449, 0.6178558,
    0.6046553, 0.6012774, 0.5829609, 0.5736387, 0.5663867, 0.5520253,
    0.5361628, 0.5293183, 0.5134413, 0.4983699, 0.4935728, 0.4788782)


def default_objective_run(objective):
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    torch.manual_seed(0)
    random.seed(0)                                                          # the edge-neighbourhood sampler draws its seed from `random`
    hist, _ = predict_links.run(small_wn18(objective), epochs=30, quiet=True, max_test=100, synthetic=True, hipgraph=False)
    return hist


@pytest.mark.parametrize("objective", [None, "negative-sampling"])
def test_the_default_objective_is_the_step_it_was(objective):
    """without the key -- and with it spelled out -- the run produces the losses it produced before the key existed, epoch by epoch"""
    hist = default_objective_run(objective)
    assert len(hist) == len(DEFAULT_OBJECTIVE_LOSSES) == 30
    worst = max(abs(x - y) / abs(y) for x, y in zip(hist, DEFAULT_OBJECTIVE_LOSSES))
    print(f"[1-n] default objective ({objective}): largest relative distance from the recorded losses {worst:.3e}")
    for k, (x, y) in enumerate(zip(hist, DEFAULT_OBJECTIVE_LOSSES)):
        assert abs(x - y) <= 1e-4 * abs(y), (k, x, y, hist)
