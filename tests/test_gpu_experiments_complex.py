"""End-to-end with decoder.model: complex.  experiments/predict_links.py on configs/rgcn/lp-WN18-1n-complex.yaml, on the pattern and the
sizes of test_gpu_experiments_1n_bce.py (the small synthetic graph, width 32 = 16 complex features, dropout off, 6 whole-graph epochs):
the step is captured by default, the captured and the eager run agree within that file's bound of 100 fp32 ulps in every epoch, and the
run is another objective than the DistMult one (lp-WN18-1n.yaml): the last epoch's loss differs by more than the bound.  One run of
configs/rgcn/lp-WN18-complex.yaml (the reference's sampled-negative objective on the ComplEx triple kernels), eager and captured.  And
utils.misc.evaluate / predict on a stub model whose decoder is a ComplEx with integer-valued parameters: the ranks and the top-k of the
float64 complex-tensor reference, on every route."""
import os
import random
import sys

import numpy as np
import pytest
import torch
import yaml

from conftest import PKG
import torch_rgcn  # noqa: F401  (at collection, before the first HIP call: the captured step is the default only then, torch_rgcn/__init__.py)

import complex_reference as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
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


def small(name, whole_graph=True, **training):
    c = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", name)))
    c["dataset"]["name"] = "fb-toy"
    c["encoder"].update(node_embedding=32, hidden1_size=32)
    c["encoder"]["edge_dropout"].update(general=0.0, self_loop=0.0)
    c["training"].update(graph_batch_size=None if whole_graph else 2000, **training)
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


def test_the_complex_1n_step_is_captured_and_is_another_objective(monkeypatch):
    captured, replays = losses(small("lp-WN18-1n-complex.yaml"), None, monkeypatch)
    assert replays == EPOCHS                                                    # captured by default, exactly as the DistMult step is
    eager, replays = losses(small("lp-WN18-1n-complex.yaml"), False, monkeypatch)
    assert replays == 0
    distmult, replays = losses(small("lp-WN18-1n.yaml"), None, monkeypatch)
    assert replays == EPOCHS
    print(f"[1-n complex] captured {captured}\n[1-n complex] eager    {eager}\n[1-n complex] distmult {distmult}")
    for k in range(EPOCHS):
        print(f"[1-n complex] epoch {k + 1}: captured vs eager {abs(captured[k] - eager[k]) / abs(eager[k]):.3e}, "
              f"complex vs distmult {abs(captured[k] - distmult[k]) / abs(distmult[k]):.3e}")
    for k in range(EPOCHS):
        assert abs(captured[k] - eager[k]) <= BOUND * abs(eager[k]), (k, captured, eager)
    last = EPOCHS - 1
    assert abs(captured[last] - distmult[last]) > BOUND * abs(distmult[last]), (captured, distmult)


def test_the_sampled_negative_objective_runs_on_the_complex_triple_kernels(monkeypatch):
    from torch_rgcn import _native
    for hipgraph in (False, None):
        _native.profile_start()
        hist, replays = losses(small("lp-WN18-complex.yaml", whole_graph=False), hipgraph, monkeypatch)
        tags = set(_native.profile_stop())
        assert replays == (0 if hipgraph is False else EPOCHS)
        print(f"[complex] sampled negatives, hipgraph={hipgraph}: {hist}")
        if hipgraph is False:                                                   # (a captured step is timed as a whole: no per-launch tags)
            assert {"complex_fwd", "complex_bwd_nodes", "complex_bwd_rel"} <= tags and not any(t.startswith("distmult_fwd") for t in tags), tags


# ----------------------------------------------------------------------------- evaluate / predict on a stub model
class _Model(torch.nn.Module):
    """encoder + decoder pair with the attribute names utils.misc looks for (as in test_gpu_topk.py): encode returns a fixed table"""

    def __init__(self, decoder, nodes):
        super().__init__()
        self.scoring_function, self.nodes = decoder, nodes

    def encode(self, graph):
        return self.nodes

    def forward(self, graph, triples):
        return self.scoring_function(triples, self.encode(graph)), 0


def test_evaluate_and_predict_on_a_complex_decoder():
    from torch_rgcn.layers import ComplEx
    from utils import misc
    N, Q, d = 63, 65, 6
    rng, nodes, rel, bias, test = cr.make_case(N, Q, d, True, integer=True, seed=5)
    more = test[rng.integers(0, Q, 3 * Q)].copy()
    more[: len(more) // 2, 0] = rng.integers(0, N, len(more) // 2)
    more[len(more) // 2:, 2] = rng.integers(0, N, len(more) - len(more) // 2)
    true = misc.generate_true_dict(np.concatenate([test, more]))
    dec = ComplEx(cr.R0, d, N, cr.R0, b_init="zeros").to(DEV)
    with torch.no_grad():
        dec.relations.copy_(torch.from_numpy(rel))
        for p, b in zip((dec.sbias, dec.pbias, dec.obias), bias):
            p.copy_(torch.from_numpy(b))
    model = _Model(dec, torch.from_numpy(nodes).to(DEV))
    n, r, b = cr.f64(nodes), cr.f64(rel), [cr.f64(x) for x in bias]
    want_ranks, want_top = [], {}
    for head in (True, False):
        s = cr.all_scores(test, head, n, r, b)
        rows, cols = misc._FilterIndex(true, N).lists(test, head)
        f = s.clone()
        f[torch.from_numpy(rows.astype(np.int64)), torch.from_numpy(cols.astype(np.int64))] = -np.inf
        t = f[torch.arange(Q), torch.from_numpy(test[:, 0 if head else 2])][:, None]
        want_ranks += ((f > t).sum(1) + ((f == t).sum(1) - 1) // 2 + 1).tolist()
        order = np.lexsort((np.broadcast_to(np.arange(N), (Q, N)), -s.numpy()), axis=1)[:, :10]
        want_top[head] = (order, np.take_along_axis(s.numpy(), order, 1))
    for kw in (dict(fused=True), dict(fused=False), dict(fused=True, device_filter=True), dict(fused=False, device_filter=True)):
        mrr, hits, ranks = misc.evaluate(model, None, test, true, N, verbose=False, **kw)
        assert ranks == want_ranks, kw
        assert mrr == sum(1.0 / x for x in want_ranks) / len(want_ranks)
    for head in (True, False):
        for fused in (None, False):
            ids, vals = misc.predict(model, None, test, N, k=10, head=head, fused=fused)
            assert np.array_equal(ids.cpu().numpy(), want_top[head][0]), (head, fused)
            assert np.array_equal(vals.cpu().numpy().astype(np.float64), want_top[head][1]), (head, fused)
