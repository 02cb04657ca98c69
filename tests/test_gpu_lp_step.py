"""The link-prediction training step as ONE computation -- node_embeddings + bias -> ReLU -> LP layer(s) on a per-step graph -> decoder ->
objective -> penalty -> backward into every parameter -- against the float64 reference of tests/lp_step_reference.py.  Each case builds
LinkPredictor / CompressionRelationPredictor from a config, overwrites every parameter with seeded values (biases nonzero), calls
experiments/predict_links.py::step_loss once and loss.backward(gradient=unit_gradient(...)) as train_step does, and compares the loss and
the .grad of EVERY entry of model.named_parameters() (none may be None, the compared names are exactly the model's).

Shapes: 300 entities, 4 relations, a message graph of 1,500 triples (node 0 the subject of a quarter, 5 % duplicates), 130 positives (a
second 128-query tile of two rows, a third 128-column tile of 44 columns), 3 sampled negatives per positive; the known triples of the
FilterIndex are the message graph's.  The cases (lp_step_reference.CASES; "b": decoder biases; N: layers; width; mode):

    objective                    penalty (0.01)    decoder     encoder                   mode     storage
    negative-sampling            schlichtkrull-l2  DistMult b  rgcn none 2 x 16          eval     fp32
    negative-sampling            plain             ComplEx     rgcn basis(2) 2 x 50      sd       fp32
    negative-sampling            l2_penalty 0      DistMult    rgcn block(4) 2 x 32      other    fp32
    negative-sampling            schlichtkrull-l2  ComplEx b   c-rgcn none 2 x 16 / 50   eval     fp32
    1-n                          schlichtkrull-l2  DistMult    rgcn none 1 x 50          eval     fp32
    1-n filtered                 schlichtkrull-l2  ComplEx b   rgcn basis(2) 2 x 16      other    fp32
    1-n filtered, smoothing 0.1  plain             DistMult b  rgcn block(4) 2 x 32      eval     fp32
    1-n filtered, smoothing 0.1  schlichtkrull-l2  ComplEx     c-rgcn none 1 x 16 / 50   other    fp32
    1-n-bce eps 0                schlichtkrull-l2  DistMult b  rgcn basis(2) 1 x 50      eval     fp32
    1-n-bce eps 0.1              schlichtkrull-l2  ComplEx     rgcn block(4) 2 x 32      other    fp32
    1-n-bce eps 0.1              plain             DistMult    c-rgcn none 2 x 16 / 50   eval     fp32
    1-n-bce eps 0                l2_penalty 0      ComplEx b   rgcn none 2 x 16          eval     fp32
    1-n                          schlichtkrull-l2  DistMult b  rgcn none 1 x 16          eval     bf16, bf16_backward native
    1-n filtered, smoothing 0.1  schlichtkrull-l2  ComplEx     rgcn basis(2) 1 x 50      eval     bf16, bf16_backward native
    1-n-bce eps 0.1              schlichtkrull-l2  DistMult b  rgcn block(4) 1 x 32      eval     bf16, bf16_backward native

mode: eval = model.eval(); other = model.train() with self_loop_type "other", self_loop 0.2 -- the keep masks of layer 1 and layer 2 are
replayed with torch.manual_seed + torch.bernoulli in the order the model draws them (and must equal the recorded masks under which the
host test checked the ReLU condition); sd = model.train() with the shipped schlichtkrull-dropout on a basis encoder, which keeps every
loop.  Out of scope: block decomposition with schlichtkrull-dropout and self_loop > 0 calls F.dropout on the self-loop messages, whose
mask cannot be replayed.  The bf16 cases have one layer: see the comment in lp_step_reference._cases.

Bounds.  fp32: the suite's parity bound, max |got - want| < 1e-4 max |want| per tensor and for the loss.  pbias under the softmax objective
is zero in exact arithmetic (both terms' gradient cells sum to zero over a row): the GPU is within 1e-4 of the candidate-side norm
(sbias / obias), the reference within 1e-9 of it -- the rule of check_loss in test_gpu_complex_all.py.  A ReLU input may not change sign:
tests/test_lp_step_reference_host.py asserts, for every case, that in the reference all of them are farther from zero than 1e-5 of their
tensor's maximum (bf16: one bf16 ulp of it, on the rounded evaluation).

bf16: 2^-8 per tensor and for the loss against the rounded float64 evaluation; no tensor has another bound.  "Rounded" is everything
DESIGN.md 4.6 rounds: the activations (the embedding ReLU's input sum, each layer's output) AND the gradients it names -- a layer's dX,
each loss term's dnodes, every parameter gradient returned in the parameter's dtype -- with the bf16 sums autograd forms where a bf16
tensor has several readers.  Measured first against the evaluation that rounds the activations alone: two cases missed 2^-8 there
(node_embeddings_bias 5.75e-3 and rgc1.bases 5.62e-3 in bf16-1n-filt-smooth-complex-basis1-50, sbias 4.78e-3 in
bf16-bce-smooth-distmult-b-block1-32), with the activations' rounding itself moving those tensors by 6.94e-3, 6.87e-3 and 4.03e-3 -- not
within a quarter of that, so not a matter of where an activation rounds.  The float64 evaluation with the gradient roundings added lies
at 5.8e-3, 5.6e-3 and 4.8e-3 from the activations-only one in those same tensors, and the GPU within 1.2e-3 of it in every tensor (most
parameter gradients bit for bit): the excess IS the gradient rounding of 4.6 -- sbias sums two terms, each rounded, in bf16 -- and the
bound stays 2^-8.  Each bf16 case still prints its distance from the activations-only evaluation, and that one's from no rounding.

Largest relative distance observed on an MI355X over the loss and every gradient, per objective: negative-sampling 3.0e-6, 1-n 2.5e-6,
1-n-bce 1.5e-6 (fp32, bound 1e-4); bf16 against the rounded evaluation: 1-n 5.8e-4, 1-n-bce 1.2e-3 (bound 2^-8 = 3.9e-3).

test_s_penalty_scales_nodes_and_relations_apart is the one place where the two scales of s_penalty differ.  Every case prints the
profile tags that ran (none is asserted as a route) and its distances."""
import os
import random
import sys

import numpy as np
import pytest
import torch

import lp_step_reference as ref
from conftest import PKG

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOUND, BF_BOUND = 1e-4, 2.0 ** -8
_REFS = {}


@pytest.fixture(autouse=True)
def _random_streams_left_as_found():
    """the cases seed the global torch generators (the keep masks are replayed from them): put them back"""
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])
    np.random.set_state(state[3])


def reference(name, keeps):
    """the float64 loss and gradients of a case, computed once and never written: bf16 cases the rounded evaluation, and beside it the
    one that rounds the activations alone and the unrounded one"""
    if name not in _REFS:
        case = ref.CASES[name]
        inp = ref.case_inputs(case)
        bf16 = case["storage"] == "bf16"
        others = [ref.loss_and_grads(case, inp, keeps, rounded=r) for r in ("activations", False)] if bf16 else None
        _REFS[name] = (ref.loss_and_grads(case, inp, keeps, rounded=bf16), others)
    return _REFS[name]


def build_model(case, inp):
    from torch_rgcn.models import CompressionRelationPredictor, LinkPredictor
    kind = CompressionRelationPredictor if case["encoder"]["model"] == "c-rgcn" else LinkPredictor
    model = kind(nnodes=ref.N, nrel=ref.R0, encoder_config=case["encoder"], decoder_config=case["decoder"]).to(DEV)
    named = dict(model.named_parameters())
    assert set(named) == set(inp["params"]), sorted(set(named) ^ set(inp["params"]))
    with torch.no_grad():
        for k, p in named.items():
            assert tuple(p.shape) == inp["params"][k].shape, k
            p.copy_(torch.from_numpy(inp["params"][k]).to(p.dtype))
    model.train(case["mode"] != "eval")
    return model.bfloat16() if case["storage"] == "bf16" else model


def run_step(case, inp, model):
    """the step as predict_links.run() sets it up and train_step runs it -> (loss, profile tags, replayed keep masks)"""
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex, unit_gradient
    from utils.misc import generate_true_dict
    bce = case["objective"] == "1-n-bce"
    train_filter = FilterIndex(generate_true_dict(inp["graph"]), ref.N, torch.device(DEV)) if case["filtered"] or bce else None
    loss_kw = {"bf16_backward": "native"} if case["storage"] == "bf16" else {}
    if case["eps"]:
        loss_kw["label_smoothing"] = case["eps"]
    graph = torch.from_numpy(inp["graph"]).to(DEV)
    batch_idx = torch.from_numpy(inp["batch"]).to(DEV)
    train_lbl = torch.empty(0, device=DEV) if inp["labels"] is None else torch.from_numpy(inp["labels"]).float().to(DEV)
    torch.manual_seed(case["mask_seed"])
    _native.profile_start()
    loss = predict_links.step_loss(model, graph, batch_idx, train_lbl, case["objective"], train_filter, loss_kw, case["decoder"]["l2_penalty"])
    loss.backward(gradient=unit_gradient(loss.device))
    tags = sorted(_native.profile_stop())
    keeps = (None, None)
    if case["mode"] == "other":       # the draws of layer 1 and layer 2, in the model's order, from the same seed
        torch.manual_seed(case["mask_seed"])
        keep = 1 - case["encoder"]["edge_dropout"]["self_loop"]
        keeps = tuple(torch.bernoulli(torch.full((ref.N,), keep, dtype=torch.float, device=DEV)).to(torch.uint8).cpu().numpy() for _ in range(2))
    return loss, tags, keeps


@pytest.mark.parametrize("name", list(ref.CASES))
def test_step_loss_and_every_gradient(name):
    case = ref.CASES[name]
    inp = ref.case_inputs(case)
    model = build_model(case, inp)
    loss, tags, keeps = run_step(case, inp, model)
    print(f"[lp-step] {name}: launched {tags}")
    if case["mode"] == "other":
        kept = [int(k.sum()) for k in keeps]
        assert all(0 < k < ref.N for k in kept), kept
        for mine, recorded in zip(keeps, ref.recorded_keeps(case)):
            assert np.array_equal(mine, recorded), "the generator draws other keep masks than those the ReLU condition was checked under"
    bf16 = case["storage"] == "bf16"
    bound = BF_BOUND if bf16 else BOUND
    (want_loss, want), others = reference(name, keeps)
    named = dict(model.named_parameters())
    assert all(p.grad is not None for p in named.values()), [k for k, p in named.items() if p.grad is None]
    assert torch.isfinite(loss).item() and loss.dim() == 0
    got = {k: p.grad.detach().double().cpu().numpy() for k, p in named.items()}
    assert set(got) == set(want) == set(named)
    dist = {"loss": ref.rel_dist(loss.item(), want_loss)}
    softmax_pbias = case["objective"] == "1-n" and "scoring_function.pbias" in got
    for k in got:
        assert got[k].shape == want[k].shape and np.isfinite(got[k]).all(), k
        if softmax_pbias and k == "scoring_function.pbias":
            continue
        dist[k] = ref.rel_dist(got[k], want[k])
    worst = max(dist.values())
    print(f"[lp-step] {name}: loss {loss.item():.6f} (reference {want_loss:.6f}); relative distances (bound {bound:.2e}): "
          + ", ".join(f"{k} {v:.2e}" for k, v in dist.items()) + f"; largest {worst:.2e}")
    if bf16:       # for the record: the GPU against the evaluation that rounds the activations alone, and how far that one is from no rounding
        (act_loss, act), (plain_loss, plain) = others
        skip = {"scoring_function.pbias"} if softmax_pbias else set()
        far = {"loss": ref.rel_dist(loss.item(), act_loss), **{k: ref.rel_dist(got[k], act[k]) for k in want if k not in skip}}
        moved = {"loss": ref.rel_dist(act_loss, plain_loss), **{k: ref.rel_dist(act[k], plain[k]) for k in want if k not in skip}}
        print(f"[lp-step] {name}: against the activations-only rounding: " + ", ".join(f"{k} {v:.2e}" for k, v in far.items()))
        print(f"[lp-step] {name}: activations-only rounding against none: " + ", ".join(f"{k} {v:.2e}" for k, v in moved.items()))
    if softmax_pbias:
        cand = max(np.abs(want["scoring_function.sbias"]).max(), np.abs(want["scoring_function.obias"]).max())
        print(f"[lp-step] {name}: pbias (zero in exact arithmetic) gpu {np.abs(got['scoring_function.pbias']).max():.2e}, reference "
              f"{np.abs(want['scoring_function.pbias']).max():.2e}, candidate-side norm {cand:.2e}")
        assert np.abs(got["scoring_function.pbias"]).max() <= bound * cand
        assert np.abs(want["scoring_function.pbias"]).max() <= 1e-9 * max(cand, 1.0)
    for k, v in dist.items():
        assert v < bound, (name, k, v)


def test_s_penalty_scales_nodes_and_relations_apart():
    """the histogram form of the schlichtkrull penalty against the gathered one where the two scales differ: in a model the embeddings and
    the relations are equally wide (and 1 / (T d) is one number), so the step cannot tell a relation scale taken from the nodes"""
    from torch_rgcn.layers import DistMult
    rng = np.random.default_rng(17)
    n, d_nodes, d_rel, t = 37, 24, 10, 150
    dec = DistMult(ref.R0, d_rel, n, ref.R0).to(DEV)
    x = rng.standard_normal((n, d_nodes))
    rel = rng.standard_normal((ref.R0, d_rel))
    batch = np.stack([rng.integers(0, n, t), rng.integers(0, ref.R0, t), rng.integers(0, n, t)], 1)
    with torch.no_grad():
        dec.relations.copy_(torch.from_numpy(rel))
    xt = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
    got = dec.s_penalty(torch.from_numpy(batch).to(DEV), xt)
    got.backward()
    x64, r64 = torch.tensor(x, requires_grad=True), torch.tensor(rel, requires_grad=True)
    want = ref.gathered_penalty(batch, x64, r64)
    gx, gr = torch.autograd.grad(want, [x64, r64])
    dist = (ref.rel_dist(got.item(), want.item()), ref.rel_dist(xt.grad.cpu().numpy(), gx.numpy()),
            ref.rel_dist(dec.relations.grad.cpu().numpy(), gr.numpy()))
    print(f"[lp-step] s_penalty at widths {d_nodes} / {d_rel}: value, dnodes, drelations {dist}")
    assert max(dist) < BOUND
