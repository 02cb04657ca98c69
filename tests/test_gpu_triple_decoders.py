"""The one autograd Function of the scored triples (functional._TripleScore) serves DistMult and ComplEx, fp32 and bf16 tables, and the
three routes of distmult_bwd.  What the folded Function newly shares is the meaning of "no ranks were counted": the atomic route, or no
triples at all.

  test_no_triples       scores of shape [0] and, after backpropagating an empty gradient, every gradient present, of its parameter's shape
                        and dtype, all zeros -- each decoder and storage, with and without biases, under every route, d = 6 (the
                        element-wise form; ComplEx half-width 3) and d = 8 (the vector form).
  test_routes_agree     T = 5 triples of small integers (exact_inputs.ints): every sum is exact in fp32 and every entity-row sum an integer
                        bf16 holds, so rounding is the identity and the order of arrival does not matter -- the scores and every gradient
                        are torch.equal across csr, split and atomic, and equal to the product formula in float64.
"""
import numpy as np
import pytest
import torch

import exact_inputs as ex

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
N, R, T = 7, 3, 5
ROUTES = ("csr", "split", "atomic")
PAIRS = [("distmult", "fp32"), ("distmult", "bf16"), ("complex", "fp32"), ("complex", "bf16")]
PAIR_IDS = ["-".join(p) for p in PAIRS]


def score_and_grads(monkeypatch, route, decoder, storage, d, with_bias, triples, gs):
    """-> (scores, [the parameters], [their gradients]) of distmult_score / complex_score under the route; integer parameters, all of them
    requiring grad"""
    from torch_rgcn import functional, routes
    routes.patch(monkeypatch, "distmult_bwd", route)
    rng = np.random.default_rng(d)
    shapes = [(N, d), (R, d)] + ([(N,), (R,), (N,)] if with_bias else [])
    params = [torch.from_numpy(ex.ints(s, -2, 2, 1.0, rng)).to(DEV) for s in shapes]
    if storage == "bf16":
        params[0] = params[0].to(BF)
    for p in params:
        p.requires_grad_(True)
    score = functional.distmult_score if decoder == "distmult" else functional.complex_score
    scores = score(triples, *params)
    scores.backward(gs)
    return scores.detach(), params, [p.grad for p in params]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("d", [6, 8])
@pytest.mark.parametrize("decoder,storage", PAIRS, ids=PAIR_IDS)
def test_no_triples(monkeypatch, decoder, storage, d, with_bias, route):
    triples = torch.empty(0, 3, dtype=torch.int64, device=DEV)
    scores, params, grads = score_and_grads(monkeypatch, route, decoder, storage, d, with_bias, triples, torch.empty(0, device=DEV))
    assert scores.shape == (0,)
    assert len(grads) == (5 if with_bias else 2)
    for p, g in zip(params, grads):
        assert g is not None and g.shape == p.shape and g.dtype == p.dtype
        assert not bool(g.float().abs().any()), "a gradient of no triples is all zeros"


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("d", [6, 8])
@pytest.mark.parametrize("decoder,storage", PAIRS, ids=PAIR_IDS)
def test_routes_agree(monkeypatch, decoder, storage, d, with_bias):
    rng = np.random.default_rng(100 + d)
    tr = np.stack([rng.integers(0, N, T), rng.integers(0, R, T), rng.integers(0, N, T)], 1).astype(np.int64)
    tr[1] = tr[0]                                               # a repeated triple: two arrivals at every row it touches
    triples = torch.from_numpy(tr).to(DEV)
    gs = torch.from_numpy(ex.ints((T,), -2, 2, 1.0, rng)).to(DEV)
    # |parameter| <= 2, |gs| <= 2: a term of an entity row is at most 2 * 2 * 2 * 2 (ComplEx: two products per element) and a row collects
    # at most 2 T = 10 of them -- 160 <= 256, integers bf16 holds; every other sum is far inside the fp32 significand
    runs = {route: score_and_grads(monkeypatch, route, decoder, storage, d, with_bias, triples, gs) for route in ROUTES}
    sc0, params, gr0 = runs["csr"]
    assert sc0.shape == (T,) and bool(sc0.abs().sum() > 0) and all(bool(g.float().abs().sum() > 0) for g in gr0), "a case that computes something"
    names = ("nodes", "relations", "sbias", "pbias", "obias")
    for route in ROUTES[1:]:
        sc, _, gr = runs[route]
        assert torch.equal(sc, sc0), f"scores: {route} against csr"
        for name, g, g0 in zip(names, gr, gr0):
            assert g.dtype == g0.dtype and torch.equal(g, g0), f"d{name}: {route} against csr"
    # and they are the right ones (ComplEx ignores the switch, so the comparison above alone would only show that it is deterministic):
    # the product formula in float64 on the same integers, through autograd -- exact, so equality
    sc_ref, gr_ref = reference(decoder, torch.from_numpy(tr), [p.detach().cpu().double() for p in params], gs.cpu().double())
    assert torch.equal(sc0.cpu().double(), sc_ref), "scores against the float64 formula"
    for name, g, g_ref in zip(names, gr0, gr_ref):
        assert torch.equal(g.cpu().double(), g_ref), f"d{name} against the float64 formula"


def reference(decoder, tr, params, gs):
    """-> (scores, [gradients]) in float64 on the CPU: DistMult sum_k s r o, ComplEx Re sum_k s r conj(o) on rows of real halves |
    imaginary halves; + sbias[s] + pbias[p] + obias[o] when there are biases"""
    params = [p.requires_grad_(True) for p in params]
    nodes, rel = params[:2]
    s, r, o = nodes[tr[:, 0]], rel[tr[:, 1]], nodes[tr[:, 2]]
    if decoder == "distmult":
        scores = (s * r * o).sum(1)
    else:
        h = nodes.shape[1] // 2
        z_re, z_im = s[:, :h] * r[:, :h] - s[:, h:] * r[:, h:], s[:, :h] * r[:, h:] + s[:, h:] * r[:, :h]      # s r
        scores = (z_re * o[:, :h] + z_im * o[:, h:]).sum(1)                                                     # Re(z conj(o))
    if len(params) == 5:
        scores = scores + params[2][tr[:, 0]] + params[3][tr[:, 1]] + params[4][tr[:, 2]]
    scores.backward(gs)
    return scores.detach(), [p.grad for p in params]
