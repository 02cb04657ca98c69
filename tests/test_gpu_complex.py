"""ComplEx on scored triples (functional.complex_score; csrc/rgcn_complex.hip) against the float64 complex-tensor reference of
tests/complex_reference.py.  Shapes (N, T, d), each for a way to go wrong:

    (1, 1, 2)        one complex feature, one entity: the triple's subject is its object
    (65, 130, 6)     h = 3 odd: the element-by-element loads, lanes with a ragged group of four
    (33, 70, 8)      h = 4: the 16-byte (fp32) / 8-byte (bf16) pieces, ONE active lane
    (129, 257, 200)  the WN18 width, 25 active lanes
    (40, 90, 520)    h = 260: a second pass of 256 features per wave, with ONE active lane in it

Every case (N > 2) holds a duplicated triple, an entity that occurs in no triple (its gradient row must come out zero, not stale) and a
triple whose subject is its object (both CSR rows of that entity carry it).  Bounds: 1e-4 relative in the max norm per array, 2^-8 for a
bf16 dnodes (one rounding of an fp32 sum: tests/test_gpu_softmax_loss_bf16.py), equality on small-integer inputs."""
import numpy as np
import pytest
import torch

import complex_reference as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
BOUND, BF_BOUND = 1e-4, 2.0 ** -8
SHAPES = [(1, 1, 2), (65, 130, 6), (33, 70, 8), (129, 257, 200), (40, 90, 520)]
_CASES = {}


def case(N, T, d, biased, storage, integer):
    """host arrays, the float64 scores and (for integer gs or random gs) the float64 gradients: computed once, shared, never written"""
    key = (N, T, d, biased, storage, integer)
    if key not in _CASES:
        rng, nodes, rel, bias, tr = cr.make_case(N, T, d, biased, storage, integer, seed=1)
        if N > 2:
            tr[tr == N - 1] = 0                                                # entity N - 1 occurs in no triple
            tr[1] = tr[0]                                                      # a duplicate
            tr[2, 2] = tr[2, 0]                                                # subject == object
        else:
            tr[:, 0] = tr[:, 2] = 0
        gs = rng.integers(-2, 3, T).astype(np.float32) if integer else rng.standard_normal(T).astype(np.float32)
        n, r = cr.f64(nodes).requires_grad_(True), cr.f64(rel).requires_grad_(True)
        b = [cr.f64(x).requires_grad_(True) for x in bias] if biased else [None] * 3
        scores = cr.triple_scores(tr, n, r, b)
        (scores * cr.f64(gs)).sum().backward()
        grads = [n.grad, r.grad] + [x.grad for x in b if x is not None]
        _CASES[key] = (nodes, rel, bias, tr, gs, scores.detach(), grads)
    return _CASES[key]


def on_device(nodes, rel, bias, storage, grad=True):
    nt = torch.from_numpy(nodes).to(DEV).to(BF if storage == "bf16" else torch.float32).requires_grad_(grad)
    rt = torch.from_numpy(rel).to(DEV).requires_grad_(grad)
    bt = [None if b is None else torch.from_numpy(b).to(DEV).requires_grad_(grad) for b in bias]
    return nt, rt, bt


def run(nodes, rel, bias, tr, gs, storage):
    from torch_rgcn import functional
    nt, rt, bt = on_device(nodes, rel, bias, storage)
    scores = functional.complex_score(torch.from_numpy(tr).to(DEV), nt, rt, *bt)
    assert scores.dtype == torch.float32 and scores.shape == (len(tr),)
    scores.backward(torch.from_numpy(gs).to(DEV))
    torch.cuda.synchronize()
    return scores.detach(), [nt.grad, rt.grad] + [b.grad for b in bt if b is not None]


@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,T,d", SHAPES)
def test_scores_and_gradients_within_the_bounds(N, T, d, storage, biased):
    nodes, rel, bias, tr, gs, want, want_g = case(N, T, d, biased, storage, False)
    scores, grads = run(nodes, rel, bias, tr, gs, storage)
    what = f"N={N} T={T} d={d} {storage} biased={biased}"
    cr.close(scores, want, what + " scores", BOUND)
    assert grads[0].dtype == (BF if storage == "bf16" else torch.float32) and grads[0].shape == (N, d)
    for name, g, w in zip(("dnodes", "drel", "dsbias", "dpbias", "dobias"), grads, want_g):
        assert g.dtype == torch.float32 or name == "dnodes", name
        cr.close(g, w, f"{what} {name}", BF_BOUND if (storage == "bf16" and name == "dnodes") else BOUND)
    if N > 2:
        assert not grads[0][N - 1].float().abs().max().item(), "the row of an entity in no triple must be written, as zeros"


@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,T,d", SHAPES)
def test_integer_inputs_give_the_reference_exactly(N, T, d, storage, biased):
    """entries in [-2, 2], biases in [-1, 1], gs in [-2, 2]: |score| <= 32 h + 3 and every gradient entry is below 16 T -- integers far
    below 2^24, so fp32 adds them exactly in any order.  A swapped half, a wrong sign or one lost triple fails here.  bf16: the scores
    (fp32 sums of exact products) equal the reference; dnodes is bf16 and only bounded."""
    nodes, rel, bias, tr, gs, want, want_g = case(N, T, d, biased, storage, True)
    scores, grads = run(nodes, rel, bias, tr, gs, storage)
    what = f"integer N={N} T={T} d={d} {storage} biased={biased}"
    cr.equal(scores, want, what + " scores")
    for name, g, w in zip(("dnodes", "drel", "dsbias", "dpbias", "dobias"), grads, want_g):
        if storage == "bf16" and name == "dnodes":
            cr.close(g, w, f"{what} {name}", BF_BOUND)
        else:
            cr.equal(g, w, f"{what} {name}")


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,T,d", SHAPES)
def test_zero_imaginary_halves_reduce_to_distmult(N, T, d, storage):
    """with real embeddings ComplEx IS DistMult on the real halves at width h: exact on integer inputs.  Ties the new kernels to the
    ones the reference's goldens pin."""
    from torch_rgcn import functional
    nodes, rel, bias, tr, *_ = case(N, T, d, True, storage, True)
    h = d // 2
    nodes, rel = nodes.copy(), rel.copy()
    nodes[:, h:] = 0
    rel[:, h:] = 0
    nt, rt, bt = on_device(nodes, rel, bias, storage, grad=False)
    tt = torch.from_numpy(tr).to(DEV)
    got = functional.complex_score(tt, nt, rt, *bt)
    want = functional.distmult_score(tt, nt[:, :h].contiguous(), rt[:, :h].contiguous(), *bt)
    assert torch.equal(got, want), (got - want).abs().max()
    cr.equal(got, cr.triple_scores(tr, cr.f64(nodes), cr.f64(rel), [cr.f64(b) for b in bias]), "reduction")
    assert got.abs().max().item() > 0 or N == 1


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,T,d", SHAPES[1:])
def test_imaginary_relations_are_antisymmetric(N, T, d, storage):
    """with the real half of the relations zero, score(s, p, o) == -score(o, p, s), exactly on integer inputs -- what DistMult cannot
    express.  (N = 1 has only s == o, whose score is then zero: the shape is left to the other tests.)"""
    from torch_rgcn import functional
    nodes, rel, _, tr, *_ = case(N, T, d, False, storage, True)
    rel = rel.copy()
    rel[:, :d // 2] = 0
    nt, rt, _ = on_device(nodes, rel, [None] * 3, storage, grad=False)
    fwd = functional.complex_score(torch.from_numpy(tr).to(DEV), nt, rt)
    back = functional.complex_score(torch.from_numpy(np.ascontiguousarray(tr[:, ::-1])).to(DEV), nt, rt)
    assert torch.equal(fwd, -back)
    assert fwd.abs().max().item() > 0, "every score is zero: the case shows nothing"
    cr.equal(fwd, cr.triple_scores(tr, cr.f64(nodes), cr.f64(rel)), "antisymmetry")


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_an_out_of_range_triple_raises_and_leaves_the_other_scores_right(storage):
    from torch_rgcn import _native, functional
    N, T, d = 33, 70, 8
    nodes, rel, bias, tr, gs, want, _ = case(N, T, d, True, storage, True)
    nt, rt, bt = on_device(nodes, rel, bias, storage, grad=False)
    for col, value in ((0, N), (2, -1), (1, cr.R0)):
        bad = tr.copy()
        bad[5, col] = value
        with pytest.raises(IndexError):
            functional.complex_score(torch.from_numpy(bad).to(DEV), nt, rt, *bt)
        # the entry point itself: the bad triple is not touched, scores 0 and raises the flag; every other score is right
        scores = torch.full((T,), 7.0, device=DEV)
        err = torch.zeros(1, dtype=torch.int32, device=DEV)
        fn = _native.lib().rgcn_complex_fwd_bf16 if storage == "bf16" else _native.lib().rgcn_complex_fwd_f32
        dp = _native._dp
        rc = fn(dp(torch.from_numpy(bad).to(DEV)), T, dp(nt), dp(rt), dp(bt[0]), dp(bt[1]), dp(bt[2]), dp(scores), N, cr.R0, d, dp(err), None, None,
                _native._stream(nt.device))
        assert rc == 0 and err.item() == 1
        w = want.clone()
        w[5] = 0
        cr.equal(scores, w, f"out of range col {col}")


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_no_triples_give_an_empty_result_and_zero_gradients(storage):
    from torch_rgcn import functional
    nodes, rel, bias, *_ = case(33, 70, 8, True, storage, True)
    nt, rt, bt = on_device(nodes, rel, bias, storage)
    for shape in ((0, 3), (2, 0, 3)):
        out = functional.complex_score(torch.zeros(shape, dtype=torch.long, device=DEV), nt, rt, *bt)
        assert out.shape == shape[:-1] and out.dtype == torch.float32
    out.sum().backward()
    for t in [nt, rt] + bt:
        assert t.grad is not None and not t.grad.float().abs().max().item()


def test_the_layer_scores_and_ignores_the_backward_route_switch(monkeypatch):
    """ComplEx(DistMult).forward is complex_score with the module's parameters, and the route distmult_bwd (csr / split / atomic) changes
    nothing: there is one ComplEx route"""
    from torch_rgcn import routes
    from torch_rgcn.layers import ComplEx
    N, T, d = 65, 130, 6
    nodes, rel, bias, tr, gs, want, want_g = case(N, T, d, True, "fp32", True)
    layer = ComplEx(cr.R0, d, N, cr.R0, b_init="zeros").to(DEV)
    with torch.no_grad():
        layer.relations.copy_(torch.from_numpy(rel))
        for p, b in zip((layer.sbias, layer.pbias, layer.obias), bias):
            p.copy_(torch.from_numpy(b))
    outs = []
    for mode in ("csr", "split", "atomic"):
        routes.patch(monkeypatch, "distmult_bwd", mode)
        x = torch.from_numpy(nodes).to(DEV).requires_grad_(True)
        layer.zero_grad()
        s = layer(torch.from_numpy(tr), x)
        s.backward(torch.from_numpy(gs).to(DEV))
        cr.equal(s, want, f"layer scores {mode}")
        cr.equal(x.grad, want_g[0], f"layer dnodes {mode}")
        cr.equal(layer.relations.grad, want_g[1], f"layer drel {mode}")
        outs.append(s.detach())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
