"""The all-candidate routes with decoder="complex" -- score_all, the fused and the materialised ranks, top-k, the 1-N softmax loss and the
K-vs-All BCE loss -- against the float64 complex-tensor reference of tests/complex_reference.py.  Only the query pass differs from
DistMult's, so the shapes (N, Q, d) aim at it and at the tile edges it feeds:

    (1, 1, 2)        one complex feature, one entity, one query
    (63, 65, 6)      h odd; a second wave-quartet of queries
    (257, 129, 50)   d no multiple of 4 or 8 (element-wise tile loads, the bf16 tail zeroed up to 64), a second 128-query tile with one
                     row, a third 128-column tile with one column
    (130, 3, 200)    the WN18 width: lanes 36 .. 63 of a query's wave own no complex feature
    (77, 10, 520)    h = 260: a lane owns up to five complex features

Bounds: 1e-4 relative in the max norm per array, 2^-8 for a bf16 dnodes, equality on small-integer inputs."""
import numpy as np
import pytest
import torch

import complex_reference as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F64 = torch.bfloat16, torch.float64
BOUND, BF_BOUND = 1e-4, 2.0 ** -8
SHAPES = [(1, 1, 2), (63, 65, 6), (257, 129, 50), (130, 3, 200), (77, 10, 520)]
EPS = (0.0, 0.1)
_CASES = {}


def case(N, Q, d, storage, integer):
    """one case, shared and never written: host arrays, known triples around the batch, and per direction the float64 scores"""
    from utils.misc import generate_true_dict
    key = (N, Q, d, storage, integer)
    if key not in _CASES:
        rng, nodes, rel, bias, batch = cr.make_case(N, Q, d, True, storage, integer, seed=2)
        more = batch[rng.integers(0, Q, 3 * Q)].copy()
        half = len(more) // 2
        more[:half, 0] = rng.integers(0, N, half)
        more[half:, 2] = rng.integers(0, N, len(more) - half)
        known = np.concatenate([batch, more])
        n, r, b = cr.f64(nodes), cr.f64(rel), [cr.f64(x) for x in bias]
        scores = {head: cr.all_scores(batch, head, n, r, b) for head in (True, False)}
        _CASES[key] = (nodes, rel, bias, batch, generate_true_dict(known), scores)
    return _CASES[key]


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def params(nodes, rel, bias, storage, grad=False):
    nt = dev(nodes, BF if storage == "bf16" else None).requires_grad_(grad)
    return nt, dev(rel).requires_grad_(grad), [dev(b).requires_grad_(grad) for b in bias]


def filter_lists(true, batch, N, head, keep_target=False):
    from utils.misc import _FilterIndex
    return _FilterIndex(true, N).lists(batch, head, keep_target=keep_target)


def masked(scores, rows, cols):
    s = scores.clone()
    s[torch.from_numpy(rows.astype(np.int64)), torch.from_numpy(cols.astype(np.int64))] = -np.inf
    return s


# ----------------------------------------------------------------------------- scores
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,d", SHAPES)
def test_score_all(N, Q, d, storage):
    from torch_rgcn import functional
    for integer in (False, True):
        nodes, rel, bias, batch, _, scores = case(N, Q, d, storage, integer)
        nt, rt, bt = params(nodes, rel, bias, storage)
        for head in (True, False):
            for b in (bt, [None] * 3):
                got = functional.distmult_score_all(dev(batch), head, nt, rt, *b, decoder="complex")
                want = scores[head] if b[0] is not None else cr.all_scores(batch, head, cr.f64(nodes), cr.f64(rel))
                what = f"score_all N={N} Q={Q} d={d} {storage} head={head} integer={integer} biased={b[0] is not None}"
                assert got.shape == (Q, N) and got.dtype == torch.float32
                if not integer:
                    cr.close(got, want, what, BOUND)
                    continue
                cr.equal(got, want, what)
                # the cell of a query's own target is the triple's score, from the triple kernels
                cell = got[torch.arange(Q), dev(batch[:, 0 if head else 2])]
                assert torch.equal(cell, functional.complex_score(dev(batch), nt, rt, *b)), what


# ----------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,d", SHAPES)
def test_ranks_fused_and_materialised(N, Q, d, storage):
    """integer inputs: greater and ties per query EQUAL those counted from the float64 scores -- unfiltered, with lists, with a FilterIndex;
    the fused route (no score matrix) and the materialised one (score_all, filter, count: what utils.misc.evaluate runs)"""
    from torch_rgcn import _native, functional
    nodes, rel, bias, batch, true, scores = case(N, Q, d, storage, True)
    nt, rt, bt = params(nodes, rel, bias, storage)
    bd = dev(batch)
    index = functional.FilterIndex(true, N, DEV)
    for head in (True, False):
        tgt = torch.from_numpy(batch[:, 0 if head else 2])
        rows, cols = filter_lists(true, batch, N, head)
        for kind in ("raw", "lists", "index"):
            s = scores[head] if kind == "raw" else masked(scores[head], rows, cols)
            t = s[torch.arange(Q), tgt][:, None]
            want_g, want_e = (s > t).sum(1).numpy(), (s == t).sum(1).numpy()
            what = f"ranks N={N} Q={Q} d={d} {storage} head={head} {kind}"
            kw = dict(filt_q=dev(rows), filt_n=dev(cols)) if kind == "lists" and len(rows) else dict(filt=index) if kind == "index" else {}
            for strips in (0, 3):
                g, e, ts = functional.distmult_rank_all(bd, head, nt, rt, *bt, strips=strips, decoder="complex", **kw)
                assert np.array_equal(g.cpu().numpy(), want_g) and np.array_equal(e.cpu().numpy(), want_e), (what, strips)
                cr.equal(ts, t[:, 0], what + " tscore")
            mat = functional.distmult_score_all(bd, head, nt, rt, *bt, decoder="complex")
            if kind == "lists" and len(rows):
                _native.rank_filter(mat, dev(rows), dev(cols))
            elif kind == "index":
                _native.rank_filter_index(mat, bd, head, index)
            g, e = _native.rank_count(mat, bd, head)
            assert np.array_equal(g.cpu().numpy(), want_g) and np.array_equal(e.cpu().numpy(), want_e), what + " materialised"
        assert want_e.min() >= 1


# ----------------------------------------------------------------------------- top-k
def topk_ref(s, k):
    """float64 ordering: score descending, id ascending; rows with fewer than k finite candidates end in id -1, score -inf"""
    Q, N = s.shape
    ids, vals = np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf)
    for q in range(Q):
        row = s[q].numpy()
        order = np.lexsort((np.arange(N), -row))
        order = order[np.isfinite(row[order])][:k]
        ids[q, :len(order)], vals[q, :len(order)] = order, row[order]
    return ids, vals


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,d", SHAPES)
def test_topk(N, Q, d, storage):
    from torch_rgcn import functional
    nodes, rel, bias, batch, true, scores = case(N, Q, d, storage, True)
    nt, rt, bt = params(nodes, rel, bias, storage)
    bd = dev(batch)
    index = functional.FilterIndex(true, N, DEV)
    for head in (True, False):
        rows, cols = filter_lists(true, batch, N, head, keep_target=True)        # prediction has no target: every known cell is out
        for k in (1, 10, 32):
            for kind in ("raw", "lists", "index"):
                s = scores[head] if kind == "raw" else masked(scores[head], rows, cols)
                want_i, want_s = topk_ref(s, k)
                if kind == "index":
                    ids, vals = functional.distmult_topk_all_index(bd, head, nt, rt, *bt, k=k, filt=index, decoder="complex")
                elif kind == "lists":
                    ids, vals = functional.complex_topk_all(bd, head, nt, rt, *bt, k=k, filt_q=dev(rows), filt_n=dev(cols))
                else:
                    ids, vals = functional.complex_topk_all(bd, head, nt, rt, *bt, k=k, strips=3)
                what = f"topk N={N} Q={Q} d={d} {storage} head={head} k={k} {kind}"
                assert np.array_equal(ids.cpu().numpy(), want_i), what
                assert np.array_equal(vals.cpu().numpy().astype(np.float64), want_s), what


# ----------------------------------------------------------------------------- losses
def loss_refs(nodes, rel, bias, batch, head, rows, cols, eps):
    """float64 autograd through the complex reference -> {"softmax" / "bce": (loss vector, [dnodes, drel, dsbias, dpbias, dobias] of its
    mean)}.  softmax: (rows, cols) are filtered out of the problem; bce: they are positive labels, beside every query's own target."""
    Q, N = len(batch), len(nodes)
    tgt = torch.from_numpy(batch[:, 0 if head else 2])
    cell = torch.zeros(Q, N, dtype=torch.bool)
    cell[torch.from_numpy(rows.astype(np.int64)), torch.from_numpy(cols.astype(np.int64))] = True
    out = {}
    for name in ("softmax", "bce"):
        leaves = [cr.f64(nodes).requires_grad_(True), cr.f64(rel).requires_grad_(True)] + [cr.f64(b).requires_grad_(True) for b in bias]
        s = cr.all_scores(batch, head, leaves[0], leaves[1], leaves[2:])
        if name == "softmax":
            allowed = ~cell
            allowed[torch.arange(Q), tgt] = True
            lse = torch.logsumexp(s.masked_fill(~allowed, -np.inf), 1)
            mean_allowed = (s * allowed).sum(1) / allowed.sum(1)
            loss = lse - (1 - eps) * s[torch.arange(Q), tgt] - eps * mean_allowed
        else:
            y = cell.clone()
            y[torch.arange(Q), tgt] = True
            ys = (1 - eps) * y.to(F64) + eps / N
            loss = (torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs())) - ys * s).sum(1) / N
        grads = torch.autograd.grad(loss.mean(), leaves)
        out[name] = (loss.detach(), list(grads))
    return out


def check_loss(got_loss, got_grads, want, what, head, bf16_dnodes, zero_query_bias, floors=(0.0, 0.0)):
    """floors (loss, gradients): what the bound is relative to where the reference itself is rounding noise around zero -- the softmax
    loss of ONE candidate, lse - (1 - eps) s - eps s, whose terms are of the size of the score and whose gradient cells are 1 - 1"""
    cr.close(got_loss, want[0], what + " loss", BOUND, floors[0])
    names = ("dnodes", "drel", "dsbias", "dpbias", "dobias")
    cand = 2 if head else 4                                                     # the candidate-side bias: sbias for head queries, obias for tail
    cand_norm = want[1][cand].abs().max().item()
    for k, (name, g, w) in enumerate(zip(names, got_grads, want[1])):
        if zero_query_bias and k >= 2 and k != cand:
            # sum_n dS[q, n] = 0 in exact arithmetic: the route returns zeros, the reference rounding noise
            assert g.float().abs().max().item() <= BOUND * cand_norm and w.abs().max().item() <= 1e-9 * max(cand_norm, 1.0), (what, name)
            continue
        cr.close(g, w, f"{what} {name}", BF_BOUND if (bf16_dnodes and name == "dnodes") else BOUND, floors[1])


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,d", SHAPES)
def test_losses_and_gradients(N, Q, d, storage):
    """softmax (eps 0 and 0.1; lists filtered out) and BCE (eps 0 and 0.1; lists as labels), loss vector and every gradient of its mean;
    strips 0 and 3; chunk_bytes = 1 cuts the backward into ceil(N / 128) chunks (three at N = 257); bf16 through "upcast" and "native" """
    from torch_rgcn import functional
    nodes, rel, bias, batch, true, scores = case(N, Q, d, storage, False)
    bd = dev(batch)
    assert len(functional.softmax_chunk_plan(Q, N, 1)) == (N + 127) // 128
    # one candidate: the softmax loss and its cells are zero in exact arithmetic; the bound is then relative to the terms they cancel from
    floors = (scores[True].abs().max().item(), float(np.abs(nodes).max() * np.abs(rel).max())) if N == 1 else (0.0, 0.0)
    for head in (True, False):
        rows, cols = filter_lists(true, batch, N, head)
        lists = dict(q=dev(rows), n=dev(cols)) if len(rows) else dict(q=None, n=None)
        for eps in EPS:
            refs = loss_refs(nodes, rel, bias, batch, head, rows, cols, eps)
            for route in (("upcast", "native") if storage == "bf16" else ("upcast",)):
                for strips, chunk_bytes in ((0, None), (3, 1)):
                    kw = dict(reduction="none", strips=strips, chunk_bytes=chunk_bytes, bf16_backward=route, label_smoothing=eps)
                    for name in ("softmax", "bce"):
                        nt, rt, bt = params(nodes, rel, bias, storage, grad=True)
                        if name == "softmax":
                            loss = functional.distmult_softmax_loss(bd, head, nt, rt, *bt, filt_q=lists["q"], filt_n=lists["n"], decoder="complex", **kw)
                        else:
                            loss = functional.complex_bce_loss(bd, head, nt, rt, *bt, lab_q=lists["q"], lab_n=lists["n"], **kw)
                        loss.mean().backward()
                        grads = [nt.grad, rt.grad] + [b.grad for b in bt]
                        assert nt.grad.dtype == nt.dtype and rt.grad.dtype == torch.float32
                        what = f"{name} N={N} Q={Q} d={d} {storage}/{route} head={head} eps={eps} strips={strips} chunk_bytes={chunk_bytes}"
                        check_loss(loss.detach(), grads, refs[name], what, head, storage == "bf16", zero_query_bias=name == "softmax",
                                   floors=floors if name == "softmax" else (0.0, 0.0))


@pytest.mark.parametrize("head", [True, False])
def test_losses_with_a_filter_index(head):
    """the index form of the filter (softmax) and of the labels (BCE) at the ragged shape: the same loss and gradients as the reference"""
    from torch_rgcn import functional
    N, Q, d = 257, 129, 50
    nodes, rel, bias, batch, true, _ = case(N, Q, d, "fp32", False)
    index = functional.FilterIndex(true, N, DEV)
    refs = {}
    for name, keep_target in (("softmax", False), ("bce", True)):
        rows, cols = filter_lists(true, batch, N, head, keep_target=keep_target)
        refs[name] = loss_refs(nodes, rel, bias, batch, head, rows, cols, 0.1)[name]
    for name in ("softmax", "bce"):
        nt, rt, bt = params(nodes, rel, bias, "fp32", grad=True)
        if name == "softmax":
            loss = functional.distmult_softmax_loss(dev(batch), head, nt, rt, *bt, filt=index, reduction="none", label_smoothing=0.1, decoder="complex")
        else:
            loss = functional.complex_bce_loss(dev(batch), head, nt, rt, *bt, labels=index, reduction="none", label_smoothing=0.1)
        loss.mean().backward()
        check_loss(loss.detach(), [nt.grad, rt.grad] + [b.grad for b in bt], refs[name], f"{name} with an index head={head}", head, False,
                   zero_query_bias=name == "softmax")


# ----------------------------------------------------------------------------- reduction to DistMult, and DistMult untouched
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,d", SHAPES)
def test_zero_imaginary_halves_reduce_to_distmult(N, Q, d, storage):
    """real embeddings: every route with decoder="complex" at width d is the DistMult call on the real halves at width h -- ranks, top-k and
    scores exactly on integer inputs, the losses within 1e-4"""
    from torch_rgcn import functional
    h = d // 2
    for integer in (True, False):
        nodes, rel, bias, batch, _, _ = case(N, Q, d, storage, integer)
        nodes, rel = nodes.copy(), rel.copy()
        nodes[:, h:] = 0
        rel[:, h:] = 0
        nt, rt, bt = params(nodes, rel, bias, storage)
        nh, rh = nt[:, :h].contiguous(), rt[:, :h].contiguous()
        bd = dev(batch)
        for head in (True, False):
            what = f"reduction N={N} Q={Q} d={d} {storage} head={head} integer={integer}"
            if integer:
                assert torch.equal(functional.distmult_score_all(bd, head, nt, rt, *bt, decoder="complex"),
                                   functional.distmult_score_all(bd, head, nh, rh, *bt)), what
                for a, b in zip(functional.distmult_rank_all(bd, head, nt, rt, *bt, decoder="complex"), functional.distmult_rank_all(bd, head, nh, rh, *bt)):
                    assert torch.equal(a, b), what
                for a, b in zip(functional.complex_topk_all(bd, head, nt, rt, *bt, k=10), functional.distmult_topk_all(bd, head, nh, rh, *bt, k=10)):
                    assert torch.equal(a, b), what
                continue
            for eps in EPS:
                kw = dict(reduction="none", label_smoothing=eps)
                cr.close(functional.distmult_softmax_loss(bd, head, nt, rt, *bt, decoder="complex", **kw),
                         functional.distmult_softmax_loss(bd, head, nh, rh, *bt, **kw).double(), f"{what} softmax eps={eps}", BOUND)
                cr.close(functional.complex_bce_loss(bd, head, nt, rt, *bt, **kw),
                         functional.distmult_bce_loss(bd, head, nh, rh, *bt, **kw).double(), f"{what} bce eps={eps}", BOUND)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_decoder_distmult_is_the_call_without_the_keyword(storage):
    from torch_rgcn import functional
    N, Q, d = 257, 129, 50
    nodes, rel, bias, batch, true, _ = case(N, Q, d, storage, False)
    bd = dev(batch)
    index = functional.FilterIndex(true, N, DEV)
    for head in (True, False):
        def both(fn, **kw):
            nt, rt, bt = params(nodes, rel, bias, storage)
            plain, keyed, other = (fn(bd, head, nt, rt, *bt, **kw, **extra) for extra in ({}, {"decoder": "distmult"}, {"decoder": "complex"}))
            plain, keyed, other = (list(r) if isinstance(r, tuple) else [r] for r in (plain, keyed, other))
            for x, y in zip(plain, keyed):
                assert torch.equal(x, y), (fn.__name__, head)
            assert not torch.equal(plain[0], other[0]), (fn.__name__, head, "ComplEx is another function of the same inputs")
        both(functional.distmult_score_all)
        both(functional.distmult_rank_all, filt=index)
        both(functional.distmult_topk_all_index, k=10, filt=index)
        # the unordered index_add_ at the end of the backward: one row per destination here would need distinct anchors -- compare the loss
        # bits and the ordered gradients (the candidate-side bias), and the rest within the suite's bound
        for smoothing in EPS:
            nt, rt, bt = params(nodes, rel, bias, storage, grad=True)
            a = functional.distmult_softmax_loss(bd, head, nt, rt, *bt, filt=index, label_smoothing=smoothing)
            b = functional.distmult_softmax_loss(bd, head, nt, rt, *bt, filt=index, label_smoothing=smoothing, decoder="distmult")
            assert torch.equal(a.detach(), b.detach())
            ga = torch.autograd.grad(a, [nt, rt] + bt)
            gb = torch.autograd.grad(b, [nt, rt] + bt)
            cand = 2 if head else 4
            assert torch.equal(ga[cand], gb[cand])
            for x, y in zip(ga, gb):
                err, norm = cr.rel_err(x, y.double())
                assert err <= (BF_BOUND if x.dtype == BF else BOUND) * max(norm, 1e-30)
