"""ComplEx under guard bands (tests/guard_bands.py): one case per new entry point -- the scoring kernel, the entity walk and the
predicate-sorted relation kernel, fp32 and bf16 -- and one per ComplEx query form (tail / head x the fp32 / bf16 query kernel), at the most
ragged shape of the ComplEx tests: d = 6 (h = 3: the element-by-element loads, one lane with three of its four features) and N = 65.
Every buffer the library sizes sits between poisoned bands: nothing may be stored outside one, and no band value (NaN) may reach a result
-- the results are compared exactly with the float64 reference on small-integer inputs."""
import numpy as np
import pytest
import torch

import complex_reference as cr
import guard_bands as gb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
N, T, D = 65, 130, 6


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_triple_entries_under_guard_bands(monkeypatch, storage):
    """rgcn_complex_fwd_*, rgcn_complex_bwd_nodes_*, rgcn_complex_bwd_rel_* through autograd, with biases"""
    from torch_rgcn import functional
    rng, nodes, rel, bias, tr = cr.make_case(N, T, D, True, storage, integer=True, seed=3)
    tr[tr == N - 1] = 0                                                        # the last entity's row has no entries: its gradient row is written all the same
    gs = rng.integers(-2, 3, T).astype(np.float32)
    n, r, b = cr.f64(nodes).requires_grad_(True), cr.f64(rel).requires_grad_(True), [cr.f64(x).requires_grad_(True) for x in bias]
    want = cr.triple_scores(tr, n, r, b)
    (want * cr.f64(gs)).sum().backward()
    with gb.Guard(monkeypatch) as guard:
        nt = guard.home(to_dev(nodes, BF if storage == "bf16" else None)).requires_grad_(True)
        rt = guard.home(to_dev(rel)).requires_grad_(True)
        bt = [guard.home(to_dev(x)).requires_grad_(True) for x in bias]
        scores = functional.complex_score(guard.home(to_dev(tr)), nt, rt, *bt)
        scores.backward(guard.home(to_dev(gs)))
        torch.cuda.synchronize()
        calls = guard.calls
        problems = guard.problems(f"complex triples {storage} N={N} T={T} d={D}")
    assert not problems, "\n".join(problems)
    assert calls >= 4                                                          # scoring, CSR placement, entity walk, relation kernel
    cr.equal(scores, want.detach(), "guarded scores")
    if storage == "bf16":
        cr.close(nt.grad, n.grad, "guarded dnodes (bf16)", 2.0 ** -8)
    else:
        cr.equal(nt.grad, n.grad, "guarded dnodes")
    cr.equal(rt.grad, r.grad, "guarded drel")
    for got, ref in zip(bt, b):
        cr.equal(got.grad, ref.grad, "guarded bias gradient")


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_query_forms_under_guard_bands(monkeypatch, storage, head):
    """the ComplEx branch of rank_query_kernel / rank_query_bf16_kernel: the query vectors (fp32 [Q][d]; bf16 three terms [Q][32], the
    tail beyond d = 6 zeroed) and what the product reads of them, through score_all and the fused ranks"""
    from torch_rgcn import functional
    Q = 5
    _, nodes, rel, bias, batch = cr.make_case(N, Q, D, True, storage, integer=True, seed=4)
    want = cr.all_scores(batch, head, cr.f64(nodes), cr.f64(rel), [cr.f64(x) for x in bias])
    tgt = torch.from_numpy(batch[:, 0 if head else 2])
    t = want[torch.arange(Q), tgt][:, None]
    with gb.Guard(monkeypatch) as guard:
        nt = guard.home(to_dev(nodes, BF if storage == "bf16" else None))
        rt = guard.home(to_dev(rel))
        bt = [guard.home(to_dev(x)) for x in bias]
        bd = guard.home(to_dev(batch))
        assert torch.isnan(torch.empty(3, device=DEV)).all()
        scores = functional.distmult_score_all(bd, head, nt, rt, *bt, decoder="complex")
        greater, ties, tscore = functional.distmult_rank_all(bd, head, nt, rt, *bt, decoder="complex")
        torch.cuda.synchronize()
        problems = guard.problems(f"complex query form {storage} head={head} N={N} Q={Q} d={D}")
    assert not problems, "\n".join(problems)
    cr.equal(scores, want, "guarded score_all")
    cr.equal(tscore, t[:, 0], "guarded tscore")
    assert np.array_equal(greater.cpu().numpy(), (want > t).sum(1).numpy()) and np.array_equal(ties.cpu().numpy(), (want == t).sum(1).numpy())
