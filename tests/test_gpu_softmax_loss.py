"""1-N softmax loss of DistMult: functional.distmult_softmax_loss -- a fused log-sum-exp forward and a chunked backward
that never hold the [Q, N] logits -- against float64 on the CPU.  The reference is computed in this file from the inputs, never from the
library's scores: s in float64, listed cells -inf (an entry on a query's own target ignored), torch.logsumexp, float64 autograd.

Bound: the suite's parity bound (README, "parity"), 1e-4 relative in the max norm of each compared array.  A bias gradient whose
reference is identically zero (the query-side ones) is compared absolutely against 1e-4 times the max norm of the candidate-side one.
Shapes and the case builder are those of test_gpu_topk.py, restated."""
import functools

import numpy as np
import pytest
import torch

import guard_bands as gb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
R0 = 5
BOUND = 1e-4
SHAPES = [(1, 1, 1), (63, 65, 6), (130, 3, 8), (257, 129, 50), (77, 10, 500), (700, 130, 24)]
F64 = torch.float64


@pytest.fixture(autouse=True)
def _random_streams_left_as_found():
    """the tests of this file seed and draw from the global generators: put them back, so that the files that run after this one see the
    streams they saw before it existed"""
    import random
    state = random.getstate(), torch.get_rng_state(), torch.cuda.get_rng_state(), np.random.get_state()
    yield
    random.setstate(state[0])
    torch.set_rng_state(state[1])
    torch.cuda.set_rng_state(state[2])
    np.random.set_state(state[3])


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def make_case(N, Q, dim, biased, storage, integer=False):
    """host arrays of one case (the builder of test_gpu_topk.py); bf16 storage: the table rounded to bf16"""
    rng = np.random.default_rng(1000 * N + 10 * Q + dim + biased)
    if integer:          # small integers: every product and sum is exact
        nodes = rng.integers(-2, 3, (N, dim)).astype(np.float32)
        copies = rng.permutation(N)[: N // 4]
        nodes[copies] = nodes[rng.integers(0, N, len(copies))]            # a quarter of the rows are copies of other rows
        rel = rng.integers(-2, 3, (R0, dim)).astype(np.float32)
        bias = [rng.integers(-1, 2, n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    else:
        nodes = rng.standard_normal((N, dim)).astype(np.float32)
        rel = rng.standard_normal((R0, dim)).astype(np.float32)
        bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    if storage == "bf16":
        nodes = torch.from_numpy(nodes).to(BF).float().numpy()
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    return rng, nodes, rel, bias, batch


def random_filter(rng, Q, N):
    """about 3 Q random cells; a query's own target may be among them: such an entry must be ignored"""
    return np.unique(np.stack([rng.integers(0, Q, 3 * Q), rng.integers(0, N, 3 * Q)], 1), axis=0)


def lists_of(filt, put=dev):
    if filt is None or not len(filt):
        return None, None
    return put(filt[:, 0].astype(np.int32)), put(filt[:, 1].astype(np.int32))


class Ref:
    """float64 on the CPU: scores, the loss vector, and the gradients of its mean"""

    def __init__(self, nodes, rel, bias, batch, head, filt, grads=True):
        n = torch.tensor(nodes, dtype=F64, requires_grad=True)
        r = torch.tensor(rel, dtype=F64, requires_grad=True)
        b = [None if x is None else torch.tensor(x, dtype=F64, requires_grad=True) for x in bias]
        bt = torch.from_numpy(batch)
        Q, N = len(batch), len(nodes)
        anchor, p, tgt = bt[:, 2 if head else 0], bt[:, 1], bt[:, 0 if head else 2]
        s = (n[anchor] * r[p]) @ n.T
        if b[0] is not None:
            sb, pb, ob = b
            s = s + ((sb[None, :] + pb[p][:, None] + ob[anchor][:, None]) if head else (sb[anchor][:, None] + pb[p][:, None] + ob[None, :]))
        mask = torch.zeros(Q, N, dtype=torch.bool)
        if filt is not None and len(filt):
            mask[torch.from_numpy(filt[:, 0]), torch.from_numpy(filt[:, 1])] = True
        mask[torch.arange(Q), tgt] = False                                  # an entry on the target is ignored
        self.scores = s.detach().numpy()
        self.mask = mask.numpy()
        loss = torch.logsumexp(s.masked_fill(mask, -float("inf")), 1) - s[torch.arange(Q), tgt]
        self.loss = loss.detach().numpy()
        if grads:
            loss.mean().backward()
            self.dnodes, self.drel = n.grad.numpy(), r.grad.numpy()
            self.dbias = [None if x is None else x.grad.numpy() for x in b]


@functools.lru_cache(maxsize=None)
def case_and_refs(N, Q, dim, biased, storage="fp32", integer=False):
    """one case with its random filters and references, computed once and shared (never written to)"""
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, biased, storage, integer)
    filts = {head: random_filter(rng, Q, N) for head in (True, False)}
    refs = {(head, f): Ref(nodes, rel, bias, batch, head, filts[head] if f else None) for head in (True, False) for f in (True, False)}
    return nodes, rel, bias, batch, filts, refs


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max(initial=0.0), np.abs(want).max(initial=0.0)


def close(got, want, what, scale=None):
    """max |got - want| <= BOUND * max |want| (scale: the norm to measure against when the reference is identically zero)"""
    err, norm = rel_err(got, want)
    norm = norm if scale is None else scale
    print(f"[softmax_loss] {what}: max err {err:.3e}, norm {norm:.3e}, relative {err / norm if norm else 0.0:.3e}")
    assert np.isfinite(np.asarray(got)).all(), what
    assert err <= BOUND * norm, (what, err, norm)


def params_on_device(nodes, rel, bias, storage="fp32", grad=(True, True, True), put=dev):
    nt = put(nodes, BF if storage == "bf16" else None)
    rt = put(rel)
    bt = [put(b) for b in bias]
    nt.requires_grad_(grad[0]); rt.requires_grad_(grad[1])
    for b in bt:
        if b is not None:
            b.requires_grad_(grad[2])
    return nt, rt, bt


def loss_of(batch_t, head, nt, rt, bt, filt=None, put=dev, **kw):
    from torch_rgcn import functional
    fq, fn = lists_of(filt, put)
    return functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, **kw)


def check_grads(ref, head, nt, rt, bt, what):
    if nt.grad is not None:
        close(nt.grad.cpu().numpy(), ref.dnodes, what + " dnodes")
    if rt.grad is not None:
        close(rt.grad.cpu().numpy(), ref.drel, what + " drel")
    if bt[0] is not None and bt[0].grad is not None:
        cand = 0 if head else 2
        cand_norm = np.abs(ref.dbias[cand]).max()
        for k, name in enumerate(("dsbias", "dpbias", "dobias")):
            if k == cand:
                close(bt[k].grad.cpu().numpy(), ref.dbias[k], f"{what} {name}")
            else:                                                           # sum_n dS[q, n] = 0: the reference is rounding noise
                assert np.abs(ref.dbias[k]).max() <= 1e-12
                close(bt[k].grad.cpu().numpy(), np.zeros_like(ref.dbias[k]), f"{what} {name} (query side)", scale=cand_norm)


def zero_grads(nt, rt, bt):
    for t in [nt, rt] + bt:
        if t is not None:
            t.grad = None


# ----------------------------------------------------------------------------- 1. forward parity
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_forward_parity(N, Q, dim, biased, storage):
    from torch_rgcn import _native
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, biased, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage, grad=(False, False, False))
    batch_t = dev(batch)
    score_all = _native.distmult_score_all_bf16 if storage == "bf16" else _native.distmult_score_all
    for head in (True, False):
        column = score_all(batch_t, head, nt, rt, *bt)[torch.arange(Q, device=DEV), batch_t[:, 0 if head else 2]].cpu().numpy()
        for filtered in (True, False):
            _native.profile_start()
            loss = loss_of(batch_t, head, nt, rt, bt, filts[head] if filtered else None, reduction="none")
            tags = set(_native.profile_stop())
            assert tags == {"lse_fused_bf16" if storage == "bf16" else "lse_fused"}, tags
            assert loss.shape == (Q,) and loss.dtype == torch.float32
            close(loss.detach().cpu().numpy(), refs[head, filtered].loss, f"{storage} N={N} Q={Q} d={dim} b={biased} head={head} filt={filtered} loss")
            fq, fn = lists_of(filts[head] if filtered else None)
            lse, tscore = _native.distmult_lse(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn)
            assert np.array_equal(tscore.cpu().numpy(), column)
            mean = loss_of(batch_t, head, nt, rt, bt, filts[head] if filtered else None)
            close(mean.detach().cpu().numpy(), refs[head, filtered].loss.mean(), "mean")


# ----------------------------------------------------------------------------- 2. gradient parity
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_gradient_parity(N, Q, dim, biased):
    """everything requires grad: reduction='none' then .mean() (a [Q] upstream gradient) and reduction='mean' from the unit gradient"""
    from torch_rgcn import _native, functional
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, biased)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        for filtered in (True, False):
            filt, ref = filts[head] if filtered else None, refs[head, filtered]
            what = f"N={N} Q={Q} d={dim} b={biased} head={head} filt={filtered}"
            zero_grads(nt, rt, bt)
            _native.profile_start()
            loss_of(batch_t, head, nt, rt, bt, filt, reduction="none").mean().backward()
            tags = set(_native.profile_stop())
            assert tags == {"lse_fused", "softmax_grad", "gemm"}, tags
            check_grads(ref, head, nt, rt, bt, what + " [none]")
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, filt)
            loss.backward(gradient=functional.unit_gradient(loss.device))
            check_grads(ref, head, nt, rt, bt, what + " [mean]")


@pytest.mark.parametrize("only", ["nodes", "relations"])
def test_gradient_parity_with_frozen_inputs(only):
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=(only == "nodes", only == "relations", False))
    batch_t = dev(batch)
    for head in (True, False):
        zero_grads(nt, rt, bt)
        loss_of(batch_t, head, nt, rt, bt, filts[head]).backward()
        assert (nt.grad is not None) == (only == "nodes") and (rt.grad is not None) == (only == "relations")
        assert all(b.grad is None for b in bt)
        check_grads(refs[head, True], head, nt, rt, bt, f"only {only} head={head}")


# ----------------------------------------------------------------------------- 3. running max
@pytest.mark.parametrize("biased", [False, True])
def test_scores_beyond_the_range_of_exp(biased):
    """integer inputs at d = 500: every score is an integer fp32 holds exactly, |s| goes beyond 200 and, unbiased, the largest score of
    every query row exceeds 88.7 = log(FLT_MAX): a log-sum-exp without the running max returns inf"""
    N, Q, dim = 77, 10, 500
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, biased, "fp32", True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        s = refs[head, False].scores
        assert np.array_equal(s, np.round(s)) and np.abs(s).max() > 88.7
        if not biased:
            assert (s.max(1) > 88.7).all()
        for filtered in (True, False):
            filt, ref = filts[head] if filtered else None, refs[head, filtered]
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, filt, reduction="none")
            assert torch.isfinite(loss).all()
            close(loss.detach().cpu().numpy(), ref.loss, f"integer b={biased} head={head} filt={filtered} loss")
            loss.mean().backward()
            check_grads(ref, head, nt, rt, bt, f"integer b={biased} head={head} filt={filtered}")


# ----------------------------------------------------------------------------- 4. mask
@pytest.mark.parametrize("N,Q,dim", [(257, 129, 50), (700, 130, 24)])
def test_the_largest_cells_are_filtered(N, Q, dim):
    """every query's three best non-target candidates are listed: ignoring the mask moves the loss by more than the bound"""
    nodes, rel, bias, batch, _, refs = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        s = refs[head, False].scores.copy()
        s[np.arange(Q), batch[:, 0 if head else 2]] = -np.inf
        best = np.argsort(-s, axis=1)[:, :3]
        filt = np.stack([np.repeat(np.arange(Q), 3), best.reshape(-1)], 1)
        ref = Ref(nodes, rel, bias, batch, head, filt)
        err, norm = rel_err(refs[head, False].loss, ref.loss)
        assert err > 10 * BOUND * norm                                       # the case is what it claims to be
        zero_grads(nt, rt, bt)
        loss = loss_of(batch_t, head, nt, rt, bt, filt, reduction="none")
        close(loss.detach().cpu().numpy(), ref.loss, f"best three filtered N={N} head={head} loss")
        loss.mean().backward()
        check_grads(ref, head, nt, rt, bt, f"best three filtered N={N} head={head}")


@pytest.mark.parametrize("biased", [False, True])
def test_everything_but_the_target_filtered_is_exactly_zero(biased):
    """lse == tscore bit for bit and exp(0) - 1 == 0: the loss and every gradient are exactly zero"""
    N, Q, dim = 130, 3, 8
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, biased)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        tgt = batch[:, 0 if head else 2]
        filt = np.array([(q, n) for q in range(Q) for n in range(N) if n != tgt[q]])
        zero_grads(nt, rt, bt)
        loss = loss_of(batch_t, head, nt, rt, bt, filt, reduction="none")
        assert (loss.detach().cpu().numpy() == 0.0).all(), loss
        loss.mean().backward()
        for t in [nt, rt] + [b for b in bt if b is not None]:
            assert t.grad is not None and (t.grad.cpu().numpy() == 0.0).all()


def test_a_list_of_the_targets_alone_changes_nothing():
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=(False, False, False))
    batch_t = dev(batch)
    for head in (True, False):
        filt = np.stack([np.arange(Q), batch[:, 0 if head else 2]], 1)
        plain = loss_of(batch_t, head, nt, rt, bt, None, reduction="none").cpu().numpy()
        listed = loss_of(batch_t, head, nt, rt, bt, filt, reduction="none").cpu().numpy()
        assert np.array_equal(plain, listed)


# ----------------------------------------------------------------------------- 5. ragged edge
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", [(130, 3, 8), (257, 129, 50)])
def test_the_last_entity_scores_highest(N, Q, dim, biased):
    """the rows past N of the last tile are clamped copies of row N - 1: were they counted, every lse would move by log(#copies).  Column 0
    of the anchors and the relations is 1 and nodes[N - 1] = 60 e_0, so the last entity's score is 60 or more for every query"""
    _, nodes, rel, bias, batch = make_case(N, Q, dim, biased, "fp32")
    nodes, rel = nodes.copy(), rel.copy()
    rel[:, 0] = 1.0
    nodes[np.unique(batch[:, [0, 2]]), 0] = 1.0
    nodes[N - 1] = 0.0
    nodes[N - 1, 0] = 60.0
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        ref = Ref(nodes, rel, bias, batch, head, None)
        assert (ref.scores.argmax(1) == N - 1).all() and (ref.scores[:, N - 1] >= 55).all()
        zero_grads(nt, rt, bt)
        loss = loss_of(batch_t, head, nt, rt, bt, None, reduction="none")
        close(loss.detach().cpu().numpy(), ref.loss, f"ragged N={N} b={biased} head={head} loss")
        loss.mean().backward()
        check_grads(ref, head, nt, rt, bt, f"ragged N={N} b={biased} head={head}")


# ----------------------------------------------------------------------------- 6. strips and chunks
def test_strips_and_chunks():
    from torch_rgcn import _native, functional
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    budgets = {1: 4 * Q * N, 3: 4 * Q * 256, 6: 1}
    for n_chunks, budget in budgets.items():
        plan = functional.softmax_chunk_plan(Q, N, budget)
        assert len(plan) == n_chunks and (n_chunks == 1 or plan[-1][1] % 128 != 0), plan
    for head in (True, False):
        filt, ref = filts[head], refs[head, True]
        for strips in (1, 2, 7, 0):
            loss = loss_of(batch_t, head, nt, rt, bt, filt, reduction="none", strips=strips)
            close(loss.detach().cpu().numpy(), ref.loss, f"strips={strips} head={head} loss")
        for n_chunks, budget in budgets.items():
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, filt, chunk_bytes=budget)
            loss.backward(gradient=functional.unit_gradient(loss.device))
            check_grads(ref, head, nt, rt, bt, f"chunks={n_chunks} head={head}")
        # the gradient cells themselves: every row of dS sums to zero
        fq, fn = lists_of(filt)
        with torch.no_grad():
            lse, _ = _native.distmult_lse(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn)
            g = torch.full((), 3.0, device=DEV)
            scale = 3.0 / Q
            for budget in budgets.values():
                rows = np.zeros(Q)
                for c_first, c_count in functional.softmax_chunk_plan(Q, N, budget):
                    dS = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, fq, fn, lse, g, Q, c_first, c_count)
                    assert dS.shape == (Q, c_count)
                    cells = dS.cpu().numpy().astype(np.float64)
                    assert (cells[ref.mask[:, c_first:c_first + c_count]] == 0.0).all()
                    rows += cells.sum(1)
                assert np.abs(rows).max() <= BOUND * scale, np.abs(rows).max()


# ----------------------------------------------------------------------------- 7. no score matrix
def test_no_score_matrix_at_fifty_thousand_entities():
    """1,024 queries x 50,000 entities: forward + backward stay below a quarter of the 205 MB of the fp32 logits (the route's own
    buffers -- the 8 MiB chunk, dnodes, the workspaces -- come to about 20 MB)"""
    from torch_rgcn import functional
    N, Q, dim = 50_000, 1_024, 32
    g = torch.Generator().manual_seed(5)
    nodes = (0.3 * torch.randn(N, dim, generator=g)).to(DEV).requires_grad_(True)
    rel = torch.randn(R0, dim, generator=g).to(DEV).requires_grad_(True)
    batch = torch.stack([torch.randint(0, N, (Q,), generator=g), torch.randint(0, R0, (Q,), generator=g),
                         torch.randint(0, N, (Q,), generator=g)], 1).to(DEV)
    assert len(functional.softmax_chunk_plan(Q, N, 8 << 20)) > 20
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    loss = functional.distmult_softmax_loss(batch, False, nodes, rel, chunk_bytes=8 << 20)
    loss.backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[softmax_loss] peak memory rise {rise} bytes; the logits of this batch = {4 * Q * N}")
    assert rise < Q * N, rise
    assert torch.isfinite(loss) and torch.isfinite(nodes.grad).all() and torch.isfinite(rel.grad).all()
    # the answer is right as well: a slice of the queries against float64
    sub = slice(0, 64)
    n64, r64, b = nodes.detach().cpu().double(), rel.detach().cpu().double(), batch.cpu()
    s = (n64[b[sub, 0]] * r64[b[sub, 1]]) @ n64.T
    want = torch.logsumexp(s, 1) - s[torch.arange(64), b[sub, 2]]
    got = functional.distmult_softmax_loss(batch[sub], False, nodes.detach(), rel.detach(), reduction="none")
    close(got.cpu().numpy(), want.numpy(), "N=50000 loss of 64 queries")


# ----------------------------------------------------------------------------- 8. no host synchronisation
def test_forward_and_backward_issue_no_synchronisation():
    from torch_rgcn import _native, functional, routes
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, _, refs = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    with routes.override(deferred_checks="1"):
        def step():
            zero_grads(nt, rt, bt)
            loss = 0.5 * (loss_of(batch_t, False, nt, rt, bt, chunk_bytes=4 * Q * 256) + loss_of(batch_t, True, nt, rt, bt))
            loss.backward(gradient=functional.unit_gradient(loss.device))
            return loss
        step()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        _native.check_deferred_errors()
        close(loss.detach().cpu().numpy(), 0.5 * (refs[False, False].loss.mean() + refs[True, False].loss.mean()), "sync-free loss")


# ----------------------------------------------------------------------------- 9. guard bands
def test_under_guard_bands(monkeypatch):
    """every buffer between two poisoned bands, the library's torch.empty buffers full of NaN before the call: nothing is stored past a
    buffer and no band value reaches a result"""
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True)
    got = {}
    with gb.Guard(monkeypatch) as guard:
        put = lambda a, dt=None: None if a is None else guard.home(dev(a, dt))  # noqa: E731
        nt, rt, bt = params_on_device(nodes, rel, bias, put=put)
        batch_t = put(batch)
        assert torch.isnan(torch.empty(3, device=DEV)).all()
        for head in (True, False):
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, filts[head], put=put, reduction="none", chunk_bytes=4 * Q * 128)
            loss.mean().backward()
            got[head] = (loss.detach().cpu().numpy(), nt.grad.cpu().numpy(), rt.grad.cpu().numpy(), [b.grad.cpu().numpy() for b in bt])
        problems = guard.problems(f"softmax loss N={N} Q={Q} d={dim}")
    assert not problems, "\n".join(problems)
    for head in (True, False):
        ref = refs[head, True]
        loss, dn, dr, db = got[head]
        close(loss, ref.loss, f"guarded head={head} loss")
        close(dn, ref.dnodes, f"guarded head={head} dnodes")
        close(dr, ref.drel, f"guarded head={head} drel")
        close(db[0 if head else 2], ref.dbias[0 if head else 2], f"guarded head={head} candidate bias")
        assert all(np.isfinite(x).all() for x in db)


# ----------------------------------------------------------------------------- the layer, bf16 policy, errors
def test_distmult_layer_passes_its_parameters_on():
    from torch_rgcn.layers import DistMult
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True)
    dm = DistMult(R0, dim, N, R0, b_init="ones").to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        for n, b in zip(("sbias", "pbias", "obias"), bias):
            getattr(dm, n).copy_(torch.from_numpy(b))
    nt = dev(nodes).requires_grad_(True)
    fq, fn = lists_of(filts[True])
    loss = dm.softmax_loss(torch.from_numpy(batch), nt, head=True, filt_q=fq, filt_n=fn, reduction="none")
    close(loss.detach().cpu().numpy(), refs[True, True].loss, "layer loss")
    loss.mean().backward()
    close(nt.grad.cpu().numpy(), refs[True, True].dnodes, "layer dnodes")
    close(dm.relations.grad.cpu().numpy(), refs[True, True].drel, "layer drel")
    close(dm.sbias.grad.cpu().numpy(), refs[True, True].dbias[0], "layer dsbias")
    plain = DistMult(R0, dim, N, R0).to(DEV)
    with torch.no_grad():
        plain.relations.copy_(torch.from_numpy(rel))
    unbiased = Ref(nodes, rel, [None] * 3, batch, False, None, grads=False)
    close(plain.softmax_loss(dev(batch), dev(nodes)).detach().cpu().numpy(), unbiased.loss.mean(), "layer, unbiased mean")


def test_bf16_nodes_that_require_grad_take_the_fp32_route():
    """the upcast policy: bf16 parameters are widened, the fp32 kernels run, dnodes comes back in bf16 (rounded once)"""
    from torch_rgcn import _native
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, _, refs = case_and_refs(N, Q, dim, True, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    _native.profile_start()
    loss = loss_of(dev(batch), False, nt, rt, bt)
    loss.backward()
    tags = set(_native.profile_stop())
    assert "lse_fused" in tags and "lse_fused_bf16" not in tags and "softmax_grad" in tags, tags
    assert nt.grad.dtype == BF and rt.grad.dtype == torch.float32
    ref = refs[False, False]
    close(loss.detach().cpu().numpy(), ref.loss.mean(), "bf16 upcast loss")
    err, norm = rel_err(nt.grad.float().cpu().numpy(), ref.dnodes)
    assert err <= 2.0 ** -8 * norm, (err, norm)                             # one rounding to bf16 (8 significand bits) of a gradient within BOUND


def test_wrapper_argument_errors():
    from torch_rgcn import _native, functional
    nodes, rel = torch.randn(10, 8, device=DEV), torch.randn(3, 8, device=DEV)
    ok = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    i32 = lambda *v: torch.tensor(v, device=DEV, dtype=torch.int32)  # noqa: E731
    for bad in ([[0, 3, 2]], [[10, 1, 2]], [[0, 1, -1]]):
        with pytest.raises((AssertionError, IndexError)):
            _native.distmult_lse(torch.tensor(bad, device=DEV), True, nodes, rel)
    for fq, fn in ((i32(2), i32(0)), (i32(-1), i32(0)), (i32(0), i32(10)), (i32(0), i32(-1))):
        with pytest.raises(IndexError):
            _native.distmult_lse(ok, True, nodes, rel, filt_q=fq, filt_n=fn)
    with pytest.raises(RuntimeError):
        _native.distmult_lse(ok.cpu(), True, nodes, rel)                                           # no CPU path
    with pytest.raises(AssertionError):
        _native.distmult_lse(ok, True, nodes, rel, torch.zeros(10, device=DEV), None, None)        # biases: all or none
    for kw in ({"strips": -1}, {"filt_q": i32(0)}):
        with pytest.raises(AssertionError):
            _native.distmult_lse(ok, True, nodes, rel, **kw)
    with pytest.raises(ValueError):
        functional.distmult_softmax_loss(ok, True, nodes, rel, reduction="sum")
    lse, tscore = _native.distmult_lse(ok[:0], True, nodes, rel)                                   # Q = 0: empty outputs
    assert lse.shape == tscore.shape == (0,)
    L = _native.lib()
    st = _native._stream(nodes.device)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    lse, g = torch.zeros(2, device=DEV), torch.ones(1, device=DEV)
    dS = torch.full((2, 10), -7.0, device=DEV)
    ws = torch.empty(_native.lse_workspace_bytes(2, 10, 8) + 1024, device=DEV, dtype=torch.uint8)

    def grad(c_first=0, c_count=10, mean_over=2, w=p(ws), out=p(dS)):
        return L.rgcn_distmult_softmax_grad_f32(p(ok), 2, 1, p(nodes), p(rel), None, None, None, None, None, 0, None, None, None, 0, p(lse), p(g), 0,
                                                mean_over, c_first, c_count, w, out, 10, 3, 8, st)
    assert grad(c_first=64) == _native.EINVAL and grad(c_first=128) == _native.EINVAL and grad(c_count=11) == _native.EINVAL
    assert grad(c_count=0) == _native.EINVAL and grad(mean_over=0) == _native.EINVAL and grad(w=None) == _native.EINVAL
    assert grad(out=None) == _native.EINVAL and grad(w=p(ws) + 4) == _native.EINVAL
    assert b"distmult_softmax_grad" in L.rgcn_last_error()
    torch.cuda.synchronize()
    assert (dS == -7.0).all()                                                                      # nothing was launched
    assert grad() == _native.OK
    torch.cuda.synchronize()
    assert torch.isfinite(dS).all()
