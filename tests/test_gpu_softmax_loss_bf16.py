"""Native bf16 backward of the 1-N softmax loss: functional.distmult_softmax_loss(..., bf16_backward="native") on a
bf16 entity table -- the bf16 strip forward, the bf16 gradient-cell kernel, fp32 contractions, dnodes rounded to bf16 once -- against
float64 on the CPU.  The case builder, the float64 reference and the comparison are those of test_gpu_softmax_loss.py, imported; the
reference for bf16 storage is float64 on the table ROUNDED to bf16 (case_and_refs(..., storage="bf16")).

Bounds.  Everything that stays fp32 (the loss, the gradient cells, drel, the bias gradients): the suite's parity bound, 1e-4 relative in
the max norm.  dnodes is bf16, one rounding of an fp32 gradient that is within 1e-4 of the reference: max |err| <= 2^-8 max |ref|, the
bound test_bf16_nodes_that_require_grad_take_the_fp32_route uses for the upcast route.  (A rounding to bf16 errs by half an ulp, at most
2^-8 of the lower end of the element's binade; the largest observed figure, 3.89e-3 = 0.995 of the bound, is such a half ulp in the
binade of a max norm just above a power of two, 0.1255.)"""
import functools

import numpy as np
import pytest
import torch

import guard_bands as gb
import torch_rgcn  # noqa: F401  (at collection, before the first HIP call: REPLAY_SAFE is decided then, torch_rgcn/__init__.py)
from test_gpu_softmax_loss import (BF, BOUND, DEV, R0, SHAPES, Ref, _random_streams_left_as_found, case_and_refs, check_grads,  # noqa: F401
                                   close, dev, lists_of, loss_of, make_case, params_on_device, rel_err, zero_grads)

pytestmark = pytest.mark.gpu

BF_BOUND = 2.0 ** -8


def native_loss(batch_t, head, nt, rt, bt, filt=None, put=dev, **kw):
    return loss_of(batch_t, head, nt, rt, bt, filt, put=put, bf16_backward="native", **kw)


def close_bf16(got, want, what):
    """a bf16 gradient against float64: max |got - want| <= 2^-8 max |want|"""
    assert got.dtype == BF, (what, got.dtype)
    got = got.float().cpu().numpy()
    err, norm = rel_err(got, want)
    print(f"[softmax_loss_bf16] {what}: max err {err:.3e}, norm {norm:.3e}, relative {err / norm if norm else 0.0:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= BF_BOUND * norm, (what, err, norm)


def check_native_grads(ref, head, nt, rt, bt, what):
    """dnodes (bf16) within 2^-8; drel and the bias gradients (fp32) as check_grads checks them"""
    dn = nt.grad
    if dn is not None:
        close_bf16(dn, ref.dnodes, what + " dnodes")
    nt.grad = None
    try:
        assert rt.grad is None or rt.grad.dtype == torch.float32
        check_grads(ref, head, nt, rt, bt, what)
    finally:
        nt.grad = dn


@functools.lru_cache(maxsize=None)
def known_of(N, Q, dim, biased, integer=False):
    """known triples around the case's batch (the batch itself and about 3 Q triples that share a query's (s, p) or (p, o)), the host
    index that turns them into filter lists, and the float64 references under that filter; computed once and shared"""
    from utils.misc import _FilterIndex, generate_true_dict
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, biased, "bf16", integer)
    rng = np.random.default_rng(17 * N + Q)
    more = batch[rng.integers(0, Q, 3 * Q)].copy()
    half = len(more) // 2
    more[:half, 0] = rng.integers(0, N, half)
    more[half:, 2] = rng.integers(0, N, len(more) - half)
    true = generate_true_dict(np.concatenate([batch, more]))
    lists_index = _FilterIndex(true, N)
    filts = {}
    for head in (True, False):
        rows, cols = lists_index.lists(batch, head, keep_target=False)
        filts[head] = np.stack([np.asarray(rows, np.int64), np.asarray(cols, np.int64)], 1)
    refs = {head: Ref(nodes, rel, bias, batch, head, filts[head]) for head in (True, False)} if not integer else None
    return true, filts, refs


def ref_cells(ref, batch, head, scale):
    """float64 scale_q (softmax - onehot) over the allowed cells, masked cells 0"""
    s = np.where(ref.mask, -np.inf, ref.scores)
    p = np.exp(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    p[np.arange(len(batch)), batch[:, 0 if head else 2]] -= 1.0
    out = np.asarray(scale, np.float64).reshape(-1, 1) * p
    out[ref.mask] = 0.0
    return out


# ----------------------------------------------------------------------------- 1. gradient cells
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_gradient_cells(N, Q, dim, biased):
    """one chunk with a scalar upstream gradient, and chunks of one tile column with a per-query one"""
    from torch_rgcn import _native, functional
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, biased, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16", grad=(False, False, False))
    batch_t = dev(batch)
    gq = np.random.default_rng(N + dim).uniform(0.5, 2.0, Q).astype(np.float32)
    for head in (True, False):
        for filtered in (True, False):
            ref = refs[head, filtered]
            fq, fn = lists_of(filts[head] if filtered else None)
            lse, _ = _native.distmult_lse(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn)
            for budget, g, scale in ((4 * Q * N, torch.full((), 3.0, device=DEV), np.full(Q, 3.0 / Q)), (1, dev(gq), gq.astype(np.float64) / Q)):
                plan = functional.softmax_chunk_plan(Q, N, budget)
                cells = np.full((Q, N), np.nan)
                _native.profile_start()
                for c_first, c_count in plan:
                    dS = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, fq, fn, lse, g, Q, c_first, c_count)
                    assert dS.shape == (Q, c_count) and dS.dtype == torch.float32
                    cells[:, c_first:c_first + c_count] = dS.cpu().numpy()
                assert set(_native.profile_stop()) == {"softmax_grad_bf16"}
                what = f"N={N} Q={Q} d={dim} b={biased} head={head} filt={filtered} chunks={len(plan)}"
                close(cells, ref_cells(ref, batch, head, scale), what + " dS")
                assert (cells[ref.mask] == 0.0).all(), what
                rows = np.abs(cells.sum(1)).max()
                assert rows <= BOUND * scale.max(), (what, rows)


# ----------------------------------------------------------------------------- 2. the bits of the fp32 kernel on exact inputs
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", [(77, 10, 500), (257, 129, 50)])
def test_same_bits_as_the_fp32_kernel_on_integer_inputs(N, Q, dim, biased):
    """small integers are exact in bf16 and every partial sum is exact in either product: with the same lse both kernels compute the same
    s and run the same epilogue"""
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, filts, _ = case_and_refs(N, Q, dim, biased, "bf16", True)
    true, _, _ = known_of(N, Q, dim, biased, True)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16", grad=(False, False, False))
    wide = nt.float()
    assert np.array_equal(wide.cpu().numpy(), nodes)
    batch_t = dev(batch)
    g = torch.full((), 3.0, device=DEV)
    for head in (True, False):
        for form in ("none", "lists", "index"):
            fq, fn = lists_of(filts[head]) if form == "lists" else (None, None)
            kw = {"filt": index} if form == "index" else {}
            lse, _ = _native.distmult_lse(batch_t, head, wide, rt, *bt, filt_q=fq, filt_n=fn, **kw)
            for c_first, c_count in functional.softmax_chunk_plan(Q, N, 4 * Q * 128):
                want = _native.distmult_softmax_grad(batch_t, head, wide, rt, *bt, fq, fn, lse, g, Q, c_first, c_count, **kw).cpu().numpy()
                got = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, fq, fn, lse, g, Q, c_first, c_count, **kw).cpu().numpy()
                assert np.isfinite(want).all() and np.abs(want).max() > 0
                assert np.array_equal(got, want), (head, form, c_first, np.abs(got - want).max())


# ----------------------------------------------------------------------------- 3. loss and gradients
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_loss_and_gradient_parity(N, Q, dim, biased):
    """everything requires grad: reduction='none' then .mean() (a [Q] upstream gradient) and reduction='mean' from the unit gradient"""
    from torch_rgcn import _native, functional
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, biased, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    batch_t = dev(batch)
    for head in (True, False):
        for filtered in (True, False):
            filt, ref = filts[head] if filtered else None, refs[head, filtered]
            what = f"native N={N} Q={Q} d={dim} b={biased} head={head} filt={filtered}"
            zero_grads(nt, rt, bt)
            _native.profile_start()
            loss = native_loss(batch_t, head, nt, rt, bt, filt, reduction="none")
            loss.mean().backward()
            tags = set(_native.profile_stop())
            assert tags == {"lse_fused_bf16", "softmax_grad_bf16", "gemm"}, tags
            assert loss.dtype == torch.float32
            close(loss.detach().cpu().numpy(), ref.loss, what + " loss")
            check_native_grads(ref, head, nt, rt, bt, what + " [none]")
            zero_grads(nt, rt, bt)
            loss = native_loss(batch_t, head, nt, rt, bt, filt)
            loss.backward(gradient=functional.unit_gradient(loss.device))
            close(loss.detach().cpu().numpy(), ref.loss.mean(), what + " mean loss")
            check_native_grads(ref, head, nt, rt, bt, what + " [mean]")


# ----------------------------------------------------------------------------- 4. frozen inputs
@pytest.mark.parametrize("only", ["nodes", "relations"])
def test_gradient_parity_with_frozen_inputs(only):
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16", grad=(only == "nodes", only == "relations", False))
    batch_t = dev(batch)
    for head in (True, False):
        zero_grads(nt, rt, bt)
        native_loss(batch_t, head, nt, rt, bt, filts[head]).backward()
        assert (nt.grad is not None) == (only == "nodes") and (rt.grad is not None) == (only == "relations")
        assert all(b.grad is None for b in bt)
        check_native_grads(refs[head, True], head, nt, rt, bt, f"native, only {only} head={head}")


# ----------------------------------------------------------------------------- 5. mask
@pytest.mark.parametrize("biased", [False, True])
def test_everything_but_the_target_filtered_is_exactly_zero(biased):
    """lse == tscore bit for bit and exp(0) - 1 == 0 in the bf16 kernels too: the loss and every gradient are exactly zero"""
    N, Q, dim = 130, 3, 8
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, biased, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    batch_t = dev(batch)
    for head in (True, False):
        tgt = batch[:, 0 if head else 2]
        filt = np.array([(q, n) for q in range(Q) for n in range(N) if n != tgt[q]])
        zero_grads(nt, rt, bt)
        loss = native_loss(batch_t, head, nt, rt, bt, filt, reduction="none")
        assert (loss.detach().cpu().numpy() == 0.0).all(), loss
        loss.mean().backward()
        assert nt.grad.dtype == BF
        for t in [nt, rt] + [b for b in bt if b is not None]:
            assert t.grad is not None and (t.grad.float().cpu().numpy() == 0.0).all()


# ----------------------------------------------------------------------------- 6. ragged edge
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", [(130, 3, 8), (257, 129, 50)])
def test_the_last_entity_scores_highest(N, Q, dim, biased):
    """the construction of test_gpu_softmax_loss.py (the rows past N of the last tile are clamped copies of row N - 1, which scores 60 or
    more for every query); 60, 1 and 0 are exact in bf16, so the table stays a bf16 table"""
    _, nodes, rel, bias, batch = make_case(N, Q, dim, biased, "bf16")
    nodes, rel = nodes.copy(), rel.copy()
    rel[:, 0] = 1.0
    nodes[np.unique(batch[:, [0, 2]]), 0] = 1.0
    nodes[N - 1] = 0.0
    nodes[N - 1, 0] = 60.0
    assert np.array_equal(torch.from_numpy(nodes).to(BF).float().numpy(), nodes)
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    batch_t = dev(batch)
    for head in (True, False):
        ref = Ref(nodes, rel, bias, batch, head, None)
        assert (ref.scores.argmax(1) == N - 1).all() and (ref.scores[:, N - 1] >= 55).all()
        zero_grads(nt, rt, bt)
        loss = native_loss(batch_t, head, nt, rt, bt, None, reduction="none")
        close(loss.detach().cpu().numpy(), ref.loss, f"native ragged N={N} b={biased} head={head} loss")
        loss.mean().backward()
        check_native_grads(ref, head, nt, rt, bt, f"native ragged N={N} b={biased} head={head}")


# ----------------------------------------------------------------------------- 7. chunks
def test_chunks():
    from torch_rgcn import _native, functional
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    batch_t = dev(batch)
    budgets = {1: 4 * Q * N, 3: 4 * Q * 256, 6: 1}
    for head in (True, False):
        for n_chunks, budget in budgets.items():
            assert len(functional.softmax_chunk_plan(Q, N, budget)) == n_chunks
            zero_grads(nt, rt, bt)
            _native.profile_start()
            loss = native_loss(batch_t, head, nt, rt, bt, filts[head], chunk_bytes=budget)
            loss.backward(gradient=functional.unit_gradient(loss.device))
            assert len(_native.profile_stop()["softmax_grad_bf16"]) == n_chunks
            close(loss.detach().cpu().numpy(), refs[head, True].loss.mean(), f"native chunks={n_chunks} head={head} loss")
            check_native_grads(refs[head, True], head, nt, rt, bt, f"native chunks={n_chunks} head={head}")


# ----------------------------------------------------------------------------- 8. lists and index
@pytest.mark.parametrize("N,Q,dim", [(700, 130, 24), (257, 129, 50)])
def test_the_index_form_equals_the_list_form(N, Q, dim):
    """the filter decides which cells are excluded and nothing else: the loss and the gradient cells are bit-identical"""
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, True, "bf16")
    true, filts, refs = known_of(N, Q, dim, True)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    batch_t = dev(batch)
    g = torch.full((), 3.0, device=DEV)
    for head in (True, False):
        fq, fn = lists_of(filts[head])
        assert fq is not None and len(fq) > Q
        for reduction in ("none", "mean"):
            zero_grads(nt, rt, bt)
            want = native_loss(batch_t, head, nt, rt, bt, filts[head], reduction=reduction)
            _native.profile_start()
            got = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt=index, reduction=reduction, bf16_backward="native")
            got.mean().backward()
            tags = set(_native.profile_stop())
            assert tags == {"lse_fused_index_bf16", "softmax_grad_index_bf16", "gemm"}, tags
            assert torch.equal(got, want), (head, reduction)
            check_native_grads(refs[head], head, nt, rt, bt, f"native index N={N} head={head} [{reduction}]")
        close(got.detach().cpu().numpy(), refs[head].loss.mean(), f"native index N={N} head={head} loss")
        with torch.no_grad():
            lse, _ = _native.distmult_lse(batch_t, head, nt, rt, *bt, filt=index)
            masked = 0
            for c_first, c_count in functional.softmax_chunk_plan(Q, N, 4 * Q * 256):
                want = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, fq, fn, lse, g, Q, c_first, c_count).clone()
                got = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, None, None, lse, g, Q, c_first, c_count, filt=index)
                assert torch.equal(got, want), (head, c_first)
                masked += int((got == 0).sum())
            assert masked >= Q, (head, masked)                                # the filter does something (the last chunk may be one column)


# ----------------------------------------------------------------------------- 9. no fp32 table
def test_no_fp32_table_at_fifty_thousand_entities():
    """1,024 queries x 50,000 entities, d = 32, a bf16 leaf: between the forward and the backward the native route holds less than a
    quarter of the fp32 copy of the table that the upcast route holds there; forward + backward stay below a quarter of the logits"""
    from torch_rgcn import functional
    N, Q, dim = 50_000, 1_024, 32
    g = torch.Generator().manual_seed(5)
    nodes = (0.3 * torch.randn(N, dim, generator=g)).to(DEV).to(BF).requires_grad_(True)
    rel = torch.randn(R0, dim, generator=g).to(DEV).requires_grad_(True)
    batch = torch.stack([torch.randint(0, N, (Q,), generator=g), torch.randint(0, R0, (Q,), generator=g),
                         torch.randint(0, N, (Q,), generator=g)], 1).to(DEV)
    assert len(functional.softmax_chunk_plan(Q, N, 8 << 20)) > 20

    def run(route):
        nodes.grad = rel.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = functional.distmult_softmax_loss(batch, False, nodes, rel, chunk_bytes=8 << 20, bf16_backward=route)
        torch.cuda.synchronize()
        held = torch.cuda.memory_allocated() - before
        loss.backward()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        print(f"[softmax_loss_bf16] {route}: held between forward and backward {held} bytes, peak rise {rise} bytes; the fp32 table = "
              f"{4 * N * dim}, the logits of this batch = {4 * Q * N}")
        assert torch.isfinite(loss) and nodes.grad.dtype == BF and torch.isfinite(nodes.grad.float()).all() and torch.isfinite(rel.grad).all()
        return held, rise, loss.detach().clone()

    held, rise, loss = run("native")
    assert held < N * dim, held
    assert rise < Q * N, rise
    held_up, _, loss_up = run("upcast")
    assert held_up >= 4 * N * dim, held_up
    close(loss.cpu().numpy(), loss_up.cpu().numpy(), "N=50000 native loss against the upcast route's")
    # the answer is right as well: a slice of the queries against float64 on the bf16 table
    nodes.grad = rel.grad = None
    sub = slice(0, 64)
    n64, r64, b = nodes.detach().float().cpu().double(), rel.detach().cpu().double(), batch.cpu()
    s = (n64[b[sub, 0]] * r64[b[sub, 1]]) @ n64.T
    want = torch.logsumexp(s, 1) - s[torch.arange(64), b[sub, 2]]
    got = functional.distmult_softmax_loss(batch[sub], False, nodes, rel, reduction="none", bf16_backward="native")
    close(got.detach().cpu().numpy(), want.numpy(), "N=50000 native loss of 64 queries")


# ----------------------------------------------------------------------------- 10. no host synchronisation, capture
def _filtered_step_case():
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, True, "bf16")
    true, _, refs = known_of(N, Q, dim, True)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    batch_t = dev(batch)
    budget = 4 * Q * 256

    def losses():
        from torch_rgcn import functional
        return 0.5 * (functional.distmult_softmax_loss(batch_t, False, nt, rt, *bt, filt=index, chunk_bytes=budget, bf16_backward="native") +
                      functional.distmult_softmax_loss(batch_t, True, nt, rt, *bt, filt=index, chunk_bytes=budget, bf16_backward="native"))
    want = 0.5 * (refs[False].loss.mean() + refs[True].loss.mean())
    return nt, rt, bt, losses, want


def test_forward_and_backward_issue_no_synchronisation():
    from torch_rgcn import _native, functional, routes
    nt, rt, bt, losses, want = _filtered_step_case()
    with routes.override(deferred_checks="1"):
        def step():
            zero_grads(nt, rt, bt)
            loss = losses()
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
    close(loss.detach().cpu().numpy(), want, "native sync-free loss")
    assert nt.grad.dtype == BF and torch.isfinite(nt.grad.float()).all()


def test_the_native_step_captured_in_a_hipgraph_matches_eager():
    """head + tail native loss with a FilterIndex and three chunks, forward + backward, captured after a warm-up on a side stream and
    replayed; the eager reference step runs AFTER the replays (test_gpu_bf16_lp.py says why).  A capture that fails raises: there is no
    eager fallback to hide behind in this test."""
    from torch_rgcn import functional, routes
    if not torch_rgcn.REPLAY_SAFE:
        pytest.skip("replays of a captured step are not safe in this process (torch_rgcn.REPLAY_SAFE)")
    nt, rt, bt, losses, want = _filtered_step_case()
    params = [nt, rt] + bt
    for t in params:
        t.grad = torch.zeros_like(t)

    def step():
        for t in params:
            t.grad.zero_()
        loss = losses()
        loss.backward(gradient=functional.unit_gradient(loss.device))
        return loss

    with routes.override(deferred_checks="1"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = step()
    replayed = []
    for _ in range(2):
        junk = (torch.arange(50_000, device=DEV) % 3).float() * torch.rand(50_000, device=DEV)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(junk).all()
        replayed.append((static_loss.detach().clone(), nt.grad.clone(), rt.grad.clone()))
    del graph, static_loss
    loss = step()
    torch.cuda.synchronize()
    eager_dn = nt.grad.float().cpu().numpy()
    for got_loss, got_dn, got_dr in replayed:
        close(got_loss.cpu().numpy(), loss.detach().cpu().numpy(), "captured native loss against eager")
        close(got_loss.cpu().numpy(), want, "captured native loss against float64")
        close_bf16(got_dn, eager_dn, "captured native dnodes against eager")
        close(got_dr.cpu().numpy(), rt.grad.cpu().numpy(), "captured native drel against eager")


# ----------------------------------------------------------------------------- 11. guard bands
@pytest.mark.parametrize("N,Q,dim", [(257, 129, 50), (700, 130, 24)])
def test_under_guard_bands(N, Q, dim, monkeypatch):
    """every buffer between two poisoned bands, the library's torch.empty buffers full of NaN before the call: nothing is stored past a
    buffer and no band value reaches a result (one tile column per chunk: several chunks, the last one ragged)"""
    nodes, rel, bias, batch, filts, refs = case_and_refs(N, Q, dim, True, "bf16")
    got = {}
    with gb.Guard(monkeypatch) as guard:
        put = lambda a, dt=None: None if a is None else guard.home(dev(a, dt))  # noqa: E731
        nt, rt, bt = params_on_device(nodes, rel, bias, "bf16", put=put)
        batch_t = put(batch)
        assert torch.isnan(torch.empty(3, device=DEV)).all()
        for head in (True, False):
            zero_grads(nt, rt, bt)
            loss = native_loss(batch_t, head, nt, rt, bt, filts[head], put=put, reduction="none", chunk_bytes=4 * Q * 128)
            loss.mean().backward()
            got[head] = (loss.detach().cpu().numpy(), nt.grad.clone(), rt.grad.cpu().numpy(), [b.grad.cpu().numpy() for b in bt])
        problems = guard.problems(f"native bf16 softmax loss N={N} Q={Q} d={dim}")
    assert not problems, "\n".join(problems)
    for head in (True, False):
        ref = refs[head, True]
        loss, dn, dr, db = got[head]
        close(loss, ref.loss, f"guarded native head={head} loss")
        close_bf16(dn, ref.dnodes, f"guarded native head={head} dnodes")
        close(dr, ref.drel, f"guarded native head={head} drel")
        close(db[0 if head else 2], ref.dbias[0 if head else 2], f"guarded native head={head} candidate bias")
        assert all(np.isfinite(x).all() for x in db)


# ----------------------------------------------------------------------------- 12. errors
def test_the_bf16_entry_points_refuse_what_the_fp32_ones_refuse():
    from torch_rgcn import _native
    nodes, rel = torch.randn(10, 8, device=DEV).to(BF), torch.randn(3, 8, device=DEV)
    ok = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    L = _native.lib()
    st = _native._stream(nodes.device)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    lse, g = torch.zeros(2, device=DEV), torch.ones(1, device=DEV)
    dS = torch.full((2, 10), -7.0, device=DEV)
    ws = torch.empty(L.rgcn_distmult_softmax_grad_workspace_bytes(2, 10, 8, 1) + 1024, device=DEV, dtype=torch.uint8)

    def lists(c_first=0, c_count=10, mean_over=2, w=p(ws), out=p(dS)):
        filt_q, filt_n, F = None, None, 0
        return L.rgcn_distmult_softmax_grad_bf16(p(ok), 2, 1, p(nodes), p(rel), None, None, None, filt_q, filt_n, F, None, None, None, 0, p(lse),
                                                 p(g), 0, mean_over, c_first, c_count, w, out, 10, 3, 8, st)

    def index(c_first=0, c_count=10, mean_over=2, w=p(ws), out=p(dS)):
        fkeys, fptr, fvals, K = None, None, None, 0
        return L.rgcn_distmult_softmax_grad_bf16(p(ok), 2, 1, p(nodes), p(rel), None, None, None, None, None, 0, fkeys, fptr, fvals, K, p(lse),
                                                 p(g), 0, mean_over, c_first, c_count, w, out, 10, 3, 8, st)

    for grad, name in ((lists, b"distmult_softmax_grad_bf16"), (index, b"distmult_softmax_grad_bf16")):
        for kw in ({"c_first": 64}, {"c_first": 128}, {"c_count": 11}, {"c_count": 0}, {"mean_over": 0}, {"w": None}, {"out": None},
                   {"w": p(ws) + 4}):
            assert grad(**kw) == _native.EINVAL, (name, kw)
            assert name in L.rgcn_last_error(), (name, kw, L.rgcn_last_error())
        torch.cuda.synchronize()
        assert (dS == -7.0).all()                                                                  # nothing was launched
    # biases partly set
    sb = torch.zeros(10, device=DEV)
    assert L.rgcn_distmult_softmax_grad_bf16(p(ok), 2, 1, p(nodes), p(rel), p(sb), None, None, None, None, 0, None, None, None, 0, p(lse), p(g), 0, 2,
                                             0, 10, p(ws), p(dS), 10, 3, 8, st) == _native.EINVAL
    # Q == 0 launches nothing
    assert L.rgcn_distmult_softmax_grad_bf16(None, 0, 1, p(nodes), p(rel), None, None, None, None, None, 0, None, None, None, 0, None, None, 0, 2, 0, 10,
                                             p(ws), None, 10, 3, 8, st) == _native.OK
    torch.cuda.synchronize()
    assert (dS == -7.0).all()
    for grad in (lists, index):
        dS.fill_(-7.0)
        assert grad() == _native.OK
        torch.cuda.synchronize()
        assert torch.isfinite(dS).all() and (dS != -7.0).all()


def test_bf16_backward_keyword():
    from torch_rgcn import _native, functional
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, _ = case_and_refs(N, Q, dim, True)
    batch_t = dev(batch)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    with pytest.raises(ValueError, match="bf16_backward"):
        loss_of(batch_t, False, nt, rt, bt, bf16_backward="fast")
    # fp32 nodes: the keyword has no effect
    for head in (True, False):
        want = loss_of(batch_t, head, nt, rt, bt, filts[head], reduction="none")
        _native.profile_start()
        got = native_loss(batch_t, head, nt, rt, bt, filts[head], reduction="none")
        got.mean().backward()
        tags = set(_native.profile_stop())
        assert tags == {"lse_fused", "softmax_grad", "gemm"}, tags
        assert np.array_equal(got.detach().cpu().numpy(), want.detach().cpu().numpy())
        assert nt.grad.dtype == torch.float32
    # bf16 nodes, a plain call: the default is the upcast route
    nodes, rel, bias, batch, _, _ = case_and_refs(N, Q, dim, True, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16")
    for kw in ({}, {"bf16_backward": "upcast"}):
        _native.profile_start()
        loss_of(batch_t, False, nt, rt, bt, **kw).backward()
        tags = set(_native.profile_stop())
        assert tags == {"lse_fused", "softmax_grad", "gemm"}, tags


# ----------------------------------------------------------------------------- 13. the layer
def test_distmult_layer_in_bf16():
    from torch_rgcn import _native
    from torch_rgcn.layers import DistMult
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, _ = case_and_refs(N, Q, dim, True, "bf16")
    dm = DistMult(R0, dim, N, R0, b_init="ones").to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        for n, b in zip(("sbias", "pbias", "obias"), bias):
            getattr(dm, n).copy_(torch.from_numpy(b))
    dm = dm.bfloat16()
    names = ("sbias", "pbias", "obias")
    assert dm.relations.dtype == BF and all(getattr(dm, n).dtype == BF for n in names)
    rounded_rel = dm.relations.detach().float().cpu().numpy()                # the reference is formed from the layer's own rounded parameters
    rounded_bias = [getattr(dm, n).detach().float().cpu().numpy() for n in names]
    nt = dev(nodes, BF).requires_grad_(True)
    for head in (True, False):
        ref = Ref(nodes, rounded_rel, rounded_bias, batch, head, filts[head])
        fq, fn = lists_of(filts[head])
        dm.zero_grad(set_to_none=True)
        nt.grad = None
        _native.profile_start()
        loss = dm.softmax_loss(torch.from_numpy(batch), nt, head=head, filt_q=fq, filt_n=fn, reduction="none", bf16_backward="native")
        loss.mean().backward()
        tags = set(_native.profile_stop())
        assert tags == {"lse_fused_bf16", "softmax_grad_bf16", "gemm"}, tags
        close(loss.detach().cpu().numpy(), ref.loss, f"bf16 layer head={head} loss")
        close_bf16(nt.grad, ref.dnodes, f"bf16 layer head={head} dnodes")
        close_bf16(dm.relations.grad, ref.drel, f"bf16 layer head={head} drel")
        cand = 0 if head else 2
        close_bf16(getattr(dm, names[cand]).grad, ref.dbias[cand], f"bf16 layer head={head} d{names[cand]}")
        cand_norm = np.abs(ref.dbias[cand]).max()
        for k, n in enumerate(names):
            grad = getattr(dm, n).grad
            assert grad.dtype == BF and torch.isfinite(grad.float()).all()
            if k != cand:                                                     # sum_n dS[q, n] = 0
                assert grad.float().abs().max().item() <= BF_BOUND * cand_norm
