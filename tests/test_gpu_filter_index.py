"""Device-resident filter index: functional.FilterIndex and the `filt=` form of every filtered route against the list
form on the same known triples.  The filter decides which cells are excluded and nothing else, and with the same mask the product kernels
do the same arithmetic: every comparison in this file is exact -- masks word for word, results with torch.equal.  No tolerance anywhere.

The lists come from utils.misc._FilterIndex.lists, the host stage every filtered route used before.  Shapes, case builder and decoder
model are those of test_gpu_softmax_loss.py / test_gpu_topk.py, restated."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
R0 = 5
SHAPES = [(1, 1, 1), (63, 65, 6), (130, 3, 8), (257, 129, 50), (77, 10, 500), (700, 130, 24)]


@pytest.fixture(autouse=True)
def _random_streams_left_as_found():
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


def spo(anchor_p_comp, head):
    """(anchor, relation, completion) rows -> (s, p, o): a head query's anchor is its object, its completion the subject"""
    a = np.asarray(anchor_p_comp, np.int64).reshape(-1, 3)
    return a[:, ::-1].copy() if head else a.copy()


# ----------------------------------------------------------------------------- 1. the mask, word for word
@functools.lru_cache(maxsize=None)
def mask_scenario(N, head):
    """known triples on relations 1 and 3 only, and queries as (anchor, relation, target) rows -- the special ones first:
         a hub key (relation 1, anchor 0) with min(300, N) completions, the columns 0, 127, 128, 255, 256, N - 1 among them;
         a key (relation 3, anchor 0) with exactly min(64, N) completions;
         a key (relation 1, anchor N - 1) whose one completion is its query's target: nothing survives keep_target = 0;
         queries on relation 0 (before the first key), 4 (past the last) and 2 (between two keys): misses."""
    rng = np.random.default_rng(7 * N + head)
    edge = np.unique([c for c in (0, 127, 128, 255, 256, N - 1) if 0 <= c < N])
    rest = np.setdiff1d(np.arange(N), edge)
    hub = np.concatenate([edge, rng.permutation(rest)[:max(0, min(300, N) - len(edge))]])
    k64 = rng.permutation(N)[:min(64, N)]
    single = N // 2
    known = [(0, 1, c) for c in hub] + [(0, 3, c) for c in k64] + [(N - 1, 1, single)]
    if N >= 3:                                                                 # (anchors 0 and N - 1 keep the completions chosen above)
        known += [(rng.integers(1, N - 1), rng.choice([1, 3]), rng.integers(0, N)) for _ in range(3 * N)]
    known += known[:10]                                                        # duplicate triples
    outside = np.setdiff1d(np.arange(N), hub)
    special = [(0, 1, hub[0]), (0, 1, hub[0]),                                 # the target among the completions; the same query twice
               (N - 1, 1, single),
               (rng.integers(0, N), 0, rng.integers(0, N)), (rng.integers(0, N), 4, rng.integers(0, N)),
               (rng.integers(0, N), 2, rng.integers(0, N)),
               (0, 3, k64[-1]), (0, 1, hub[-1]), (0, 1, outside[0] if len(outside) else hub[0]), (0, 3, rng.integers(0, N))]
    special = special[N % 3:] + special[:N % 3]                                # (small Q: another head of the list for another N)
    random = [(rng.integers(0, N), rng.integers(0, R0), rng.integers(0, N)) for _ in range(130)]
    return spo(known, head), spo(special + random, head), len(hub)


def reference_mask(lists_index, batch, head, keep_target, c_first, c_count):
    rows, cols = lists_index.lists(batch, head, keep_target=keep_target)
    sel = (cols >= c_first) & (cols < c_first + c_count)
    rows, cols = rows[sel].astype(np.int64), cols[sel].astype(np.int64) - c_first
    mask = np.zeros((len(batch), (c_count + 31) // 32), np.uint32)
    np.bitwise_or.at(mask, (rows, cols >> 5), (np.uint32(1) << (cols & 31).astype(np.uint32)))
    return mask


def device_mask(index, batch, head, keep_target, c_first=0, c_count=None):
    from torch_rgcn import _native
    return _native.filter_mask_index(dev(batch), head, index, keep_target, c_first, c_count).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("Q", [1, 3, 65, 130])
@pytest.mark.parametrize("N", [1, 31, 32, 33, 129, 700])
def test_mask_word_for_word(N, Q):
    from torch_rgcn.functional import FilterIndex
    from utils.misc import _FilterIndex, generate_true_dict
    for head in (True, False):
        known, queries, n_hub = mask_scenario(N, head)
        true = generate_true_dict(known)
        lists_index, index = _FilterIndex(true, N), FilterIndex(true, N, DEV)
        batch = queries[:Q]
        assert n_hub == min(300, N)
        for keep_target in (False, True):
            want = reference_mask(lists_index, batch, head, keep_target, 0, N)
            got = device_mask(index, batch, head, keep_target)
            assert got.shape == want.shape == (Q, (N + 31) // 32)
            assert np.array_equal(got, want), (N, Q, head, keep_target, np.argwhere(got != want)[:5])
        if Q >= 65:                                                             # the scenario is what it claims to be
            kept = reference_mask(lists_index, batch, head, True, 0, N)
            dropped = reference_mask(lists_index, batch, head, False, 0, N)
            bits = lambda m: np.array([bin(int(w)).count("1") for w in m.reshape(-1)]).reshape(m.shape).sum(1)   # noqa: E731
            assert bits(kept).max() == n_hub and (bits(kept) == 0).any()
            assert (bits(kept) != bits(dropped)).any()                          # some target sits among its key's completions ...
            assert ((bits(kept) == 1) & (bits(dropped) == 0)).any() or N == 1   # ... and one key has nothing else


@pytest.mark.parametrize("N", [257, 700])
def test_mask_of_a_chunk_of_columns(N):
    """the gradient's chunks: the hub key has a completion at c_first - 1, c_first, c_end - 1 and c_end of every chunk"""
    from torch_rgcn.functional import FilterIndex
    from utils.misc import _FilterIndex, generate_true_dict
    for head in (True, False):
        known, queries, _ = mask_scenario(N, head)
        true = generate_true_dict(known)
        lists_index, index = _FilterIndex(true, N), FilterIndex(true, N, DEV)
        batch = queries[:65]
        hub = set(lists_index.lists(spo([(0, 1, 0)], head), head, keep_target=True)[1].tolist())
        for c_first, c_count in ((0, N), (128, 128), (128, N - 128)):
            c_end = c_first + c_count
            assert all(c in hub for c in (c_first - 1, c_first, c_end - 1, c_end) if 0 <= c < N)
            for keep_target in (False, True):
                want = reference_mask(lists_index, batch, head, keep_target, c_first, c_count)
                got = device_mask(index, batch, head, keep_target, c_first, c_count)
                assert np.array_equal(got, want), (N, head, c_first, c_count, keep_target, np.argwhere(got != want)[:5])
                assert want.any()


def test_an_index_without_keys_filters_nothing():
    from torch_rgcn.functional import FilterIndex
    from utils.misc import generate_true_dict
    index = FilterIndex(generate_true_dict(np.zeros((0, 3), np.int64)), 33, DEV)
    assert all(t[0].shape[0] == 0 for t in index.tables)
    _, queries, _ = mask_scenario(33, False)
    for head in (True, False):
        assert not device_mask(index, queries[:65], head, True).any()


# ----------------------------------------------------------------------------- 2. the routes, bit for bit
def make_case(N, Q, dim, biased, storage):
    rng = np.random.default_rng(1000 * N + 10 * Q + dim + biased)
    nodes = rng.standard_normal((N, dim)).astype(np.float32)
    rel = rng.standard_normal((R0, dim)).astype(np.float32)
    bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    if storage == "bf16":
        nodes = torch.from_numpy(nodes).to(BF).float().numpy()
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    return rng, nodes, rel, bias, batch


@functools.lru_cache(maxsize=None)
def case(N, Q, dim, biased, storage="fp32"):
    """one case with its known triples: the batch itself (every target is a known completion) and about 3 Q more that share a
    query's (s, p) or (p, o), so that both directions' filters are hit; computed once and shared (never written to)"""
    from utils.misc import _FilterIndex, generate_true_dict
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, biased, storage)
    more = batch[rng.integers(0, Q, 3 * Q)].copy()
    more[: len(more) // 2, 0] = rng.integers(0, N, len(more) // 2)             # other heads of a query's (p, o)
    more[len(more) // 2:, 2] = rng.integers(0, N, len(more) - len(more) // 2)  # other tails of a query's (s, p)
    known = np.concatenate([batch, more, rng.integers(0, min(N, R0), (Q, 3))])
    true = generate_true_dict(known)
    return nodes, rel, bias, batch, true, _FilterIndex(true, N)


def lists_on_device(lists_index, batch, head, keep_target=False):
    rows, cols = lists_index.lists(batch, head, keep_target=keep_target)
    return (dev(rows), dev(cols)) if len(rows) else (None, None)


def params_on_device(nodes, rel, bias, storage="fp32", grad=False):
    nt, rt, bt = dev(nodes, BF if storage == "bf16" else None), dev(rel), [dev(b) for b in bias]
    for t in [nt, rt] + bt:
        if t is not None:
            t.requires_grad_(grad)
    return nt, rt, bt


@pytest.fixture
def fixed_order_sums():
    """the route's last sums -- dnodes[anchor] += ..., drel[p] += ... -- are index_add_, fp32 atomics whose order differs from run to run
    (functional.distmult_softmax_loss says so); torch's deterministic mode adds them in a fixed order, for the list form and the index
    form alike, so that gradients can be compared bit for bit"""
    was = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True)
    yield
    torch.use_deterministic_algorithms(was[0], warn_only=was[1])


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_rank_and_topk_equal_the_list_form(N, Q, dim, biased, storage):
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, true, lists_index = case(N, Q, dim, biased, storage)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    suffix = "_bf16" if storage == "bf16" else ""
    for head in (True, False):
        fq, fn = lists_on_device(lists_index, batch, head)
        want = functional.distmult_rank_all(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn)
        _native.profile_start()
        got = functional.distmult_rank_all(batch_t, head, nt, rt, *bt, filt=index)
        assert set(_native.profile_stop()) == {"rank_fused_index" + suffix}
        assert all(torch.equal(g, w) for g, w in zip(got, want)), (head, "rank")
        if N > 1:
            raw = functional.distmult_rank_all(batch_t, head, nt, rt, *bt)
            assert not torch.equal(raw[0], want[0]) or not torch.equal(raw[1], want[1]) or Q < 5     # the filter does something
        fq, fn = lists_on_device(lists_index, batch, head, keep_target=True)
        for k in (1, 10, 32):
            want = functional.distmult_topk_all(batch_t, head, nt, rt, *bt, k=k, filt_q=fq, filt_n=fn)
            _native.profile_start()
            got = functional.distmult_topk_all_index(batch_t, head, nt, rt, *bt, k=k, filt=index)
            assert set(_native.profile_stop()) == {"topk_fused_index" + suffix}
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (head, k)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_loss_equals_the_list_form(N, Q, dim, biased, storage):
    """forward, both storages (bf16: nothing requires grad, the bf16 kernels run)"""
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, true, lists_index = case(N, Q, dim, biased, storage)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    for head in (True, False):
        fq, fn = lists_on_device(lists_index, batch, head)
        for reduction in ("none", "mean"):
            want = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, reduction=reduction)
            _native.profile_start()
            got = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt=index, reduction=reduction)
            assert set(_native.profile_stop()) == {"lse_fused_index_bf16" if storage == "bf16" else "lse_fused_index"}
            assert torch.equal(got, want), (head, reduction)
        if N > 1 and Q >= 5 and dim <= 50:      # the filter does something (at d = 500 one score dominates a row: a filtered cell adds nothing)
            assert not torch.equal(want, functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt))


def grads_of(loss, nt, rt, bt):
    from torch_rgcn import functional
    for t in [nt, rt] + bt:
        if t is not None:
            t.grad = None
    if loss.dim():
        loss.mean().backward()
    else:
        loss.backward(gradient=functional.unit_gradient(loss.device))
    return [t.grad.clone() for t in [nt, rt] + bt if t is not None]


@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_gradients_equal_the_list_form(N, Q, dim, biased, fixed_order_sums):
    """the loss and all five gradients (two without biases), from a [Q] upstream gradient and from the unit gradient"""
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, true, lists_index = case(N, Q, dim, biased)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=True)
    batch_t = dev(batch)
    for head in (True, False):
        fq, fn = lists_on_device(lists_index, batch, head)
        for reduction in ("none", "mean"):
            want_loss = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, reduction=reduction)
            want = grads_of(want_loss, nt, rt, bt)
            _native.profile_start()
            got_loss = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt=index, reduction=reduction)
            got = grads_of(got_loss, nt, rt, bt)
            assert set(_native.profile_stop()) == {"lse_fused_index", "softmax_grad_index", "gemm"}
            assert torch.equal(got_loss, want_loss)
            assert len(got) == len(want) == (5 if biased else 2)
            for k, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), (head, reduction, k, (g - w).abs().max().item())


def test_strips_and_chunks_equal_the_list_form(fixed_order_sums):
    """strips and chunk_bytes forced as test_gpu_softmax_loss.py::test_strips_and_chunks forces them: the gradient runs 1, 3 and 6 chunks"""
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, true, lists_index = case(N, Q, dim, True)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=True)
    batch_t = dev(batch)
    budgets = {1: 4 * Q * N, 3: 4 * Q * 256, 6: 1}
    for n_chunks, budget in budgets.items():
        assert len(functional.softmax_chunk_plan(Q, N, budget)) == n_chunks
    for head in (True, False):
        fq, fn = lists_on_device(lists_index, batch, head)
        for strips in (1, 2, 7, 0):
            want = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, reduction="none", strips=strips)
            got = functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt=index, reduction="none", strips=strips)
            assert torch.equal(got, want), (head, strips)
            want = functional.distmult_rank_all(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, strips=strips)
            got = functional.distmult_rank_all(batch_t, head, nt, rt, *bt, filt=index, strips=strips)
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (head, strips)
        for n_chunks, budget in budgets.items():
            want = grads_of(functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, chunk_bytes=budget), nt, rt, bt)
            _native.profile_start()
            got = grads_of(functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt=index, chunk_bytes=budget), nt, rt, bt)
            assert len(_native.profile_stop()["softmax_grad_index"]) == n_chunks
            for k, (g, w) in enumerate(zip(got, want)):
                assert torch.equal(g, w), (head, n_chunks, k)
        # the gradient cells of every chunk themselves
        with torch.no_grad():
            lse, _ = _native.distmult_lse(batch_t, head, nt, rt, *bt, filt=index)
            g = torch.full((), 3.0, device=DEV)
            for c_first, c_count in functional.softmax_chunk_plan(Q, N, budgets[3]):
                want = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, fq, fn, lse, g, Q, c_first, c_count).clone()
                got = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, None, None, lse, g, Q, c_first, c_count, filt=index)
                assert torch.equal(got, want) and (got == 0).any(), (head, c_first)


@pytest.mark.parametrize("N,Q,dim", [(130, 3, 8), (257, 129, 50), (700, 130, 24)])
def test_rank_filter_equals_the_list_form(N, Q, dim):
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, true, lists_index = case(N, Q, dim, True)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        scores = _native.distmult_score_all(batch_t, head, nt, rt, *bt)
        for keep_target in (False, True):
            fq, fn = lists_on_device(lists_index, batch, head, keep_target=keep_target)
            want = _native.rank_filter(scores.clone(), fq, fn)
            got = _native.rank_filter_index(scores.clone(), batch_t, head, index, keep_target=keep_target)
            assert torch.equal(got, want) and (want == float("-inf")).any(), (head, keep_target)
            assert keep_target == bool((want[torch.arange(Q), batch_t[:, 0 if head else 2]] == float("-inf")).all())


# ----------------------------------------------------------------------------- 3. evaluate and predict
class _Model(torch.nn.Module):
    """encoder + DistMult pair with the attribute names utils.misc looks for (as in test_gpu_topk.py)"""

    def __init__(self, decoder, nodes):
        super().__init__()
        self.scoring_function, self.nodes = decoder, nodes

    def encode(self, graph):
        return self.nodes

    def forward(self, graph, triples):
        return self.scoring_function(triples, self.encode(graph)), 0


def _model(nodes, rel, bias, N):
    from torch_rgcn.layers import DistMult
    dm = DistMult(R0, nodes.shape[1], N, R0, b_init="ones").to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        for n, b in zip(("sbias", "pbias", "obias"), bias):
            getattr(dm, n).copy_(torch.from_numpy(b))
    return _Model(dm, dev(nodes))


def _no_host_lists(monkeypatch):
    from utils import misc

    def refuse(*a, **k):
        raise AssertionError("a host filter list was formed although device_filter=True")
    monkeypatch.setattr(misc, "_filter_index", refuse)


@pytest.mark.parametrize("fused", [True, False])
def test_evaluate_with_the_device_filter_returns_the_same_ranks(fused, monkeypatch):
    from torch_rgcn import _native
    from utils import misc
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, true, _ = case(N, Q, dim, True)
    model = _model(nodes, rel, bias, N)
    mrr, hits, ranks = misc.evaluate(model, None, batch, true, N, verbose=False, fused=fused)
    raw = misc.evaluate(model, None, batch, true, N, verbose=False, fused=fused, filter_candidates=False)[2]
    assert ranks != raw
    _no_host_lists(monkeypatch)
    _native.profile_start()
    mrr_d, hits_d, ranks_d = misc.evaluate(model, None, batch, true, N, verbose=False, fused=fused, device_filter=True)
    tags = set(_native.profile_stop())
    assert tags == ({"rank_fused_index"} if fused else {"score_all", "rank_filter_index", "rank_count"}), tags
    assert ranks_d == ranks and mrr_d == mrr and hits_d == hits
    assert misc.evaluate(model, None, batch, true, N, verbose=False, fused=fused, device_filter=True, filter_candidates=False)[2] == raw
    assert len(misc._DEVICE_FILTER_CACHE) >= 1 and misc._device_filter_index(true, N, DEV) is misc._device_filter_index(true, N, DEV)


@pytest.mark.parametrize("k", [10, 40])
def test_predict_with_the_device_filter_returns_the_same_rows(k, monkeypatch):
    """predict's parameter list stays as it was: the device filter is asked for by passing a FilterIndex as `true_triples`"""
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    from utils import misc
    N, Q, dim = 257, 129, 50
    assert _native.TOPK_MAX < 40
    nodes, rel, bias, batch, true, _ = case(N, Q, dim, True)
    model = _model(nodes, rel, bias, N)
    want = {head: misc.predict(model, None, batch, N, k=k, head=head, true_triples=true) for head in (True, False)}
    plain = misc.predict(model, None, batch, N, k=k, head=False)
    assert not torch.equal(plain[0], want[False][0])
    _no_host_lists(monkeypatch)
    for head in (True, False):
        _native.profile_start()
        ids, scores = misc.predict(model, None, batch, N, k=k, head=head, true_triples=FilterIndex(true, N, DEV))
        tags = set(_native.profile_stop())
        assert tags == ({"topk_fused_index"} if k <= _native.TOPK_MAX else {"score_all", "rank_filter_index"}), tags
        assert torch.equal(ids, want[head][0]) and torch.equal(scores, want[head][1]), (k, head)
    with pytest.raises(ValueError):
        misc.predict(model, None, batch, N, k=k, true_triples=FilterIndex(true, N + 1, DEV))
    with pytest.raises(ValueError):
        misc.predict(model, None, batch, N, k=k, true_triples=FilterIndex(true, N, "cpu"))


# ----------------------------------------------------------------------------- 4. no synchronisation, capture
def test_the_filtered_loss_with_an_index_issues_no_synchronisation():
    """as test_gpu_softmax_loss.py::test_forward_and_backward_issue_no_synchronisation, filtered: the list form reads its lists back
    (checked_queries), the index form reads nothing"""
    from torch_rgcn import _native, functional, routes
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, true, lists_index = case(N, Q, dim, True)
    index = FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=True)
    batch_t = dev(batch)
    lists = {head: lists_on_device(lists_index, batch, head) for head in (True, False)}

    def step(**kw):
        for t in [nt, rt] + bt:
            t.grad = None
        f = lambda head: kw if kw else dict(filt_q=lists[head][0], filt_n=lists[head][1])  # noqa: E731
        loss = 0.5 * (functional.distmult_softmax_loss(batch_t, False, nt, rt, *bt, chunk_bytes=4 * Q * 256, **f(False)) +
                      functional.distmult_softmax_loss(batch_t, True, nt, rt, *bt, **f(True)))
        loss.backward(gradient=functional.unit_gradient(loss.device))
        return loss
    want = step().detach().clone()
    with routes.override(deferred_checks="1"):
        step(filt=index)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            loss = step(filt=index)
            with pytest.raises(RuntimeError):                                  # the detector sees the list form's read-back
                step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        _native.check_deferred_errors()
    assert torch.equal(loss.detach(), want)


def test_a_captured_filtered_step_replays_on_another_batch():
    """One filtered forward + backward captured on static input buffers after a warm-up on a side stream (experiments/predict_links.py's
    procedure), replayed on the batch it was captured with and on a DIFFERENT one copied into the buffer: loss and gradients equal the
    eager list-form call on that batch.  Every query of a batch has an anchor and a relation of its own (257 entities and 129 relations
    for 129 queries), so the index_add_ sums that close the backward add one row per destination and have one answer."""
    from torch_rgcn import functional, routes
    from torch_rgcn.functional import FilterIndex
    from utils.misc import _FilterIndex, generate_true_dict
    N, Q, dim, n_rel = 257, 129, 50, 129
    rng = np.random.default_rng(11)
    nodes = rng.standard_normal((N, dim)).astype(np.float32)
    rel = rng.standard_normal((n_rel, dim)).astype(np.float32)
    bias = [rng.standard_normal(n).astype(np.float32) for n in (N, n_rel, N)]
    batches = [np.stack([rng.permutation(N)[:Q], rng.permutation(n_rel)[:Q], rng.integers(0, N, Q)], 1) for _ in range(2)]
    more = np.concatenate(batches)[rng.integers(0, 2 * Q, 8 * Q)]
    more[:, 2] = rng.integers(0, N, len(more))                                 # other tails of the queries' (s, p)
    true = generate_true_dict(np.concatenate(batches + [more]))
    lists_index, index = _FilterIndex(true, N), FilterIndex(true, N, DEV)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=True)
    params = [nt, rt] + bt

    def step(batch_t, **kw):
        for t in params:
            t.grad.zero_()
        loss = functional.distmult_softmax_loss(batch_t, False, nt, rt, *bt, chunk_bytes=4 * Q * 128, **kw)
        loss.backward(gradient=functional.unit_gradient(loss.device))
        return loss

    # Before the capture nothing touches the leaves but the side-stream warm-up, and the eager reference runs AFTER the replays, as in
    # test_gpu_bf16_lp.py::test_distmult_bf16_step_captured_in_a_hipgraph_matches_eager: a leaf's AccumulateGrad node remembers the
    # stream that was current when it was made, and an eager step on the default stream whose output is still alive would hand the
    # capture accumulators bound to the legacy default stream, which cannot be captured.
    for t in params:
        t.grad = torch.zeros_like(t)
    static = dev(batches[0]).clone()
    with routes.override(deferred_checks="1"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step(static, filt=index)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_loss = step(static, filt=index)
    replayed = []
    for b in batches:                                                          # one capture, two replays
        static.copy_(dev(b))
        graph.replay()
        torch.cuda.synchronize()
        replayed.append([static_loss.detach().clone()] + [t.grad.clone() for t in params])
    del graph, static_loss
    assert not torch.equal(replayed[0][0], replayed[1][0])
    for b, got in zip(batches, replayed):
        fq, fn = lists_on_device(lists_index, b, False)
        assert fq is not None and len(fq) > Q
        loss = step(dev(b), filt_q=fq, filt_n=fn)
        want = [loss.detach()] + [t.grad for t in params]
        for k, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(g, w), (k, (g - w).abs().max().item())
        del loss


# ----------------------------------------------------------------------------- 5. argument errors
def test_argument_errors():
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    from torch_rgcn.layers import DistMult
    from utils.misc import generate_true_dict
    nodes, rel = torch.randn(10, 8, device=DEV), torch.randn(3, 8, device=DEV)
    ok = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    true = generate_true_dict(np.array([[0, 1, 2], [0, 1, 5], [3, 2, 4]]))
    index = FilterIndex(true, 10, DEV)
    i32 = lambda *v: torch.tensor(v, device=DEV, dtype=torch.int32)  # noqa: E731
    topk = lambda **kw: functional.distmult_topk_all_index(ok, False, nodes, rel, k=3, **kw)  # noqa: E731  (no lists to pass beside it)
    topk(filt=index)
    with pytest.raises(ValueError):
        topk()
    with pytest.raises(TypeError):
        topk(filt=index, filt_q=i32(0), filt_n=i32(5))
    with pytest.raises(ValueError, match="is on"):
        topk(filt=FilterIndex(true, 10, "cpu"))
    with pytest.raises(ValueError, match="built for"):
        topk(filt=FilterIndex(true, 11, DEV))
    calls = (lambda **kw: functional.distmult_rank_all(ok, False, nodes, rel, **kw),
             lambda **kw: functional.distmult_softmax_loss(ok, False, nodes, rel, **kw),
             lambda **kw: DistMult(3, 8, 10, 3).to(DEV).softmax_loss(ok, nodes, **kw))
    for call in calls:
        call(filt=index)                                                        # fine
        with pytest.raises(ValueError, match="mutually exclusive"):
            call(filt=index, filt_q=i32(0), filt_n=i32(5))
        with pytest.raises(ValueError, match="is on"):
            call(filt=FilterIndex(true, 10, "cpu"))
        with pytest.raises(ValueError, match="built for"):
            call(filt=FilterIndex(true, 11, DEV))
        with pytest.raises(TypeError):
            call(filt=(i32(0), i32(5)))
    with pytest.raises(IndexError):
        FilterIndex(true, 5, DEV)                                               # entity 5 of the second triple is out of range
    # the C entry point: bad arguments launch nothing
    L, st = _native.lib(), _native._stream(nodes.device)
    keys, ptr, vals = index.tables[1]
    mask = torch.full((2, 1), 7, device=DEV, dtype=torch.int32)
    p = lambda t: t.data_ptr()  # noqa: E731

    def fill(K=keys.shape[0], k=p(keys), c_first=0, c_count=10, out=p(mask), n=10):
        return L.rgcn_filter_mask_index(p(ok), 2, 0, k, p(ptr), p(vals), K, 0, c_first, c_count, out, n, st)
    assert fill(K=-1) == _native.EINVAL and fill(k=None) == _native.EINVAL and fill(c_count=0) == _native.EINVAL
    assert fill(c_first=5, c_count=6) == _native.EINVAL and fill(out=None) == _native.EINVAL and fill(n=0) == _native.EINVAL
    assert b"filter_mask_index" in L.rgcn_last_error()
    torch.cuda.synchronize()
    assert (mask == 7).all()
    assert fill() == _native.OK
    torch.cuda.synchronize()
    assert mask.cpu().view(-1).tolist() == [1 << 5, 0]                          # (0, 1, ?): 2 is the target, 5 the other known tail
