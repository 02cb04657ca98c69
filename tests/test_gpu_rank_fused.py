"""The fused ranking evaluator: greater / ties / target score straight from the entity table, against the materialised
route on the same inputs -- distmult_score_all[_bf16], rank_filter, rank_count -- and against a numpy restatement of filter and count on the
downloaded score matrix.  Ranks are integers and the target score comes from the same product and epilogue: everything is array_equal,
there is no tolerance in this file."""
import numpy as np
import pytest
import torch

import guard_bands as gb
from conftest import load_golden
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
R0 = 5
SHAPES = [(1, 1, 1), (63, 65, 6), (130, 3, 8), (257, 129, 50), (77, 10, 500), (700, 130, 24)]


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def make_case(N, Q, dim, biased, storage, integer=False):
    """host arrays of one case; bf16 storage: the table rounded to bf16 (kept as the fp32 values of those bf16 numbers)"""
    rng = np.random.default_rng(1000 * N + 10 * Q + dim + biased)
    if integer:          # small integers: every product and sum is exact, equal rows give equal scores in any order
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


def random_filter(rng, batch, N, head):
    """as test_gpu_eval.py::test_score_all_vs_oracle: about 3 Q random cells, never the target"""
    Q = len(batch)
    filt = np.unique(np.stack([rng.integers(0, Q, 3 * Q), rng.integers(0, N, 3 * Q)], 1), axis=0)
    return filt[filt[:, 1] != batch[:, 0 if head else 2][filt[:, 0]]]


def on_device(nodes, rel, bias, batch, storage, put=dev):
    return put(batch), put(nodes, BF if storage == "bf16" else None), put(rel), [put(b) for b in bias]


def materialised(batch_t, head, nodes_t, rel_t, bias_t, filt):
    """the existing route -> (greater, ties, target scores before filtering) as numpy, checked against numpy on the downloaded matrix"""
    from torch_rgcn import _native
    score_all = _native.distmult_score_all_bf16 if nodes_t.dtype == BF else _native.distmult_score_all
    sc = score_all(batch_t, head, nodes_t, rel_t, *bias_t)
    got = sc.cpu().numpy()
    Q = got.shape[0]
    target = batch_t.cpu().numpy()[:, 0 if head else 2]
    tscore = got[np.arange(Q), target].copy()
    ref = got.copy()
    if filt is not None and len(filt):
        _native.rank_filter(sc, dev(filt[:, 0].astype(np.int32)), dev(filt[:, 1].astype(np.int32)))
        ref[filt[:, 0], filt[:, 1]] = -np.inf
    g, t = _native.rank_count(sc, batch_t, head)
    g, t = g.cpu().numpy(), t.cpu().numpy()
    true = ref[np.arange(Q), target][:, None]
    assert np.array_equal(g, (ref > true).sum(1)) and np.array_equal(t, (ref == true).sum(1))
    return g, t, tscore


def fused(batch_t, head, nodes_t, rel_t, bias_t, filt, strips=0, put=dev):
    from torch_rgcn import _native
    fq = fn = None
    if filt is not None:
        fq, fn = put(filt[:, 0].astype(np.int32)), put(filt[:, 1].astype(np.int32))
    g, t, ts = _native.distmult_rank_fused(batch_t, head, nodes_t, rel_t, *bias_t, filt_q=fq, filt_n=fn, strips=strips)
    assert g.dtype == torch.int64 and t.dtype == torch.int64 and ts.dtype == torch.float32
    return g.cpu().numpy(), t.cpu().numpy(), ts.cpu().numpy()


def same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x,
                                                    y.view(np.int32) if y.dtype == np.float32 else y) for x, y in zip(a, b))


# ----------------------------------------------------------------------------- parity
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_parity_with_the_materialised_route(N, Q, dim, biased, storage):
    """N and Q off the 128 tiles, N off the 32-bit mask words, d off 4, 8 and 32, fewer than one tile, two query blocks"""
    from torch_rgcn import _native
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, biased, storage)
    args = on_device(nodes, rel, bias, batch, storage)
    for head in (True, False):
        filt = random_filter(rng, batch, N, head)
        want = materialised(args[0], head, *args[1:], filt)
        _native.profile_start()
        got = fused(args[0], head, *args[1:], filt)
        tags = set(_native.profile_stop())
        assert tags == {"rank_fused_bf16" if storage == "bf16" else "rank_fused"}, tags
        assert same(got, want), (head, [np.flatnonzero(x != y)[:5] for x, y in zip(got, want)])
        # raw ranks: F = 0 equals the old route without rank_filter
        assert same(fused(args[0], head, *args[1:], None), materialised(args[0], head, *args[1:], None)), head


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_every_strip_count_gives_the_same_counts(storage):
    """N = 700: 6 candidate tiles, the last ragged -- 6, 3, 2 (and 1), 1 and 1-or-0 tiles per workgroup, strips that own no tile"""
    N, Q, dim = 700, 130, 24
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage)
    args = on_device(nodes, rel, bias, batch, storage)
    for head in (True, False):
        filt = random_filter(rng, batch, N, head)
        want = fused(args[0], head, *args[1:], filt, strips=0)
        assert same(want, materialised(args[0], head, *args[1:], filt))
        for strips in (1, 2, 4, 6, 9):
            assert same(fused(args[0], head, *args[1:], filt, strips=strips), want), (head, strips)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,dim", [(257, 129, 8), (700, 130, 24)])
def test_exact_ties_and_duplicated_filter_entries(N, Q, dim, storage):
    """integer embeddings, a quarter of the rows copies of others: many candidates tie the target exactly; the filter takes tied cells and
    greater cells away and repeats entries"""
    from torch_rgcn import _native
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage, integer=True)
    args = on_device(nodes, rel, bias, batch, storage)
    for head in (True, False):
        target = batch[:, 0 if head else 2]
        score_all = _native.distmult_score_all_bf16 if storage == "bf16" else _native.distmult_score_all
        sc = score_all(args[0], head, *args[1:2], args[2], *args[3]).cpu().numpy()
        true = sc[np.arange(Q), target][:, None]
        not_target = np.arange(N)[None, :] != target[:, None]
        tied, above = np.argwhere((sc == true) & not_target), np.argwhere((sc > true) & not_target)
        assert len(tied) > Q // 2 and len(above) > Q                       # the case is what it claims to be
        cells = np.concatenate([tied[::2], above[::3], random_filter(rng, batch, N, head)])
        listed = np.concatenate([cells, cells[::2], cells[:7]])            # duplicated entries
        unique = np.unique(cells, axis=0)
        want = materialised(args[0], head, *args[1:], unique)
        raw = materialised(args[0], head, *args[1:], None)
        assert (want[1] < raw[1]).any() and (want[0] < raw[0]).any()       # the filter did remove ties and greater cells
        assert (want[1] > 1).any()                                         # and exact ties remain
        assert same(fused(args[0], head, *args[1:], listed), want), head
        assert same(fused(args[0], head, *args[1:], np.concatenate([listed, listed])), want), head     # the list passed twice over
        assert same(fused(args[0], head, *args[1:], None), raw), head


# ----------------------------------------------------------------------------- evaluate()
class _Model(torch.nn.Module):
    """encoder + DistMult pair with the attribute names utils.misc.evaluate looks for (as in test_gpu_eval.py)"""

    def __init__(self, decoder, nodes=None, layer=None, emb=None):
        super().__init__()
        self.scoring_function, self.layer = decoder, layer
        self.nodes, self.emb = nodes, emb
        self.encoder_calls = 0

    def encode(self, graph):
        self.encoder_calls += 1
        return self.nodes if self.layer is None else self.layer(graph, torch.relu(self.emb))

    def forward(self, graph, triples):
        return self.scoring_function(triples, self.encode(graph)), 0


def _decoder(d, N, n_rel, biased):
    from torch_rgcn.layers import DistMult
    dm = DistMult(n_rel, d["nodes"].shape[1], N, n_rel, b_init="ones" if biased else None).to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(d["relations"]))
        if biased:
            for n in ("sbias", "pbias", "obias"):
                getattr(dm, n).copy_(torch.from_numpy(d[n]))
    return dm


def _evaluate_tags(misc, *args, **kw):
    from torch_rgcn import _native
    _native.profile_start()
    out = misc.evaluate(*args, **kw)
    return out, _native.profile_stop()


def test_goldens_with_ties_on_the_fused_route():
    from utils import misc
    d = load_golden("g7_eval_ties")
    N, n_rel = int(d["num_nodes"]), int(d["num_rels"])
    model = _Model(_decoder(d, N, n_rel, True), nodes=torch.from_numpy(d["nodes"]).to(DEV))
    test = torch.from_numpy(d["test"])
    true_triples = misc.generate_true_dict(np.concatenate([d["known"], d["known"][:10], d["test"]]))
    for tag, filt in (("filtered", True), ("raw", False)):
        for bs in (25, 7, 1):
            (mrr, hits, ranks), tags = _evaluate_tags(misc, model, None, test, true_triples, N, batch_size=bs, filter_candidates=filt,
                                                      verbose=False, fused=True)
            assert ranks == d[f"ranks_{tag}"].tolist(), (tag, bs)
            assert abs(mrr - float(d[f"mrr_{tag}"])) < 1e-12 and np.allclose(hits, d[f"hits_{tag}"], atol=1e-12)
            assert "rank_fused" in tags and "score_all" not in tags and "rank_count" not in tags, sorted(tags)


def test_golden_lp_encoder_on_the_fused_route():
    from torch_rgcn.layers import RelationalGraphConvolutionLP
    from utils import misc
    d = load_golden("g7_eval_lp")
    N, n_rel = int(d["num_nodes"]), int(d["num_rels"])
    dim = d["emb"].shape[1]
    layer = RelationalGraphConvolutionLP(num_nodes=N, num_relations=2 * n_rel + 1, in_features=dim, out_features=dim,
                                         edge_dropout={"general": 0.5, "self_loop": 0.2, "self_loop_type": "schlichtkrull-dropout"},
                                         decomposition={"type": "basis", "num_bases": 2}, w_init="glorot-normal",
                                         b_init="zeros").to(DEV)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.from_numpy(d["layer_param_" + n]))
    model = _Model(_decoder(d, N, n_rel, False), layer=layer, emb=torch.from_numpy(d["emb"]).to(DEV)).eval()
    true_triples = misc.generate_true_dict(np.concatenate([d["train"], d["valid"], d["test"]]))
    train = torch.from_numpy(d["train"])
    for tag, filt in (("filtered", True), ("raw", False)):
        model.encoder_calls = 0
        (mrr, hits, ranks), tags = _evaluate_tags(misc, model, train, torch.from_numpy(d["test"]), true_triples, N, batch_size=7,
                                                  filter_candidates=filt, verbose=False, fused=True)
        assert model.encoder_calls == 1                                 # encode once, rank many
        assert ranks == d[f"ranks_{tag}"].tolist(), tag
        assert abs(mrr - float(d[f"mrr_{tag}"])) < 1e-9
        assert "rank_fused" in tags and "score_all" not in tags and "rank_count" not in tags, sorted(tags)


def test_link_predictor_in_bf16_ranks_the_same_on_both_routes():
    from torch_rgcn.models import LinkPredictor
    from utils import misc
    N, n_rel, dim = 200, 4, 16
    torch.manual_seed(0)
    model = LinkPredictor(nnodes=N, nrel=n_rel, encoder_config={"node_embedding": dim, "hidden1_size": dim, "num_layers": 1,
                                                                "decomposition": {"type": "basis", "num_bases": 2},
                                                                "weight_init": "glorot-normal", "bias_init": "zeros"},
                          decoder_config={"weight_init": "standard-normal", "bias_init": "normal",
                                          "l2_penalty_type": "schlichtkrull-l2", "l2_penalty": 0.01}).to(DEV).bfloat16().eval()
    graph = torch.from_numpy(oracle.synthetic_triples(N, n_rel, 1200, 4))
    test = oracle.synthetic_triples(N, n_rel, 40, 6)
    true_triples = misc.generate_true_dict(np.concatenate([graph.numpy(), test]))
    (_, _, want), old_tags = _evaluate_tags(misc, model, graph, torch.from_numpy(test), true_triples, N, batch_size=7, verbose=False,
                                            fused=False)
    (mrr, _, ranks), tags = _evaluate_tags(misc, model, graph, torch.from_numpy(test), true_triples, N, batch_size=7, verbose=False,
                                           fused=True)
    assert "distmult_score_all_bf16" in old_tags and "rank_fused_bf16" not in old_tags
    assert "rank_fused_bf16" in tags and "rank_fused" not in tags and "distmult_score_all_bf16" not in tags and "rank_count" not in tags
    assert ranks == want and len(ranks) == 80 and 0 < mrr <= 1


def test_a_test_set_past_the_score_budget_is_ranked_in_one_launch_per_direction(monkeypatch):
    """the capability: with the score budget at 64 KiB the materialised route chunks 300 queries x 4,099 entities; fused=None goes fused,
    one launch per direction, and the call's peak memory stays under a quarter of the score matrix of the same batch"""
    from torch_rgcn import _native
    from utils import misc
    N, n_rel, dim, Q = 4_099, 6, 24, 300
    g = torch.Generator().manual_seed(7)
    d = {"nodes": torch.randn(N, dim, generator=g).numpy(), "relations": torch.randn(n_rel, dim, generator=g).numpy()}
    model = _Model(_decoder(d, N, n_rel, False), nodes=torch.from_numpy(d["nodes"]).to(DEV))
    test = torch.from_numpy(_native.synthetic_triples_host(N, n_rel, Q, 5))
    known = _native.synthetic_triples_host(N, n_rel, 20_000, 6)
    known[:3000, :2] = test[:, :2].numpy()[np.arange(3000) % Q]           # filters that are hit, head and ...
    known[3000:6000, 1:] = test[:, 1:].numpy()[np.arange(3000) % Q]       # ... tail
    true_triples = misc.generate_true_dict(np.concatenate([known, test.numpy()]))
    monkeypatch.setattr(misc, "_SCORE_BYTES", 64 * 1024)
    assert misc.use_fused(Q, N) and not misc.use_fused(Q, N, False)
    (_, _, want), old_tags = _evaluate_tags(misc, model, None, test, true_triples, N, verbose=False, fused=False)
    assert len(old_tags["score_all"]) > 2 and "rank_fused" not in old_tags          # the old route now chunks
    (_, _, ranks), tags = _evaluate_tags(misc, model, None, test, true_triples, N, verbose=False)
    assert len(tags["rank_fused"]) == 2 and "score_all" not in tags and "rank_count" not in tags, {k: len(v) for k, v in tags.items()}
    assert ranks == want and len(ranks) == 2 * Q
    misc._filter_index(true_triples, N)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    assert misc.evaluate(model, None, test, true_triples, N, verbose=False)[2] == want
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[rank_fused] peak memory rise {rise} bytes; Q x N = {Q * N}; the score matrix of this batch = {4 * Q * N}")
    assert rise < Q * N, rise


# ----------------------------------------------------------------------------- errors
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_wrapper_argument_errors(storage):
    from torch_rgcn import _native
    nodes = torch.randn(10, 8, device=DEV).to(BF if storage == "bf16" else torch.float32)
    rel = torch.randn(3, 8, device=DEV)
    ok = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    i32 = lambda *v: torch.tensor(v, device=DEV, dtype=torch.int32)  # noqa: E731
    for bad in ([[0, 3, 2]], [[10, 1, 2]], [[0, 1, -1]]):                                           # relation / node out of range
        with pytest.raises((AssertionError, IndexError)):
            _native.distmult_rank_fused(torch.tensor(bad, device=DEV), True, nodes, rel)
    for fq, fn in ((i32(2), i32(0)), (i32(-1), i32(0)), (i32(0), i32(10)), (i32(0), i32(-1))):       # filter entry out of range
        with pytest.raises(IndexError):
            _native.distmult_rank_fused(ok, True, nodes, rel, filt_q=fq, filt_n=fn)
    with pytest.raises(RuntimeError):
        _native.distmult_rank_fused(ok.cpu(), True, nodes, rel)                                      # no CPU path
    with pytest.raises(RuntimeError):
        _native.distmult_rank_fused(ok, True, nodes.cpu(), rel)
    with pytest.raises(AssertionError):
        _native.distmult_rank_fused(ok, True, nodes, rel, torch.zeros(10, device=DEV), None, None)   # biases: all or none
    with pytest.raises(AssertionError):
        _native.distmult_rank_fused(ok, True, nodes, rel, strips=-1)
    with pytest.raises(AssertionError):
        _native.distmult_rank_fused(ok, True, nodes, rel, filt_q=i32(0))                             # one list without the other
    g, t, ts = _native.distmult_rank_fused(ok[:0], True, nodes, rel)                                 # Q = 0: empty outputs
    assert g.shape == t.shape == ts.shape == (0,) and g.dtype == t.dtype == torch.int64 and ts.dtype == torch.float32
    g, t, ts = _native.distmult_rank_fused(ok, True, nodes, rel, filt_q=i32(0, 1), filt_n=i32(5, 5))
    assert g.shape == t.shape == ts.shape == (2,)


def test_c_abi_argument_errors():
    from torch_rgcn import _native
    L = _native.lib()
    N, dim, Q = 10, 8, 2
    nodes, rel = torch.randn(N, dim, device=DEV), torch.randn(3, dim, device=DEV)
    nodes16 = nodes.to(BF)
    batch = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    fq, fn = torch.tensor([0], device=DEV, dtype=torch.int32), torch.tensor([5], device=DEV, dtype=torch.int32)
    ws = torch.empty(_native.rank_fused_workspace_bytes(Q, N, dim, 0, True) + 16, device=DEV, dtype=torch.uint8)
    g, t = torch.full((Q,), -7, device=DEV), torch.full((Q,), -7, device=DEV)
    ts = torch.full((Q,), -7.0, device=DEV)
    st = _native._stream(nodes.device)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    assert p(ws) % 16 == 0

    def f32(w=p(ws), gp=p(g), tp=p(t), tsp=p(ts), strips=0, F=0, q=None, n=None):
        return L.rgcn_distmult_rank_fused_f32(p(batch), Q, 1, p(nodes), p(rel), None, None, None, q, n, F, None, None, None, 0, strips, w, gp, tp, tsp,
                                              N, 3, dim, st)

    def b16(w=p(ws), gp=p(g), tp=p(t), tsp=p(ts), strips=0, F=0, q=None, n=None):
        return L.rgcn_distmult_rank_fused_bf16(p(batch), Q, 1, p(nodes16), p(rel), None, None, None, q, n, F, None, None, None, 0, strips, w, gp, tp, tsp,
                                               N, 3, dim, st)

    for call in (f32, b16):
        assert call(w=None) == _native.EINVAL and call(gp=None) == _native.EINVAL and call(tsp=None) == _native.EINVAL
        assert call(tp=None) == _native.EINVAL
        assert call(w=p(ws) + 4) == _native.EINVAL                        # misaligned workspace
        assert call(strips=-1) == _native.EINVAL
        assert call(F=1) == _native.EINVAL and call(F=1, q=p(fq)) == _native.EINVAL and call(F=1, n=p(fn)) == _native.EINVAL
        assert call(F=-1) == _native.EINVAL
        assert b"rank_fused" in L.rgcn_last_error()
    torch.cuda.synchronize()
    assert g.tolist() == [-7] * Q and t.tolist() == [-7] * Q and ts.tolist() == [-7.0] * Q          # nothing was launched
    # biases partly set; Q == 0 is fine with nothing else set
    assert L.rgcn_distmult_rank_fused_f32(p(batch), Q, 1, p(nodes), p(rel), p(ts), None, None, None, None, 0, None, None, None, 0, 0, p(ws), p(g),
                                          p(t), p(ts), N, 3, dim, st) == _native.EINVAL
    assert L.rgcn_distmult_rank_fused_f32(None, 0, 1, None, None, None, None, None, None, None, 0, None, None, None, 0, 0, None, None, None, None,
                                          N, 3, dim, st) == _native.OK
    assert L.rgcn_distmult_rank_fused_bf16(None, 0, 1, None, None, None, None, None, None, None, 0, None, None, None, 0, 0, None, None, None, None,
                                           N, 3, dim, st) == _native.OK
    # and the good call, through the same closures
    assert f32(F=1, q=p(fq), n=p(fn)) == _native.OK
    want = _native.distmult_rank_fused(batch, True, nodes, rel, filt_q=fq, filt_n=fn)
    assert torch.equal(g, want[0]) and torch.equal(t, want[1]) and torch.equal(ts, want[2])
    assert b16() == _native.OK
    want = _native.distmult_rank_fused(batch, True, nodes16, rel)
    assert torch.equal(g, want[0]) and torch.equal(t, want[1]) and torch.equal(ts, want[2])


# ----------------------------------------------------------------------------- guard bands
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,dim", [(1, 1, 1), (257, 129, 50)])
def test_under_guard_bands(monkeypatch, N, Q, dim, storage):
    """every buffer between two poisoned bands, inputs included: no kernel of the fused route touches memory outside them"""
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage)
    plain = on_device(nodes, rel, bias, batch, storage)
    filts = {head: random_filter(rng, batch, N, head) for head in (True, False)}
    want = {head: materialised(plain[0], head, *plain[1:], filts[head]) for head in (True, False)}
    with gb.Guard(monkeypatch) as guard:
        put = lambda a, dt=None: None if a is None else guard.home(dev(a, dt))  # noqa: E731
        args = on_device(nodes, rel, bias, batch, storage, put=put)
        got = {}
        for head in (True, False):
            got[head] = fused(args[0], head, *args[1:], filts[head], put=put)
            got[head, "raw"] = fused(args[0], head, *args[1:], None, strips=3, put=put)
        problems = guard.problems(f"rank_fused {storage} N={N} Q={Q} d={dim}")
    assert not problems, "\n".join(problems)
    for head in (True, False):
        assert same(got[head], want[head]), head
        assert same(got[head, "raw"], materialised(plain[0], head, *plain[1:], None)), head
