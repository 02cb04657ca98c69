"""Top-k link prediction: the k best completions of every query straight from the entity table, against the materialised
route on the same inputs -- distmult_score_all[_bf16], rank_filter on the full lists (targets included), the matrix downloaded and every
row sorted by (score descending, id ascending) in numpy.  The product and the epilogue are shared with the score-all kernels, so ids and
scores are compared with array_equal: there is no tolerance in this file (+0 and -0 compare equal)."""
import numpy as np
import pytest
import torch

import guard_bands as gb
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
R0 = 5
INF = float("inf")
SHAPES = [(1, 1, 1), (63, 65, 6), (130, 3, 8), (257, 129, 50), (77, 10, 500), (700, 130, 24)]
KS = (1, 3, 10, 32)


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def make_case(N, Q, dim, biased, storage, integer=False):
    """host arrays of one case (the builder of test_gpu_rank_fused.py); bf16 storage: the table rounded to bf16"""
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


def random_filter(rng, Q, N):
    """about 3 Q random cells; a query's own `batch` target may be among them: prediction has no target"""
    return np.unique(np.stack([rng.integers(0, Q, 3 * Q), rng.integers(0, N, 3 * Q)], 1), axis=0)


def on_device(nodes, rel, bias, batch, storage, put=dev):
    return put(batch), put(nodes, BF if storage == "bf16" else None), put(rel), [put(b) for b in bias]


def lists_of(filt, put=dev):
    if filt is None or not len(filt):
        return None, None
    return put(filt[:, 0].astype(np.int32)), put(filt[:, 1].astype(np.int32))


def reference_matrix(batch_t, head, nodes_t, rel_t, bias_t, filt):
    """the materialised route: the filtered score matrix, downloaded -- computed once per case and shared by every k"""
    from torch_rgcn import _native
    score_all = _native.distmult_score_all_bf16 if nodes_t.dtype == BF else _native.distmult_score_all
    sc = score_all(batch_t, head, nodes_t, rel_t, *bias_t)
    fq, fn = lists_of(filt)
    if fq is not None:
        _native.rank_filter(sc, fq, fn)
    return sc.cpu().numpy()


def topk_of_matrix(sc, k):
    Q, N = sc.shape
    ids, scores = np.full((Q, k), -1, np.int64), np.full((Q, k), -np.inf, np.float32)
    cols = np.arange(N)
    for q in range(Q):
        order = np.lexsort((cols, -sc[q]))
        order = order[sc[q][order] > -np.inf][:k]
        ids[q, :len(order)], scores[q, :len(order)] = order, sc[q][order]
    return ids, scores


def topk(batch_t, head, nodes_t, rel_t, bias_t, filt, k, strips=0, put=dev):
    from torch_rgcn import _native
    fq, fn = lists_of(filt, put)
    ids, scores = _native.distmult_topk(batch_t, head, nodes_t, rel_t, *bias_t, k=k, filt_q=fq, filt_n=fn, strips=strips)
    assert ids.dtype == torch.int64 and scores.dtype == torch.float32 and ids.shape == scores.shape == (batch_t.shape[0], k)
    return ids.cpu().numpy(), scores.cpu().numpy()


def same(got, want):
    return got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def first_difference(got, want):
    rows = np.flatnonzero((got[0] != want[0]).any(1) | (got[1] != want[1]).any(1))[:3]
    return [(int(q), got[0][q].tolist(), want[0][q].tolist(), got[1][q].tolist(), want[1][q].tolist()) for q in rows]


# ----------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_parity_with_the_materialised_route(N, Q, dim, biased, storage):
    """N and Q off the 128 tiles, N off the 32-bit mask words, d off 4, 8 and 32, k > N, fewer than one tile, two query blocks"""
    from torch_rgcn import _native
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, biased, storage)
    args = on_device(nodes, rel, bias, batch, storage)
    for head in (True, False):
        for filt in (random_filter(rng, Q, N), None):
            matrix = reference_matrix(args[0], head, *args[1:], filt)
            for k in KS:
                want = topk_of_matrix(matrix, k)
                _native.profile_start()
                got = topk(args[0], head, *args[1:], filt, k)
                tags = set(_native.profile_stop())
                assert tags == {"topk_fused_bf16" if storage == "bf16" else "topk_fused"}, tags
                assert same(got, want), (head, filt is not None, k, first_difference(got, want))


# ----------------------------------------------------------------------------- 2. ties and strips
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_ties_come_in_ascending_id_for_every_strip_count(storage):
    """integer inputs, a quarter of the rows copies of others: exact scores, many of them equal.  N = 700 is 6 candidate tiles, the last
    ragged: 6, 3, 2, 1 and 1-or-0 tiles per workgroup, strips that own no tile"""
    N, Q, dim, k = 700, 130, 24, 10
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage, integer=True)
    args = on_device(nodes, rel, bias, batch, storage)
    for head in (True, False):
        filt = random_filter(rng, Q, N)
        want = topk_of_matrix(reference_matrix(args[0], head, *args[1:], filt), k)
        tied = want[1][:, 1:] == want[1][:, :-1]
        assert tied.sum() > Q                                              # the case is what it claims to be
        assert (want[0][:, 1:][tied] > want[0][:, :-1][tied]).all()
        for strips in (0, 1, 2, 3, 5, 6, 7, 50):
            got = topk(args[0], head, *args[1:], filt, k, strips=strips)
            assert same(got, want), (head, strips, first_difference(got, want))
            assert (got[0][:, 1:][tied] > got[0][:, :-1][tied]).all()


# ----------------------------------------------------------------------------- 3. boundaries
PLANTED = [0, 63, 64, 127, 128, 191, 255, 256, 640, 699]


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_winners_at_every_edge_come_back_in_order(storage):
    """each query's 10 best candidates sit on the first and last columns of wave halves, tiles, strips and the ragged last tile, with
    distinct known scores; every other score is lower"""
    N, Q, dim, k = 700, 130, 8, 10
    rng = np.random.default_rng(11)
    nodes = rng.integers(-2, 3, (N, dim)).astype(np.float32)
    nodes[PLANTED, 0] = 20 - np.arange(10)                                # 20, 19, ... 11; everything else holds -2 .. 2 there
    subjects = np.setdiff1d(np.arange(N), PLANTED)[rng.permutation(N - 10)[:Q]]
    weight = rng.integers(1, 4, Q).astype(np.float32)
    nodes[subjects] = 0
    nodes[subjects, 0] = weight                                           # score(q, n) = weight[q] * nodes[n, 0]
    rel = np.ones((R0, dim), np.float32)
    batch = np.stack([subjects, rng.integers(0, R0, Q), subjects], 1)
    args = on_device(nodes, rel, [None] * 3, batch, storage)
    want_ids = np.tile(np.array(PLANTED, np.int64), (Q, 1))
    want_scores = weight[:, None] * (20 - np.arange(10, dtype=np.float32))[None, :]
    for head in (True, False):
        assert same(topk_of_matrix(reference_matrix(args[0], head, *args[1:], None), k), (want_ids, want_scores))
        for strips in (1, 6):
            got = topk(args[0], head, *args[1:], None, k, strips=strips)
            assert same(got, (want_ids, want_scores)), (head, strips, first_difference(got, (want_ids, want_scores)))


# ----------------------------------------------------------------------------- 4. heavy filtering
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_heavy_filtering_pads_and_excludes_the_batch_target(storage):
    N, Q, dim, k = 65, 4, 6, 10
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage)
    args = on_device(nodes, rel, bias, batch, storage)
    for head in (True, False):
        col = 0 if head else 2
        best = int(np.argmax(reference_matrix(args[0], head, *args[1:], None)[3]))
        b = batch.copy()
        b[3, col] = best                                                  # query 3's `batch` target is its best candidate (the column is ignored)
        case = (dev(b),) + tuple(args[1:])
        target = b[:, col]
        left = np.array([3, 40, 64])
        filt = np.array([(0, n) for n in range(N) if n not in left] + [(1, n) for n in range(N)] + [(3, best)])
        want = topk_of_matrix(reference_matrix(case[0], head, *case[1:], filt), k)
        assert topk(case[0], head, *case[1:], None, k)[0][3, 0] == best   # without the entry it comes first
        got = topk(case[0], head, *case[1:], filt, k)
        assert same(got, want), (head, first_difference(got, want))
        ids, scores = got
        assert sorted(ids[0, :3].tolist()) == left.tolist() and (ids[0, 3:] == -1).all() and (scores[0, 3:] == -np.inf).all()
        assert (ids[1] == -1).all() and (scores[1] == -np.inf).all()
        assert (ids[2] >= 0).all() and np.isfinite(scores[2]).all()
        assert (ids[3] >= 0).all() and int(target[3]) not in ids[3].tolist()          # unlike ranking, which ignores such an entry
        listed = set(map(tuple, filt.tolist()))
        assert not any((q, int(n)) in listed for q in range(Q) for n in ids[q])


# ----------------------------------------------------------------------------- models for predict()
class _Model(torch.nn.Module):
    """encoder + DistMult pair with the attribute names utils.misc looks for (as in test_gpu_rank_fused.py)"""

    def __init__(self, decoder, nodes):
        super().__init__()
        self.scoring_function, self.nodes = decoder, nodes
        self.encoder_calls = 0

    def encode(self, graph):
        self.encoder_calls += 1
        return self.nodes

    def forward(self, graph, triples):
        return self.scoring_function(triples, self.encode(graph)), 0


def _decoder(nodes, rel, bias, N, n_rel):
    from torch_rgcn.layers import DistMult
    dm = DistMult(n_rel, nodes.shape[1], N, n_rel, b_init="ones" if bias[0] is not None else None).to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        if bias[0] is not None:
            for n, b in zip(("sbias", "pbias", "obias"), bias):
                getattr(dm, n).copy_(torch.from_numpy(b))
    return dm


def _predict_tags(misc, *args, **kw):
    from torch_rgcn import _native
    _native.profile_start()
    out = misc.predict(*args, **kw)
    tags = _native.profile_stop()
    return (out[0].cpu().numpy(), out[1].cpu().numpy()), tags


# ----------------------------------------------------------------------------- 5. k over the native limit
def test_k_over_the_native_limit():
    from torch_rgcn import _native
    from utils import misc
    N, Q, dim = 130, 9, 8
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, "fp32")
    args = on_device(nodes, rel, bias, batch, "fp32")
    assert _native.TOPK_MAX == 32
    with pytest.raises(_native.NativeLibraryError, match="native limit of 32"):
        _native.distmult_topk(args[0], False, args[1], args[2], *args[3], k=33)
    model = _Model(_decoder(nodes, rel, bias, N, R0), args[1])
    known = np.concatenate([batch, np.stack([rng.integers(0, N, 300), rng.integers(0, R0, 300), rng.integers(0, N, 300)], 1)])
    known[:100, :2] = batch[np.arange(100) % Q, :2]                       # filters that are hit, tail and ...
    known[100:200, 1:] = batch[np.arange(100) % Q, 1:]                    # ... head
    true_triples = misc.generate_true_dict(known)
    for head in (True, False):
        rows, cols = misc._filter_index(true_triples, N).lists(batch, head, keep_target=True)
        assert len(rows) > 2 * Q
        matrix = reference_matrix(args[0], head, *args[1:], np.stack([rows, cols], 1))
        got, tags = _predict_tags(misc, model, None, batch, N, k=40, head=head, true_triples=true_triples)
        assert "score_all" in tags and "topk_fused" not in tags, sorted(tags)
        want = topk_of_matrix(matrix, 40)
        assert same(got, want), (head, first_difference(got, want))
        forced, tags = _predict_tags(misc, model, None, batch, N, k=40, head=head, true_triples=true_triples, fused=True)
        assert "score_all" in tags and "topk_fused" not in tags and same(forced, want)         # a larger k: the fallback, whatever `fused` says
        # at the limit the kernel route serves, and agrees
        got, tags = _predict_tags(misc, model, None, batch, N, k=32, head=head, true_triples=true_triples)
        assert set(tags) == {"topk_fused"} and same(got, topk_of_matrix(matrix, 32))


# ----------------------------------------------------------------------------- 6. guard bands
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_under_guard_bands(monkeypatch, storage):
    """every buffer between two poisoned bands, inputs included, the outputs full of NaN before the call: no kernel of the route touches
    memory outside them, and every output cell is written"""
    N, Q, dim, k = 257, 129, 50, 10
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage)
    plain = on_device(nodes, rel, bias, batch, storage)
    filts = {head: random_filter(rng, Q, N) for head in (True, False)}
    want = {head: topk_of_matrix(reference_matrix(plain[0], head, *plain[1:], filts[head]), k) for head in (True, False)}
    raw = {head: topk_of_matrix(reference_matrix(plain[0], head, *plain[1:], None), k) for head in (True, False)}
    with gb.Guard(monkeypatch) as guard:
        put = lambda a, dt=None: None if a is None else guard.home(dev(a, dt))  # noqa: E731
        args = on_device(nodes, rel, bias, batch, storage, put=put)
        assert torch.isnan(torch.empty(3, device=DEV)).all()              # what the route's torch.empty outputs hold before the call
        got = {}
        for head in (True, False):
            got[head] = topk(args[0], head, *args[1:], filts[head], k, put=put)
            got[head, "raw"] = topk(args[0], head, *args[1:], None, k, strips=3, put=put)
        problems = guard.problems(f"topk {storage} N={N} Q={Q} d={dim}")
    assert not problems, "\n".join(problems)
    for head in (True, False):
        for key, ref in ((head, want[head]), ((head, "raw"), raw[head])):
            assert not np.isnan(got[key][1]).any() and (got[key][0] >= 0).all()
            assert same(got[key], ref), (key, first_difference(got[key], ref))


# ----------------------------------------------------------------------------- 7. consistency with the evaluator
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_consistent_with_the_fused_evaluator(storage):
    """with the lists ranking uses (the target itself never on them): a target with at most 10 candidates at or above it is among the 10
    returned, and a returned target has fewer than 10 above it"""
    from torch_rgcn import functional
    from utils import misc
    N, Q, dim, k = 300, 120, 16, 10
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, True, storage, integer=True)      # integers: ties at the k-th place do occur
    args = on_device(nodes, rel, bias, batch, storage)
    seen = {"in": 0, "out": 0, "sure": 0}
    for head in (True, False):
        col = 0 if head else 2
        raw = reference_matrix(args[0], head, *args[1:], None)
        b = batch.copy()
        order = np.argsort(-raw, axis=1, kind="stable")
        near = np.arange(Q) % 3 == 0                                       # a third of the targets near the top, the rest where they fell
        b[near, col] = order[near, (np.arange(Q) % 14)[near]]
        known = np.concatenate([b, np.stack([rng.integers(0, N, 900), rng.integers(0, R0, 900), rng.integers(0, N, 900)], 1)])
        known[:300, 1:] = b[np.arange(300) % Q, 1:]
        known[300:600, :2] = b[np.arange(300) % Q, :2]
        rows, cols = misc._FilterIndex(misc.generate_true_dict(known), N).lists(b, head)          # keep_target=False
        assert len(rows) > Q and not (cols == b[rows, col]).any()
        bt, fq, fn = dev(b), dev(rows), dev(cols)
        greater, ties, _ = (t.cpu().numpy() for t in functional.distmult_rank_all(bt, head, *args[1:3], *args[3], filt_q=fq, filt_n=fn))
        ids = functional.distmult_topk_all(bt, head, *args[1:3], *args[3], k=k, filt_q=fq, filt_n=fn)[0].cpu().numpy()
        inside = (ids == b[:, col][:, None]).any(1)
        assert inside[greater + ties <= k].all(), np.flatnonzero(~inside & (greater + ties <= k))
        assert (greater[inside] < k).all(), np.flatnonzero(inside & (greater >= k))
        seen["in"] += int(inside.sum()); seen["out"] += int((~inside).sum()); seen["sure"] += int((greater + ties <= k).sum())
    assert min(seen.values()) > 5, seen                                    # both sides of both implications were exercised


# ----------------------------------------------------------------------------- 8. utils.misc.predict end to end
def test_predict_end_to_end_on_a_link_predictor(monkeypatch):
    """predict() on a LinkPredictor, fp32 and bf16: the kernel route against the fallback, exactly.  The encoder adds messages with
    floating-point atomics, so two encodings of one graph differ in the last bit: each storage is encoded once, by the model, and the calls
    that are compared with each other get that encoding (and are counted: one encoding per call)"""
    from torch_rgcn.models import LinkPredictor
    from utils import misc
    N, n_rel, dim, k = 200, 4, 16, 10
    torch.manual_seed(0)
    model = LinkPredictor(nnodes=N, nrel=n_rel, encoder_config={"node_embedding": dim, "hidden1_size": dim, "num_layers": 1,
                                                                "decomposition": {"type": "basis", "num_bases": 2},
                                                                "weight_init": "glorot-normal", "bias_init": "zeros"},
                          decoder_config={"weight_init": "standard-normal", "bias_init": "normal",
                                          "l2_penalty_type": "schlichtkrull-l2", "l2_penalty": 0.01}).to(DEV).eval()
    graph = torch.from_numpy(oracle.synthetic_triples(N, n_rel, 1200, 4))
    queries = oracle.synthetic_triples(N, n_rel, 40, 6)
    true_triples = misc.generate_true_dict(np.concatenate([graph.numpy(), queries]))
    for tag in ("topk_fused", "topk_fused_bf16"):
        if tag == "topk_fused_bf16":
            monkeypatch.undo()
            model = model.bfloat16()
        with torch.no_grad():
            x = model.encode(graph)
        assert x.dtype == (BF if tag == "topk_fused_bf16" else torch.float32) and x.shape == (N, dim)
        calls = []
        monkeypatch.setattr(model, "encode", lambda g, x=x: calls.append(g) or x)
        for head in (True, False):
            want, old_tags = _predict_tags(misc, model, graph, queries, N, k=k, head=head, true_triples=true_triples, fused=False)
            got, tags = _predict_tags(misc, model, graph, torch.from_numpy(queries), N, k=k, head=head, true_triples=true_triples)
            assert tag in tags and not any("score_all" in t for t in tags), sorted(tags)
            assert any("score_all" in t for t in old_tags) and not any(t.startswith("topk_fused") for t in old_tags), sorted(old_tags)
            assert got[0].shape == (40, k) and same(got, want), (tag, head, first_difference(got, want))
            table = true_triples[0 if head else 1]
            for (s, p, o), row in zip(queries.tolist(), got[0].tolist()):
                known = table.get((p, o) if head else (s, p), [])
                assert (o if not head else s) in known and not set(row) & set(known), (s, p, o, row)
            assert (got[0] >= 0).all() and (np.diff(got[1], axis=1) <= 0).all()
            # without the dictionaries nothing is excluded: the best unfiltered candidates score at least as high
            free, _ = _predict_tags(misc, model, graph, queries, N, k=k, head=head)
            assert (free[1] >= got[1]).all()
        assert len(calls) == 6 and all(g is graph for g in calls)         # one encoding per call of predict()


# ----------------------------------------------------------------------------- 9. no score matrix
def test_no_score_matrix_at_forty_thousand_entities():
    """2,000 queries x 40,000 entities: the call's peak memory stays far under the 320 MB of the fp32 score matrix (the workspace is 10 MB
    of mask and the strips' lists), and the answer is the fallback's"""
    from utils import misc
    N, Q, dim, k = 40_000, 2_000, 32, 10
    g = torch.Generator().manual_seed(7)
    nodes, rel = torch.randn(N, dim, generator=g).numpy(), torch.randn(R0, dim, generator=g).numpy()
    model = _Model(_decoder(nodes, rel, [None] * 3, N, R0), torch.from_numpy(nodes).to(DEV))
    rng = np.random.default_rng(3)
    queries = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    known = np.stack([rng.integers(0, N, 8_000), rng.integers(0, R0, 8_000), rng.integers(0, N, 8_000)], 1)
    known[:6_000, :2] = queries[np.arange(6_000) % Q, :2]                 # three known tails per query
    true_triples = misc.generate_true_dict(np.concatenate([known, queries]))
    want, old_tags = _predict_tags(misc, model, None, queries, N, k=k, true_triples=true_triples, fused=False)
    assert len(old_tags["score_all"]) >= 2                                # the fallback chunks
    misc._filter_index(true_triples, N)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids, scores = misc.predict(model, None, queries, N, k=k, true_triples=true_triples)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"[topk] peak memory rise {rise} bytes; the score matrix of this batch = {4 * Q * N}")
    assert rise < 4 * Q * N, rise
    got = (ids.cpu().numpy(), scores.cpu().numpy())
    assert same(got, want), first_difference(got, want)
    hit = sum(1 for (s, p, o), row in zip(queries.tolist(), got[0].tolist()) if set(row) & set(true_triples[1][(s, p)]))
    assert hit == 0


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
            _native.distmult_topk(torch.tensor(bad, device=DEV), True, nodes, rel)
    for fq, fn in ((i32(2), i32(0)), (i32(-1), i32(0)), (i32(0), i32(10)), (i32(0), i32(-1))):       # filter entry out of range
        with pytest.raises(IndexError):
            _native.distmult_topk(ok, True, nodes, rel, filt_q=fq, filt_n=fn)
    with pytest.raises(RuntimeError):
        _native.distmult_topk(ok.cpu(), True, nodes, rel)                                            # no CPU path
    with pytest.raises(AssertionError):
        _native.distmult_topk(ok, True, nodes, rel, torch.zeros(10, device=DEV), None, None)         # biases: all or none
    for kw in ({"strips": -1}, {"k": 0}, {"k": -2}, {"k": 2.0}, {"filt_q": i32(0)}):
        with pytest.raises(AssertionError):
            _native.distmult_topk(ok, True, nodes, rel, **kw)
    ids, scores = _native.distmult_topk(ok[:0], True, nodes, rel, k=4)                               # Q = 0: empty outputs
    assert ids.shape == scores.shape == (0, 4) and ids.dtype == torch.int64 and scores.dtype == torch.float32


def test_c_abi_argument_errors():
    from torch_rgcn import _native
    L = _native.lib()
    N, dim, Q, k = 10, 8, 2, 3
    nodes, rel = torch.randn(N, dim, device=DEV), torch.randn(3, dim, device=DEV)
    nodes16 = nodes.to(BF)
    batch = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    fq, fn = torch.tensor([0], device=DEV, dtype=torch.int32), torch.tensor([5], device=DEV, dtype=torch.int32)
    ws = torch.empty(_native.topk_workspace_bytes(Q, N, dim, 32, 0, True) + 16, device=DEV, dtype=torch.uint8)
    ids, sc = torch.full((Q, 32), -7, device=DEV), torch.full((Q, 32), -7.0, device=DEV)
    st = _native._stream(nodes.device)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    assert p(ws) % 16 == 0

    def f32(w=p(ws), ip=p(ids), sp=p(sc), strips=0, F=0, q=None, n=None, k=k):
        return L.rgcn_distmult_topk_f32(p(batch), Q, 1, p(nodes), p(rel), None, None, None, q, n, F, None, None, None, 0, k, strips, w, ip, sp,
                                        N, 3, dim, st)

    def b16(w=p(ws), ip=p(ids), sp=p(sc), strips=0, F=0, q=None, n=None, k=k):
        return L.rgcn_distmult_topk_bf16(p(batch), Q, 1, p(nodes16), p(rel), None, None, None, q, n, F, None, None, None, 0, k, strips, w, ip, sp,
                                         N, 3, dim, st)

    for call in (f32, b16):
        assert call(w=None) == _native.EINVAL and call(ip=None) == _native.EINVAL and call(sp=None) == _native.EINVAL
        assert call(w=p(ws) + 4) == _native.EINVAL                        # misaligned workspace
        assert call(strips=-1) == _native.EINVAL and call(k=0) == _native.EINVAL and call(k=-1) == _native.EINVAL
        assert call(F=1) == _native.EINVAL and call(F=1, q=p(fq)) == _native.EINVAL and call(F=1, n=p(fn)) == _native.EINVAL
        assert call(F=-1) == _native.EINVAL
        assert b"distmult_topk" in L.rgcn_last_error()
        assert call(k=33) == _native.EUNSUPPORTED and b"native limit of 32" in L.rgcn_last_error()
    torch.cuda.synchronize()
    assert (ids == -7).all() and (sc == -7.0).all()                       # nothing was launched
    # biases partly set; Q == 0 is fine with nothing else set
    assert L.rgcn_distmult_topk_f32(p(batch), Q, 1, p(nodes), p(rel), p(sc), None, None, None, None, 0, None, None, None, 0, k, 0, p(ws), p(ids),
                                    p(sc), N, 3, dim, st) == _native.EINVAL
    assert L.rgcn_distmult_topk_f32(None, 0, 1, None, None, None, None, None, None, None, 0, None, None, None, 0, k, 0, None, None, None,
                                    N, 3, dim, st) == _native.OK
    assert L.rgcn_distmult_topk_bf16(None, 0, 1, None, None, None, None, None, None, None, 0, None, None, None, 0, k, 0, None, None, None,
                                     N, 3, dim, st) == _native.OK
    # and the good call, through the same closures: rows of k in the first Q * k cells of the outputs
    assert f32(F=1, q=p(fq), n=p(fn)) == _native.OK
    want = _native.distmult_topk(batch, True, nodes, rel, k=k, filt_q=fq, filt_n=fn)
    assert torch.equal(ids.flatten()[:Q * k].view(Q, k), want[0]) and torch.equal(sc.flatten()[:Q * k].view(Q, k), want[1])
    assert 5 not in want[0][0].tolist() and (ids.flatten()[Q * k:] == -7).all()
    assert b16(k=32) == _native.OK                                        # k > N: ten candidates, then the padding
    want = _native.distmult_topk(batch, True, nodes16, rel, k=32)
    assert torch.equal(ids, want[0]) and torch.equal(sc, want[1])
    assert (ids[:, :N] >= 0).all() and (ids[:, N:] == -1).all() and (sc[:, N:] == -INF).all()
