"""The 1-N multi-label BCE loss of DistMult: functional.distmult_bce_loss -- the strip pass that sums softplus(s) and the
positive scores per query, the gradient cells sigmoid(s) - y', the query-side bias gradients -- against float64 on the CPU.  The
reference is computed in this file from the inputs, never from the library's scores:

    y[q, n]  = 1 on the query's own target and on every listed / known cell, else 0;       y' = (1 - eps) y + eps / N
    loss[q]  = (1 / N) sum_n (softplus(s[q, n]) - y'[q, n] s[q, n])

with s in float64 and float64 autograd.  Every reference is compared, when it is built, with
torch.nn.functional.binary_cross_entropy_with_logits(s, y') in float64 to 1e-12: the closed form is checked against an independent one.

Bound: the suite's parity bound (README, "parity"), 1e-4 relative in the max norm of each compared array.  One array is not fp32: dnodes
of a bf16 table is bf16, one rounding of an fp32 gradient within 1e-4 -- half an ulp of bf16, 2^-8 of the max norm, the bound
test_gpu_softmax_loss_bf16.py derives.  Unlike the softmax loss no reference here is identically zero: the rows of the gradient cells do
not sum to zero, so all three bias gradients are compared relatively, the query-side ones by name.  The case builder of
test_gpu_softmax_loss_smooth.py is restated here, not imported."""
import functools

import numpy as np
import pytest
import torch

import guard_bands as gb
import torch_rgcn  # noqa: F401

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
F64 = torch.float64
R0 = 5
BOUND = 1e-4
BF_BOUND = 2.0 ** -8
SHAPES = [(1, 1, 1), (63, 65, 6), (130, 3, 8), (257, 129, 50), (77, 10, 500), (700, 130, 24)]
EPS = (0.0, 0.1)
STRIPS = (0, 1, 3, 64)
MODES = ["fp32", "upcast", "native"]        # the storage and, for bf16, the route of a table that trains
KINDS = (None, "random", "known", "index")  # the positives: the targets alone, random lists, the known completions as lists / as an index


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


def make_case(N, Q, dim, biased, storage, integer=False, scale=1.0):
    """host arrays of one case; bf16 storage: the table rounded to bf16; scale: a factor on the entity table (a power of two)"""
    rng = np.random.default_rng(1000 * N + 10 * Q + dim + biased)
    if integer:          # small integers: every product and sum is exact
        nodes = rng.integers(-2, 3, (N, dim)).astype(np.float32)
        copies = rng.permutation(N)[: N // 4]
        nodes[copies] = nodes[rng.integers(0, N, len(copies))]
        rel = rng.integers(-2, 3, (R0, dim)).astype(np.float32)
        bias = [rng.integers(-1, 2, n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    else:
        nodes = rng.standard_normal((N, dim)).astype(np.float32) * np.float32(scale)
        rel = rng.standard_normal((R0, dim)).astype(np.float32)
        bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    if storage == "bf16":
        nodes = torch.from_numpy(nodes).to(BF).float().numpy()
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    return rng, nodes, rel, bias, batch


def random_labels(rng, batch, N, head):
    """about 3 Q random cells, NOT deduplicated, then the own targets of every other query and a second copy of the first Q cells: a
    listed target must stay a label, and a duplicate must not count twice"""
    Q = len(batch)
    cells = np.stack([rng.integers(0, Q, 3 * Q), rng.integers(0, N, 3 * Q)], 1)
    own = np.stack([np.arange(0, Q, 2), batch[::2, 0 if head else 2]], 1)
    return np.concatenate([cells, own, cells[:Q]]).astype(np.int64)


def known_labels(batch, N):
    """known triples around the batch (the batch itself and about 3 Q triples that share a query's (s, p) or (p, o)) -> the dictionary a
    FilterIndex is built from, and per direction the same cells as (query, entity) lists, own targets among them"""
    from utils.misc import generate_true_dict
    Q = len(batch)
    rng = np.random.default_rng(17 * N + Q)
    more = batch[rng.integers(0, Q, 3 * Q)].copy()
    half = len(more) // 2
    more[:half, 0] = rng.integers(0, N, half)
    more[half:, 2] = rng.integers(0, N, len(more) - half)
    known = np.concatenate([batch, more])
    lists = {}
    for head in (True, False):
        cells = set()
        for q, (s, p, o) in enumerate(batch):
            same = known[(known[:, 1] == p) & ((known[:, 2] == o) if head else (known[:, 0] == s))]
            cells.update((q, int(n)) for n in same[:, 0 if head else 2])
        lists[head] = np.array(sorted(cells), dtype=np.int64)
    return generate_true_dict(known), lists


def lists_of(cells, put=dev):
    if cells is None or not len(cells):
        return None, None
    return put(cells[:, 0].astype(np.int32)), put(cells[:, 1].astype(np.int32))


class Ref:
    """float64 on the CPU: scores, labels, and per eps the loss vector and the gradients of its mean"""

    def __init__(self, nodes, rel, bias, batch, head, cells, eps=EPS, grads=True):
        n = torch.tensor(nodes, dtype=F64, requires_grad=True)
        r = torch.tensor(rel, dtype=F64, requires_grad=True)
        b = [None if x is None else torch.tensor(x, dtype=F64, requires_grad=True) for x in bias]
        leaves = [n, r] + [x for x in b if x is not None]
        bt = torch.from_numpy(batch)
        Q, N = len(batch), len(nodes)
        anchor, p, tgt = bt[:, 2 if head else 0], bt[:, 1], bt[:, 0 if head else 2]
        s = (n[anchor] * r[p]) @ n.T
        if b[0] is not None:
            sb, pb, ob = b
            s = s + ((sb[None, :] + pb[p][:, None] + ob[anchor][:, None]) if head else (sb[anchor][:, None] + pb[p][:, None] + ob[None, :]))
        y = torch.zeros(Q, N, dtype=torch.bool)
        if cells is not None and len(cells):
            y[torch.from_numpy(cells[:, 0]), torch.from_numpy(cells[:, 1])] = True
        y[torch.arange(Q), tgt] = True                                      # the target is a label, listed or not
        self.scores, self.y = s.detach().numpy(), y.numpy()
        self.npos = y.sum(1).numpy()
        self.ps = s.detach().masked_fill(~y, 0.0).sum(1).numpy()
        self.sp = torch.nn.functional.softplus(s.detach()).sum(1).numpy()
        self.loss, self.dnodes, self.drel, self.dbias = {}, {}, {}, {}
        yf = y.to(F64)
        for e in eps:
            ys = (1 - e) * yf + e / N
            loss = (torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs())) - ys * s).sum(1) / N
            self.loss[e] = loss.detach().numpy()
            bce = torch.nn.functional.binary_cross_entropy_with_logits(s.detach(), ys, reduction="none").mean(1).numpy()
            assert np.abs(bce - self.loss[e]).max() <= 1e-12 * max(np.abs(bce).max(), 1.0), (e, np.abs(bce - self.loss[e]).max())
            whole = float(torch.nn.functional.binary_cross_entropy_with_logits(s.detach(), ys))
            assert abs(whole - self.loss[e].mean()) <= 1e-12 * max(abs(whole), 1.0)
            if grads:
                g = torch.autograd.grad(loss.mean(), leaves, retain_graph=True)
                self.dnodes[e], self.drel[e] = g[0].numpy(), g[1].numpy()
                self.dbias[e] = [None] * 3 if b[0] is None else [x.numpy() for x in g[2:]]


@functools.lru_cache(maxsize=None)
def case_and_refs(N, Q, dim, biased, storage="fp32", integer=False, scale=1.0):
    """one case with its label sets and references, computed once and shared (never written to).  labels / refs are keyed (head, kind)
    with kind None (the targets alone), "random" (lists with own targets and duplicates) or "known" (what a FilterIndex of `true` holds)"""
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, biased, storage, integer, scale)
    true, known = known_labels(batch, N)
    labels = {}
    for head in (True, False):
        labels[head, None], labels[head, "random"], labels[head, "known"] = None, random_labels(rng, batch, N, head), known[head]
    refs = {k: Ref(nodes, rel, bias, batch, k[0], c, grads=not integer) for k, c in labels.items()}
    return nodes, rel, bias, batch, labels, refs, true


def close(got, want, what, bound=BOUND):
    """max |got - want| <= bound * max |want|"""
    if torch.is_tensor(got):
        got = got.detach().float().cpu().numpy()
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err, norm = np.abs(got - want).max(initial=0.0), np.abs(want).max(initial=0.0)
    print(f"[bce_loss] {what}: max err {err:.3e}, norm {norm:.3e}, relative {err / norm if norm else 0.0:.3e}")
    assert np.isfinite(got).all(), what
    assert err <= bound * norm, (what, err, norm)


def params_on_device(nodes, rel, bias, storage="fp32", grad=(True, True, True), put=dev):
    nt = put(nodes, BF if storage == "bf16" else None)
    rt = put(rel)
    bt = [put(b) for b in bias]
    nt.requires_grad_(grad[0]); rt.requires_grad_(grad[1])
    for b in bt:
        if b is not None:
            b.requires_grad_(grad[2])
    return nt, rt, bt


def storage_of(mode):
    return "fp32" if mode == "fp32" else "bf16"


def loss_of(batch_t, head, nt, rt, bt, labels=None, put=dev, mode="fp32", **kw):
    """labels: None, an array of (query, entity) cells (the list form) or a FilterIndex"""
    from torch_rgcn import functional
    if mode != "fp32":
        kw["bf16_backward"] = mode
    if labels is not None and not isinstance(labels, np.ndarray):
        return functional.distmult_bce_loss(batch_t, head, nt, rt, *bt, labels=labels, **kw)
    lq, ln = lists_of(labels, put)
    return functional.distmult_bce_loss(batch_t, head, nt, rt, *bt, lab_q=lq, lab_n=ln, **kw)


def check_grads(ref, eps, head, nt, rt, bt, what):
    if nt.grad is not None:
        assert nt.grad.dtype == nt.dtype
        close(nt.grad, ref.dnodes[eps], what + " dnodes", bound=BF_BOUND if nt.dtype == BF else BOUND)
    if rt.grad is not None:
        close(rt.grad, ref.drel[eps], what + " drel")
    if bt[0] is not None and bt[0].grad is not None:
        cand = 0 if head else 2
        for k, name in enumerate(("dsbias", "dpbias", "dobias")):
            assert np.abs(ref.dbias[eps][k]).max() > 0.0                    # the query-side ones too: their rows do not sum to zero
            close(bt[k].grad, ref.dbias[eps][k], f"{what} {name} ({'candidate' if k == cand else 'query'} side)")


def zero_grads(nt, rt, bt):
    for t in [nt, rt] + bt:
        if t is not None:
            t.grad = None


def the_labels(labels, true, head, kind, N):
    """what loss_of takes for one kind of labels: "index" is the known completions as a FilterIndex"""
    from torch_rgcn.functional import FilterIndex
    if kind == "index":
        return FilterIndex(true, N, DEV), "known"
    return labels[head, kind], kind


# ----------------------------------------------------------------------------- 1. forward and gradient parity
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_forward_and_gradient_parity(N, Q, dim, biased, mode):
    """the loss vector (reduction='none') for every `strips`, its mean, and the gradients of the mean; head and tail; every kind of
    labels; both eps"""
    from torch_rgcn import _native, functional
    storage = storage_of(mode)
    nodes, rel, bias, batch, labels, refs, true = case_and_refs(N, Q, dim, biased, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    bf = "_bf16" if mode == "native" else ""
    for head in (True, False):
        for kind in KINDS:
            lab, ref_kind = the_labels(labels, true, head, kind, N)
            ref = refs[head, ref_kind]
            for eps in EPS:
                what = f"{mode} N={N} Q={Q} d={dim} b={biased} head={head} labels={kind} eps={eps}"
                for strips in STRIPS[1:]:
                    with torch.no_grad():
                        close(loss_of(batch_t, head, nt, rt, bt, lab, mode=mode, reduction="none", strips=strips, label_smoothing=eps),
                              ref.loss[eps], f"{what} strips={strips} loss")
                zero_grads(nt, rt, bt)
                _native.profile_start()
                loss = loss_of(batch_t, head, nt, rt, bt, lab, mode=mode, reduction="none", label_smoothing=eps)
                assert loss.shape == (Q,) and loss.dtype == torch.float32
                close(loss, ref.loss[eps], what + " loss")
                loss.mean().backward()
                tags = set(_native.profile_stop())
                assert tags == {"bce_sums" + bf, "bce_grad" + bf, "gemm"}, tags
                check_grads(ref, eps, head, nt, rt, bt, what + " [none]")
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, lab, mode=mode, label_smoothing=EPS[1])
            close(loss, ref.loss[EPS[1]].mean(), what + " mean loss")
            loss.backward(gradient=functional.unit_gradient(loss.device))
            check_grads(ref, EPS[1], head, nt, rt, bt, what + " [mean]")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("frozen", ["nodes", "relations", "biases"])
def test_gradient_parity_with_frozen_inputs(frozen, mode):
    """each input frozen in turn: the others still match, the frozen one gets no gradient"""
    N, Q, dim = 257, 129, 50
    storage = storage_of(mode)
    nodes, rel, bias, batch, labels, refs, _ = case_and_refs(N, Q, dim, True, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage, grad=(frozen != "nodes", frozen != "relations", frozen != "biases"))
    batch_t = dev(batch)
    for head in (True, False):
        zero_grads(nt, rt, bt)
        loss_of(batch_t, head, nt, rt, bt, labels[head, "random"], mode=mode, label_smoothing=0.1).backward()
        assert (nt.grad is None) == (frozen == "nodes") and (rt.grad is None) == (frozen == "relations")
        assert all((b.grad is None) == (frozen == "biases") for b in bt)
        check_grads(refs[head, "random"], 0.1, head, nt, rt, bt, f"{mode} frozen {frozen} head={head}")


def test_a_bf16_table_that_does_not_train_runs_the_bf16_forward():
    from torch_rgcn import _native
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, labels, refs, _ = case_and_refs(N, Q, dim, True, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16", grad=(False, False, False))
    for mode in ("upcast", "native"):
        _native.profile_start()
        loss = loss_of(dev(batch), True, nt, rt, bt, labels[True, "random"], mode=mode, reduction="none", label_smoothing=0.1)
        assert set(_native.profile_stop()) == {"bce_sums_bf16"}
        close(loss, refs[True, "random"].loss[0.1], f"bf16 forward alone [{mode}]")
    nt.requires_grad_(True)                                                     # and one that trains, upcast: the fp32 route
    _native.profile_start()
    loss_of(dev(batch), True, nt, rt, bt, labels[True, "random"], mode="upcast", label_smoothing=0.1).backward()
    tags = set(_native.profile_stop())
    assert "bce_sums" in tags and "bce_grad" in tags and not any(t.endswith("_bf16") for t in tags), tags
    assert nt.grad.dtype == BF


# ----------------------------------------------------------------------------- 2. ps and npos are exact
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_the_positive_sum_and_the_label_count_are_exact(N, Q, dim, biased, storage):
    """integer inputs (entries in [-2, 2], biases in [-1, 1]): every score is an integer and every partial sum of a row stays below 2^24
    (|s| <= 8 d + 3, and (8 * 500 + 3) * 77 and (8 * 50 + 3) * 700 are below 2^24), so fp32 adds them exactly in any order: ps must
    EQUAL the float64 sum over the labels and npos their count, for every number of strips -- with 64 most strips of these shapes have no
    tile.  One lost, doubled or misplaced label bit, a dropped target or one column beyond N counted fails this where the parity bound
    would not see it.  The list form and the index form of the same labels give the same bits, and so do two calls."""
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, labels, refs, true = case_and_refs(N, Q, dim, biased, storage, True)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage, grad=(False, False, False))
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    for head in (True, False):
        got = {}
        for kind in KINDS:
            ref = refs[head, "known" if kind == "index" else kind]
            assert np.array_equal(ref.scores, np.round(ref.scores)) and np.abs(ref.scores).sum(1).max() < 2 ** 24
            lq, ln = lists_of(None if kind == "index" else labels[head, kind])
            for strips in STRIPS:
                kw = dict(lab_q=lq, lab_n=ln, strips=strips, labels=index if kind == "index" else None)
                sp, ps, npos = _native.distmult_bce_sums(batch_t, head, nt, rt, *bt, **kw)
                assert sp.dtype == ps.dtype == torch.float32 and npos.dtype == torch.int32 and sp.shape == ps.shape == npos.shape == (Q,)
                what = (storage, N, Q, dim, biased, head, kind, strips)
                assert np.array_equal(npos.cpu().numpy(), ref.npos), what
                assert np.array_equal(ps.cpu().numpy().astype(np.float64), ref.ps), what
                close(sp, ref.sp, f"integer sp {what}")
                again = _native.distmult_bce_sums(batch_t, head, nt, rt, *bt, **kw)
                assert torch.equal(again[0], sp) and torch.equal(again[1], ps) and torch.equal(again[2], npos), what
                got[kind, strips] = sp, ps, npos
        for strips in STRIPS:
            assert all(torch.equal(a, b) for a, b in zip(got["known", strips], got["index", strips])), (head, strips)


# ----------------------------------------------------------------------------- 3. scores beyond the range of exp
@pytest.mark.parametrize("mode", ["fp32", "native"])
def test_scores_beyond_the_range_of_exp(mode):
    """the entity table times 4: the float64 scores pass +100 and -100, where log(1 + exp(s)) is infinite in fp32"""
    N, Q, dim = 257, 129, 50
    storage = storage_of(mode)
    nodes, rel, bias, batch, labels, refs, _ = case_and_refs(N, Q, dim, True, storage, False, 4.0)
    for head in (True, False):
        s = refs[head, "random"].scores
        assert s.max() > 100.0 and s.min() < -100.0, (s.min(), s.max())
        with np.errstate(over="ignore"):
            assert not np.isfinite(np.log1p(np.exp(s.astype(np.float32)))).all()   # the naive form does overflow here
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    for head in (True, False):
        ref = refs[head, "random"]
        for eps in EPS:
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, labels[head, "random"], mode=mode, reduction="none", label_smoothing=eps)
            assert torch.isfinite(loss).all()
            close(loss, ref.loss[eps], f"large scores {mode} head={head} eps={eps} loss")
            loss.mean().backward()
            check_grads(ref, eps, head, nt, rt, bt, f"large scores {mode} head={head} eps={eps}")


# ----------------------------------------------------------------------------- 4. chunks; lists and index
@pytest.mark.parametrize("N,Q,dim,n_chunks", [(257, 129, 50, 3), (700, 130, 24, 6)])
def test_chunks(N, Q, dim, n_chunks):
    """chunk_bytes = 4 Q 128: chunks of one tile column, the last ragged and narrower than a tile"""
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    budget = 4 * Q * 128
    plan = functional.softmax_chunk_plan(Q, N, budget)
    assert len(plan) == n_chunks and plan[-1][1] < 128
    nodes, rel, bias, batch, labels, refs, true = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    for head in (True, False):
        ref = refs[head, "known"]
        for eps in EPS:
            grads = []
            for chunk_bytes in (budget, None):
                zero_grads(nt, rt, bt)
                loss = loss_of(batch_t, head, nt, rt, bt, index, reduction="none", chunk_bytes=chunk_bytes, label_smoothing=eps)
                loss.mean().backward()
                check_grads(ref, eps, head, nt, rt, bt, f"N={N} chunks={n_chunks if chunk_bytes else 1} head={head} eps={eps}")
                grads.append([nt.grad.cpu().numpy(), rt.grad.cpu().numpy()] + [b.grad.cpu().numpy() for b in bt])
            for k, (x, y) in enumerate(zip(*grads)):
                close(x, y, f"N={N} chunk plans against each other head={head} eps={eps} [{k}]")
    # integer inputs: sigmoid(s) - dS / scale is the label, to rounding -- every label bit of every chunk is recovered exactly, and the
    # list form and the index form of the same labels write the same bits
    nodes, rel, bias, batch, labels, refs, true = case_and_refs(N, Q, dim, True, "fp32", True)
    nt, rt, bt = params_on_device(nodes, rel, bias, grad=(False, False, False))
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    g = torch.full((), 2.0, device=DEV)
    for head in (True, False):
        ref = refs[head, "known"]
        lq, ln = lists_of(labels[head, "known"])
        sig = 1.0 / (1.0 + np.exp(-ref.scores))
        tgt = batch[:, 0 if head else 2]
        for c_first, c_count in plan:
            listed = _native.distmult_bce_grad(batch_t, head, nt, rt, *bt, lq, ln, g, 1, c_first, c_count).clone()
            got = _native.distmult_bce_grad(batch_t, head, nt, rt, *bt, None, None, g, 1, c_first, c_count, labels=index)
            assert torch.equal(got, listed), (head, c_first)
            y = np.rint(sig[:, c_first:c_first + c_count] - got.cpu().numpy().astype(np.float64) * (N / 2.0))
            assert np.array_equal(y, ref.y[:, c_first:c_first + c_count].astype(np.float64)), (head, c_first)
            inside = (tgt >= c_first) & (tgt < c_first + c_count)
            assert (y[np.nonzero(inside)[0], tgt[inside] - c_first] == 1.0).all()       # the targets of this chunk
            smooth = _native.distmult_bce_grad(batch_t, head, nt, rt, *bt, None, None, g, 1, c_first, c_count, labels=index, label_smoothing=0.25)
            want = (sig[:, c_first:c_first + c_count] - 0.75 * ref.y[:, c_first:c_first + c_count] - 0.25 / N) * (2.0 / N)
            close(smooth, want, f"N={N} smoothed cells head={head} c_first={c_first}")


# ----------------------------------------------------------------------------- 5. no queries
def test_no_queries_behave_as_the_softmax_loss_does():
    from torch_rgcn import functional
    nodes, rel, bias, _, _, _, _ = case_and_refs(130, 3, 8, True)
    empty = torch.empty(0, 3, dtype=torch.int64, device=DEV)
    for fn in (functional.distmult_softmax_loss, functional.distmult_bce_loss):
        nt, rt, bt = params_on_device(nodes, rel, bias)
        vec = fn(empty, True, nt, rt, *bt, reduction="none")
        assert vec.shape == (0,) and vec.dtype == torch.float32
        vec.sum().backward()
        for t in [nt, rt] + bt:
            assert t.grad is not None and t.grad.shape == t.shape and (t.grad == 0).all(), fn.__name__
        assert torch.isnan(fn(empty, True, nt, rt, *bt)), fn.__name__            # the mean of nothing, both


# ----------------------------------------------------------------------------- 6. no host synchronisation
@pytest.mark.parametrize("mode", ["fp32", "native"])
def test_forward_and_backward_issue_no_synchronisation(mode):
    from torch_rgcn import _native, functional, routes
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 700, 130, 24
    storage = storage_of(mode)
    nodes, rel, bias, batch, _, refs, true = case_and_refs(N, Q, dim, True, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    with routes.override(deferred_checks="1"):
        def step():
            zero_grads(nt, rt, bt)
            loss = 0.5 * (loss_of(batch_t, False, nt, rt, bt, index, mode=mode, chunk_bytes=4 * Q * 256, label_smoothing=0.1) +
                          loss_of(batch_t, True, nt, rt, bt, mode=mode, label_smoothing=0.1))
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
        close(loss, 0.5 * (refs[False, "known"].loss[0.1].mean() + refs[True, None].loss[0.1].mean()), f"sync-free loss [{mode}]")


# ----------------------------------------------------------------------------- 7. guard bands
@pytest.mark.parametrize("kind", ["random", "index"])
@pytest.mark.parametrize("mode", ["fp32", "native"])
def test_under_guard_bands(mode, kind, monkeypatch):
    """one case per new kernel route (fp32 / bf16 strip pass and gradient cells, labels from the lists / from the index): every buffer
    between two poisoned bands, the library's torch.empty buffers full of NaN before the call"""
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 257, 129, 50
    storage = storage_of(mode)
    nodes, rel, bias, batch, labels, refs, true = case_and_refs(N, Q, dim, True, storage)
    index = FilterIndex(true, N, DEV) if kind == "index" else None
    got = {}
    with gb.Guard(monkeypatch) as guard:
        put = lambda a, dt=None: None if a is None else guard.home(dev(a, dt))  # noqa: E731
        nt, rt, bt = params_on_device(nodes, rel, bias, storage, put=put)
        batch_t = put(batch)
        assert torch.isnan(torch.empty(3, device=DEV)).all()
        for head in (True, False):
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, index if kind == "index" else labels[head, "random"], put=put, mode=mode,
                           reduction="none", chunk_bytes=4 * Q * 128, label_smoothing=0.1)
            loss.mean().backward()
            got[head] = (loss.detach().cpu().numpy(), nt.grad.float().cpu().numpy(), rt.grad.cpu().numpy(), [b.grad.cpu().numpy() for b in bt])
        problems = guard.problems(f"bce loss {mode} {kind} N={N} Q={Q} d={dim}")
    assert not problems, "\n".join(problems)
    for head in (True, False):
        ref = refs[head, "known" if kind == "index" else "random"]
        loss, dn, dr, db = got[head]
        close(loss, ref.loss[0.1], f"guarded {mode} {kind} head={head} loss")
        close(dn, ref.dnodes[0.1], f"guarded {mode} {kind} head={head} dnodes", bound=BF_BOUND if storage == "bf16" else BOUND)
        close(dr, ref.drel[0.1], f"guarded {mode} {kind} head={head} drel")
        for k in range(3):
            close(db[k], ref.dbias[0.1][k], f"guarded {mode} {kind} head={head} bias {k}")


# ----------------------------------------------------------------------------- the layer, the entry points
def test_distmult_layer_passes_its_arguments_on():
    from torch_rgcn.layers import DistMult
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, labels, refs, _ = case_and_refs(N, Q, dim, True)
    dm = DistMult(R0, dim, N, R0, b_init="ones").to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        for n, b in zip(("sbias", "pbias", "obias"), bias):
            getattr(dm, n).copy_(torch.from_numpy(b))
    nt = dev(nodes).requires_grad_(True)
    lq, ln = lists_of(labels[True, "random"])
    ref = refs[True, "random"]
    loss = dm.bce_loss(torch.from_numpy(batch), nt, head=True, lab_q=lq, lab_n=ln, reduction="none", label_smoothing=0.1)
    close(loss, ref.loss[0.1], "layer loss")
    diff, norm = np.abs(ref.loss[0.1] - ref.loss[0.0]).max(), np.abs(ref.loss[0.0]).max()
    assert diff > 10 * BOUND * norm                                            # the keyword is not merely accepted
    diff = np.abs(ref.loss[0.0] - refs[True, None].loss[0.0]).max()
    assert diff > 10 * BOUND * norm                                            # nor are the lists
    loss.mean().backward()
    close(nt.grad, ref.dnodes[0.1], "layer dnodes")
    close(dm.relations.grad, ref.drel[0.1], "layer drel")
    for k, n in enumerate(("sbias", "pbias", "obias")):
        close(getattr(dm, n).grad, ref.dbias[0.1][k], "layer d" + n)


def test_the_entry_points_refuse_bad_arguments():
    from torch_rgcn import _native
    nodes, rel = torch.randn(10, 8, device=DEV), torch.randn(3, 8, device=DEV)
    ok = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    L, st = _native.lib(), _native._stream(nodes.device)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    g = torch.ones(1, device=DEV)
    sp, ps, npos = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, device=DEV, dtype=torch.int32)
    lq, ln = torch.tensor([0], device=DEV, dtype=torch.int32), torch.tensor([5], device=DEV, dtype=torch.int32)
    keys, ptr = torch.tensor([0], device=DEV), torch.tensor([0, 1], device=DEV)
    dS = torch.full((2, 10), -7.0, device=DEV)
    ws = torch.empty(_native.bce_sums_workspace_bytes(2, 10, 8) + 1024, device=DEV, dtype=torch.uint8)

    def fwd(sp_=p(sp), npos_=p(npos), w=p(ws), F=0, K=0):
        return L.rgcn_distmult_bce_sums_f32(p(ok), 2, 1, p(nodes), p(rel), None, None, None, p(lq) if F else None, p(ln) if F else None, F,
                                            p(keys) if K else None, p(ptr) if K else None, p(ln) if K else None, K, 0, w, sp_, p(ps), npos_,
                                            10, 3, 8, st)

    def grad(gs=p(g), c_first=0, F=0, K=0):
        return L.rgcn_distmult_bce_grad_f32(p(ok), 2, 1, p(nodes), p(rel), None, None, None, p(lq) if F else None, p(ln) if F else None, F,
                                            p(keys) if K else None, p(ptr) if K else None, p(ln) if K else None, K, gs, 0, 2, None, c_first, 10,
                                            p(ws), p(dS), 10, 3, 8, st)
    assert fwd(sp_=None) == _native.EINVAL and fwd(npos_=None) == _native.EINVAL and fwd(w=p(ws) + 4) == _native.EINVAL
    assert fwd(F=1, K=1) == _native.EINVAL                                      # the lists and the index together
    assert grad(gs=None) == _native.EINVAL and grad(c_first=64) == _native.EINVAL and grad(F=1, K=1) == _native.EINVAL
    assert b"distmult_bce_grad" in L.rgcn_last_error()
    torch.cuda.synchronize()
    assert (dS == -7.0).all()                                                  # nothing was launched
    assert fwd() == _native.OK and grad() == _native.OK
    torch.cuda.synchronize()
    assert torch.isfinite(dS).all() and (npos == 1).all()                      # 1-vs-All: the target alone
    assert fwd(F=1) == _native.OK
    torch.cuda.synchronize()
    assert npos.tolist() == [2, 1]                                             # query 0: its target 0 and the listed 5
    out = _native.distmult_bce_sums(ok[:0], True, nodes, rel)                  # Q = 0: empty outputs
    assert all(t.shape == (0,) for t in out)
