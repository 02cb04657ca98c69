"""Label smoothing in the 1-N softmax loss of DistMult: functional.distmult_softmax_loss(..., label_smoothing=eps) --
the strip pass that carries the sum and the count of the allowed scores beside (max, sum exp), and the gradient cells with the two more
terms -- against float64 on the CPU.  The reference is computed in this file from the inputs, never from the library's scores:

    loss[q] = lse[q] - (1 - eps) s[q, t_q] - (eps / n_q) sum_{n allowed} s[q, n]

with s in float64, listed cells removed, an entry on a query's own target ignored, n_q the number of allowed cells, float64 autograd.
For the unfiltered cases every reference is compared, when it is built, with torch.nn.functional.cross_entropy(label_smoothing=eps) in
float64 to 1e-12: the closed form is checked against an independent one.

Bound: the suite's parity bound (README, "parity"), 1e-4 relative in the max norm of each compared array; a bias gradient whose
reference is identically zero (the query-side ones) is compared absolutely against 1e-4 of the candidate-side norm.  One array is not
fp32: dnodes of a bf16 table is bf16, one rounding of an fp32 gradient within 1e-4 -- half an ulp of bf16, 2^-8 of the max norm, the
bound test_gpu_softmax_loss_bf16.py derives for the unsmoothed route.  With one entity (N = 1) the loss and every gradient are zero in
exact arithmetic -- lse = s, and s - (1 - eps) s - eps s -- and their float64 references are rounding noise of 1e-17: like the query-side
bias gradients they are compared absolutely, against 1e-4 of the norm of the term the others cancel against (lse, and the gradient of
mean lse).  The case builder and the float64 reference of
test_gpu_softmax_loss.py are restated here, not imported."""
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
EPS = (0.1, 0.25)
STRIPS = (0, 1, 3, 64)
MODES = ["fp32", "upcast", "native"]        # the storage and, for bf16, the route of a table that trains


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


def make_case(N, Q, dim, biased, storage, integer=False):
    """host arrays of one case; bf16 storage: the table rounded to bf16"""
    rng = np.random.default_rng(1000 * N + 10 * Q + dim + biased)
    if integer:          # small integers: every product and sum is exact
        nodes = rng.integers(-2, 3, (N, dim)).astype(np.float32)
        copies = rng.permutation(N)[: N // 4]
        nodes[copies] = nodes[rng.integers(0, N, len(copies))]
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


def known_filter(batch, N):
    """known triples around the batch (the batch itself and about 3 Q triples that share a query's (s, p) or (p, o)) -> the dictionary a
    FilterIndex is built from, and per direction the same filter as (query, entity) lists, own targets among them"""
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


def lists_of(filt, put=dev):
    if filt is None or not len(filt):
        return None, None
    return put(filt[:, 0].astype(np.int32)), put(filt[:, 1].astype(np.int32))


class Ref:
    """float64 on the CPU: scores, the allowed cells, and per eps the loss vector and the gradients of its mean"""

    def __init__(self, nodes, rel, bias, batch, head, filt, eps=EPS, grads=True):
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
        mask = torch.zeros(Q, N, dtype=torch.bool)
        if filt is not None and len(filt):
            mask[torch.from_numpy(filt[:, 0]), torch.from_numpy(filt[:, 1])] = True
        mask[torch.arange(Q), tgt] = False                                  # an entry on the target is ignored
        self.scores, self.mask = s.detach().numpy(), mask.numpy()
        self.cnt = (~mask).sum(1).numpy()
        self.ssum = s.detach().masked_fill(mask, 0.0).sum(1).numpy()
        lse = torch.logsumexp(s.masked_fill(mask, -float("inf")), 1)
        self.lse = lse.detach().numpy()
        st = s[torch.arange(Q), tgt]
        # N = 1: everything is zero in exact arithmetic; the norms of lse and of the gradient of its mean are what errors are measured against
        self.zero_scale = None
        if N == 1:
            g = torch.autograd.grad(lse.mean(), leaves, retain_graph=True)
            self.zero_scale = {"loss": float(lse.detach().abs().max()), "dnodes": float(g[0].abs().max()), "drel": float(g[1].abs().max()),
                               "dbias": 1.0}                                 # (d lse / d bias is 1 for the one entity)
        self.loss, self.dnodes, self.drel, self.dbias = {}, {}, {}, {}
        for e in eps:
            loss = lse - (1 - e) * st - (e / (~mask).sum(1).to(F64)) * s.masked_fill(mask, 0.0).sum(1)
            self.loss[e] = loss.detach().numpy()
            if not mask.any():                                              # the closed form against torch's own, an independent formula
                ce = torch.nn.functional.cross_entropy(s.detach(), tgt, reduction="none", label_smoothing=e).numpy()
                assert np.abs(ce - self.loss[e]).max() <= 1e-12 * max(np.abs(ce).max(), 1.0), (e, np.abs(ce - self.loss[e]).max())
            if grads:
                g = torch.autograd.grad(loss.mean(), leaves, retain_graph=True)
                self.dnodes[e], self.drel[e] = g[0].numpy(), g[1].numpy()
                self.dbias[e] = [None] * 3 if b[0] is None else [x.numpy() for x in g[2:]]


@functools.lru_cache(maxsize=None)
def case_and_refs(N, Q, dim, biased, storage="fp32", integer=False):
    """one case with its filters and references, computed once and shared (never written to).  filts / refs are keyed (head, kind) with
    kind None (unfiltered), "random" (a list of about 3 Q random cells) or "known" (the lists a FilterIndex of `true` stands for)"""
    rng, nodes, rel, bias, batch = make_case(N, Q, dim, biased, storage, integer)
    true, known = known_filter(batch, N)
    filts = {}
    for head in (True, False):
        filts[head, None], filts[head, "random"], filts[head, "known"] = None, random_filter(rng, Q, N), known[head]
    refs = {k: Ref(nodes, rel, bias, batch, k[0], f, grads=not integer) for k, f in filts.items()}
    return nodes, rel, bias, batch, filts, refs, true


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max(initial=0.0), np.abs(want).max(initial=0.0)


def close(got, want, what, scale=None, bound=BOUND):
    """max |got - want| <= bound * max |want| (scale: the norm to measure against when the reference is identically zero)"""
    if torch.is_tensor(got):
        got = got.detach().float().cpu().numpy()
    err, norm = rel_err(got, want)
    norm = norm if scale is None else scale
    print(f"[softmax_loss_smooth] {what}: max err {err:.3e}, norm {norm:.3e}, relative {err / norm if norm else 0.0:.3e}")
    assert np.isfinite(np.asarray(got)).all(), what
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


def loss_of(batch_t, head, nt, rt, bt, filt=None, put=dev, mode="fp32", **kw):
    """filt: None, an array of (query, entity) cells (the list form) or a FilterIndex"""
    from torch_rgcn import functional
    if mode != "fp32":
        kw["bf16_backward"] = mode
    if filt is not None and not isinstance(filt, np.ndarray):
        return functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt=filt, **kw)
    fq, fn = lists_of(filt, put)
    return functional.distmult_softmax_loss(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, **kw)


def close_loss(got, ref, eps, what, mean=False):
    want = ref.loss[eps].mean() if mean else ref.loss[eps]
    close(got, want, what, scale=None if ref.zero_scale is None else ref.zero_scale["loss"])


def check_grads(ref, eps, head, nt, rt, bt, what):
    zs = ref.zero_scale or {}
    if nt.grad is not None:
        assert nt.grad.dtype == nt.dtype
        close(nt.grad, ref.dnodes[eps], what + " dnodes", scale=zs.get("dnodes"), bound=BF_BOUND if nt.dtype == BF else BOUND)
    if rt.grad is not None:
        close(rt.grad, ref.drel[eps], what + " drel", scale=zs.get("drel"))
    if bt[0] is not None and bt[0].grad is not None:
        cand = 0 if head else 2
        cand_norm = zs.get("dbias", np.abs(ref.dbias[eps][cand]).max())
        if zs:
            for k, name in enumerate(("dsbias", "dpbias", "dobias")):
                close(bt[k].grad, ref.dbias[eps][k], f"{what} {name} (one entity)", scale=cand_norm)
            return
        for k, name in enumerate(("dsbias", "dpbias", "dobias")):
            if k == cand:
                close(bt[k].grad, ref.dbias[eps][k], f"{what} {name}")
            else:                                                           # sum_n dS[q, n] = 0: the reference is rounding noise
                assert np.abs(ref.dbias[eps][k]).max() <= 1e-12
                close(bt[k].grad, np.zeros_like(ref.dbias[eps][k]), f"{what} {name} (query side)", scale=cand_norm)


def zero_grads(nt, rt, bt):
    for t in [nt, rt] + bt:
        if t is not None:
            t.grad = None


def the_filter(filts, true, head, kind, N):
    """what loss_of takes for one kind of filter: "index" is the known filter as a FilterIndex"""
    from torch_rgcn.functional import FilterIndex
    if kind == "index":
        return FilterIndex(true, N, DEV), "known"
    return filts[head, kind], kind


# ----------------------------------------------------------------------------- 1. forward and gradient parity
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_forward_and_gradient_parity(N, Q, dim, biased, mode):
    """the loss vector (reduction='none') and the gradients of the mean; head and tail; unfiltered, a random list, the known completions
    as lists and as a FilterIndex; both eps"""
    from torch_rgcn import _native, functional
    storage = storage_of(mode)
    nodes, rel, bias, batch, filts, refs, true = case_and_refs(N, Q, dim, biased, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    bf = "_bf16" if mode == "native" else ""
    for head in (True, False):
        for kind in (None, "random", "known", "index"):
            filt, ref_kind = the_filter(filts, true, head, kind, N)
            ref = refs[head, ref_kind]
            ix = "_index" if kind == "index" else ""
            for eps in EPS:
                what = f"{mode} N={N} Q={Q} d={dim} b={biased} head={head} filt={kind} eps={eps}"
                zero_grads(nt, rt, bt)
                _native.profile_start()
                loss = loss_of(batch_t, head, nt, rt, bt, filt, mode=mode, reduction="none", label_smoothing=eps)
                assert loss.shape == (Q,) and loss.dtype == torch.float32
                close_loss(loss, ref, eps, what + " loss")
                loss.mean().backward()
                tags = set(_native.profile_stop())
                assert tags == {"lse_smooth" + ix + bf, "softmax_grad_smooth" + ix + bf, "gemm"}, tags
                check_grads(ref, eps, head, nt, rt, bt, what + " [none]")
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, filt, mode=mode, label_smoothing=EPS[0])
            close_loss(loss, ref, EPS[0], what + " mean loss", mean=True)
            loss.backward(gradient=functional.unit_gradient(loss.device))
            check_grads(ref, EPS[0], head, nt, rt, bt, what + " [mean]")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("only", ["nodes", "relations"])
def test_gradient_parity_with_frozen_inputs(only, mode):
    N, Q, dim = 257, 129, 50
    storage = storage_of(mode)
    nodes, rel, bias, batch, filts, refs, _ = case_and_refs(N, Q, dim, True, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage, grad=(only == "nodes", only == "relations", False))
    batch_t = dev(batch)
    for head in (True, False):
        zero_grads(nt, rt, bt)
        loss_of(batch_t, head, nt, rt, bt, filts[head, "random"], mode=mode, label_smoothing=0.1).backward()
        assert (nt.grad is not None) == (only == "nodes") and (rt.grad is not None) == (only == "relations")
        assert all(b.grad is None for b in bt)
        check_grads(refs[head, "random"], 0.1, head, nt, rt, bt, f"{mode} only {only} head={head}")


def test_a_bf16_table_that_does_not_train_runs_the_bf16_forward():
    from torch_rgcn import _native
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, refs, _ = case_and_refs(N, Q, dim, True, "bf16")
    nt, rt, bt = params_on_device(nodes, rel, bias, "bf16", grad=(False, False, False))
    for mode in ("upcast", "native"):
        _native.profile_start()
        loss = loss_of(dev(batch), True, nt, rt, bt, filts[True, "random"], mode=mode, reduction="none", label_smoothing=0.1)
        assert set(_native.profile_stop()) == {"lse_smooth_bf16"}
        close(loss, refs[True, "random"].loss[0.1], f"bf16 forward alone [{mode}]")
    nt.requires_grad_(True)                                                     # and one that trains, upcast: the fp32 smoothed route
    _native.profile_start()
    loss_of(dev(batch), True, nt, rt, bt, filts[True, "random"], mode="upcast", label_smoothing=0.1).backward()
    tags = set(_native.profile_stop())
    assert "lse_smooth" in tags and "softmax_grad_smooth" in tags and not any(t.endswith("_bf16") for t in tags), tags
    assert nt.grad.dtype == BF


# ----------------------------------------------------------------------------- 2. ssum and cnt are exact
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("N,Q,dim", SHAPES)
def test_the_sum_and_the_count_are_exact(N, Q, dim, biased, storage):
    """integer inputs (entries in [-2, 2], biases in [-1, 1]): every score is an integer and every partial sum of a row stays below 2^24
    (|s| <= 8 d + 3, and (8 * 500 + 3) * 77 and (8 * 50 + 3) * 700 are below 2^24), so fp32 adds them exactly in any order: ssum must
    EQUAL the float64 sum and cnt the count, for every number of strips -- with 64 most strips of these shapes have no tile.  One lost
    or doubled cell fails this where the parity bound would not see it."""
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, filts, refs, true = case_and_refs(N, Q, dim, biased, storage, True)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage, grad=(False, False, False))
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    for head in (True, False):
        for kind in (None, "random", "known", "index"):
            ref = refs[head, "known" if kind == "index" else kind]
            assert np.array_equal(ref.scores, np.round(ref.scores)) and np.abs(ref.scores).sum(1).max() < 2 ** 24
            fq, fn = lists_of(None if kind == "index" else filts[head, kind])
            for strips in STRIPS:
                lse, tscore, ssum, cnt = _native.distmult_lse_smooth(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn, strips=strips,
                                                                     filt=index if kind == "index" else None)
                assert ssum.dtype == torch.float32 and cnt.dtype == torch.int32 and ssum.shape == cnt.shape == (Q,)
                what = (storage, N, Q, dim, biased, head, kind, strips)
                assert np.array_equal(cnt.cpu().numpy(), ref.cnt), what
                assert np.array_equal(ssum.cpu().numpy().astype(np.float64), ref.ssum), what
                assert np.array_equal(tscore.cpu().numpy().astype(np.float64), ref.scores[np.arange(Q), batch[:, 0 if head else 2]]), what
                close(lse, ref.lse, f"integer lse {what}")


# ----------------------------------------------------------------------------- 3. the forward's bits are the unsmoothed route's
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,dim", [(130, 3, 8), (257, 129, 50), (77, 10, 500), (700, 130, 24)])
def test_lse_and_tscore_are_bitwise_the_unsmoothed_ones(N, Q, dim, storage):
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    nodes, rel, bias, batch, filts, _, true = case_and_refs(N, Q, dim, True, storage)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage, grad=(False, False, False))
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    for head in (True, False):
        for kind in (None, "random", "index"):
            fq, fn = lists_of(None if kind == "index" else filts[head, kind])
            kw = dict(filt_q=fq, filt_n=fn, filt=index if kind == "index" else None)
            for strips in STRIPS:
                want = _native.distmult_lse(batch_t, head, nt, rt, *bt, strips=strips, **kw)
                got = _native.distmult_lse_smooth(batch_t, head, nt, rt, *bt, strips=strips, **kw)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (storage, N, head, kind, strips)
                again = _native.distmult_lse_smooth(batch_t, head, nt, rt, *bt, strips=strips, **kw)
                assert all(torch.equal(a, b) for a, b in zip(got, again)), "one `strips`, one answer"


# ----------------------------------------------------------------------------- 4. eps = 0 changes nothing
def test_zero_smoothing_is_the_call_without_the_keyword():
    """reduction='none' and one chunk: no unordered sum takes part in the loss, the gradient cells or the two contractions, so the loss,
    the candidate-side bias gradient and every row of dnodes that index_add_ does not touch are bitwise equal.  The rows index_add_
    writes (the anchors' rows of dnodes, all of drel) are fp32 atomics: they may differ by what two runs of the call WITHOUT the keyword
    differ by, which is measured here from two such runs and not assumed: asserted at (130, 3, 8), where a row receives at most three
    terms, and printed at (700, 130, 24), where the order of 26 atomics per relation row need not repeat in a third run."""
    from torch_rgcn import _native
    for N, Q, dim in [(130, 3, 8), (700, 130, 24)]:
        nodes, rel, bias, batch, filts, _, _ = case_and_refs(N, Q, dim, True)
        nt, rt, bt = params_on_device(nodes, rel, bias)
        batch_t = dev(batch)
        for head in (True, False):
            def run(**kw):
                zero_grads(nt, rt, bt)
                _native.profile_start()
                loss = loss_of(batch_t, head, nt, rt, bt, filts[head, "random"], reduction="none", chunk_bytes=4 * Q * N, **kw)
                loss.mean().backward()
                tags = set(_native.profile_stop())
                return loss.detach().clone(), nt.grad.clone(), rt.grad.clone(), [b.grad.clone() for b in bt], tags
            a, b, z = run(), run(), run(label_smoothing=0.0)
            assert z[4] == a[4] == {"lse_fused", "softmax_grad", "gemm"}, z[4]     # the same calls
            assert torch.equal(z[0], a[0])
            assert all(torch.equal(x, y) for x, y in zip(z[3], a[3]))
            anchors = torch.zeros(N, dtype=torch.bool, device=DEV)
            anchors[batch_t[:, 2 if head else 0]] = True
            assert torch.equal(z[1][~anchors], a[1][~anchors])
            tol_n, tol_r = (a[1] - b[1]).abs().max().item(), (a[2] - b[2]).abs().max().item()
            print(f"[softmax_loss_smooth] eps=0 N={N} head={head}: two unsmoothed runs differ by {tol_n:.3e} (dnodes) {tol_r:.3e} (drel); "
                  f"eps=0 differs by {(z[1] - a[1]).abs().max().item():.3e} {(z[2] - a[2]).abs().max().item():.3e}")
            if N == 130:
                assert (z[1] - a[1]).abs().max().item() <= tol_n and (z[2] - a[2]).abs().max().item() <= tol_r


# ----------------------------------------------------------------------------- 5. strips and chunks, lists and index
def test_strips_and_chunks():
    from torch_rgcn import _native, functional
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 700, 130, 24
    nodes, rel, bias, batch, filts, refs, true = case_and_refs(N, Q, dim, True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    index = FilterIndex(true, N, DEV)
    budgets = {6: 1, 3: 4 * Q * 256, 1: functional.SOFTMAX_CHUNK_BYTES}
    for n_chunks, budget in budgets.items():
        assert len(functional.softmax_chunk_plan(Q, N, budget)) == n_chunks
    eps = 0.1
    for head in (True, False):
        ref = refs[head, "known"]
        for strips in STRIPS:
            close(loss_of(batch_t, head, nt, rt, bt, index, reduction="none", strips=strips, label_smoothing=eps), ref.loss[eps],
                  f"strips={strips} head={head} loss")
        losses, grads = [], []
        for n_chunks, budget in budgets.items():
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, index, reduction="none", chunk_bytes=budget, label_smoothing=eps)
            loss.mean().backward()
            check_grads(ref, eps, head, nt, rt, bt, f"chunks={n_chunks} head={head}")
            losses.append(loss.detach().clone())
            grads.append([nt.grad.cpu().numpy(), rt.grad.cpu().numpy()] + [b.grad.cpu().numpy() for b in bt])
        assert torch.equal(losses[0], losses[1]) and torch.equal(losses[0], losses[2])
        for other in grads[1:]:
            for k, (x, y) in enumerate(zip(grads[0], other)):
                close(x, y, f"chunk plans against each other head={head} [{k}]")        # (the query-side bias gradients: zeros both)
        # the list form and the index form: the same excluded cells, the same bits -- the loss and the gradient cells; every row of dS sums to 0
        listed = loss_of(batch_t, head, nt, rt, bt, filts[head, "known"], reduction="none", label_smoothing=eps)
        assert torch.equal(listed.detach(), losses[0])
        fq, fn = lists_of(filts[head, "known"])
        with torch.no_grad():
            lse, _, _, cnt = _native.distmult_lse_smooth(batch_t, head, nt, rt, *bt, filt=index)
            keep, uni = torch.full((1,), 1.0 - eps, device=DEV), eps / cnt.float()
            g = torch.full((), 3.0, device=DEV)
            for budget in budgets.values():
                rows = np.zeros(Q)
                for c_first, c_count in functional.softmax_chunk_plan(Q, N, budget):
                    want = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, fq, fn, lse, g, Q, c_first, c_count, keep=keep, uni=uni).clone()
                    got = _native.distmult_softmax_grad(batch_t, head, nt, rt, *bt, None, None, lse, g, Q, c_first, c_count, filt=index,
                                                        keep=keep, uni=uni)
                    assert torch.equal(got, want), (head, c_first)
                    cells = got.cpu().numpy().astype(np.float64)
                    assert (cells[ref.mask[:, c_first:c_first + c_count]] == 0.0).all()
                    rows += cells.sum(1)
                assert np.abs(rows).max() <= BOUND * 3.0 / Q, np.abs(rows).max()


# ----------------------------------------------------------------------------- 6. everything but the target filtered
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("biased", [False, True])
def test_everything_but_the_target_filtered_is_exactly_zero(biased, mode):
    """integer inputs, eps = 0.25: cnt == 1, lse == tscore == ssum bit for bit, s - 0.75 s - 0.25 s == 0 and exp(0) - 0.75 - 0.25 == 0:
    the loss and every gradient are exactly zero"""
    from torch_rgcn import _native
    N, Q, dim = 130, 3, 8
    storage = storage_of(mode)
    nodes, rel, bias, batch, _, _, _ = case_and_refs(N, Q, dim, biased, storage, True)
    nt, rt, bt = params_on_device(nodes, rel, bias, storage)
    batch_t = dev(batch)
    for head in (True, False):
        tgt = batch[:, 0 if head else 2]
        filt = np.array([(q, n) for q in range(Q) for n in range(N) if n != tgt[q]])
        fq, fn = lists_of(filt)
        with torch.no_grad():
            lse, tscore, ssum, cnt = _native.distmult_lse_smooth(batch_t, head, nt, rt, *bt, filt_q=fq, filt_n=fn)
        assert (cnt == 1).all() and torch.equal(lse, tscore) and torch.equal(ssum, tscore)
        zero_grads(nt, rt, bt)
        loss = loss_of(batch_t, head, nt, rt, bt, filt, mode=mode, reduction="none", label_smoothing=0.25)
        assert (loss.detach().cpu().numpy() == 0.0).all(), loss
        loss.mean().backward()
        for t in [nt, rt] + [b for b in bt if b is not None]:
            assert t.grad is not None and (t.grad.float().cpu().numpy() == 0.0).all()


# ----------------------------------------------------------------------------- 7. running max
@pytest.mark.parametrize("biased", [False, True])
def test_scores_beyond_the_range_of_exp(biased):
    """integer inputs at d = 500: |s| goes beyond 200 and, unbiased, the largest score of every query row exceeds 88.7 = log(FLT_MAX)"""
    N, Q, dim = 77, 10, 500
    nodes, rel, bias, batch, filts, _, _ = case_and_refs(N, Q, dim, biased, "fp32", True)
    nt, rt, bt = params_on_device(nodes, rel, bias)
    batch_t = dev(batch)
    for head in (True, False):
        for kind in (None, "random"):
            ref = Ref(nodes, rel, bias, batch, head, filts[head, kind])
            s = ref.scores
            assert np.array_equal(s, np.round(s)) and np.abs(s).max() > 88.7 and (biased or (s.max(1) > 88.7).all())
            for eps in EPS:
                zero_grads(nt, rt, bt)
                loss = loss_of(batch_t, head, nt, rt, bt, filts[head, kind], reduction="none", label_smoothing=eps)
                assert torch.isfinite(loss).all()
                close(loss, ref.loss[eps], f"integer b={biased} head={head} filt={kind} eps={eps} loss")
                loss.mean().backward()
                check_grads(ref, eps, head, nt, rt, bt, f"integer b={biased} head={head} filt={kind} eps={eps}")


# ----------------------------------------------------------------------------- 8. no host synchronisation
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


# ----------------------------------------------------------------------------- 9. guard bands
@pytest.mark.parametrize("kind", ["random", "index"])
@pytest.mark.parametrize("mode", ["fp32", "native"])
def test_under_guard_bands(mode, kind, monkeypatch):
    """one case per new kernel route (fp32 / bf16 strip pass and gradient cells, mask from the lists / from the index): every buffer
    between two poisoned bands, the library's torch.empty buffers full of NaN before the call"""
    from torch_rgcn.functional import FilterIndex
    N, Q, dim = 257, 129, 50
    storage = storage_of(mode)
    nodes, rel, bias, batch, filts, refs, true = case_and_refs(N, Q, dim, True, storage)
    index = FilterIndex(true, N, DEV) if kind == "index" else None
    got = {}
    with gb.Guard(monkeypatch) as guard:
        put = lambda a, dt=None: None if a is None else guard.home(dev(a, dt))  # noqa: E731
        nt, rt, bt = params_on_device(nodes, rel, bias, storage, put=put)
        batch_t = put(batch)
        assert torch.isnan(torch.empty(3, device=DEV)).all()
        for head in (True, False):
            zero_grads(nt, rt, bt)
            loss = loss_of(batch_t, head, nt, rt, bt, index if kind == "index" else filts[head, "random"], put=put, mode=mode,
                           reduction="none", chunk_bytes=4 * Q * 128, label_smoothing=0.1)
            loss.mean().backward()
            got[head] = (loss.detach().cpu().numpy(), nt.grad.float().cpu().numpy(), rt.grad.cpu().numpy(), [b.grad.cpu().numpy() for b in bt])
        problems = guard.problems(f"smoothed softmax loss {mode} {kind} N={N} Q={Q} d={dim}")
    assert not problems, "\n".join(problems)
    for head in (True, False):
        ref = refs[head, "known" if kind == "index" else "random"]
        loss, dn, dr, db = got[head]
        close(loss, ref.loss[0.1], f"guarded {mode} {kind} head={head} loss")
        close(dn, ref.dnodes[0.1], f"guarded {mode} {kind} head={head} dnodes", bound=BF_BOUND if storage == "bf16" else BOUND)
        close(dr, ref.drel[0.1], f"guarded {mode} {kind} head={head} drel")
        close(db[0 if head else 2], ref.dbias[0.1][0 if head else 2], f"guarded {mode} {kind} head={head} candidate bias")
        assert all(np.isfinite(x).all() for x in db)


# ----------------------------------------------------------------------------- the layer, errors
def test_distmult_layer_passes_the_keyword_on():
    from torch_rgcn.layers import DistMult
    N, Q, dim = 257, 129, 50
    nodes, rel, bias, batch, filts, refs, _ = case_and_refs(N, Q, dim, True)
    dm = DistMult(R0, dim, N, R0, b_init="ones").to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        for n, b in zip(("sbias", "pbias", "obias"), bias):
            getattr(dm, n).copy_(torch.from_numpy(b))
    nt = dev(nodes).requires_grad_(True)
    fq, fn = lists_of(filts[True, "random"])
    ref = refs[True, "random"]
    loss = dm.softmax_loss(torch.from_numpy(batch), nt, head=True, filt_q=fq, filt_n=fn, reduction="none", label_smoothing=0.25)
    close(loss, ref.loss[0.25], "layer loss")
    err, norm = rel_err(ref.loss[0.25], ref.loss[0.1])
    assert err > 10 * BOUND * norm                                             # the keyword is not merely accepted
    loss.mean().backward()
    close(nt.grad, ref.dnodes[0.25], "layer dnodes")
    close(dm.relations.grad, ref.drel[0.25], "layer drel")
    close(dm.sbias.grad, ref.dbias[0.25][0], "layer dsbias")


def test_the_entry_points_refuse_null_outputs_and_inputs():
    from torch_rgcn import _native
    nodes, rel = torch.randn(10, 8, device=DEV), torch.randn(3, 8, device=DEV)
    ok = torch.tensor([[0, 1, 2], [3, 2, 4]], device=DEV)
    L, st = _native.lib(), _native._stream(nodes.device)
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    lse, g = torch.zeros(2, device=DEV), torch.ones(1, device=DEV)
    ts, ss, cn = torch.zeros(2, device=DEV), torch.zeros(2, device=DEV), torch.zeros(2, device=DEV, dtype=torch.int32)
    keep, uni = torch.full((1,), 0.9, device=DEV), torch.full((2,), 0.01, device=DEV)
    dS = torch.full((2, 10), -7.0, device=DEV)
    ws = torch.empty(_native.lse_smooth_workspace_bytes(2, 10, 8) + 1024, device=DEV, dtype=torch.uint8)

    def fwd(ssum=p(ss), cnt=p(cn), w=p(ws)):
        return L.rgcn_distmult_lse_smooth_f32(p(ok), 2, 1, p(nodes), p(rel), None, None, None, None, None, 0, None, None, None, 0, 0, w, p(lse), p(ts),
                                              ssum, cnt, 10, 3, 8, st)

    def grad(k=p(keep), u=p(uni), c_first=0):
        return L.rgcn_distmult_softmax_grad_smooth_f32(p(ok), 2, 1, p(nodes), p(rel), None, None, None, None, None, 0, None, None, None, 0, p(lse), p(g),
                                                       k, u, 0, 2, c_first, 10, p(ws), p(dS), 10, 3, 8, st)
    assert fwd(ssum=None) == _native.EINVAL and fwd(cnt=None) == _native.EINVAL and fwd(w=p(ws) + 4) == _native.EINVAL
    assert grad(k=None) == _native.EINVAL and grad(u=None) == _native.EINVAL and grad(c_first=64) == _native.EINVAL
    assert b"distmult_softmax_grad_smooth" in L.rgcn_last_error()
    torch.cuda.synchronize()
    assert (dS == -7.0).all()                                                  # nothing was launched
    assert fwd() == _native.OK and grad() == _native.OK
    torch.cuda.synchronize()
    assert torch.isfinite(dS).all() and (cn == 10).all()
    out = _native.distmult_lse_smooth(ok[:0], True, nodes, rel)                # Q = 0: empty outputs
    assert all(t.shape == (0,) for t in out)
