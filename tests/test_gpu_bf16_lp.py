"""bf16 link prediction: the DistMult decoder and the ranking evaluator on a bf16 entity table.

Contract under test: nodes bf16; relations and biases fp32 or bf16 (widened once per call); scores fp32, [T] and [Q, N]; dnodes bf16 -- an
fp32 sum per entity rounded once --; drel and the bias gradients fp32 sums in the parameter's dtype.  The evaluator runs on
v_mfma_f32_16x16x32_bf16 with the fp32 query vector carried as three bf16 terms, so it adds what the fp32 evaluator adds on the widened
table: the float64 oracle on the widened nodes is the reference under the project's fp32 bound (1e-4 of the largest score), and on inputs
whose every partial sum is exact the scores EQUAL it.

Bounds.  TOL = 1e-4: the fp32-arithmetic bound of tests/test_gpu_eval.py.  2^-8: one rounding to bf16 (8 significand bits, half an ulp
is 2^-9 of the element, bounded by 2^-8 of the largest under the max-norm), the bound of tests/test_gpu_bf16.py."""
import contextlib

import numpy as np
import pytest
import torch

import exact_inputs as ex
from conftest import load_golden
from oracle import oracle
from torch_rgcn import routes

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
TOL = 1e-4
BF_TOL = 2.0 ** -8


def bf16_round(a):
    """numpy fp32 -> the nearest bf16 (ties to even), as fp32"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(BF).float().numpy()


def dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def rel_err(got, ref):
    got = got.detach().float().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-30))


def expand(batch, N, head):
    """the [Q, N, 3] candidate tensor of the reference (utils/misc.py:78-83)"""
    toscore = np.repeat(batch[:, None, :], N, axis=1)
    toscore[:, :, 0 if head else 2] = np.arange(N)[None, :]
    return toscore


# ----------------------------------------------------------------------------- 1. score-all against float64
SCORE_SHAPES = [(1, 1, 1, False, False), (63, 65, 6, True, False), (130, 3, 8, False, False), (257, 129, 50, False, True),
                (64, 64, 16, True, False), (100, 40, 32, False, False), (100, 40, 33, True, True), (77, 10, 500, False, False),
                (1000, 200, 200, True, False)]


@pytest.mark.parametrize("N,Q,dim,biased,rel_bf16", SCORE_SHAPES)
def test_score_all_bf16_vs_oracle(N, Q, dim, biased, rel_bf16):
    """one tile / several tiles of queries and of candidates, K below, at and past a step of 32, d % 8 == 0 (16-byte loads) and not"""
    from torch_rgcn import _native
    from torch_rgcn import functional as F_
    rng = np.random.default_rng(N + Q + dim)
    R0 = 5
    nodes = bf16_round(rng.standard_normal((N, dim)))
    rel = rng.standard_normal((R0, dim)).astype(np.float32)
    bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    if rel_bf16:                         # bf16 parameters: what the kernel sees is their widened value
        rel, bias = bf16_round(rel), [None if b is None else bf16_round(b) for b in bias]
    pdt = BF if rel_bf16 else torch.float32
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    for head in (True, False):
        want = oracle.distmult_forward(expand(batch, N, head), nodes, rel, *bias)
        _native.profile_start()
        got_t = F_.distmult_score_all(dev(batch), head, dev(nodes, BF), dev(rel, pdt), *[dev(b, pdt) for b in bias])
        tags = set(_native.profile_stop())
        assert tags == {"distmult_score_all_bf16"}, tags
        assert got_t.dtype == torch.float32 and got_t.shape == (Q, N)
        got = got_t.cpu().numpy()
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-30)
        print(f"[bf16 score_all] N={N} Q={Q} d={dim} head={head}: rel-max error {err:.2e}")
        assert err < TOL, head
        # filter + count against a numpy restatement on the SAME score matrix (exact)
        filt = np.unique(np.stack([rng.integers(0, Q, 3 * Q), rng.integers(0, N, 3 * Q)], 1), axis=0)
        target = batch[:, 0 if head else 2]
        filt = filt[filt[:, 1] != target[filt[:, 0]]]
        if len(filt):
            _native.rank_filter(got_t, dev(filt[:, 0].astype(np.int32)), dev(filt[:, 1].astype(np.int32)))
        ref = got.copy()
        ref[filt[:, 0], filt[:, 1]] = -np.inf
        assert np.array_equal(got_t.cpu().numpy(), ref)
        g, t = _native.rank_count(got_t, dev(batch), head)
        true = ref[np.arange(Q), target][:, None]
        assert np.array_equal(g.cpu().numpy(), (ref > true).sum(1)) and np.array_equal(t.cpu().numpy(), (ref == true).sum(1))


# ----------------------------------------------------------------------------- 2. score-all, exact
def test_score_all_bf16_exact_needs_all_three_terms():
    """Nodes in {-1, 0, 1}, relation entries in {+-1, +-c}, c = 1 + 2^-9 + 2^-17: the query element c splits into hi = 1, mid = 2^-9,
    lo = 2^-17, every product and every partial sum is a multiple of 2^-17 below 2^5 (22 bits, in any order), so every score EQUALS the
    float64 product.  Checked on the CPU (asserted below for the hi/mid/lo sums; the count with a term dropped was measured once on these
    very inputs): without lo, or without mid and lo, 82 % of the scores change."""
    from torch_rgcn import _native
    N, R0, Q, d = 300, 5, 70, 24
    c = 1 + 2.0 ** -9 + 2.0 ** -17
    rng = np.random.default_rng(24)
    nodes = rng.integers(-1, 2, (N, d)).astype(np.float32)
    rel = (rng.choice([1.0, c], (R0, d)) * rng.choice([-1.0, 1.0], (R0, d))).astype(np.float32)
    assert float(np.float32(c)) == c and np.array_equal(bf16_round(nodes), nodes)
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    for head in (True, False):
        q = nodes[batch[:, 2 if head else 0]] * rel[batch[:, 1]]
        hi = bf16_round(q); mid = bf16_round(q - hi); lo = bf16_round(q - hi - mid)
        assert np.array_equal(hi.astype(np.float64) + mid + lo, q.astype(np.float64)) and (lo != 0).mean() > 0.2
        want = q.astype(np.float64) @ nodes.astype(np.float64).T
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want) and np.abs(want).max() < 32
        assert np.array_equal(want * 2 ** 17, np.rint(want * 2 ** 17))
        assert ((hi.astype(np.float64) + mid) @ nodes.astype(np.float64).T != want).mean() > 0.5     # a lost term does not pass
        assert np.array_equal(oracle.distmult_forward(expand(batch, N, head), nodes, rel).astype(np.float64), want)
        got = _native.distmult_score_all_bf16(dev(batch), head, dev(nodes, BF), dev(rel))
        ex.assert_equal_exact(got, want.astype(np.float32), f"scores head={head}")


def test_query_terms_sum_to_the_fp32_product_bit_for_bit():
    """general bf16 nodes and fp32 relations (the products are NOT exact): the three bf16 terms the query kernel leaves in its scratch sum,
    in float64, to float32(nodes[fixed] * rel[p]) in every element -- the number the fp32 evaluator multiplies with, not the unrounded
    product a fused multiply-subtract would split.  One element lies above the largest bf16 (hi is clamped, not inf).  Then d = 1 against a
    candidate row 1.0: the score IS that product."""
    from torch_rgcn import _native
    N, R0, Q, d = 40, 5, 64, 50
    rng = np.random.default_rng(7)
    nodes = bf16_round(rng.standard_normal((N, d)) * np.exp2(rng.integers(-20, 20, (N, d))))
    rel = (rng.standard_normal((R0, d)) * np.exp2(rng.integers(-20, 20, (R0, d)))).astype(np.float32)
    nodes[3, 0], rel[1, 0] = np.float32(2.0 ** 128 - 2.0 ** 120), np.float32(1.003)      # the largest bf16; the product is finite and above it
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    batch[:, [0, 2]] = np.where(batch[:, [0, 2]] == 3, 4, batch[:, [0, 2]])              # entity 3 is the fixed end of query 0 only
    batch[0] = (3, 1, 3)
    assert np.isfinite(nodes[3, 0] * rel[1, 0]) and np.isinf(bf16_round(nodes[3, 0] * rel[1, 0])) and bf16_round(nodes[3, 0]) == nodes[3, 0]
    nb, tb, rl = dev(nodes, BF), dev(batch), dev(rel)
    dpad = (d + 31) // 32 * 32
    nbytes = int(_native.lib().rgcn_distmult_score_all_bf16_workspace_bytes(Q, d))
    assert nbytes == 3 * Q * dpad * 2
    for head in (True, False):
        qsplit = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
        scores = torch.empty(Q, N, device=DEV)
        _native._check(_native.lib().rgcn_distmult_score_all_bf16(tb.data_ptr(), Q, 1 if head else 0, nb.data_ptr(), rl.data_ptr(), None, None, None,
                                                                 qsplit.data_ptr(), None, scores.data_ptr(), N, R0, d,
                                                                 _native._stream(nb.device)), "score_all_bf16")
        terms = qsplit.view(BF).view(3, Q, dpad).float().cpu().numpy().astype(np.float64)
        want = nodes[batch[:, 2 if head else 0]] * rel[batch[:, 1]]                       # numpy float32: the correctly rounded product
        assert want.dtype == np.float32 and np.isfinite(want).all() and np.isfinite(terms).all()
        assert not np.array_equal(want.astype(np.float64), nodes[batch[:, 2 if head else 0]].astype(np.float64) * rel[batch[:, 1]])
        assert np.array_equal(terms[:, :, d:], np.zeros((3, Q, dpad - d)))               # the K tail is zeroed
        assert np.array_equal(terms.sum(0)[:, :d], want.astype(np.float64)), f"hi + mid + lo != fl(x r), head={head}"
    # d = 1, candidate 0 is 1.0: scores[q, 0] == float32(nodes[fixed] * rel[p])
    n1 = bf16_round(rng.standard_normal((N, 1)))
    n1[0, 0] = 1.0
    r1 = rng.standard_normal((R0, 1)).astype(np.float32)
    for head in (True, False):
        got = _native.distmult_score_all_bf16(tb, head, dev(n1, BF), dev(r1)).cpu().numpy()
        want = (n1[batch[:, 2 if head else 0]] * r1[batch[:, 1]])[:, 0]
        assert np.array_equal(got[:, 0], want), head


# ----------------------------------------------------------------------------- 3. decoder against the reference's vectors
def _golden_decoder(d, tag, b_init, pdt):
    from torch_rgcn.layers import DistMult
    N, R0 = int(d["num_nodes"]), int(d["num_rels"])
    dm = DistMult(R0, d["nodes"].shape[1], N, R0, b_init=b_init).to(DEV)
    with torch.no_grad():
        for n, p in dm.named_parameters():
            p.copy_(torch.from_numpy(d[f"{tag}_param_{n}"]))
    return dm.to(pdt)


@pytest.mark.parametrize("pdt", [torch.float32, BF], ids=["params_fp32", "params_bf16"])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_g5_distmult_bf16(monkeypatch, bwd, pdt):
    """golden g5_distmult with the nodes rounded to bf16, the float64 oracle evaluated on the widened copy (and on the widened parameters
    where those are bf16); biased and unbiased, [T, 3] and [B, S, 3] triples"""
    from torch_rgcn import _native
    routes.patch(monkeypatch, "distmult_bwd", bwd)
    d = load_golden("g5_distmult")
    nodes32 = bf16_round(d["nodes"])
    for tag, b_init in (("nb", None), ("b", "normal")):
        dm = _golden_decoder(d, tag, b_init, pdt)
        par = {n: p.detach().float().cpu().numpy() for n, p in dm.named_parameters()}
        bias = [par.get(n) for n in ("sbias", "pbias", "obias")]
        for nm in ("2", "3"):
            tr, gs = d["triples" + nm], d[f"{tag}_g{nm}"]
            sc_ref = oracle.distmult_forward(tr, nodes32, par["relations"], *bias)
            dn, dr, dsb, dpb, dob = oracle.distmult_backward(tr, nodes32, par["relations"], gs, b_init is not None)
            nodes = dev(nodes32, BF).requires_grad_(True)
            dm.zero_grad(set_to_none=True)
            _native.profile_start()
            sc = dm(dev(tr), nodes)
            sc.backward(dev(gs))
            tags = set(_native.profile_stop())
            assert sc.dtype == torch.float32 and sc.shape == tr.shape[:-1] and rel_err(sc, sc_ref) < TOL
            assert nodes.grad.dtype == BF and rel_err(nodes.grad, dn) <= BF_TOL
            grads = {"relations": dr, "sbias": dsb, "pbias": dpb, "obias": dob}
            for n, p in dm.named_parameters():
                assert p.grad.dtype == pdt
                # an fp32 sum; a bf16 parameter receives it rounded once
                assert rel_err(p.grad, grads[n]) < (TOL if pdt == torch.float32 else BF_TOL), n
            bwd_tags = {t for t in tags if t.startswith("distmult_bwd")}
            R0, width = par["relations"].shape
            want = {"atomic": {"distmult_bwd"}, "split": {"distmult_bwd_rel_bf16", "distmult_bwd_nodes_bf16"},
                    "csr": {"distmult_bwd_all_bf16"} if _native.distmult_bwd_all_supported(R0, width) else
                    {"distmult_bwd_rel_bf16", "distmult_bwd_nodes_bf16"}}[bwd]
            assert "distmult_fwd_bf16" in tags and "distmult_fwd" not in tags and bwd_tags == want, (sorted(tags), sorted(want))


# ----------------------------------------------------------------------------- 4. decoder, exact
@pytest.mark.parametrize("frozen", [(), ("nodes",), ("relations",), ("biases",), ("nodes", "relations", "biases")],
                         ids=["all", "nodes_frozen", "relations_frozen", "biases_frozen", "all_frozen"])
@pytest.mark.parametrize("d", [50, 300])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_distmult_bf16_exact(monkeypatch, bwd, d, frozen):
    distmult_bf16_exact(monkeypatch, bwd, d, frozen, gmax=2)


@pytest.mark.parametrize("d", [50, 300])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_distmult_bf16_exact_sums_that_need_the_rounding(monkeypatch, bwd, d):
    """the same case with score gradients in [-16, 16]: the hub's sums pass 256, where bf16 no longer holds every integer -- a second
    rounding (a partial sum stored as bf16 and read back) would show"""
    distmult_bf16_exact(monkeypatch, bwd, d, (), gmax=16)


def distmult_bf16_exact(monkeypatch, bwd, d, frozen, gmax, guard=None):
    """the construction of test_gpu_exact.py's distmult_exact on bf16 nodes: integer embeddings in [-2, 2], repeated triples, a 700-triple hub
    that is subject and object.  Every sum is an integer inside the fp32 significand: scores, drel and the bias gradients EQUAL the oracle,
    dnodes EQUALS the oracle's sum rounded once to bf16.  d = 50: element loads; d = 300: quarter-row loads, two passes of 256 features.  Both relation tables fit the LDS, so csr is
    the one-walk kernel and split the predicate-sorted kernel plus the entity walk.  guard: a guard_bands.Guard, not yet entered -- parameters,
    embeddings, triples and the score gradient move into guarded allocations, forward and backward run under it, its findings are asserted"""
    from torch_rgcn import _native
    from torch_rgcn.layers import DistMult
    frozen = frozenset(frozen)
    with_bias = True
    routes.patch(monkeypatch, "distmult_bwd", bwd)
    N, R0, T = 300, 5, 4000
    rng = np.random.default_rng(d)
    tr = np.stack([rng.integers(0, N, T), rng.integers(0, R0, T), rng.integers(0, N, T)], 1).astype(np.int64)
    tr[:700, 0] = 17
    tr[700:1400, 2] = 17
    tr[1400:1500] = tr[0]                                       # repeated triples
    tr = tr[(tr[:, 0] != 3) & (tr[:, 2] != 3)]                  # entity 3 is never scored: its gradient row is written, as zeros
    nodes = ex.ints((N, d), -2, 2, 0.5, rng)
    rel = ex.ints((R0, d), -2, 2, 1.0, rng)
    sb, ob, pb = ex.ints((N,), -2, 2, 1.0, rng), ex.ints((N,), -2, 2, 1.0, rng), ex.ints((R0,), -2, 2, 1.0, rng)
    gs = ex.ints((len(tr),), -gmax, gmax, 0.7, rng)
    bias = (sb, pb, ob)
    # proof: every term an integer, the sums of absolute values inside the significand
    a_sc = oracle.distmult_forward(tr, np.abs(nodes), np.abs(rel), *(np.abs(b) for b in bias))
    a_gr = oracle.distmult_backward(tr, np.abs(nodes), np.abs(rel), np.abs(gs), with_bias)
    bits = {"scores": float(np.log2(max(a_sc.max(), 1)))} | {k: float(np.log2(max(a.max(), 1))) for k, a in
                                                             zip(("dnodes", "drel", "dsb", "dpb", "dob"), a_gr)}
    assert max(bits.values()) <= ex.MAX_BITS, bits
    sc_ref = oracle.distmult_forward(tr, nodes, rel, *bias)
    dn, dr, dsb, dpb, dob = oracle.distmult_backward(tr, nodes, rel, gs, with_bias)
    assert gmax == 2 or not np.array_equal(bf16_round(dn), dn), "sums that need the rounding"

    dm = DistMult(R0, d, N, R0, b_init="normal").to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        dm.sbias.copy_(torch.from_numpy(sb)); dm.obias.copy_(torch.from_numpy(ob)); dm.pbias.copy_(torch.from_numpy(pb))
    dm.relations.requires_grad_("relations" not in frozen)
    for b in (dm.sbias, dm.pbias, dm.obias):
        b.requires_grad_("biases" not in frozen)
    any_grad = frozen != {"nodes", "relations", "biases"}
    asked = []                                                  # ranks= of every call of the scoring kernel's wrapper
    inner = _native.distmult_fwd_bf16
    monkeypatch.setattr(_native, "distmult_fwd_bf16", lambda *a, ranks=False: (asked.append(ranks), inner(*a, ranks=ranks))[1])
    home = (lambda t: t) if guard is None else guard.home
    with contextlib.nullcontext() if guard is None else guard:
        if guard is not None:
            for p in dm.parameters():
                p.data = home(p.data)
        nd = home(dev(nodes, BF)).requires_grad_("nodes" not in frozen)
        _native.profile_start()
        sc = dm(home(dev(tr)), nd)
        if any_grad:
            sc.backward(home(dev(gs)))
        tags = set(_native.profile_stop())
        guard_problems = [] if guard is None else guard.problems()
    print(f"[exact] distmult bf16 {bwd} d={d} frozen {sorted(frozen)}: tags {sorted(tags)} | proof bits "
          + " ".join(f"{k} {v:.1f}" for k, v in bits.items()))
    assert asked == [any_grad and bwd != "atomic"], asked       # no CSR ranks counted when nothing needs a gradient
    assert not guard_problems, "\n".join(guard_problems)
    split = {"distmult_bwd_rel_bf16", "distmult_bwd_nodes_bf16"}
    want = {"atomic": {"distmult_bwd"}, "split": split,
            "csr": {"distmult_bwd_all_bf16"} if _native.distmult_bwd_all_supported(R0, d) else split}[bwd] if any_grad else set()
    assert "distmult_fwd_bf16" in tags and {t for t in tags if t.startswith("distmult_bwd")} == want, (sorted(tags), sorted(want))
    assert sc.dtype == torch.float32
    ex.assert_equal_exact(sc, sc_ref, "scores")
    if "nodes" in frozen:
        assert nd.grad is None
    else:
        assert nd.grad.dtype == BF and torch.equal(nd.grad.cpu(), torch.from_numpy(dn).to(BF)), "dnodes"
        assert float(nd.grad[3].float().abs().max()) == 0.0
    if "relations" in frozen:
        assert dm.relations.grad is None
    else:
        ex.assert_equal_exact(dm.relations.grad, dr, "drelations")
    if "biases" in frozen:
        assert dm.sbias.grad is None and dm.pbias.grad is None and dm.obias.grad is None
    else:
        ex.assert_equal_exact(dm.sbias.grad, dsb, "dsbias")
        ex.assert_equal_exact(dm.pbias.grad, dpb, "dpbias")
        ex.assert_equal_exact(dm.obias.grad, dob, "dobias")


@pytest.mark.parametrize("bwd", ["csr", "split"])
def test_distmult_bf16_step_issues_no_synchronisation(monkeypatch, bwd):
    """the launchers neither allocate on the device side nor synchronise (the LP step is replayed as a hipGraph by default): with the range
    checks deferred, forward + backward run under torch's sync debug mode"""
    from torch_rgcn.layers import DistMult
    routes.patch(monkeypatch, "distmult_bwd", bwd)
    routes.patch(monkeypatch, "deferred_checks", "1")
    N, R0, d, T = 500, 6, 40, 3000
    torch.manual_seed(1)
    dm = DistMult(R0, d, N, R0, b_init="normal").to(DEV)
    nodes = torch.randn(N, d, device=DEV).to(BF).requires_grad_(True)
    tr = torch.from_numpy(oracle.synthetic_triples(N, R0, T, 9)).to(DEV)
    g = torch.randn(T, device=DEV)

    def step():
        nodes.grad = None
        dm.zero_grad(set_to_none=True)
        dm(tr, nodes).backward(g)
    step()                                   # warm-up: allocator, pinned flag buffers
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    from torch_rgcn import _native
    _native.check_deferred_errors()
    assert nodes.grad.dtype == BF and bool(torch.isfinite(nodes.grad.float()).all())


@pytest.mark.parametrize("bwd", ["csr", "split"])
def test_distmult_bf16_step_captured_in_a_hipgraph_matches_eager(monkeypatch, bwd):
    """forward + backward of the bf16 decoder captured with torch.cuda.graph after a warm-up on a side stream, replayed after unrelated eager
    kernels: scores and gradients agree with the eager step (fp32 sums in arrival order: the fp32 bound; dnodes: one bf16 rounding).

    The eager reference step runs AFTER the replays: before the capture nothing touches these leaves but the side-stream warm-up (as in
    tests/test_gpu_syncfree.py).  A leaf's AccumulateGrad node remembers the stream that was current when it was made and lives as long as
    some autograd graph holds it, so an eager step on the default stream whose output is kept would hand the capture accumulators bound
    to the legacy default stream, which cannot be captured."""
    from torch_rgcn import _native
    from torch_rgcn.layers import DistMult
    routes.patch(monkeypatch, "distmult_bwd", bwd)
    routes.patch(monkeypatch, "deferred_checks", "1")
    N, R0, d, T = 500, 6, 40, 3000
    torch.manual_seed(2)
    dm = DistMult(R0, d, N, R0, b_init="normal").to(DEV)
    nodes = torch.randn(N, d, device=DEV).to(BF).requires_grad_(True)
    tr = torch.from_numpy(oracle.synthetic_triples(N, R0, T, 10)).to(DEV)
    gvec = torch.randn(T, device=DEV)
    tensors = [nodes] + list(dm.parameters())
    for t in tensors:
        t.grad = torch.zeros_like(t)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            dm(tr, nodes).backward(gvec)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc = dm(tr, nodes)
        sc.backward(gvec)
    replayed = []
    for _ in range(2):
        for t in tensors:
            t.grad.zero_()
        junk = (torch.arange(50_000, device=DEV) % 3).float() * torch.rand(50_000, device=DEV)
        g.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(junk).all()
        replayed.append([sc.detach().clone()] + [t.grad.clone() for t in tensors])
    del g, sc
    for t in tensors:
        t.grad = None
    sc_e = dm(tr, nodes)
    sc_e.backward(gvec)
    torch.cuda.synchronize()
    _native.check_deferred_errors()
    eager = [sc_e.detach()] + [t.grad for t in tensors]
    for got in replayed:
        assert torch.equal(got[0], eager[0])                                     # one wave per triple, a fixed order
        assert got[1].dtype == BF and rel_err(got[1], eager[1].float().cpu().numpy().astype(np.float64)) <= BF_TOL
        for x, y in zip(got[2:], eager[2:]):
            assert rel_err(x, y.cpu().numpy().astype(np.float64)) < TOL


# ----------------------------------------------------------------------------- 5. s_penalty
def test_s_penalty_counts_past_256_in_bf16():
    """N = 10, T = 4000: every entity is scored about 400 times on each side, and a bf16 histogram stops counting at 256"""
    from torch_rgcn.layers import DistMult
    N, R0, dim, T = 10, 7, 24, 4000
    g = torch.Generator().manual_seed(3)
    dm = DistMult(R0, dim, N, R0).to(DEV)
    nodes = torch.randn(N, dim, generator=g).to(DEV).to(BF).requires_grad_(True)
    tr = torch.stack([torch.randint(0, N, (T,), generator=g), torch.randint(0, R0, (T,), generator=g),
                      torch.randint(0, N, (T,), generator=g)], dim=1).to(DEV)
    assert int(torch.bincount(tr[:, 0], minlength=N).min()) > 256
    pen = dm.s_penalty(tr, nodes)
    assert pen.dtype == BF
    gn, gr = torch.autograd.grad(pen, [nodes, dm.relations])
    assert gn.dtype == BF and gr.dtype == torch.float32
    wide = nodes.detach().float().requires_grad_(True)
    s, p, o = tr[..., 0], tr[..., 1], tr[..., 2]
    ref = wide[s, :].pow(2).mean() + dm.relations[p, :].pow(2).mean() + wide[o, :].pow(2).mean()
    rn, rr = torch.autograd.grad(ref, [wide, dm.relations])
    print(f"[bf16 s_penalty] {pen.item():.6f} against {ref.item():.6f}")
    assert abs(pen.item() - ref.item()) <= BF_TOL * abs(ref.item())
    assert (gn.float() - rn).abs().max().item() <= BF_TOL * rn.abs().max().item()
    assert (gr - rr).abs().max().item() <= BF_TOL * rr.abs().max().item()


# ----------------------------------------------------------------------------- 6. whole model
def test_link_predictor_in_bf16():
    from torch_rgcn import _native
    from torch_rgcn.models import LinkPredictor
    from utils import misc
    N, R0, dim = 200, 4, 16
    torch.manual_seed(0)
    model = LinkPredictor(nnodes=N, nrel=R0, encoder_config={"node_embedding": dim, "hidden1_size": dim, "num_layers": 1,
                                                             "decomposition": {"type": "basis", "num_bases": 2},
                                                             "weight_init": "glorot-normal", "bias_init": "zeros"},
                          decoder_config={"weight_init": "standard-normal", "bias_init": "normal",
                                          "l2_penalty_type": "schlichtkrull-l2", "l2_penalty": 0.01}).to(DEV).bfloat16().eval()
    assert all(p.dtype == BF for p in model.parameters())
    graph = torch.from_numpy(oracle.synthetic_triples(N, R0, 1200, 4))
    batch = torch.from_numpy(oracle.synthetic_triples(N, R0, 300, 5)).to(DEV)
    scores, pen = model(graph, batch)
    x = model.encode(graph).detach()
    assert x.dtype == BF and scores.dtype == torch.float32 and scores.shape == (300,)
    dec = model.scoring_function
    want = oracle.distmult_forward(batch.cpu().numpy(), x.float().cpu().numpy(), dec.relations.detach().float().cpu().numpy(),
                                   *(b.detach().float().cpu().numpy() for b in (dec.sbias, dec.pbias, dec.obias)))
    assert rel_err(scores, want) < TOL
    labels = (torch.arange(300, device=DEV) % 2).float()
    loss = torch.nn.functional.binary_cross_entropy_with_logits(scores, labels) + 0.01 * pen.float()
    loss.backward()
    for n, p in model.named_parameters():
        assert p.grad is not None and p.grad.dtype == p.dtype and bool(torch.isfinite(p.grad.float()).all()), n

    calls, encode = [], model.encode
    model.encode = lambda g: (calls.append(1), encode(g))[1]
    test = oracle.synthetic_triples(N, R0, 40, 6)
    true_triples = misc.generate_true_dict(np.concatenate([graph.numpy(), test]))
    _native.profile_start()
    mrr, hits, ranks = misc.evaluate(model, graph, torch.from_numpy(test), true_triples, N, batch_size=7, verbose=False)
    tags = set(_native.profile_stop())
    assert len(calls) == 1 and "distmult_score_all_bf16" in tags and "score_all" not in tags
    tb = torch.from_numpy(test).to(DEV)
    for hx, head in enumerate((True, False)):
        sc = _native.distmult_score_all_bf16(tb, head, x, dec.relations.detach().float(),
                                             *(b.detach().float() for b in (dec.sbias, dec.pbias, dec.obias)))
        misc.filter_scores(sc, tb, true_triples, head=head)
        true = sc.gather(1, tb[:, 0 if head else 2][:, None])
        assert ranks[40 * hx: 40 * (hx + 1)] == ((sc > true).sum(1) + ((sc == true).sum(1) - 1) // 2 + 1).tolist()
    assert 0 < mrr <= 1


# ----------------------------------------------------------------------------- 7. errors
def test_bf16_decoder_and_evaluator_argument_errors():
    from torch_rgcn import _native
    from torch_rgcn.layers import DistMult
    N, R0, dim = 10, 3, 8
    dm = DistMult(R0, dim, N, R0).to(DEV)
    nodes = torch.randn(N, dim, device=DEV).to(BF)
    rel = torch.randn(R0, dim, device=DEV)
    ok = torch.tensor([[0, 1, 2]], device=DEV)
    with pytest.raises(TypeError):
        dm(ok, nodes.to(torch.float16))                                                           # fp16 is no storage type
    with pytest.raises(TypeError):
        _native.distmult_score_all_bf16(ok, True, nodes.to(torch.float16), rel)
    with pytest.raises(TypeError):
        _native.distmult_score_all_bf16(ok, True, nodes, rel.to(BF))                              # the wrapper takes widened parameters
    with pytest.raises(RuntimeError):
        dm(ok, nodes.cpu())                                                                       # no CPU path
    with pytest.raises(RuntimeError):
        _native.distmult_score_all_bf16(ok.cpu(), True, nodes, rel)
    for bad in ([[0, 3, 2]], [[10, 1, 2]], [[0, 1, -1]]):                                         # relation / node out of range
        with pytest.raises(IndexError):
            dm(torch.tensor(bad, device=DEV), nodes)
        with pytest.raises(IndexError):
            _native.distmult_score_all_bf16(torch.tensor(bad, device=DEV), True, nodes, rel)
    with pytest.raises(AssertionError):
        _native.distmult_score_all_bf16(ok, True, nodes, rel, torch.zeros(N, device=DEV), None, None)   # biases: all or none
    with pytest.raises(AssertionError):
        _native.distmult_fwd_bf16(ok, nodes, rel, torch.zeros(N, device=DEV), None, None)
    sc = _native.distmult_score_all_bf16(ok[:0], True, nodes, rel)
    assert sc.shape == (0, N) and sc.dtype == torch.float32
    assert dm(ok[:0], nodes).shape == (0,)
