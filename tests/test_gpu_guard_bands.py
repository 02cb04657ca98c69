"""Guard bands on the GPU: no kernel writes or reads outside the buffers it was given (tests/guard_bands.py).

Every case runs an existing value check -- the exact funnels of test_gpu_exact.py / test_gpu_bf16_lp.py with guard=, or the comparison of
the named test for the direct _native calls -- with every buffer the library sizes itself between two bands of 0xFF bytes, its inputs
moved into such allocations too (Guard.home), and floating-point torch.empty interiors full of NaN.  Every case asserts

  1. guard.check() is empty: no band byte changed;
  2. no non-const pointer of a native call pointed outside the guarded allocations, but for ALLOW;
  3. at least one native call was made (the case prints `calls / guarded pointers / total pointers`);
  4. the value (and tag / count / split) assertions of the funnel, which a stray load of a band's NaN or a never-written NaN interior
     fails.

One case per kernel route, on the fixture with the most ragged edge that still selects it (N = 16, 3001 and 40 009 against the tile
heights, odd bf16 rows of 20, 60 and 1000 bytes, the smallest hubs that split); no capture, sync-debug, multi-process or multi-GPU
case (the patched constructors launch fill kernels and the check synchronises).

Not seen by the guard: buffers ATen allocates behind const pointers (autograd's gradient buffers, .contiguous() / .float() / torch.cat /
index_select results -- G, widened X and W, the unit lists of the CSR plans) and anything inside a captured graph; the last test prints
them per entry point.

First full run on an MI355X: 126 guarded cases, 1061 native calls, 7286 of 7465 pointers inside a guarded allocation (all 179 others
const), 4925 guarded allocations, no damaged band, no NaN in a result, ALLOW empty."""
import contextlib

import numpy as np
import pytest
import torch
from torch_rgcn import routes

import guard_bands as gb
import test_gpu_bf16_lp as lp16
import test_gpu_exact as tex
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
F32 = torch.float32

# (function, parameter, reason): non-const pointers that may point outside the guarded allocations.  Admissible only for a buffer that ATen
# allocated AND whose size this library does not compute; an entry that no case uses fails test_allow_list_has_no_unused_entry.
ALLOW = (
)
_USED = set()
_RAN = set()


def guard_of(monkeypatch):
    return gb.Guard(monkeypatch, allow=ALLOW)


def finish(guard, label, case_id):
    """conditions 1 - 3 of a direct-call case (the funnels do the same through Guard.problems)"""
    problems = guard.problems(label)
    _USED.update(guard.allow_used)
    _RAN.add(case_id)
    assert not problems, label + "\n" + "\n".join(problems)


# ----------------------------------------------------------------------------- the helper itself, on device memory it owns
def test_guarded_tensors_on_the_device_and_a_reported_overrun(monkeypatch):
    with gb.Guard(monkeypatch, native=False) as guard:
        for shape in ((0,), (1,), (5, 7)):
            for dtype in (BF, torch.int32, torch.uint8, F32):
                for t in (torch.empty(shape, dtype=dtype, device=DEV), torch.zeros(shape, dtype=dtype, device=DEV),
                          torch.full(shape, 3, dtype=dtype, device=DEV), torch.empty_like(torch.ones(shape, dtype=dtype, device=DEV))):
                    gb.assert_allocator_like(t, shape, dtype)
                    assert t.is_cuda
        assert bool(torch.empty((9, 3), dtype=BF, device=DEV).isnan().all()) and bool(torch.empty(5, device=DEV).isnan().all())
        assert bool((torch.zeros(7, device=DEV) == 0).all()) and bool((torch.full((7,), 2.5, device=DEV) == 2.5).all())
        pinned = torch.empty(1, dtype=torch.int32, pin_memory=True)
        assert pinned.is_pinned() and not pinned.is_cuda
        up = torch.from_numpy(np.arange(6, dtype=np.int32)).to(DEV)           # a host array on its way to the device: adopted
        assert guard.records[-1].kind == "upload" and guard.records[-1].start == up.data_ptr() and up.tolist() == [0, 1, 2, 3, 4, 5]
        gb.assert_allocator_like(up, (6,), torch.int32)
        assert up.to(torch.int64).tolist() == up.tolist() and guard.records[-1].start == up.data_ptr()        # on the device already: ATen's
        n = len(guard.records)
        h = guard.home(torch.arange(15, device=DEV, dtype=F32).view(3, 5).to(BF))
        gb.assert_allocator_like(h, (3, 5), BF)
        assert len(guard.records) == n + 1 and guard.check() == []
        h.view(-1)[-1] = 7.0                                               # the last element in range: nothing to report
        assert guard.check() == []
        rec = guard.records[-1]
        assert rec.start == h.data_ptr() and rec.nbytes == 30
        # one bf16 element past the end of the [3, 5] tensor, through as_strided on the arena (h's own storage ends where h ends): the
        # store lands in the helper's own upper band
        torch.as_strided(rec.arena.view(BF), (1,), (1,), rec.lo // 2 + 15).fill_(2.0)
        problems = guard.check()
        assert len(problems) == 1, problems
        assert "home (3, 5) bfloat16" in problems[0] and "test_gpu_guard_bands.py" in problems[0], problems[0]
        assert "upper band damaged" in problems[0] and "offset 0 past the tensor's end" in problems[0] and "00 40 ff" in problems[0], problems[0]
        torch.as_strided(rec.arena.view(BF), (1,), (1,), rec.lo // 2 - 1).fill_(2.0)
        problems = guard.check()
        assert len(problems) == 2 and any("lower band damaged" in p and "offset -2 from" in p for p in problems), problems


# ----------------------------------------------------------------------------- layers, through run_exact(guard=)
S0, S1 = {"sparse_path": "0"}, {"sparse_path": "1"}
TWO_PASS = tex.TWO_PASS_BWD
WIDE_TAGS = ("rel_rows", "segment_sum_wide", "rel_wgrad")
FB_TILE = dict(mode="basis", featureless=True, vmax=1)

LAYER_CASES = [
    # id, routes, fixture, d_in, d_out, run_exact keywords
    ("tile-plain-relu", S0, "plain", 16, 16, dict(relu=True, expect=("spmm", "bwd_fused"), forbid=("spmm_csr", "spmm_scatter", "spmm_blk"))),
    ("tile-hub12-vertical", S0, "hub12", 16, 16, dict(vertical=True, expect=("spmm", "wgrad", "colsum"), forbid=("bwd_fused",), split="plan")),
    ("tile-n3001", S0, "n3001", 16, 16, dict(relu=True, expect=("spmm",), forbid=("spmm_csr", "spmm_scatter"))),
    ("tile-n16", S0, "n16", 16, 16, dict(expect=("spmm",), forbid=("spmm_csr", "spmm_scatter"))),
    ("csr-hub10-relu", dict(S1, spmm_csr="1"), "hub10", 16, 16, dict(relu=True, expect=("spmm_csr",) + TWO_PASS, forbid=("spmm", "bwd_fused"), split="csr")),
    ("csr-n3001", dict(S1, spmm_csr="1"), "n3001", 16, 16, dict(vertical=True, expect=("spmm_csr",) + TWO_PASS, forbid=("spmm", "bwd_fused"))),
    ("csr-r59", dict(S1, spmm_csr="1"), "r59", 16, 16, dict(expect=("spmm_csr",) + TWO_PASS, forbid=("spmm", "bwd_fused"))),
    ("twopass-hub10-relu", dict(S1, spmm_csr="0"), "hub10", 16, 16, dict(relu=True, expect=("spmm_scatter",) + TWO_PASS, forbid=("spmm", "spmm_csr"), split="csr")),
    ("twopass-n16", dict(S1, spmm_csr="0"), "n16", 16, 16, dict(expect=("spmm_scatter",) + TWO_PASS, forbid=("spmm", "spmm_csr"))),
    ("bwd-split-relu", dict(S0, bwd="split"), "plain", 16, 16, dict(relu=True, expect=("spmm",), forbid=("bwd_fused",), seed=3)),
    ("bwd-deterministic", dict(S0, deterministic="1"), "plain", 16, 16, dict(expect=("spmm", "bwd_fused"), seed=3)),
    ("deterministic-hub12", dict(S0, deterministic="1"), "hub12", 16, 16, dict(expect=("spmm", "bwd_fused"))),
    ("softwin-owner-relu", S0, "big_r9", 16, 16, dict(relu=True, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",))),
    ("softwin-hub-pieces", S0, "big_r9hub", 16, 16, dict(vertical=True, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), split="win")),
    ("blk-bwd-relu", dict(S0, bwd_kernel="blk", bwd_own="0"), "big_r9", 16, 16, dict(relu=True, expect=("bwd_fused",), forbid=("wgrad",))),
    ("blk-bwd-hub", dict(S0, bwd_kernel="blk", bwd_own="0"), "big_r9hub", 16, 16, dict(expect=("bwd_fused",), forbid=("wgrad",), split="bwd_blk")),
    ("lean-bwd-relu", dict(S0, bwd_kernel="lean", bwd_own="0"), "big_r9", 16, 16, dict(relu=True, vertical=True, expect=("bwd_fused",), forbid=("wgrad",))),
    ("lean-bwd-hub", dict(S0, bwd_kernel="lean", bwd_own="0"), "big_r9hub", 16, 16, dict(expect=("spmm", "wgrad"), forbid=("bwd_fused",))),
    ("blk-fwd-sparse-relu", S1, "big_r70", 16, 16, dict(relu=True, expect=("spmm_blk",) + TWO_PASS, forbid=("spmm_scatter", "spmm_csr", "spmm"))),
    ("w10x11-plain", S0, "plain", 10, 11, dict(expect=("spmm", "bwd_fused"), seed=21)),
    ("w10x11-hub12", S0, "hub12", 10, 11, dict(vertical=True, expect=("spmm", "wgrad"), split="plan", seed=21)),
    ("w48x80-wide", {}, "wide", 48, 80, dict(vmax=1, expect=WIDE_TAGS, seed=128)),
    ("w48x80-widehub10", {}, "widehub10", 48, 80, dict(vmax=1, vertical=True, expect=WIDE_TAGS, split="csr", seed=128)),
    ("basis-wide", {}, "wide", 64, 64, dict(mode="basis", vmax=1, num_bases=3, expect=("basis_aggregate", "gemm"))),
    ("basis-widehub10", {}, "widehub10", 64, 64, dict(mode="basis", vmax=1, num_bases=3, vertical=True, expect=("basis_aggregate", "gemm"), split="csr")),
    ("block-24x3x4-relu", {"block_path": "2"}, "widehub10", 72, 96, dict(mode="block", num_blocks=24, relu=True, vmax=1, expect=("block_spmm", "block_wgrad"),
                                                                        forbid=("spmm", "rel_rows"), split="csr")),
    ("block-100x5x5", {"block_path": "2"}, "narrowhub10", 500, 500, dict(mode="block", num_blocks=100, vmax=1, expect=("block_spmm", "block_wgrad"),
                                                                         forbid=("spmm", "rel_rows"), split="csr")),
    ("block-100x5x5-plain-relu", {"block_path": "2"}, "narrow", 500, 500, dict(mode="block", num_blocks=100, relu=True, vmax=1,
                                                                               expect=("block_spmm", "block_wgrad"), forbid=("spmm", "rel_rows"))),
    ("block-lds-table-relu", {}, "big", 32, 32, dict(mode="block", num_blocks=8, relu=True, expect=("block_spmm", "block_wgrad"), forbid=("spmm",))),
    ("diag-30", {}, "widehub10", 30, 30, dict(mode="diag", expect=("diag_spmm", "diag_wgrad"), forbid=("spmm",), split="csr")),
    ("featureless-csr-d10", {"featureless_csr": "1"}, "hub10", None, 10, dict(featureless=True, expect=("featureless_csr_fwd", "featureless_csr_wgrad"),
                                                                              forbid=("featureless_fwd", "featureless_wgrad"), split="csr")),
    ("featureless-tile-d10", {"featureless_csr": "0"}, "hub12", None, 10, dict(featureless=True, expect=("featureless_fwd", "featureless_wgrad"),
                                                                               forbid=("featureless_csr_fwd", "featureless_csr_wgrad"), split="fwd_plan")),
    ("featureless-tile-n3001", {"featureless_csr": "0"}, "n3001", None, 10, dict(featureless=True, expect=("featureless_fwd", "featureless_wgrad"))),
    ("featureless-csr-n16", {"featureless_csr": "1"}, "n16", None, 10, dict(featureless=True, expect=("featureless_csr_fwd", "featureless_csr_wgrad"))),
    ("fbasis-src-4x10-hub10", {}, "hub10", None, 10, dict(FB_TILE, num_bases=4, expect=("fbasis_fwd", "fbasis_bwd"), split="fbasis")),
    ("fbasis-src-64x11", {}, "plain", None, 11, dict(FB_TILE, num_bases=64, expect=("fbasis_fwd", "fbasis_bwd"))),
] + [
    (f"fbasis-tile-{mode}-{fix}", {"fbasis_inplace_mb": "0", "fbasis_tile": mode}, fix, None, 10,
     dict(FB_TILE, num_bases=B, expect=("fbasis_tile_fwd", "fbasis_tile_bwd"), split="fbasis" if fix == "n3001" else None))
    for mode in ("ranges", "nodes") for fix, B in (("n3001", 40), ("n16", 5))
] + [
    (f"fbasis-tile16-{mode}-{fix}", {"fbasis_tile": mode}, fix, None, 10,
     dict(FB_TILE, num_bases=B, param_dtypes={"bases": BF}, expect=("fbasis_tile_fwd_bf16", "fbasis_tile_bwd_bf16"),
          forbid=("fbasis_tile_fwd", "fbasis_tile_bwd"), split="fbasis" if fix == "n3001" else None))
    for mode in ("ranges", "nodes", "nodes2") for fix, B in (("n3001", 40), ("n16", 5))
] + [
    # bf16 features: rows of 20 and 22 bytes, 60 (diagonal 30) and 1000 (500-wide blocks)
    ("bf16-wave-10x16-hub12-relu", {}, "hub12", 10, 16, dict(relu=True, dtype=BF, expect=tex.WAVE16, forbid=tex.FP32_TAGS + tex.NATIVE16, split="plan", seed=5)),
    ("bf16-wave-10x11-plain", {}, "plain", 10, 11, dict(dtype=BF, expect=tex.WAVE16, forbid=tex.FP32_TAGS + tex.NATIVE16, seed=21)),
    ("bf16-wave-16x16-plain", {}, "plain", 16, 16, dict(dtype=BF, expect=tex.WAVE16, forbid=tex.FP32_TAGS + tex.NATIVE16, seed=5)),
    ("bf16-wave-64x64-hub12", {}, "hub12", 64, 64, dict(dtype=BF, expect=tex.WAVE16, forbid=tex.FP32_TAGS + tex.NATIVE16, split="plan", seed=5)),
    ("bf16-wave-n3001-p16", {}, "n3001", 10, 16, dict(relu=True, dtype=BF, pdtype=BF, expect=tex.WAVE16, forbid=tex.FP32_TAGS + tex.NATIVE16, seed=5)),
    ("bf16-native-p32-relu", {}, "big_r9", 16, 16, dict(relu=True, dtype=BF, expect=tex.NATIVE16, forbid=tex.FP32_TAGS + tex.WAVE16, seed=6)),
    ("bf16-native-p16", {}, "big_r9", 16, 16, dict(vertical=True, dtype=BF, pdtype=BF, expect=tex.NATIVE16, forbid=tex.FP32_TAGS + tex.WAVE16, seed=6)),
    ("bf16-block-20x4x4-p16-relu", {}, "widehub10", 80, 80, dict(mode="block", num_blocks=20, relu=True, dtype=BF, pdtype=BF, vmax=1, expect=tex.BLOCK16,
                                                                 forbid=tex.FORBID16, split="csr")),
    ("bf16-block-100x5x5-p32-relu", {}, "narrowhub10", 500, 500, dict(mode="block", num_blocks=100, relu=True, dtype=BF, vmax=1, expect=tex.BLOCK16,
                                                                      forbid=tex.FORBID16, split="csr")),
    ("bf16-block-100x5x5-p16", {}, "narrow", 500, 500, dict(mode="block", num_blocks=100, dtype=BF, pdtype=BF, vmax=1, expect=tex.BLOCK16,
                                                            forbid=tex.FORBID16)),
    ("bf16-block-lds-table-relu", {}, "big", 32, 32, dict(mode="block", num_blocks=8, relu=True, dtype=BF, expect=tex.BLOCK16, forbid=tex.FORBID16)),
    ("bf16-diag-30-p16", {}, "widehub10", 30, 30, dict(mode="diag", dtype=BF, pdtype=BF, expect=tex.DIAG16, forbid=tex.FORBID16, split="csr")),
    ("bf16-diag-30-p32", {}, "wide", 30, 30, dict(mode="diag", dtype=BF, expect=tex.DIAG16, forbid=tex.FORBID16)),
]

LP_EXPECT = {"none-16": (("spmm", "bwd_fused"), tex.WAVE16),
             "none-20x128": (WIDE_TAGS, ("spmm",)),
             "block-80": (("block_spmm", "block_wgrad", "gemm"), ("spmm", "rel_rows")),
             "block-80-bf16": (tex.BLOCK16 + ("colsum_bf16", "gemm"), tex.FORBID16),
             "none-16-bf16": (tex.WAVE16, tex.FP32_TAGS)}


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_layer_routes_under_guard(monkeypatch, case):
    name, route, fix, d_in, d_out, kw = case
    guard = guard_of(monkeypatch)
    with routes.override(**route):
        _, layer = tex.run_exact(fix, d_in, d_out, guard=guard, **kw)
    assert guard.calls > 0 and not guard._active
    if name.startswith(("softwin-owner", "bf16-native")):
        from torch_rgcn import _native
        graph = layer._graph
        assert getattr(graph.win_plan("fwd"), "soft_windows", False)
        assert graph._plans.get(("win", "bwd_own", _native.bwd_own_rows(graph.num_nodes))) is not None, "the relation-owner backward did not run"
    _USED.update(guard.allow_used)
    _RAN.add("layer:" + name)


def test_bf16_soft_window_forward_hub_pieces_under_guard(monkeypatch):
    """test_gpu_exact.py::test_bf16_soft_window_forward_hub_pieces on the 40 009-node hub graph: rgcn_spmm_blk_bf16 on a plan with hub
    pieces (fp32 atomics into a scratch the wrapper sizes, rounded afterwards), called on the layer's own soft-window plan, forward only"""
    import exact_inputs as ex
    from torch_rgcn import _native
    fx = tex.fixture("big_r9hub")
    params, bias, X, _, ref, bits = tex.exact_case("big_r9hub", False, 16, 16, "none", False, False, False, 3, 2, 2, 0.5, 0)
    layer = tex.make_layer(fx, params, bias, 16, 16, "none", False, False, 3, 2, False)
    with routes.override(sparse_path="0"), guard_of(monkeypatch) as guard:
        for p in layer.parameters():
            p.data = guard.home(p.data)
        graph = layer._graph_on(torch.device(DEV))
        plan = graph.win_plan("fwd")
        assert plan is not None and getattr(plan, "soft_windows", False)
        n_split = _native._blk_units(plan)[2]
        Xd = tex._dev(X, BF)
        if graph.perm is not None:
            Xd = Xd.index_select(0, graph.inv)
        _native.profile_start()
        out = _native.spmm_blk_bf16(guard.home(Xd), layer.weights.detach(), layer.bias.detach(), plan)
        tags = set(_native.profile_stop())
        if graph.perm is not None:
            out = out.index_select(0, graph.perm)
        assert n_split > 0 and tags == {"spmm_blk_bf16"}, (n_split, sorted(tags))
        assert out.dtype == BF
        ex.assert_equal_exact(out, ref["out"], "out", fx["deg_s"])
        finish(guard, f"spmm_blk_bf16 on hub pieces (split {n_split})", "softwin16-hub")


@pytest.mark.parametrize("case", sorted(LP_EXPECT))
def test_lp_layer_under_guard(monkeypatch, case):
    """the per-call graph of the link-prediction layer on the 2^10 hub: dev_lp_expand, dev_edge_norm and the CSR builders under guard too"""
    mode, dims, *bf = case.split("-")
    d_in, d_out = (int(dims), int(dims)) if "x" not in dims else map(int, dims.split("x"))
    kw = dict(mode="block", num_blocks=20, vmax=1) if mode == "block" else {}
    expect, forbid = LP_EXPECT[case]
    guard = guard_of(monkeypatch)
    tex.run_exact("hub10", d_in, d_out, dtype=BF if bf else F32, lp=True, seed=9, expect=expect, forbid=forbid, guard=guard, **kw)
    assert guard.calls > 0
    _USED.update(guard.allow_used)
    _RAN.add("lp:" + case)


# ----------------------------------------------------------------------------- decoder, through the distmult funnels
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("d", [50, 52, 300])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_distmult_under_guard(monkeypatch, bwd, d, storage):
    guard = guard_of(monkeypatch)
    if storage == "fp32":
        tex.distmult_exact(monkeypatch, bwd, d, True, guard=guard)
    else:
        lp16.distmult_bf16_exact(monkeypatch, bwd, d, (), 2, guard=guard)
    assert guard.calls > 0
    _USED.update(guard.allow_used)
    _RAN.add(f"distmult:{bwd}-{d}-{storage}")


# ----------------------------------------------------------------------------- direct _native calls, inputs home()d
def _np_dev(guard, a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return guard.home(t if dtype is None else t.to(dtype))


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("N,Q,dim,biased", [(1, 1, 1, False), (63, 65, 6, True), (257, 129, 50, False), (77, 10, 500, False)])
def test_evaluator_under_guard(monkeypatch, N, Q, dim, biased, storage):
    """test_gpu_eval.py::test_score_all_vs_oracle / test_gpu_bf16_lp.py::test_score_all_bf16_vs_oracle, then rank_filter and rank_count on
    the guarded score matrix (the comparison of those tests: 1e-4 of the largest score, filter and counts exact)"""
    from torch_rgcn import _native
    rng = np.random.default_rng(N + Q + dim)
    R0 = 5
    nodes = rng.standard_normal((N, dim)).astype(np.float32)
    if storage == "bf16":
        nodes = lp16.bf16_round(nodes)
    rel = rng.standard_normal((R0, dim)).astype(np.float32)
    bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    batch = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    score_all = _native.distmult_score_all if storage == "fp32" else _native.distmult_score_all_bf16
    with guard_of(monkeypatch) as guard:
        dev = lambda a, dt=None: _np_dev(guard, a, dt)  # noqa: E731
        for head in (True, False):
            want = oracle.distmult_forward(lp16.expand(batch, N, head), nodes, rel, *bias)
            sc = score_all(dev(batch), head, dev(nodes, BF if storage == "bf16" else None), dev(rel), *[dev(b) for b in bias])
            got = sc.cpu().numpy()
            assert got.shape == (Q, N) and sc.dtype == F32
            assert np.abs(got - want).max() < 1e-4 * max(np.abs(want).max(), 1e-30), head
            filt = np.unique(np.stack([rng.integers(0, Q, 3 * Q), rng.integers(0, N, 3 * Q)], 1), axis=0)
            target = batch[:, 0 if head else 2]
            filt = filt[filt[:, 1] != target[filt[:, 0]]]
            if len(filt):
                _native.rank_filter(sc, dev(filt[:, 0].astype(np.int32)), dev(filt[:, 1].astype(np.int32)))
            ref = got.copy()
            ref[filt[:, 0], filt[:, 1]] = -np.inf
            assert np.array_equal(sc.cpu().numpy(), ref)
            g, t = _native.rank_count(sc, dev(batch), head)
            true = ref[np.arange(Q), target][:, None]
            assert np.array_equal(g.cpu().numpy(), (ref > true).sum(1)) and np.array_equal(t.cpu().numpy(), (ref == true).sum(1))
        finish(guard, f"evaluator {storage} N={N} Q={Q} d={dim}", f"eval:{storage}-{N}")


@pytest.mark.parametrize("M,N,K", [(7, 5, 3), (130, 127, 33), (257, 129, 4), (60, 212, 24), (68, 100, 52)])
@pytest.mark.parametrize("bm", ["128", "64", "0"])
def test_gemm_under_guard(monkeypatch, M, N, K, bm):
    """test_gpu_gemm.py::test_gemm_layouts_and_edges: all four layouts, plain and split-K 5 with bias (the scratch of
    rgcn_gemm_scratch_floats between bands), relative error under 2e-6 against float64"""
    from test_gpu_gemm import _rel
    from torch_rgcn import _native
    routes.patch(monkeypatch, "gemm_bm", bm)
    rng = np.random.default_rng(M * 31 + N * 7 + K)
    with guard_of(monkeypatch) as guard:
        for ta, tb in ((False, False), (False, True), (True, False), (True, True)):
            A = rng.standard_normal((K, M) if ta else (M, K)).astype(np.float32)
            B = rng.standard_normal((N, K) if tb else (K, N)).astype(np.float32)
            bias = rng.standard_normal(N).astype(np.float32)
            ref = (A.T if ta else A).astype(np.float64) @ (B.T if tb else B).astype(np.float64)
            At, Bt = _np_dev(guard, A), _np_dev(guard, B)
            assert _rel(_native.gemm(At, Bt, trans_a=ta, trans_b=tb).cpu().numpy(), ref) < 2e-6, (ta, tb)
            got = _native.gemm(At, Bt, bias=_np_dev(guard, bias), trans_a=ta, trans_b=tb, split_k=5)
            assert _rel(got.cpu().numpy(), ref + bias) < 2e-6, (ta, tb)
        finish(guard, f"gemm {M}x{N}x{K} bm={bm}", f"gemm:{M}-{bm}")


@pytest.mark.parametrize("N,R0,E,d_in,d_out,B", [(257, 2, 900, 130, 7, 1), (700, 3, 5000, 64, 72, 5)])
def test_basis_aggregate_and_gemm_under_guard(monkeypatch, N, R0, E, d_in, d_out, B):
    """test_gpu_gemm.py::test_basis_forward_aggregate_then_product, graph and CSR built under the guard"""
    from torch_rgcn import _native
    from torch_rgcn.graph import graph_from_nc_triples
    R = 2 * R0 + 1
    tp = oracle.add_inverse_and_self(oracle.synthetic_triples(N, R0, E, seed=N % 97), N, R0)
    gen = torch.Generator().manual_seed(N)
    with guard_of(monkeypatch) as guard:
        g = graph_from_nc_triples(tp, N, R, False, torch.device(DEV))
        X = guard.home(torch.randn(N, d_in, generator=gen).to(DEV))
        comps = guard.home(torch.randn(R, B, generator=gen).to(DEV))
        bases = guard.home((torch.randn(B, d_in, d_out, generator=gen) * 0.1).to(DEV))
        bias = guard.home(torch.randn(d_out, generator=gen).to(DEV))
        csr = g.csr("fwd")
        ag = _native.basis_aggregate(X, comps, csr, B, d_in, 1)
        rp = csr.rowptr[: N + 1].long()
        rows = torch.repeat_interleave(torch.arange(N, device=DEV), rp[1:] - rp[:-1])
        M = rows.numel()
        msg = (comps[csr.rel[:M].long()].double()[:, :, None] * (X[csr.src[:M].long()].double() * csr.val[:M, None].double())[:, None, :]).reshape(M, B * d_in)
        ag_ref = torch.zeros(N, B * d_in, device=DEV, dtype=torch.float64).index_add_(0, rows, msg)
        assert ((ag.double() - ag_ref).abs().max() / ag_ref.abs().max()).item() < 1e-5
        out = _native.gemm(ag, bases.view(B * d_in, d_out), bias=bias)
        ref = ag_ref @ bases.view(B * d_in, d_out).double() + bias.double()
        assert ((out.double() - ref).abs().max() / ref.abs().max()).item() < 1e-5
        finish(guard, f"basis aggregate + gemm N={N} B={B}", f"basis:{N}")


@pytest.mark.parametrize("N,C,n_lab,padded", [(300, 11, 300, False), (5, 64, 1, False), (1000, 3, 77, True)])
def test_ce_head_under_guard(monkeypatch, N, C, n_lab, padded):
    """test_gpu_parity.py::test_masked_cross_entropy_head_matches_torch and ..._on_padded_rows_and_unit_gradient: loss and gradient against
    nn.CrossEntropyLoss within 1e-5; padded: the logits are the first C columns of a zero-padded [N, 16] buffer, and so is the gradient"""
    from test_gpu_parity import rel_err
    from torch_rgcn.functional import MaskedCrossEntropy
    gen = torch.Generator().manual_seed(N + C)
    logits = (3 * torch.randn(N, C, generator=gen)).to(DEV)
    idx = torch.randperm(N, generator=gen)[:n_lab].to(DEV)
    labels = torch.randint(0, C, (n_lab,), generator=gen).to(DEV)
    b = logits.clone().requires_grad_(True)
    lb = torch.nn.CrossEntropyLoss()(b[idx, :], labels)
    (2.5 * lb).backward()
    with guard_of(monkeypatch) as guard:
        head = MaskedCrossEntropy(guard.home(idx), guard.home(labels), N)
        if padded:
            full = torch.zeros(N, 16, device=DEV)
            full[:, :C] = logits
            base = full.requires_grad_(True)
            a = base[:, :C]
        else:
            base = a = guard.home(logits).requires_grad_(True)
        la = head(a)
        (2.5 * la).backward()
        assert abs(la.item() - lb.item()) <= 1e-5 * max(abs(lb.item()), 1e-3)
        assert rel_err(base.grad[:, :C], b.grad.cpu().numpy()) < 1e-5
        if padded:
            assert float(base.grad[:, C:].abs().max()) == 0.0
        finish(guard, f"ce_head N={N} C={C} padded={padded}", f"ce:{N}")


@pytest.mark.parametrize("T", [1, 777])
def test_bce_head_under_guard(monkeypatch, T):
    """test_gpu_parity.py::test_bce_with_logits_head_matches_torch (T = 1 and a T that is no multiple of the kernel's block; the workspace
    of rgcn_bce_head_workspace_bytes is reallocated between bands): loss within 2e-6, gradient within 1e-6, twice through the workspace"""
    from torch_rgcn import _native
    gen = torch.Generator().manual_seed(T)
    x0 = (torch.randn(T, generator=gen) * 12.0).to(DEV)
    y0 = torch.rand(T, generator=gen).round().to(DEV)
    xr = x0.clone().requires_grad_(True)
    ref = torch.nn.functional.binary_cross_entropy_with_logits(xr, y0)
    gref, = torch.autograd.grad(ref, xr)
    with guard_of(monkeypatch) as guard:
        x, y = guard.home(x0), guard.home(y0)
        for _ in range(2):
            loss, ds = _native.bce_head(x, y)
            assert abs(loss.item() - ref.item()) <= 2e-6 * abs(ref.item()) + 1e-12
            assert (ds - gref).abs().max().item() <= 1e-6 * gref.abs().max().item() + 1e-12
        finish(guard, f"bce_head T={T}", f"bce:{T}")


@pytest.mark.parametrize("n,d", [(1, 1), (77, 11), (3001, 10), (1000, 500), (257, 63)])
def test_colsum_under_guard(monkeypatch, n, d):
    """column sums of small integers (exact in fp32 in any order: n * 2 < 2^24), fp32 and bf16 storage; the scratch of
    rgcn_colsum_scratch_floats between bands"""
    from torch_rgcn import _native
    import exact_inputs as ex
    G = ex.ints((n, d), -2, 2, 0.7, n + d)
    want = G.astype(np.float64).sum(0)
    with guard_of(monkeypatch) as guard:
        ex.assert_equal_exact(_native.colsum(_np_dev(guard, G)), want, "colsum")
        ex.assert_equal_exact(_native.colsum_bf16(_np_dev(guard, G, BF)), want, "colsum_bf16")
        finish(guard, f"colsum n={n} d={d}", f"colsum:{n}")


@pytest.mark.parametrize("N,R0,E", [(40, 2, 7), (700, 5, 9000)])
def test_lp_expand_and_edge_norm_under_guard(monkeypatch, N, R0, E):
    """test_gpu_build.py::test_device_lp_expand_and_norm_bit_exact"""
    from test_gpu_build import graph
    from torch_rgcn import _native as nat
    T = graph(N, R0, E, N + E)
    keep = np.random.default_rng(N).integers(0, 2, N).astype(np.uint8)
    R = 2 * R0 + 1
    with guard_of(monkeypatch) as guard:
        for k in (None, keep):
            s, p, o, alive, err = nat.dev_lp_expand(_np_dev(guard, T), N, R0, None if k is None else _np_dev(guard, k))
            assert int(err.item()) == 0
            tp, n_self = oracle.lp_augment(T, N, R0, k)
            live = alive.cpu().numpy().astype(bool)
            got = np.stack([s.cpu().numpy(), p.cpu().numpy(), o.cpu().numpy()], 1)[live]
            assert np.array_equal(got, tp)
            for vertical in (True, False):
                val = nat.dev_edge_norm(s, p, o, alive, N, R, vertical, E).cpu().numpy()
                assert np.array_equal(val[live], oracle.edge_norm(tp, N, R, vertical, E, n_self))
                assert np.all(val[~live] == 0)
        finish(guard, f"lp_expand + edge_norm N={N} E={E}", f"expand:{N}")


@pytest.mark.parametrize("N,R,M,tile", [(50, 5, 700, 16), (3000, 21, 50000, 128)])
def test_device_plan_under_guard(monkeypatch, N, R, M, tile):
    """test_gpu_build.py::test_device_plan_equals_host_plan, with want_pack"""
    from test_gpu_build import canon
    from torch_rgcn import _native as nat
    rng = np.random.default_rng(N + M)
    dst = rng.integers(0, N, M).astype(np.int32)
    dst[:M // 4] = 3
    src = rng.integers(0, N, M).astype(np.int32)
    rel = rng.integers(0, R, M).astype(np.int32)
    val = rng.random(M).astype(np.float32) + 0.1
    alive = np.ones(M, np.uint8)
    alive[rng.integers(0, M, M // 7)] = 0
    live = alive.astype(bool)
    hp = nat.build_plan_host(dst[live], src[live], rel[live], val[live], N, N, R, tile, 64, want_runs=True, want_pack=True)
    with guard_of(monkeypatch) as guard:
        t = lambda a: _np_dev(guard, a)  # noqa: E731
        dp = nat.build_plan_device(t(dst), t(src), t(rel), t(val), t(alive), N, N, R, tile, int(live.sum()), 64, want_runs=True, want_pack=True)
        assert (dp.m_pad, dp.n_chunks, dp.n_tiles, dp.n_units, dp.n_split) == (hp.m_pad, hp.n_chunks, hp.n_tiles, hp.n_units, hp.n_split)
        assert np.array_equal(dp.tile_ptr.cpu().numpy()[:hp.n_tiles + 1], hp.tile_ptr)
        assert np.array_equal(dp.chunk_rel.cpu().numpy()[:hp.n_chunks], hp.chunk_rel[:hp.n_chunks])
        assert np.array_equal(dp.run_ptr.cpu().numpy()[:hp.n_tiles * (R + 1)], hp.run_ptr[:hp.n_tiles * (R + 1)])
        assert np.array_equal(dp.units.cpu().numpy()[:hp.n_units], hp.units[:hp.n_units])
        assert dp.max_run_chunks == hp.max_run_chunks
        starts = hp.run_ptr.reshape(-1, R + 1)[:, :R].ravel()
        a = canon(dp.src.cpu().numpy(), dp.dst.cpu().numpy(), dp.val.cpu().numpy(), starts, hp.m_pad)
        b = canon(hp.src, hp.dst, hp.val, starts, hp.m_pad)
        real = b[2] != 0                  # pads copy "the last real source of the bucket", which depends on the free order: real slots only
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
        assert np.array_equal(a[0][real], b[0][real])
        pk = dp.pack.cpu().numpy()[:hp.m_pad]
        d = dp.dst.cpu().numpy()[:hp.m_pad]
        assert np.array_equal(pk[:, 0] & 0xFFFFFF, dp.src.cpu().numpy()[:hp.m_pad])
        assert np.array_equal((pk[:, 0].view(np.uint32) >> 24), np.where(d < 0, 255, d % tile).astype(np.uint32))
        assert np.array_equal(pk[:, 1].view(np.float32), dp.val.cpu().numpy()[:hp.m_pad])
        finish(guard, f"build_plan_device N={N} M={M} tile={tile}", f"plan:{N}")


@pytest.mark.parametrize("N,R,M,rows,own", [(37, 3, 11, 16, False), (500, 1, 3000, 977, False), (6400, 100, 10_000, 64, False),
                                            (900, 20, 30_000, 128, True)])
def test_softwin_plan_under_guard(monkeypatch, N, R, M, rows, own):
    """test_gpu_softwin_build.py: the plan built through rgcn_softwin_order / rgcn_softwin_fill (the rocPRIM temporary of
    rgcn_softwin_tmp_bytes and every max(n, 1)-sized array between bands) satisfies the invariants of test_softwin_plan.py and equals the
    torch-op builder's; own: the relation-owner plan of 12 waves x 9 relations"""
    from test_softwin_plan import check_owner_plan, check_plan, random_messages
    from torch_rgcn import _native
    dst, src, rel, val, alive = random_messages(N, R, M, False, 7 if own else N + M)
    with guard_of(monkeypatch) as guard:
        g = [t if t is None else guard.home(t.to(DEV)) for t in (dst, src, rel, val, alive)]
        if own:
            p = _native.build_softwin_plan(*g, N, N, R, rows, own_waves=12, own_per_wave=9)
            assert p.src.is_cuda and p.own_waves == 12
            check_owner_plan(p, dst, src, rel, val, alive, N, R, rows, 12, 9)
        else:
            p = _native.build_softwin_plan(*g, N, N, R, rows)
            assert p.src.is_cuda
            check_plan(p, dst, src, rel, val, alive, N, R, rows)
        problems = guard.problems(f"softwin plan N={N} R={R} M={M} rows={rows} own={own}")
    if not own:                                    # the torch-op builder, not under guard: the same plan
        with routes.override(softwin_build="torch"):
            q = _native.build_softwin_plan(*[t if t is None else t.to(DEV) for t in (dst, src, rel, val, alive)], N, N, R, rows)
        assert (q.m_pad, q.n_chunks, q.n_messages, q.max_run_chunks) == (p.m_pad, p.n_chunks, p.n_messages, p.max_run_chunks)
        assert torch.equal(q.tile_ptr.cpu(), p.tile_ptr.cpu()) and torch.equal(q.run_ptr.cpu(), p.run_ptr.cpu())
        assert torch.equal(q.chunk_rel.cpu(), p.chunk_rel.cpu())
        assert torch.equal(q.src.cpu()[:p.m_pad], p.src.cpu()[:p.m_pad])
    _USED.update(guard.allow_used)
    _RAN.add(f"softwin:{N}")
    assert not problems, "\n".join(problems)


# ----------------------------------------------------------------------------- the allow-list and the totals
N_CASES = len(LAYER_CASES) + len(LP_EXPECT) + 1 + 18 + 8 + 15 + 2 + 3 + 2 + 5 + 2 + 2 + 4


def test_allow_list_has_no_unused_entry():
    """runs last: every entry of ALLOW was needed by a case of this module (checked when the whole module ran), and the totals"""
    print(f"[guard] totals: {gb.TOTALS}")
    print("[guard] const pointers outside the guarded allocations (inputs ATen made; function.parameter: calls): "
          + ", ".join(f"{fn}.{par}: {n}" for (fn, par), n in sorted(gb.UNSEEN_INPUTS.items())))
    assert all(len(e) == 3 and e[2] for e in ALLOW)
    if len(_RAN) < N_CASES:
        print(f"[guard] {len(_RAN)} of {N_CASES} cases ran in this session: the allow-list is checked by a run of the whole module")
        return
    unused = [e for e in ALLOW if (e[0], e[1]) not in _USED]
    assert not unused, f"allow-list entries that no case needed: {unused}"
