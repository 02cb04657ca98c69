"""Exact-arithmetic parity: every element of out, dX, db and every parameter gradient EQUAL to the float64 oracle, no tolerance.

The max-norm metric of tests/test_gpu_parity.py (1e-4 of the largest element) is set by the degree-1 rows; the rows where kernels go wrong
-- hub rows: cut into pieces, merged with atomics, split over lane groups, rounded by a second launch -- carry numbers 1 / degree as large,
and a kernel that loses a few of a hub's messages passes it (tests/test_exact_inputs.py records the figures).  Here the graphs have
power-of-two normalisation constants and every other input is a small integer (tests/exact_inputs.py): all partial sums are exact in fp32
in any order, so a correct kernel and the oracle agree bit for bit in value, and one lost, duplicated or misrouted message does not.

Every case: the route is forced as the test of that route in test_gpu_parity.py / test_gpu_bf16*.py forces it; assert_provably_exact runs
on the CPU before the first launch; the profile tags of the kernels that must have run are asserted, and the route's own split indicator
for the hub family (plan.n_split, _csr_units(csr)[2], _blk_units(plan)[2]); each case prints tags, indicator and proof bound in bits.

Fixture families.  plain: N = 2000, groups of 1 .. 16, values in {-2 .. 2}.  hub: N = 2048, relation 0 holds a 2^h hub (and three smaller
ones); h is the smallest size at which the route's indicator is positive -- 2^12 for the 16-message chunks of the tile plans (a unit holds
256 chunks), 2^10 for the 512-entry pieces of the CSR units, 2^15 for the tall tiles of the block-tile kernels -- and the default tile plan
also runs the 2^15 hub.  Wide layers use N = 1000 (500-wide: N = 300) and values in {-1, 0, 1}.  big: 66 000 nodes, the size class of the soft-window /
relation-owner / block-tile kernels.

EXCEPTED (case, tensor) pairs -- a gradient that sums over all relations in a hub case, compared under the 1e-4 max-norm because no hub size
that still splits passes the proof bound: none."""
import contextlib
import functools

import numpy as np
import pytest
import torch
from torch_rgcn import routes

import exact_inputs as ex
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
EXCEPTED = ()          # (case id, tensor name, printed bound)

FIX = {
    # name: (N, R0, groups per relation, hub_log2, seed)
    "plain": (2000, 3, 1000, None, 101),
    "hub10": (2048, 3, 1200, 10, 102),
    "hub12": (2048, 3, 1200, 12, 103),
    "hub15": (2048, 3, 1200, 15, 104),
    "r1": (2000, 1, 1500, None, 105),
    "r1hub": (2000, 1, 1500, 10, 115),
    "r59": (3000, 59, 40, None, 106),
    "wide": (1000, 3, 400, None, 107),
    "widehub10": (1000, 3, 400, 10, 108),
    "narrow": (300, 3, 40, None, 118),            # 500-wide layers: the oracle's dense 500 x 500 product per message sets the test's time
    "narrowhub10": (300, 3, 40, 10, 119),
    "n3001": (3001, 6, 900, 10, 110),
    "n16": (16, 6, 6, None, 111),
    "big": (66_000, 5, 30_000, None, 112),
    "bighub": (66_000, 5, 30_000, 15, 113),
    "big_r70": (40_000, 70, 600, None, 114),
    "big_r9": (40_009, 9, 5000, None, 116),
    "big_r9hub": (40_009, 9, 5000, 15, 117),
}


@functools.lru_cache(maxsize=None)
def fixture(name):
    N, R0, groups, hub, seed = FIX[name]
    T = ex.pow2_triples(N, R0, groups, hub_log2=hub, seed=seed, max_log2=2 if name == "n16" else 4)
    tp = oracle.add_inverse_and_self(T, N, R0)
    R = 2 * R0 + 1
    return dict(name=name, N=N, R0=R0, R=R, tp=tp, val={v: oracle.nc_edge_norm(tp, N, R, v) for v in (False, True)},
                deg_s=np.bincount(tp[:, 0], minlength=N), deg_o=np.bincount(tp[:, 2], minlength=N))


@functools.lru_cache(maxsize=None)
def lp_fixture(name):
    """the LP layer's message list on the base triples of fixture `name` (oracle.lp_augment, every self loop kept: eval mode) and its
    normalisation constants -- powers of two under the LP count formula too (tests/test_exact_inputs.py; asserted again by the proof)"""
    N, R0, groups, hub, seed = FIX[name]
    T = ex.pow2_triples(N, R0, groups, hub_log2=hub, seed=seed)
    tp, n_self = oracle.lp_augment(T, N, R0, None)
    R = 2 * R0 + 1
    return dict(name="lp:" + name, N=N, R0=R0, R=R, T=T, tp=tp, val={False: oracle.edge_norm(tp, N, R, False, len(T), n_self)},
                deg_s=np.bincount(tp[:, 0], minlength=N), deg_o=np.bincount(tp[:, 2], minlength=N))


def _param_shapes(R, N, d_in, d_out, mode, featureless, num_bases, num_blocks, lp):
    """the parameters of the layer, by name, in the order their values are drawn (make_layer copies them into the module and checks the
    names; a shape that differs from the module's raises there)"""
    rows = N if featureless else d_in
    if mode == "diag":
        return {"weights": (R, d_in)}                                       # (diagonal layers have no bias)
    if mode == "none":
        shapes = {"weights": (R, rows, d_out)}
    elif mode == "basis":
        shapes = {"bases": (num_bases, rows, d_out), "comps": (R, num_bases)}
    else:
        shapes = {"blocks": (R - 1 if lp else R, num_blocks, d_in // num_blocks, d_out // num_blocks)}
        if lp:
            shapes["blocks_self"] = (d_in, d_out)
    shapes["bias"] = (d_out,)
    return shapes


@functools.lru_cache(maxsize=32)
def exact_case(fix, lp, d_in, d_out, mode, featureless, vertical, relu, num_bases, num_blocks, vmax, density, seed):
    """-> (params, bias, X, g, reference, proof bits) of one case, all on the CPU: seeded integer inputs, assert_provably_exact, the oracle
    forward, the ReLU mask from its exact sign, the oracle backward.  A pure function of its arguments, so the cache only saves oracle time:
    the same case under another ROUTE or storage type (spmm_csr 1 / 0, bwd_kernel blk / lean, bwd_own 1 / 0, fbasis_tile modes, fp32 / bf16
    features and parameters) asks for the same answer, mostly in consecutive tests.  The arrays are shared: read-only."""
    fx = lp_fixture(fix) if lp else fixture(fix)
    tp, val, N, R = fx["tp"], fx["val"][vertical], fx["N"], fx["R"]
    rng = np.random.default_rng(seed)
    # parameters at full density (the featureless tables are met once per message; sparse weights would leave all-zero rows), X and g at `density`
    params = {n: ex.ints(shape, -vmax, vmax, 1.0, rng) for n, shape in
              _param_shapes(R, N, d_in, d_out, mode, featureless, num_bases, num_blocks, lp).items()}
    bias = params.pop("bias", None)
    X = None if featureless else ex.ints((N, d_in), -vmax, vmax, density, rng)
    g = ex.ints((N, d_out), -vmax, vmax, density, rng)
    W = oracle.expand_weights(params, mode)
    out = oracle.rgcn_forward(tp, val, N, R, X, W, bias)
    g_eff = g * (out > 0) if relu else g
    bits = ex.assert_provably_exact(tp, val, N, R, X, params, mode, bias, g_eff)
    dX, dW, db = oracle.rgcn_backward(tp, val, N, R, X, W, g_eff, X is not None)
    ref = {"out": np.maximum(out, 0) if relu else out, "dX": dX, "db": db, "grads": oracle.contract_weight_grads(dW, params, mode)}
    for a in (X, g, bias, ref["out"], dX, db, *params.values(), *ref["grads"].values()):
        if a is not None:
            a.flags.writeable = False
    return params, bias, X, g, ref, bits


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(DEV).to(dtype)          # (np.array: a writable copy of a cached read-only array)


def _split(graph, kind, d_in, d_out):
    """the route's own split indicator (> 0: hub rows / tiles are cut into pieces that several waves or workgroups sum)"""
    from torch_rgcn import _native
    if kind == "plan":
        return min(graph.fwd_plan(d_out).n_split, graph.bwd_plan(d_in).n_split)
    if kind == "fwd_plan":
        return graph.fwd_plan(d_out).n_split
    if kind == "csr":
        return min(_native._csr_units(graph.csr("fwd"))[2], _native._csr_units(graph.csr("bwd"))[2])
    if kind == "win":
        return _native._blk_units(graph.win_plan("fwd"))[2]
    if kind == "bwd_blk":
        return _native._blk_units(graph.bwd_blk_plan())[2]
    if kind == "fbasis":
        return graph.fbasis_plan().units_dst[2]
    raise KeyError(kind)


def make_layer(fx, params, bias, d_in, d_out, mode, featureless, vertical, num_bases, num_blocks, lp):
    """the module with the case's integer parameters, moved to the GPU"""
    from torch_rgcn.layers import RelationalGraphConvolutionLP, RelationalGraphConvolutionNC
    N, R = fx["N"], fx["R"]
    decomp = {"none": None, "basis": {"type": "basis", "num_bases": num_bases}, "block": {"type": "block", "num_blocks": num_blocks},
              "diag": None}[mode]
    if lp:
        layer = RelationalGraphConvolutionLP(num_nodes=N, num_relations=R, in_features=d_in, out_features=d_out, decomposition=decomp,
                                             edge_dropout={"general": 0.5, "self_loop": 0.2, "self_loop_type": "schlichtkrull-dropout"},
                                             w_init="glorot-normal", b_init="zeros").eval()
    else:
        layer = RelationalGraphConvolutionNC(triples=torch.from_numpy(fx["tp"]), num_nodes=N, num_relations=R,
                                             in_features=None if featureless else d_in, out_features=d_out, decomposition=decomp,
                                             vertical_stacking=vertical, diag_weight_matrix=(mode == "diag"))
    values = dict(params, **({} if bias is None else {"bias": bias}))
    assert set(values) == {n for n, _ in layer.named_parameters()}, (sorted(values), [n for n, _ in layer.named_parameters()])
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.from_numpy(np.array(values[n])))
    return layer.to(DEV)


def run_exact(fix, d_in, d_out, mode="none", featureless=False, vertical=False, relu=False, dtype=torch.float32, pdtype=torch.float32,
              num_bases=3, num_blocks=2, vmax=2, density=0.5, expect=(), forbid=(), split=None, seed=0, param_dtypes=None, lp=False,
              frozen=(), counts=None, guard=None):
    """one layer, forward and backward, on the fixture `fix`; every result equal to the oracle.  lp: the link-prediction layer in eval mode
    (no dropout), the graph handed over per call.  frozen: names out of "X", the layer's parameter names and "bias" that get no gradient
    (requires_grad False before the forward) -- their .grad must stay None, and everything else is compared with the SAME reference: the
    gradient of a tensor does not depend on which other tensors are frozen.  counts: {profile tag: launches} that must match exactly (the
    forward and the feature gradient share a tag: only the count tells them apart).  guard: a guard_bands.Guard, not yet entered -- the
    parameters, X, the upstream gradient and the LP triples move into guarded allocations, the first call (graph and plans), forward and
    backward run under it, and what it finds (damaged bands, written buffers that no band protects) joins the problems of the case; every
    other assertion is unchanged, so a guard that moved the case to another route fails it.  -> (profile tags, the layer)"""
    from torch_rgcn import _native
    frozen = frozenset(frozen)
    fx = lp_fixture(fix) if lp else fixture(fix)
    params, bias, X, g, ref, bits = exact_case(fix, lp, d_in, d_out, mode, featureless, vertical, relu, num_bases, num_blocks, vmax, density,
                                               seed)                                  # the proof: on the CPU, before any launch
    layer = make_layer(fx, params, bias, d_in, d_out, mode, featureless, vertical, num_bases, num_blocks, lp)
    if pdtype != torch.float32:
        layer = layer.to(pdtype)
    for n, dt in (param_dtypes or {}).items():
        getattr(layer, n).data = getattr(layer, n).data.to(dt)
    names = {n for n, _ in layer.named_parameters()} | (set() if featureless else {"X"})
    assert frozen <= names and frozen != names, (sorted(frozen), sorted(names))
    for n in frozen - {"X"}:
        getattr(layer, n).requires_grad_(False)
    home = (lambda t: t) if guard is None else guard.home
    with contextlib.nullcontext() if guard is None else guard:
        if guard is not None:
            for p in layer.parameters():
                p.data = home(p.data)
        Xd = None if featureless else home(_dev(X, dtype)).requires_grad_("X" not in frozen)
        _native.profile_start()
        if lp:
            out = layer(home(torch.from_numpy(fx["T"]).to(DEV)), Xd)
        elif relu:
            out = layer.forward_activated(Xd, "relu", private=True)
        else:
            out = layer(Xd) if Xd is not None else layer()
        out.backward(home(_dev(g, out.dtype)))
        launches = {k: len(v) for k, v in _native.profile_stop().items()}
        guard_problems = [] if guard is None else guard.problems()
    tags = set(launches)
    ind = None if split is None else int(_split(layer._graph, split, d_in, d_out))
    case = f"{fx['name']} {d_in}x{d_out} {mode}{' featureless' if featureless else ''}{' vertical' if vertical else ''}{' relu' if relu else ''}" \
           f"{' bf16' if dtype == BF or param_dtypes else ''}{' p16' if pdtype == BF else ''}" \
           f"{' frozen {' + ', '.join(sorted(frozen)) + '}' if frozen else ''}"
    print(f"[exact] {case}: tags {sorted(tags)} | split {ind} | proof bits " + " ".join(f"{k} {v:.1f}" for k, v in bits.items()))

    problems = list(guard_problems)

    def check(got, want, name, degree=None):
        try:
            ex.assert_equal_exact(got, want, name, degree)
        except AssertionError as e:
            problems.append(str(e))
    want_dtype = BF if (dtype == BF or (featureless and param_dtypes)) else torch.float32
    if out.dtype != want_dtype:
        problems.append(f"out is {out.dtype}")
    check(out, ref["out"], "out", fx["deg_s"])
    for n in sorted(frozen):
        if (Xd if n == "X" else getattr(layer, n)).grad is not None:
            problems.append(f"{n} is frozen and has a gradient")
    if Xd is not None and "X" not in frozen:
        if Xd.grad.dtype != dtype:
            problems.append(f"dX is {Xd.grad.dtype}")
        check(Xd.grad, ref["dX"], "dX", fx["deg_o"])
    if bias is not None and "bias" not in frozen:
        check(layer.bias.grad, ref["db"], "db")
    for n, gv in ref["grads"].items():
        if n in frozen:
            continue
        p = getattr(layer, n)
        if p.grad.dtype != p.dtype:
            problems.append(f"grad of {n} is {p.grad.dtype}, the parameter {p.dtype}")
        check(p.grad, gv, "d" + n)
    for t in expect:
        if t not in tags:
            problems.append(f"kernel tag {t} did not run: {sorted(tags)}")
    for t in forbid:
        if t in tags:
            problems.append(f"kernel tag {t} ran: {sorted(tags)}")
    for t, n in (counts or {}).items():
        if launches.get(t, 0) != n:
            problems.append(f"kernel tag {t}: {launches.get(t, 0)} launches, {n} expected: {launches}")
    if split is not None and ind <= 0:
        problems.append(f"split indicator '{split}' is {ind}: the hub is not cut into pieces on this route")
    assert not problems, case + "\n" + "\n".join(problems)
    return tags, layer


BOTH = pytest.mark.parametrize("vertical", [False, True], ids=["horizontal", "vertical"])
RELU = pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
TWO_PASS_BWD = ("bwd_scatter_dw", "segment_sum")
# the bf16 storage twins (tests/test_gpu_bf16*.py) and what must not run next to them
WAVE16 = ("spmm_bf16", "wgrad_bf16", "colsum_bf16")
NATIVE16 = ("spmm_blk_bf16", "bwd_own_bf16")
FP32_TAGS = ("spmm_blk", "bwd_fused", "spmm", "wgrad", "wgrad_tiled", "colsum")
BLOCK16 = ("block_spmm_bf16", "block_wgrad_bf16")
DIAG16 = ("diag_spmm_bf16", "diag_wgrad_bf16")
FORBID16 = ("block_spmm", "block_wgrad", "diag_spmm", "diag_wgrad", "spmm", "wgrad", "spmm_bf16", "wgrad_bf16", "rel_rows")


# ----------------------------------------------------------------------------- fp32, width 16
@BOTH
@RELU
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub12", "plan"), ("hub15", "plan")])
def test_wave_owned_tile_plan(monkeypatch, fix, split, relu, vertical):
    """the default of small graphs with dense buckets (forced: sparse_path=0): rgcn_spmm_f32 on wave-owned tiles, hub tiles cut into units
    that merge with atomics; the fused backward, or -- hub-split plans, which the wave-owned backward kernels refuse -- spmm + wgrad"""
    routes.patch(monkeypatch, "sparse_path", "0")
    run_exact(fix, 16, 16, vertical=vertical, relu=relu, expect=("spmm", "bwd_fused") if split is None else ("spmm", "wgrad", "colsum"),
              forbid=("spmm_csr", "spmm_scatter", "spmm_blk") + (() if split is None else ("bwd_fused",)), split=split)


@BOTH
@RELU
@pytest.mark.parametrize("csr", ["1", "0"], ids=["one-pass-csr", "two-pass"])
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub10", "csr"), ("r1", None), ("r1hub", "csr"), ("r59", None)])
def test_sparse_bucket_routes(monkeypatch, fix, split, csr, relu, vertical):
    """sparse_path=1: the one-pass CSR forward (W of up to 120 relations in LDS: r59 is 119) or transform + segment sum, and the relation-major
    two-pass backward; hub rows are CSR units cut into 512-entry pieces; one relation pair (r1)"""
    routes.patch(monkeypatch, "sparse_path", "1")
    routes.patch(monkeypatch, "spmm_csr", csr)
    run_exact(fix, 16, 16, vertical=vertical, relu=relu, expect=(("spmm_csr",) if csr == "1" else ("spmm_scatter",)) + TWO_PASS_BWD,
              forbid=("spmm", "bwd_fused") + (("spmm_scatter",) if csr == "1" else ("spmm_csr",)), split=split)


@BOTH
@RELU
@pytest.mark.parametrize("bwd", ["fused", "split", "deterministic"])
def test_backward_variants(monkeypatch, bwd, relu, vertical):
    """fused kernel with the atomic dW flush, the two-pass backward (bwd=split), the fixed-order partial reduction (deterministic=1)"""
    routes.patch(monkeypatch, "sparse_path", "0")
    if bwd == "deterministic":
        routes.patch(monkeypatch, "deterministic", "1")
    if bwd == "split":
        routes.patch(monkeypatch, "bwd", "split")
    tags, _ = run_exact("plain", 16, 16, vertical=vertical, relu=relu, expect=("spmm",), seed=3)
    assert ("bwd_fused" in tags) == (bwd != "split"), sorted(tags)


@BOTH
@pytest.mark.parametrize("fix", ["hub12", "hub15"])
def test_deterministic_hub_is_one_unit(monkeypatch, fix, vertical):
    """deterministic=1 on a hub graph: no pieces (a hub tile is one long unit), the same exact result"""
    routes.patch(monkeypatch, "sparse_path", "0")
    routes.patch(monkeypatch, "deterministic", "1")
    _, layer = run_exact(fix, 16, 16, vertical=vertical, expect=("spmm", "bwd_fused"))
    graph = layer._graph
    assert graph.fwd_plan(16).n_split == 0 and graph.bwd_plan(16).n_split == 0


@BOTH
@RELU
@pytest.mark.parametrize("fix,split", [("big", None), ("bighub", "win")])
def test_soft_window_forward_and_relation_owner_backward(fix, split, relu, vertical):
    """large static graph, dense buckets: rgcn_spmm_blk_f32 on the soft-window plan (with a hub: tiles cut into pieces that add into a zeroed
    output; the ReLU epilogue then leaves the route) and the relation-owner backward"""
    from torch_rgcn import _native
    hub_relu = relu and split is not None
    _, layer = run_exact(fix, 16, 16, vertical=vertical, relu=relu, expect=("spmm", "bwd_fused") if hub_relu else ("spmm_blk", "bwd_fused"),
                         forbid=("spmm_blk",) if hub_relu else ("spmm",), split=split)
    graph = layer._graph
    assert getattr(graph.win_plan("fwd"), "soft_windows", False)
    if split is None:
        assert graph._plans.get(("win", "bwd_own", _native.bwd_own_rows(graph.num_nodes))) is not None, "the relation-owner backward did not run"


@BOTH
@pytest.mark.parametrize("own", ["1", "0"])
def test_relation_owner_backward_on_and_off(own, vertical):
    """bwd_own=1: rgcn_bwd_own_f32 (dW in the registers of the relation's owner wave); 0: the block-tile backward on the same graph"""
    from torch_rgcn import _native
    from torch_rgcn import functional as F_
    with routes.override(bwd_own=own):
        _, layer = run_exact("big", 16, 16, vertical=vertical, expect=("spmm_blk", "bwd_fused"), seed=1)
        graph = layer._graph
        assert (graph._plans.get(("win", "bwd_own", _native.bwd_own_rows(graph.num_nodes))) is not None) == (own == "1")
        assert F_._backward_route(graph, 16, 16)[0] == ("own" if own == "1" else "blk")


@BOTH
@RELU
def test_block_tile_forward_sparse_buckets(monkeypatch, relu, vertical):
    """sparse buckets and more relations than the one-pass CSR kernel holds (R = 141): ONE launch of the block-tile forward kernel"""
    routes.patch(monkeypatch, "sparse_path", "1")
    run_exact("big_r70", 16, 16, vertical=vertical, relu=relu, expect=("spmm_blk",) + TWO_PASS_BWD, forbid=("spmm_scatter", "spmm_csr", "spmm"))


@BOTH
@RELU
@pytest.mark.parametrize("kernel", ["blk", "lean"])
@pytest.mark.parametrize("fix", ["big_r9", "big_r9hub"])
def test_block_tile_backward(monkeypatch, fix, kernel, relu, vertical):
    """bwd_kernel=blk: the block-tile backward (dX tile in LDS doubles, dW of all relations resident; a hub tile walked in pieces);
    lean: the wave-owned window kernel (hub-split plans fall back to the two-pass backward)"""
    from torch_rgcn import _native
    from torch_rgcn import functional as F_
    routes.patch(monkeypatch, "bwd_kernel", kernel)
    routes.patch(monkeypatch, "sparse_path", "0")
    routes.patch(monkeypatch, "bwd_own", "0")
    hub = fix == "big_r9hub"
    _, layer = run_exact(fix, 16, 16, vertical=vertical, relu=relu, expect=("spmm", "wgrad") if (hub and kernel == "lean") else ("bwd_fused",),
                         forbid=("bwd_fused",) if (hub and kernel == "lean") else ("wgrad",), split="bwd_blk" if (hub and kernel == "blk") else None)
    assert (_native.bwd_blk_rows(40_009, 19) > 64) == (kernel == "blk")
    assert F_._backward_route(layer._graph, 16, 16)[0] == ("blk" if kernel == "blk" else "split" if hub else "lean")


# ----------------------------------------------------------------------------- the dense-weight featured layer's routes, by name
S0 = dict(sparse_path="0")
R9 = dict(S0, bwd_own="0")
ROUTES = [
    # (fixture, route switches, relu, 4 x 4 blocks) -> (forward, backward) of functional._forward_route / _backward_route, read off their conditions
    #  and the fixtures' sizes; the tests above expect the tags of the same kernels for the same rows
    ("plain", S0, False, False, "tiles", "lean"),                    # N = 2000: no tall tiles; spmm + bwd_fused (test_wave_owned_tile_plan)
    ("plain", dict(S0, bwd="split"), False, False, "tiles", "split"),
    ("plain", dict(S0, deterministic="1"), False, False, "tiles", "lean"),      # (test_backward_variants: bwd_fused in this mode too)
    ("hub12", S0, False, False, "tiles", "split"),                   # hub-split wave-owned plan: spmm + wgrad
    ("plain", dict(sparse_path="1", spmm_csr="1"), False, False, "csr", "scatter"),     # R = 7 <= 120; N < 4096: no block-tile backward
    ("plain", dict(sparse_path="1", spmm_csr="0"), False, False, "two_pass", "scatter"),
    ("big_r70", dict(sparse_path="1"), False, False, "blk", "scatter"),         # R = 141 > 120; dW of 141 relations leaves the LDS no 64 rows
    ("big", {}, False, False, "win", "own"),
    ("big", dict(bwd_own="0"), False, False, "win", "blk"),
    ("bighub", {}, False, False, "win", "blk"),                      # hub pieces in the owner plan too (the inverse relations): block-tile kernel
    ("bighub", {}, True, False, "tiles", "blk"),                     # the ReLU epilogue leaves a forward plan with hub pieces
    ("big_r9", dict(R9, bwd_kernel="blk"), False, False, "win", "blk"),
    ("big_r9", dict(R9, bwd_kernel="lean"), False, False, "win", "lean"),
    ("big_r9hub", dict(R9, bwd_kernel="lean"), False, False, "win", "split"),
    ("plain", dict(sparse_path="1"), False, True, "block_csr", "scatter"),
]


@pytest.mark.parametrize("fix,switches,relu,blocks,fwd,bwd", ROUTES,
                         ids=[f"{r[0]}-{'-'.join(f'{k}={v}' for k, v in r[1].items()) or 'defaults'}{'-relu' * r[2]}{'-blocks' * r[3]}" for r in ROUTES])
def test_route_names(fix, switches, relu, blocks, fwd, bwd):
    """the two decisions of _RelationalMP, asked with the layer's graph and the shapes alone: the names, and "split" -- which asks the graph
    for no fused-backward plan -- whenever X or W is frozen.  No tensors, no oracle: one forward on zeros builds the graph"""
    from torch_rgcn import functional as F_
    fx = fixture(fix)
    mode = "block" if blocks else "none"
    shapes = _param_shapes(fx["R"], fx["N"], 16, 16, mode, False, 3, 4, False)
    params = {n: np.zeros(shape, np.float32) for n, shape in shapes.items()}
    layer = make_layer(fx, params, params.pop("bias"), 16, 16, mode, False, False, 3, 4, False)
    with routes.override(**switches), torch.no_grad():
        layer(torch.zeros(fx["N"], 16, device=DEV))
        graph = layer._graph
        before = set(graph._plans)
        assert F_._backward_route(graph, 16, 16, need_x=False, diag4=blocks)[0] == "split"
        assert F_._backward_route(graph, 16, 16, need_w=False, diag4=blocks)[0] == "split"
        assert set(graph._plans) == before, "a frozen input: no plan is asked for"
        got = F_._forward_route(graph, fx["R"], 16, 16, relu=relu, blocks4=blocks)[0], F_._backward_route(graph, 16, 16, diag4=blocks)[0]
    assert got == (fwd, bwd), got


# ----------------------------------------------------------------------------- fp32, other widths
NARROW = {"wide": "narrow", "widehub10": "narrowhub10"}
WIDTHS = [(10, 11), (16, 4), (32, 32), (64, 3), (48, 80), (200, 200), (7, 130)]


@BOTH
@pytest.mark.parametrize("d_in,d_out", WIDTHS, ids=lambda v: str(v))
@pytest.mark.parametrize("family", ["plain", "hub"])
def test_other_widths(monkeypatch, family, d_in, d_out, vertical):
    """padded widths on the MFMA block kernels (up to 64), the generic-width kernel, and the relation-grouped gather-GEMM + row sum above
    64 (200 x 200, 7 x 130, 48 x 80: rgcn_gemm_f32 tags rel_rows / segment_sum_wide / rel_wgrad)"""
    wide = max(d_in, d_out) > 64
    if wide:
        fix, split, vmax = ("wide", None, 1) if family == "plain" else ("widehub10", "csr", 1)
        expect = ("rel_rows", "segment_sum_wide", "rel_wgrad")
    else:
        routes.patch(monkeypatch, "sparse_path", "0")
        fix, split, vmax = ("plain", None, 2) if family == "plain" else ("hub12", "plan", 2)
        expect = ("spmm", "bwd_fused") if (family == "plain" and max(d_in, d_out) <= 16) else ("spmm", "wgrad")
    run_exact(fix, d_in, d_out, vertical=vertical, relu=(d_in == 32), vmax=vmax, expect=expect, split=split, seed=d_in + d_out)


# ----------------------------------------------------------------------------- decompositions
@BOTH
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
def test_basis_featured_aggregate_then_gemm(fix, split, vertical):
    """64 x 64, B = 3: aggregate per basis on the CSR (hub rows in pieces), then contract on rgcn_gemm_f32.  dbases sums over all relations:
    its grid is the smallest val of the graph, which the 2^10 hub of the CSR units leaves inside the proof bound"""
    run_exact(fix, 64, 64, mode="basis", vertical=vertical, vmax=1, num_bases=3, expect=("basis_aggregate", "gemm"), split=split)


@pytest.mark.parametrize("nb,bi,bo", [(20, 4, 4), (100, 5, 5), (24, 3, 4), (4, 4, 4)], ids=lambda v: str(v))
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
@RELU
def test_block_kernels(fix, split, nb, bi, bo, relu):
    """block_path=2: the blocks applied as they are (rgcn_block_spmm_f32 both ways, rgcn_block_wgrad_f32): fixed 4 x 4, 5 x 5 in two trips of
    the block loop, run-time 3 x 4, and width 16"""
    fix = NARROW[fix] if nb == 100 else fix
    with routes.override(block_path="2"):
        run_exact(fix, nb * bi, nb * bo, mode="block", num_blocks=nb, relu=relu, vmax=1, expect=("block_spmm", "block_wgrad"),
                  forbid=("spmm", "rel_rows"), split=split)


@RELU
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_block_table_in_lds(dtype, relu):
    """many units and a small block table: the persistent-workgroup form with the table in LDS (8 blocks of 4 x 4 on the big graph)"""
    bf = dtype == BF
    run_exact("big", 32, 32, mode="block", num_blocks=8, relu=relu, dtype=dtype, expect=BLOCK16 if bf else ("block_spmm", "block_wgrad"),
              forbid=FORBID16 if bf else ("spmm",))


@pytest.mark.parametrize("d", [30, 32, 100])
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
def test_diagonal_kernels(fix, split, d):
    run_exact(fix, d, d, mode="diag", expect=("diag_spmm", "diag_wgrad"), forbid=("spmm",), split=split)


@pytest.mark.parametrize("route", ["1", "0"], ids=["csr", "tile"])
@pytest.mark.parametrize("d_out", [16, 10])
@pytest.mark.parametrize("family", ["plain", "hub"])
def test_featureless(monkeypatch, family, route, d_out):
    """the weight table R x N x d on the destination-major CSR kernels (hub rows: 512-entry pieces, the 2^10 hub) and on the tile-plan
    kernels (hub tiles cut into units: the 2^12 hub -- the route of test_hub_node_tile_splitting_vs_oracle's featureless case)"""
    routes.patch(monkeypatch, "featureless_csr", route)
    csr = ("featureless_csr_fwd", "featureless_csr_wgrad")
    tile = ("featureless_fwd", "featureless_wgrad")
    fix, split = ("plain", None) if family == "plain" else (("hub10", "csr") if route == "1" else ("hub12", "fwd_plan"))
    run_exact(fix, None, d_out, featureless=True, expect=csr if route == "1" else tile, forbid=tile if route == "1" else csr, split=split)


@pytest.mark.parametrize("B,d", [(4, 10), (30, 16), (64, 11)])
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub10", "fbasis")])
def test_featureless_basis_source_major(fix, split, B, d):
    run_exact(fix, None, d, mode="basis", featureless=True, num_bases=B, vmax=1, expect=("fbasis_fwd", "fbasis_bwd"),
              forbid=("fbasis_tile_fwd", "fbasis_tile_bwd"), split=split)


@pytest.mark.parametrize("mode", ["ranges", "nodes"])
@pytest.mark.parametrize("fix,B,d", [("n3001", 40, 10), ("n16", 5, 10)])
def test_featureless_basis_tile_kernels(monkeypatch, fix, B, d, mode):
    """the table walked in the parameter's [B, N, d] layout (fbasis_inplace_mb=0): a node count off the 16-node grid with a hub, and N = 16"""
    routes.patch(monkeypatch, "fbasis_inplace_mb", "0")
    routes.patch(monkeypatch, "fbasis_tile", mode)
    run_exact(fix, None, d, mode="basis", featureless=True, num_bases=B, vmax=1, expect=("fbasis_tile_fwd", "fbasis_tile_bwd"),
              split="fbasis" if fix == "n3001" else None)


# ----------------------------------------------------------------------------- bf16: 100 % equal to the rounded oracle
@RELU
@pytest.mark.parametrize("d_in,d_out", [(16, 16), (10, 16), (64, 64)], ids=lambda v: str(v))
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub12", "plan")])
def test_bf16_wave_owned(fix, split, d_in, d_out, relu):
    """rgcn_spmm_bf16 (forward and dX; hub pieces summed in an fp32 scratch and rounded by a second launch), rgcn_wgrad_bf16, rgcn_colsum_bf16"""
    run_exact(fix, d_in, d_out, relu=relu, dtype=BF, expect=WAVE16, forbid=FP32_TAGS + NATIVE16, split=split, seed=5)


@BOTH
@RELU
@pytest.mark.parametrize("pdtype", [torch.float32, BF], ids=["p32", "p16"])
def test_bf16_soft_window_and_relation_owner(pdtype, relu, vertical):
    """rgcn_spmm_blk_bf16 / rgcn_bwd_own_bf16; bf16 parameters: gradients equal to the exact value rounded once"""
    run_exact("big", 16, 16, vertical=vertical, relu=relu, dtype=BF, pdtype=pdtype, expect=NATIVE16, forbid=FP32_TAGS + WAVE16, seed=6)


@BOTH
def test_bf16_soft_window_forward_hub_pieces(vertical):
    """rgcn_spmm_blk_bf16 on a plan with hub pieces: fp32 atomics into a scratch, rounded afterwards.  Through the layer this form is out of
    reach -- the inverse relations make every hub destination a hub source too, the relation-owner plan then has pieces as well, and
    _bf16_native_plans hands such graphs to the wave-owned kernels -- so the kernel is called on the layer's own soft-window plan, forward only"""
    from torch_rgcn import _native
    fx = fixture("bighub")
    params, bias, X, _, ref, bits = exact_case("bighub", False, 16, 16, "none", False, vertical, False, 3, 2, 2, 0.5, 0)
    layer = make_layer(fx, params, bias, 16, 16, "none", False, vertical, 3, 2, False)
    graph = layer._graph_on(torch.device(DEV))
    plan = graph.win_plan("fwd")
    assert plan is not None and getattr(plan, "soft_windows", False)
    n_split = _native._blk_units(plan)[2]
    Xd = _dev(X, BF)
    if graph.perm is not None:          # plans on locality-relabelled ids: features in through inv, output back through perm (as the layer does)
        Xd = Xd.index_select(0, graph.inv)
    _native.profile_start()
    out = _native.spmm_blk_bf16(Xd.contiguous(), layer.weights.detach(), layer.bias.detach(), plan)
    tags = set(_native.profile_stop())
    if graph.perm is not None:
        out = out.index_select(0, graph.perm)
    print(f"[exact] bighub 16x16 spmm_blk_bf16{' vertical' if vertical else ''}: tags {sorted(tags)} | split {n_split} | proof bits out {bits['out']:.1f}")
    assert n_split > 0 and tags == {"spmm_blk_bf16"}, (n_split, sorted(tags))
    assert out.dtype == BF
    ex.assert_equal_exact(out, ref["out"], "out", fx["deg_s"])


@RELU
@pytest.mark.parametrize("pdtype", [torch.float32, BF], ids=["p32", "p16"])
@pytest.mark.parametrize("nb,bi,bo", [(20, 4, 4), (100, 5, 5)], ids=lambda v: str(v))
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
def test_bf16_block_kernels(fix, split, nb, bi, bo, pdtype, relu):
    """8-byte loads (4 x 4 blocks) and 2-byte loads (5 x 5: 10-byte segments); hub pieces: fp32 atomics into the scratch, rounded (and the
    ReLU applied) by the second launch"""
    fix = NARROW[fix] if nb == 100 else fix
    run_exact(fix, nb * bi, nb * bo, mode="block", num_blocks=nb, relu=relu, dtype=BF, pdtype=pdtype, vmax=1, expect=BLOCK16, forbid=FORBID16,
              split=split)


@pytest.mark.parametrize("pdtype", [torch.float32, BF], ids=["p32", "p16"])
@pytest.mark.parametrize("d", [32, 30])
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
def test_bf16_diagonal_kernels(fix, split, d, pdtype):
    """8-byte loads (rows of 32) and 2-byte loads (rows of 30 are 60 bytes)"""
    run_exact(fix, d, d, mode="diag", dtype=BF, pdtype=pdtype, expect=DIAG16, forbid=FORBID16, split=split)


@pytest.mark.parametrize("mode", ["ranges", "nodes", "nodes2"])
@pytest.mark.parametrize("fix,B,d", [("n3001", 40, 10), ("n16", 5, 10)])
def test_bf16_featureless_basis_tile_kernels(fix, B, d, mode):
    """bf16 bases table: out and dbases equal to the exact value rounded once, dcomps and db exact fp32"""
    with routes.override(fbasis_tile=mode):
        run_exact(fix, None, d, mode="basis", featureless=True, num_bases=B, vmax=1, param_dtypes={"bases": BF},
                  expect=("fbasis_tile_fwd_bf16", "fbasis_tile_bwd_bf16"), forbid=("fbasis_tile_fwd", "fbasis_tile_bwd"),
                  split="fbasis" if fix == "n3001" else None)


# ----------------------------------------------------------------------------- LP layer (eval mode: no dropout; per-call graph, rowptr path)
@pytest.mark.parametrize("fix", ["plain", "hub10"])
@pytest.mark.parametrize("case", ["none-16", "none-20x128", "block-80", "block-80-bf16", "none-16-bf16"])
def test_lp_layer(fix, case):
    """the link-prediction layer: [T | inverses | T | self loops] built per call, no work units (every row one unit, also the hub's).  Block
    decomposition: block-diagonal relations plus a dense self-loop weight -- in bf16 the dense term is added in fp32 before the one rounding"""
    mode, dims, *bf = case.split("-")
    d_in, d_out = (int(dims), int(dims)) if "x" not in dims else map(int, dims.split("x"))
    dtype = BF if bf else torch.float32
    kw = dict(mode="block", num_blocks=20, vmax=1) if mode == "block" else {}
    expect, forbid = {"none-16": (("spmm", "bwd_fused"), WAVE16),
                      "none-20x128": (("rel_rows", "segment_sum_wide", "rel_wgrad"), ("spmm",)),
                      "block-80": (("block_spmm", "block_wgrad", "gemm"), ("spmm", "rel_rows")),
                      "block-80-bf16": (BLOCK16 + ("colsum_bf16", "gemm"), FORBID16),
                      "none-16-bf16": (WAVE16, FP32_TAGS)}[case]
    run_exact(fix, d_in, d_out, dtype=dtype, lp=True, seed=9, expect=expect, forbid=forbid, **kw)


# ----------------------------------------------------------------------------- DistMult
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("d", [50, 52, 300])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_distmult(monkeypatch, bwd, d, with_bias):
    """integer embeddings, repeated triples, a hub subject that is a hub object too: scores and every gradient equal to the oracle.  All
    terms are integers (grid 1): the proof bound is the oracle on the absolute values"""
    distmult_exact(monkeypatch, bwd, d, with_bias)


def distmult_exact(monkeypatch, bwd, d, with_bias, frozen=(), guard=None):
    """the body of test_distmult.  frozen: names out of "nodes", "relations", "biases" (the three bias vectors together) that get no
    gradient: theirs must stay None, the others equal the same oracle gradients.  All of them frozen: forward only -- the scores exact and
    no CSR ranks counted by the scoring kernel.  guard: as in run_exact -- parameters, embeddings, triples and the score gradient in guarded
    allocations, forward and backward under the guard, its findings asserted with the rest"""
    from torch_rgcn import _native
    frozen = frozenset(frozen)
    assert frozen <= {"nodes", "relations", "biases"} and (with_bias or "biases" not in frozen)
    from torch_rgcn.layers import DistMult
    routes.patch(monkeypatch, "distmult_bwd", bwd)
    N, R0, T = 300, 5, 4000
    rng = np.random.default_rng(d)
    tr = np.stack([rng.integers(0, N, T), rng.integers(0, R0, T), rng.integers(0, N, T)], 1).astype(np.int64)
    tr[:700, 0] = 17
    tr[700:1400, 2] = 17
    tr[1400:1500] = tr[0]                                       # repeated triples
    tr = tr[(tr[:, 0] != 3) & (tr[:, 2] != 3)]
    nodes = ex.ints((N, d), -2, 2, 0.5, rng)
    rel = ex.ints((R0, d), -2, 2, 1.0, rng)
    sb, ob, pb = ex.ints((N,), -2, 2, 1.0, rng), ex.ints((N,), -2, 2, 1.0, rng), ex.ints((R0,), -2, 2, 1.0, rng)
    gs = ex.ints((len(tr),), -2, 2, 0.7, rng)
    bias = (sb, pb, ob) if with_bias else (None, None, None)
    # proof: every term an integer, the sums of absolute values inside the significand
    a_sc = oracle.distmult_forward(tr, np.abs(nodes), np.abs(rel), *(None if b is None else np.abs(b) for b in bias))
    a_gr = oracle.distmult_backward(tr, np.abs(nodes), np.abs(rel), np.abs(gs), with_bias)
    bits = {"scores": np.log2(max(a_sc.max(), 1))} | {k: float(np.log2(max(a.max(), 1))) for k, a in zip(("dnodes", "drel", "dsb", "dpb", "dob"), a_gr)
                                                     if a is not None}
    assert max(bits.values()) <= ex.MAX_BITS, bits
    sc_ref = oracle.distmult_forward(tr, nodes, rel, *bias)
    dn, dr, dsb, dpb, dob = oracle.distmult_backward(tr, nodes, rel, gs, with_bias)

    dm = DistMult(R0, d, N, R0, b_init="normal" if with_bias else None).to(DEV)
    with torch.no_grad():
        dm.relations.copy_(torch.from_numpy(rel))
        if with_bias:
            dm.sbias.copy_(torch.from_numpy(sb)); dm.obias.copy_(torch.from_numpy(ob)); dm.pbias.copy_(torch.from_numpy(pb))
    dm.relations.requires_grad_("relations" not in frozen)
    if with_bias:
        for b in (dm.sbias, dm.pbias, dm.obias):
            b.requires_grad_("biases" not in frozen)
    any_grad = frozen != ({"nodes", "relations", "biases"} if with_bias else {"nodes", "relations"})
    asked = []                                                  # ranks= of every call of the scoring kernel's wrapper
    inner = _native.distmult_fwd
    monkeypatch.setattr(_native, "distmult_fwd", lambda *a, ranks=False: (asked.append(ranks), inner(*a, ranks=ranks))[1])
    home = (lambda t: t) if guard is None else guard.home
    with contextlib.nullcontext() if guard is None else guard:
        if guard is not None:
            for p in dm.parameters():
                p.data = home(p.data)
        nd = home(torch.from_numpy(nodes).to(DEV)).requires_grad_("nodes" not in frozen)
        _native.profile_start()
        sc = dm(home(torch.from_numpy(tr).to(DEV)), nd)
        if any_grad:
            sc.backward(home(torch.from_numpy(gs).to(DEV)))
        tags = set(_native.profile_stop())
        guard_problems = [] if guard is None else guard.problems()
    print(f"[exact] distmult {bwd} d={d} bias={with_bias}{' frozen {' + ', '.join(sorted(frozen)) + '}' if frozen else ''}: tags {sorted(tags)} "
          f"| proof bits " + " ".join(f"{k} {v:.1f}" for k, v in bits.items()))
    # the scoring kernel counts the CSR ranks when anything needs a gradient and the backward will walk the CSRs
    assert asked == [any_grad and bwd != "atomic"], asked
    assert not guard_problems, "\n".join(guard_problems)
    # csr: every gradient from the two CSR walks where the relation table fits (distmult_bwd_all_supported), else the split form; split:
    # predicate-sorted kernel + entity gradients from the CSRs; atomic: the scatter kernel alone.  (The backward computes every gradient
    # whatever is frozen: autograd drops what nobody asked for.)
    want = {"atomic": {"distmult_bwd"}, "split": {"distmult_bwd", "distmult_bwd_nodes"},
            "csr": {"distmult_bwd_all"} if _native.distmult_bwd_all_supported(R0, d) else {"distmult_bwd", "distmult_bwd_nodes"}}[bwd]
    if not any_grad:
        want = set()
    assert "distmult_fwd" in tags and {t for t in tags if t.startswith("distmult_bwd")} == want, (sorted(tags), sorted(want))
    if d <= 52:
        assert _native.distmult_bwd_all_supported(R0, d), "the csr route's own kernel is not exercised at any tested width"
    ex.assert_equal_exact(sc, sc_ref, "scores")
    if "nodes" in frozen:
        assert nd.grad is None
    else:
        ex.assert_equal_exact(nd.grad, dn, "dnodes")
        assert float(nd.grad[3].abs().max()) == 0.0
    if "relations" in frozen:
        assert dm.relations.grad is None
    else:
        ex.assert_equal_exact(dm.relations.grad, dr, "drelations")
    if with_bias and "biases" in frozen:
        assert dm.sbias.grad is None and dm.pbias.grad is None and dm.obias.grad is None
    elif with_bias:
        ex.assert_equal_exact(dm.sbias.grad, dsb, "dsbias")
        ex.assert_equal_exact(dm.pbias.grad, dpb, "dpbias")
        ex.assert_equal_exact(dm.obias.grad, dob, "dobias")
