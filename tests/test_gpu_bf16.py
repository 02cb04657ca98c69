"""bf16 storage for featured layers: bf16 features in, bf16 out and feature gradient, fp32 arithmetic, one rounding.

The fp32 reference is the layer's own fp32 route on the widened inputs (the suite pins that route to the C oracle); one small case goes
to the oracle directly.  Criteria: out / dX equal the rounded fp32 result in >= 99.9 % of the elements and differ by at most one bf16
ulp elsewhere (the sum order may differ; where the reference runs other kernels, elements whose sums cancel may move by fp32 round-off of
the largest element); dW / db within 1e-4 relative."""
import numpy as np
import pytest
import torch
from torch_rgcn import routes  # noqa: E402

from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32)


def assert_rounded(a, ref32, name, cancel_ok=False):
    """a (bf16) = ref32 rounded to bf16, up to one ulp in at most 0.1 % of the elements.  cancel_ok: the reference ran other kernels (another
    sum order) -- an element whose sum cancels may then also move by fp32 round-off of the largest element"""
    assert a.dtype == BF and a.shape == ref32.shape, (name, a.dtype, a.shape, ref32.shape)
    r = ref32.to(BF)
    same = (a == r) | (torch.isnan(a) & torch.isnan(r))
    frac = same.float().mean().item()
    ulp = (_bits(a) - _bits(r)).abs()
    # an element whose sum cancels (|value| << the largest) can move by more than one of ITS ulps under another fp32 sum order: fp32 noise
    cancel = ((a.float() - ref32).abs() <= 2 ** -16 * float(ref32.abs().max())) & cancel_ok
    assert frac >= 0.999, f"{name}: {100 * frac:.3f} % equal to the rounded fp32 result"
    assert bool(((ulp <= 1) | same | cancel).all()), f"{name}: more than one bf16 ulp off (max {int(ulp.max())})"


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _graph(N, R0, E, seed, hub=False):
    T = oracle.synthetic_triples(N, R0, E, seed=seed)
    if hub:          # a destination with many messages: its tile is cut into pieces that different workgroups sum
        rng = np.random.default_rng(seed)
        h = np.stack([np.zeros(40_000, np.int64), rng.integers(0, R0, 40_000), rng.integers(0, N, 40_000)], 1)
        T = np.concatenate([T, h.astype(T.dtype)])
    return torch.from_numpy(oracle.add_inverse_and_self(T, N, R0)), 2 * R0 + 1


def _nc(tp, N, R, d_in, d_out, vertical=False, bias=True, decomposition=None, seed=0):
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.manual_seed(seed)
    layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=R, in_features=d_in, out_features=d_out, bias=bias,
                                         vertical_stacking=vertical, decomposition=decomposition).to(DEV)
    if bias:
        with torch.no_grad():
            layer.bias.normal_()
    return layer


def _run(layer, X, G, relu=False):
    """(out, dX, {param: grad}) of one forward / backward with upstream gradient G"""
    X = X.detach().clone().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    out = layer.forward_activated(X, "relu", private=True) if relu else layer(X)
    out.backward(G.to(out.dtype))
    return out.detach(), X.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


FP32_TAGS = ("spmm_blk", "bwd_fused", "spmm", "wgrad", "wgrad_tiled", "colsum")


def _compare(layer, X16, G16, relu=False, expect=None, forbid=FP32_TAGS, cancel_ok=False):
    """the bf16 run against the fp32 route on the widened inputs; expect / forbid: profile tags"""
    from torch_rgcn import _native
    _native.profile_start()
    out, dX, grads = _run(layer, X16, G16, relu)
    torch.cuda.synchronize()
    tags = set(_native.profile_stop())
    out32, dX32, grads32 = _run(layer, X16.float(), G16.float(), relu)
    assert out.dtype == BF and dX.dtype == BF
    assert_rounded(out, out32, "out", cancel_ok)
    assert_rounded(dX, dX32, "dX", cancel_ok)
    for n, p in layer.named_parameters():
        assert grads[n].dtype == p.dtype, (n, grads[n].dtype, p.dtype)
        assert rel(grads[n].float(), grads32[n].float()) <= (1e-4 if p.dtype == torch.float32 else 2 ** -8), n
    if expect is not None:
        for t in expect:
            assert t in tags, (t, sorted(tags))
        for t in forbid:
            assert t not in tags, (t, sorted(tags))
    return out, dX, grads, tags


NATIVE = ("spmm_blk_bf16", "bwd_own_bf16")
WAVE = ("spmm_bf16", "wgrad_bf16", "colsum_bf16")
N70, E70 = 70_000, 1_200_000


@pytest.mark.parametrize("R0", [5, 50])
@pytest.mark.parametrize("vertical", [False, True])
def test_softwin_route(R0, vertical):
    """S1-shaped graph: the soft-window forward and the relation-owner backward read and write bf16 rows; bias, no bias, fused ReLU"""
    tp, R = _graph(N70, R0, E70, seed=700 + R0)
    X = torch.randn(N70, 16, device=DEV).to(BF)
    G = torch.randn(N70, 16, device=DEV).to(BF)
    for bias, relu in ((True, False), (False, True), (True, True)):
        layer = _nc(tp, N70, R, 16, 16, vertical=vertical, bias=bias, seed=R0)
        _compare(layer, X, G, relu=relu, expect=NATIVE)


@pytest.mark.parametrize("switch", ["softwin", "bwd_own"])
def test_wave_owned_route_under_general_switches(switch):
    """softwin=0 / bwd_own=0: the wave-owned bf16 kernels (rgcn_spmm_bf16 forward and dX, rgcn_wgrad_bf16, rgcn_colsum_bf16); the same
    criteria against the fp32 route, and agreement with the soft-window route"""
    tp, R = _graph(N70, 5, E70, seed=705)
    X = torch.randn(N70, 16, device=DEV).to(BF)
    G = torch.randn(N70, 16, device=DEV).to(BF)
    layer = _nc(tp, N70, R, 16, 16, seed=5)
    nat = _compare(layer, X, G, expect=NATIVE)
    with routes.override(**{switch: "0"}):
        layer = _nc(tp, N70, R, 16, 16, seed=5)
        wave = _compare(layer, X, G, expect=WAVE, forbid=FP32_TAGS + NATIVE, cancel_ok=True)
    # (each is its own fp32 sum rounded once; their sum orders differ, so near-cancelling elements may differ by more than one ulp)
    assert rel(wave[0].float(), nat[0].float()) <= 2 ** -8
    assert rel(wave[1].float(), nat[1].float()) <= 2 ** -8
    assert rel(wave[2]["weights"], nat[2]["weights"]) < 1e-4
    assert rel(wave[2]["bias"], nat[2]["bias"]) < 1e-4


def test_am_shaped_hub_pieces_through_the_layer():
    """AM-shaped (R = 267, sparse buckets) with a hub destination: the wave-owned plan cuts its tile into pieces that different waves sum.
    The bf16 forward sums them in an fp32 scratch and rounds once: every run equals the rounded fp32 result (the pieces' fp32 atomics add in
    arrival order, so two runs may differ in the last fp32 bit of a hub row -- and, rarely, in a bf16 ulp: no bit-identity is asserted)"""
    from torch_rgcn import _native
    N, R0, E = 20_000, 133, 160_000
    tp, R = _graph(N, R0, E, seed=711, hub=True)
    assert R == 267
    layer = _nc(tp, N, R, 16, 16, seed=1)
    X = torch.randn(N, 16, device=DEV).to(BF)
    G = torch.randn(N, 16, device=DEV).to(BF)
    assert layer._graph_on(torch.device(DEV)).fwd_plan(16).n_split > 0, "no hub pieces in the plan"
    o1 = _compare(layer, X, G, expect=WAVE, forbid=FP32_TAGS + NATIVE, cancel_ok=True)[0]
    o2 = _compare(layer, X, G, expect=WAVE, forbid=FP32_TAGS + NATIVE, cancel_ok=True)[0]
    assert rel(o1.float(), o2.float()) <= 2 ** -8


@pytest.mark.parametrize("dims", [(10, 16), (16, 32), (32, 64), (64, 10), (20, 36), (100, 100)])
def test_widths(dims):
    """padded widths up to 64 on the native routes (16 x 16: soft-window, else wave-owned; the ReLU epilogue on the wider ones); 100 x 100 on
    the upcast route (no bf16 tags), output cast back"""
    d_in, d_out = dims
    tp, R = _graph(N70, 5, E70, seed=720)
    X = torch.randn(N70, d_in, device=DEV).to(BF)
    G = torch.randn(N70, d_out, device=DEV).to(BF)
    layer = _nc(tp, N70, R, d_in, d_out, seed=2)
    pad = max(d_in + (-d_in % 16), d_out + (-d_out % 16))
    if pad == 16:
        _compare(layer, X, G, expect=NATIVE)
    elif pad <= 64:
        _compare(layer, X, G, relu=True, expect=WAVE, forbid=FP32_TAGS + NATIVE)
    else:
        _compare(layer, X, G, expect=(), forbid=NATIVE + WAVE)


@pytest.mark.parametrize("decomp", [None, {"type": "basis", "num_bases": 3}, {"type": "block", "num_blocks": 4},
                                    {"type": "block", "num_blocks": 2}, "diag"])
@pytest.mark.parametrize("pdtype", [torch.float32, torch.bfloat16])
def test_decompositions_and_parameter_dtypes(decomp, pdtype):
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    tp, R = _graph(N70, 5, E70, seed=730)
    torch.manual_seed(4)
    if decomp == "diag":
        layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N70, num_relations=R, in_features=16, out_features=16,
                                             diag_weight_matrix=True).to(DEV)
    else:
        layer = _nc(tp, N70, R, 16, 16, decomposition=decomp, seed=4)
    layer = layer.to(pdtype)
    X = torch.randn(N70, 16, device=DEV).to(BF)
    G = torch.randn(N70, 16, device=DEV).to(BF)
    other = decomp == "diag" or (isinstance(decomp, dict) and decomp["type"] == "block")    # the fp32 route runs the block / diag kernels
    if pdtype == torch.float32:
        _compare(layer, X, G, expect=NATIVE, cancel_ok=other)
        return
    # bf16 parameters: the reference is the fp32 route on the widened parameters (a copy of the layer in fp32)
    import copy
    ref = copy.deepcopy(layer).float()
    from torch_rgcn import _native
    _native.profile_start()
    out, dX, grads = _run(layer, X, G)
    tags = set(_native.profile_stop())
    out32, dX32, grads32 = _run(ref, X.float(), G.float())
    assert set(NATIVE) <= tags, sorted(tags)
    assert_rounded(out, out32, "out", other)
    assert_rounded(dX, dX32, "dX", other)
    for n, p in layer.named_parameters():
        assert p.dtype == BF and grads[n].dtype == BF, n
        assert rel(grads[n].float(), grads32[n].to(BF).float()) <= 2 ** -7, n


def _lp(N, R0, decomposition=None, d=16):
    from torch_rgcn.layers import RelationalGraphConvolutionLP
    torch.manual_seed(0)
    ed = {"general": 0.5, "self_loop": 0.2, "self_loop_type": "schlichtkrull-dropout"}
    return RelationalGraphConvolutionLP(num_nodes=N, num_relations=2 * R0 + 1, in_features=d, out_features=d, edge_dropout=ed,
                                        decomposition=decomposition, w_init="glorot-normal", b_init="zeros").to(DEV)


def _lp_run(layer, graph, x, g, seed=1):
    torch.manual_seed(seed)          # the edge mask and the self-loop dropout draw from the generator: the same draws for both dtypes
    x = x.detach().clone().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    out = layer(graph, x)
    out.backward(g)
    return out.detach(), x.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


def test_lp_layer_per_call_graph_native_and_no_sync():
    """the LP layer's per-call (sync-free) graph on the wave-owned bf16 kernels: the contract against the fp32 route, and a step that issues no
    host synchronisation (device build, deferred checks)"""
    from torch_rgcn import _native
    N, R0, E = 6000, 9, 8000
    layer = _lp(N, R0)
    layer.eval()
    graph = torch.from_numpy(oracle.synthetic_triples(N, R0, E, 3)).to(DEV)
    X = torch.randn(N, 16, device=DEV).to(BF)
    G = torch.randn(N, 16, device=DEV).to(BF)
    _native.profile_start()
    out, dX, gr = _lp_run(layer, graph, X, G)
    tags = set(_native.profile_stop())
    assert set(WAVE) <= tags and not (set(FP32_TAGS) & tags), sorted(tags)
    out32, dX32, gr32 = _lp_run(layer, graph, X.float(), G.float())
    assert_rounded(out, out32, "out", cancel_ok=True)
    assert_rounded(dX, dX32, "dX", cancel_ok=True)
    for n in gr:
        assert gr[n].dtype == torch.float32 and rel(gr[n], gr32[n]) <= 1e-4, n
    torch.cuda.synchronize()
    with routes.override(deferred_checks="1"):
        _lp_run(layer, graph, X, G)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            _lp_run(layer, graph, X, G)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()


@pytest.mark.parametrize("training", [False, True])
def test_lp_block_decomposition(training):
    """LP block decomposition: cat([block_diag(blocks), blocks_self]) as the dense fp32 W; in training mode (schlichtkrull-dropout) the dropped
    self-loop messages are added before the one rounding (upcast route)"""
    N, R0, E = 6000, 9, 8000
    layer = _lp(N, R0, decomposition={"type": "block", "num_blocks": 4})
    layer.train(training)
    graph = torch.from_numpy(oracle.synthetic_triples(N, R0, E, 5)).to(DEV)
    X = torch.randn(N, 16, device=DEV).to(BF)
    G = torch.randn(N, 16, device=DEV).to(BF)
    out, dX, gr = _lp_run(layer, graph, X, G)
    out32, dX32, gr32 = _lp_run(layer, graph, X.float(), G.float())
    assert_rounded(out, out32, "out", cancel_ok=True)
    assert_rounded(dX, dX32, "dX", cancel_ok=True)
    for n in gr:
        assert gr[n].dtype == torch.float32 and rel(gr[n], gr32[n]) <= 1e-4, n


def test_small_case_vs_oracle():
    """out, dX and dW within 2^-8 relative of the C oracle evaluated on the widened inputs (native route)"""
    N, R0, E = 40_000, 7, 400_000
    T = oracle.synthetic_triples(N, R0, E, seed=3)
    tp = oracle.add_inverse_and_self(T, N, R0)
    R = 2 * R0 + 1
    layer = _nc(torch.from_numpy(tp), N, R, 16, 16, seed=9)
    X = torch.randn(N, 16, device=DEV).to(BF)
    G = torch.randn(N, 16, device=DEV).to(BF)
    from torch_rgcn import _native
    _native.profile_start()
    out, dX, grads = _run(layer, X, G)
    tags = set(_native.profile_stop())
    assert set(NATIVE) <= tags, sorted(tags)
    v = oracle.nc_edge_norm(tp, N, R, False)
    Xn, Gn = X.float().cpu().numpy(), G.float().cpu().numpy()
    w, b = layer.weights.detach().cpu().numpy(), layer.bias.detach().cpu().numpy()
    out_o = oracle.rgcn_forward(tp, v, N, R, Xn, w, b)
    dx_o, dw_o, _ = oracle.rgcn_backward(tp, v, N, R, Xn, w, Gn)
    assert rel(out.float().cpu(), torch.from_numpy(out_o)) <= 2 ** -8
    assert rel(dX.float().cpu(), torch.from_numpy(dx_o)) <= 2 ** -8
    assert rel(grads["weights"].cpu(), torch.from_numpy(dw_o)) <= 2 ** -8


def test_full_size_s1():
    """S1 (1 M nodes, 10 M triples, R = 101): one layer against the fp32 route; the bench.py-shaped two-layer step in bf16 against fp32"""
    from torch_rgcn import _native
    N, R0, E = 1_000_000, 50, 10_000_000
    T = _native.synthetic_triples_host(N, R0, E, 0)
    tp = torch.from_numpy(_native.add_inverse_and_self_host(T, N, R0))
    R = 2 * R0 + 1
    l1 = _nc(tp, N, R, 16, 16, vertical=False, seed=11)
    l2 = _nc(tp, N, R, 16, 16, vertical=True, seed=12)
    X = torch.randn(N, 16, device=DEV).to(BF)
    G = torch.randn(N, 16, device=DEV).to(BF)
    _compare(l1, X, G, expect=NATIVE)

    def step(x):
        x = x.detach().clone().requires_grad_(True)
        l1.zero_grad(set_to_none=True)
        l2.zero_grad(set_to_none=True)
        out = l2(l1.forward_activated(x, "relu", private=True))
        loss = out.float().pow(2).mean()
        loss.backward()
        return loss.detach(), x.grad.float(), [p.grad.float() for p in (*l1.parameters(), *l2.parameters())]
    loss, dX, gr = step(X)
    loss32, dX32, gr32 = step(X.float())
    assert abs(loss.item() - loss32.item()) <= 2e-2 * abs(loss32.item())
    assert rel(dX, dX32) <= 2e-2
    for a, b in zip(gr, gr32):
        assert rel(a, b) <= 2e-2


def test_errors_and_deterministic_upcast():
    from torch_rgcn import _native
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    N, R0, E = 3000, 4, 20_000
    tp, R = _graph(N, R0, E, seed=740)
    layer = _nc(tp, N, R, 16, 16, seed=3)
    X = torch.randn(N, 16, device=DEV)
    with pytest.raises(TypeError, match="bfloat16"):
        layer(X.half())
    layer_bf = _nc(tp, N, R, 16, 16, seed=3).to(BF)
    with pytest.raises(TypeError, match="bfloat16"):
        layer_bf(X)                                   # fp32 features, bf16 parameters
    fl = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=R, in_features=None, out_features=8).to(DEV).to(BF)
    with pytest.raises(TypeError, match="float32"):
        fl()
    # deterministic: the upcast route, bit-reproducible
    big, Rb = _graph(N70, 5, E70, seed=741)
    with routes.override(deterministic="1"):
        lay = _nc(big, N70, Rb, 16, 16, seed=3)
        Xb = torch.randn(N70, 16, device=DEV).to(BF)
        Gb = torch.randn(N70, 16, device=DEV).to(BF)
        _native.profile_start()
        a = _run(lay, Xb, Gb)
        tags = set(_native.profile_stop())
        b = _run(lay, Xb, Gb)
    assert not (set(NATIVE) & tags), sorted(tags)
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int16), b[1].view(torch.int16))
    assert torch.equal(a[2]["weights"], b[2]["weights"])
