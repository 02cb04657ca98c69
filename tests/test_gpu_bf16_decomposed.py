"""bf16 storage for block-diagonal and diagonal layers without dense weights: the bf16 forms of the block / diagonal CSR
kernels (rgcn_block_spmm_bf16, rgcn_block_wgrad_bf16, rgcn_diag_spmm_bf16, rgcn_diag_wgrad_bf16).

Criteria as in test_gpu_bf16.py.  The reference is the layer's own fp32 route on the widened inputs: the fp32 block / diagonal kernels, of which
the bf16 kernels are storage twins (same products, same sum order).  out / dX are bf16, equal to the rounded fp32 result in >= 99.9 % of the
elements and at most one bf16 ulp off elsewhere; the cancellation allowance applies only where hub pieces (fp32 atomics in arrival order) or
the LP layer's self-loop sum change the order.  fp32 parameter gradients within 1e-4 relative, bf16 ones within 2^-7 and in the parameter's
dtype.  Every route test asserts the new profile tags and the absence of the fp32 / dense-weight ones."""
import copy

import numpy as np
import pytest
import torch
from torch_rgcn import routes  # noqa: E402

from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16

BLOCK = ("block_spmm_bf16", "block_wgrad_bf16")
DIAG = ("diag_spmm_bf16", "diag_wgrad_bf16")
# the fp32 kernels, the dense-weight bf16 kernels and the gather-GEMM of the upcast route
FORBID = ("block_spmm", "block_wgrad", "diag_spmm", "diag_wgrad", "spmm", "wgrad", "wgrad_tiled", "colsum", "spmm_blk", "bwd_fused",
          "rel_rows", "segment_sum_wide", "rel_wgrad", "spmm_scatter", "segment_sum", "bwd_scatter_dw", "spmm_bf16", "wgrad_bf16",
          "spmm_blk_bf16", "bwd_own_bf16")
N70, E70 = 70_000, 1_200_000


def _bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32)


def assert_rounded(a, ref32, name, cancel_ok=False):
    """test_gpu_bf16.assert_rounded: a (bf16) = ref32 rounded to bf16, up to one ulp in at most 0.1 % of the elements; cancel_ok: another sum
    order -- an element whose sum cancels may also move by fp32 round-off of the largest element"""
    assert a.dtype == BF and a.shape == ref32.shape, (name, a.dtype, a.shape, ref32.shape)
    r = ref32.to(BF)
    same = (a == r) | (torch.isnan(a) & torch.isnan(r))
    frac = same.float().mean().item()
    ulp = (_bits(a) - _bits(r)).abs()
    cancel = ((a.float() - ref32).abs() <= 2 ** -16 * float(ref32.abs().max())) & cancel_ok
    print(f"{name}: {100 * frac:.4f} % equal, max ulp {int(ulp.max())}")
    assert frac >= 0.999, f"{name}: {100 * frac:.3f} % equal to the rounded fp32 result"
    assert bool(((ulp <= 1) | same | cancel).all()), f"{name}: more than one bf16 ulp off (max {int(ulp.max())})"


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


_GRAPHS = {}


def _graph(N, R0, E, seed, hub=False):
    key = (N, R0, E, seed, hub)
    if key not in _GRAPHS:
        T = oracle.synthetic_triples(N, R0, E, seed=seed)
        if hub:          # a destination (and source) with many messages: its row is cut into pieces that different lane groups sum
            rng = np.random.default_rng(seed)
            h = np.stack([np.zeros(40_000, np.int64), rng.integers(0, R0, 40_000), rng.integers(0, N, 40_000)], 1)
            T = np.concatenate([T, h.astype(T.dtype)])
        _GRAPHS[key] = (oracle.add_inverse_and_self(T, N, R0), 2 * R0 + 1)
    tp, R = _GRAPHS[key]
    return torch.from_numpy(tp), R


def _block_layer(tp, N, R, nb, bi, bo, bias=True, seed=0, pdtype=torch.float32):
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.manual_seed(seed)
    layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=R, in_features=nb * bi, out_features=nb * bo, bias=bias,
                                         decomposition={"type": "block", "num_blocks": nb}).to(DEV)
    if bias:
        with torch.no_grad():
            layer.bias.normal_()
    return layer.to(pdtype)


def _diag_layer(tp, N, R, d, seed=0, pdtype=torch.float32):
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.manual_seed(seed)
    return RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=R, in_features=d, out_features=d,
                                        diag_weight_matrix=True).to(DEV).to(pdtype)


def _run(layer, X, G, relu=False):
    X = X.detach().clone().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    out = layer.forward_activated(X, "relu", private=True) if relu else layer(X)
    out.backward(G.to(out.dtype))
    return out.detach(), X.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


def _compare(layer, X16, G16, relu=False, expect=None, forbid=FORBID, cancel_ok=False):
    """the bf16 run against the fp32 route on the widened inputs (bf16 parameters: on a widened copy of the layer); expect / forbid: profile tags"""
    from torch_rgcn import _native
    _native.profile_start()
    out, dX, grads = _run(layer, X16, G16, relu)
    torch.cuda.synchronize()
    tags = set(_native.profile_stop())
    ref = layer
    if any(p.dtype == BF for p in layer.parameters()):
        # bf16 parameters: a widened copy of the layer ON THE SAME GRAPH (a rebuilt graph may order a row's entries differently: another
        # fp32 sum order, which is not what this comparison is about)
        ref = copy.deepcopy(layer).float()
        ref.triples, ref._graph, ref._graph_key = layer.triples, layer._graph, layer._graph_key
    out32, dX32, grads32 = _run(ref, X16.float(), G16.float(), relu)
    assert_rounded(out, out32, "out", cancel_ok)
    assert_rounded(dX, dX32, "dX", cancel_ok)
    for n, p in layer.named_parameters():
        assert grads[n].dtype == p.dtype, (n, grads[n].dtype, p.dtype)
        if p.dtype == torch.float32:
            err, bound = rel(grads[n], grads32[n]), 1e-4
        else:
            err, bound = rel(grads[n].float(), grads32[n].to(BF).float()), 2 ** -7
        print(f"grad {n}: {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (n, err)
    if expect is not None:
        for t in expect:
            assert t in tags, (t, sorted(tags))
        for t in forbid:
            assert t not in tags, (t, sorted(tags))
    return out, dX, grads, tags


def _xg(N, d_in, d_out, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(N, d_in, device=DEV, generator=g).to(BF), torch.randn(N, d_out, device=DEV, generator=g).to(BF)


SMALL = (3000, 4, 20_000)

# (nb, bi, bo): fixed 4 x 4 (8-byte loads, 32 lanes per message) | 8 x 8 | 2 x 2 (64 lanes per message) | 100 blocks of 5 x 5 (the block
# loop runs twice; 10-byte segments) | run-time sizes 3 x 4 (72 -> 96 features; the backward reads transposed) | width 32
SHAPES = [(20, 4, 4), (10, 8, 8), (40, 2, 2), (100, 5, 5), (24, 3, 4), (8, 4, 4)]


@pytest.mark.parametrize("pdtype", [torch.float32, BF], ids=["p32", "p16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_block_forms(shape, pdtype):
    """every instantiation of block_csr_kernel / block_wgrad_kernel in bf16: bias with the fused ReLU, and no bias"""
    nb, bi, bo = shape
    N = SMALL[0]
    tp, R = _graph(*SMALL, seed=801)
    X, G = _xg(N, nb * bi, nb * bo, seed=nb)
    for bias, relu in ((True, True), (False, False)):
        layer = _block_layer(tp, N, R, nb, bi, bo, bias=bias, seed=nb + bi, pdtype=pdtype)
        expect = BLOCK + (("colsum_bf16",) if bias else ())
        _compare(layer, X, G, relu=relu, expect=expect)


def test_fp32_route_equals_itself():
    """the reference side: the fp32 block route run twice is bit-identical on a graph without hub pieces (so is the bf16 route: the kernels
    are storage twins, and nothing adds in arrival order except the parameter gradients' atomics)"""
    N = SMALL[0]
    tp, R = _graph(*SMALL, seed=801)
    X, G = _xg(N, 80, 80, seed=1)
    layer = _block_layer(tp, N, R, 20, 4, 4, seed=1)
    a, b = _run(layer, X.float(), G.float()), _run(layer, X.float(), G.float())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    a, b = _run(layer, X, G), _run(layer, X, G)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


def test_block_table_in_lds():
    """70 k units and a 5.6 KB block table: block_csr_lds_kernel<4, 4> (persistent workgroups, the table in LDS)"""
    tp, R = _graph(N70, 5, E70, seed=802)
    X, G = _xg(N70, 32, 32, seed=2)
    layer = _block_layer(tp, N70, R, 8, 4, 4, seed=2)
    _compare(layer, X, G, relu=True, expect=BLOCK + ("colsum_bf16",))


def test_block_hub_pieces():
    """hub rows cut into RGCN_U_SHARED pieces: fp32 atomics into the scratch, rounded by the second launch; ReLU applied after the rounding.
    The pieces add in arrival order: two runs agree within 2^-8, no bit-identity"""
    from torch_rgcn import _native
    N, R0, E = 20_000, 133, 160_000
    tp, R = _graph(N, R0, E, seed=711, hub=True)
    layer = _block_layer(tp, N, R, 20, 4, 4, seed=3)
    graph = layer._graph_on(torch.device(DEV))
    assert _native._csr_units(graph.csr("fwd"))[2] > 0 and _native._csr_units(graph.csr("bwd"))[2] > 0, "no hub pieces"
    X, G = _xg(N, 80, 80, seed=3)
    o1 = _compare(layer, X, G, relu=True, expect=BLOCK + ("colsum_bf16",), cancel_ok=True)
    o2 = _compare(layer, X, G, relu=True, expect=BLOCK + ("colsum_bf16",), cancel_ok=True)
    assert rel(o1[0].float(), o2[0].float()) <= 2 ** -8
    assert rel(o1[1].float(), o2[1].float()) <= 2 ** -8


def test_width_16_forced_and_default():
    """block_path=2 / diag_path=2 take the new kernels at width 16 too; without the switch a width-16 layer keeps the soft-window kernels"""
    tp, R = _graph(*SMALL, seed=801)
    N = SMALL[0]
    X, G = _xg(N, 16, 16, seed=4)
    with routes.override(block_path="2"):
        _compare(_block_layer(tp, N, R, 4, 4, 4, seed=4), X, G, relu=True, expect=BLOCK + ("colsum_bf16",))
    with routes.override(diag_path="2"):
        _compare(_diag_layer(tp, N, R, 16, seed=4), X, G, expect=DIAG)
    big, Rb = _graph(N70, 5, E70, seed=802)
    Xb, Gb = _xg(N70, 16, 16, seed=5)
    for layer in (_block_layer(big, N70, Rb, 4, 4, 4, seed=5), _diag_layer(big, N70, Rb, 16, seed=5)):
        _compare(layer, Xb, Gb, expect=("spmm_blk_bf16", "bwd_own_bf16"), forbid=BLOCK + DIAG, cancel_ok=True)


@pytest.mark.parametrize("pdtype", [torch.float32, BF], ids=["p32", "p16"])
@pytest.mark.parametrize("d", [32, 100, 30])
def test_diag_forms(d, pdtype):
    """diagonal weights: 8-byte loads (32, 100), 2-byte loads (rows of 30 are 60 bytes)"""
    N = SMALL[0]
    tp, R = _graph(*SMALL, seed=801)
    X, G = _xg(N, d, d, seed=d)
    _compare(_diag_layer(tp, N, R, d, seed=d, pdtype=pdtype), X, G, expect=DIAG)
    _compare(_diag_layer(tp, N, R, d, seed=d, pdtype=pdtype), X, G, relu=True, expect=DIAG)


def test_diag_hub_pieces():
    from torch_rgcn import _native
    N, R0, E = 20_000, 133, 160_000
    tp, R = _graph(N, R0, E, seed=711, hub=True)
    layer = _diag_layer(tp, N, R, 32, seed=6)
    graph = layer._graph_on(torch.device(DEV))
    assert _native._csr_units(graph.csr("fwd"))[2] > 0 and _native._csr_units(graph.csr("bwd"))[2] > 0, "no hub pieces"
    X, G = _xg(N, 32, 32, seed=6)
    o1 = _compare(layer, X, G, expect=DIAG, cancel_ok=True)
    o2 = _compare(layer, X, G, expect=DIAG, cancel_ok=True)
    assert rel(o1[0].float(), o2[0].float()) <= 2 ** -8
    assert rel(o1[1].float(), o2[1].float()) <= 2 ** -8


# ----------------------------------------------------------------------------- LP layer
LP_N, LP_R0, LP_E, LP_D, LP_NB = 6000, 9, 8000, 80, 20
LP_TAGS = ("block_spmm_bf16", "block_wgrad_bf16", "colsum_bf16", "gemm")


def _lp(self_loop_type="schlichtkrull-dropout"):
    from torch_rgcn.layers import RelationalGraphConvolutionLP
    torch.manual_seed(0)
    ed = {"general": 0.5, "self_loop": 0.2, "self_loop_type": self_loop_type}
    layer = RelationalGraphConvolutionLP(num_nodes=LP_N, num_relations=2 * LP_R0 + 1, in_features=LP_D, out_features=LP_D, edge_dropout=ed,
                                         decomposition={"type": "block", "num_blocks": LP_NB}, w_init="glorot-normal", b_init="zeros").to(DEV)
    with torch.no_grad():
        layer.bias.normal_()
    return layer


def _lp_run(layer, graph, x, g, seed=1):
    torch.manual_seed(seed)          # the node mask and the self-loop dropout draw from the generator: the same draws for both dtypes
    x = x.detach().clone().requires_grad_(True)
    layer.zero_grad(set_to_none=True)
    out = layer(graph, x)
    out.backward(g)
    return out.detach(), x.grad, {n: p.grad.clone() for n, p in layer.named_parameters()}


def _lp_compare(layer):
    from torch_rgcn import _native
    graph = torch.from_numpy(oracle.synthetic_triples(LP_N, LP_R0, LP_E, 5)).to(DEV)
    X, G = _xg(LP_N, LP_D, LP_D, seed=7)
    _native.profile_start()
    out, dX, gr = _lp_run(layer, graph, X, G)
    torch.cuda.synchronize()
    tags = set(_native.profile_stop())
    for t in LP_TAGS:
        assert t in tags, (t, sorted(tags))
    for t in FORBID:
        assert t not in tags, (t, sorted(tags))
    out32, dX32, gr32 = _lp_run(layer, graph, X.float(), G.float())
    assert_rounded(out, out32, "out", cancel_ok=True)
    assert_rounded(dX, dX32, "dX", cancel_ok=True)
    assert set(gr) == {"blocks", "blocks_self", "bias"}
    for n in gr:
        err = rel(gr[n], gr32[n])
        print(f"grad {n}: {err:.3e}")
        assert gr[n].dtype == torch.float32 and err <= 1e-4, (n, err)
    return graph, X, G


def test_lp_eval_and_no_sync():
    """LP block decomposition on a per-call graph (no work units: the rowptr path): block part + self-loop part rounded once, and a step that
    issues no host synchronisation"""
    layer = _lp()
    layer.eval()
    graph, X, G = _lp_compare(layer)
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


def test_lp_training_schlichtkrull_dropout():
    """training mode, schlichtkrull-dropout: the dropout of the self-loop messages is drawn inside the autograd Function with
    torch.native_dropout -- the same draws as the fp32 route's nn.functional.dropout from the same seed (a mismatch fails the comparison)"""
    layer = _lp()
    layer.train()
    _lp_compare(layer)


def test_lp_training_node_keep_mask():
    """training mode with another self_loop_type (self_loop = 0.2): the self-loop messages of the nodes whose loop was dropped are masked"""
    layer = _lp(self_loop_type="other")
    layer.train()
    _lp_compare(layer)


# ----------------------------------------------------------------------------- against the C oracle
@pytest.mark.parametrize("mode", ["block", "diag"])
def test_vs_oracle(mode):
    """out, dX and the parameter gradients within 2^-8 relative of the C oracle on the widened inputs"""
    N, R0, E = SMALL
    T = oracle.synthetic_triples(N, R0, E, seed=801)
    tp = oracle.add_inverse_and_self(T, N, R0)
    R = 2 * R0 + 1
    if mode == "block":
        layer, d, expect, pname = _block_layer(torch.from_numpy(tp), N, R, 20, 4, 4, seed=9), 80, BLOCK, "blocks"
    else:
        layer, d, expect, pname = _diag_layer(torch.from_numpy(tp), N, R, 32, seed=9), 32, DIAG, "weights"
    X, G = _xg(N, d, d, seed=9)
    from torch_rgcn import _native
    _native.profile_start()
    out, dX, grads = _run(layer, X, G)
    tags = set(_native.profile_stop())
    assert set(expect) <= tags and not (set(FORBID) & tags), sorted(tags)
    params = {pname: getattr(layer, pname).detach().cpu().numpy()}
    bias = layer.bias.detach().cpu().numpy() if layer.bias is not None else None
    res = oracle.nc_layer(tp, N, R, X.float().cpu().numpy(), params, mode, bias, False, g=G.float().cpu().numpy())
    assert rel(out.float().cpu(), torch.from_numpy(res["out"])) <= 2 ** -8
    assert rel(dX.float().cpu(), torch.from_numpy(res["dX"])) <= 2 ** -8
    assert rel(grads[pname].cpu(), torch.from_numpy(res["grads"][pname])) <= 2 ** -8
    if bias is not None:
        assert rel(grads["bias"].cpu(), torch.from_numpy(res["db"])) <= 2 ** -8


# ----------------------------------------------------------------------------- fallbacks, errors, C ABI
@pytest.mark.parametrize("how", ["deterministic", "host_graph"])
def test_fallbacks_keep_the_upcast_route(how):
    N = SMALL[0]
    tp, R = _graph(*SMALL, seed=801)
    X, G = _xg(N, 80, 80, seed=10)
    Xd, Gd = _xg(N, 32, 32, seed=10)
    kw = {"deterministic": "1"} if how == "deterministic" else {"graph_build": "host"}
    with routes.override(**kw):
        _compare(_block_layer(tp, N, R, 20, 4, 4, seed=10), X, G, relu=True, expect=(), forbid=BLOCK + DIAG, cancel_ok=True)
        _compare(_diag_layer(tp, N, R, 32, seed=10), Xd, Gd, expect=(), forbid=BLOCK + DIAG, cancel_ok=True)


def test_fp16_features_raise():
    N = SMALL[0]
    tp, R = _graph(*SMALL, seed=801)
    with pytest.raises(TypeError, match="bfloat16"):
        _block_layer(tp, N, R, 20, 4, 4)(torch.randn(N, 80, device=DEV).half())
    with pytest.raises(TypeError, match="bfloat16"):
        _diag_layer(tp, N, R, 32)(torch.randn(N, 32, device=DEV).half())


def test_cabi_argument_checks():
    """9 x 9 blocks: RGCN_EUNSUPPORTED from both block entry points; neither out nor scratch: RGCN_EINVAL"""
    from torch_rgcn import _native
    L = _native.lib()
    EINVAL, EUNSUPPORTED = 1, 5
    n, nb = 8, 2
    z16 = torch.zeros(n * nb * 9, dtype=BF, device=DEV)
    z32 = torch.zeros(3 * nb * 81, device=DEV)
    idx = torch.zeros(64, dtype=torch.int32, device=DEV)
    p, null = _native._dp, None

    def spmm(out, scratch, b):
        return L.rgcn_block_spmm_bf16(p(z16), p(z32), null, out, scratch, null, p(idx), n, 0, p(idx), p(idx), p(z32), n, 3, nb, b, b, 0, null)
    assert spmm(p(z16), p(z32), 9) == EUNSUPPORTED
    assert spmm(null, null, 4) == EINVAL
    assert L.rgcn_block_wgrad_bf16(p(z16), p(z16), p(z32), p(idx), p(idx), p(z32), p(idx), p(idx), 0, 3, nb, 9, 9, null) == EUNSUPPORTED
    assert L.rgcn_diag_spmm_bf16(p(z16), p(z32), null, null, null, p(idx), n, 0, p(idx), p(idx), p(z32), n, 3, 8, null) == EINVAL
    torch.cuda.synchronize()
