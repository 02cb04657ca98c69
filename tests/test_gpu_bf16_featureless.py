"""bf16 storage for featureless layers with basis decomposition: a bf16 bases table in, bf16 out and dbases, fp32 arithmetic
(fp64 where the tile kernels sum in LDS doubles), one rounding.

The fp32 reference is the same layer run on the widened parameters, with the fp32 route pinned to the same tile kernels
(fbasis_inplace_mb=0); one small case goes to the C oracle directly.  Criteria as tests/test_gpu_bf16.py: out / dbases equal the rounded fp32
result in >= 99.9 % of the elements and differ by at most one bf16 ulp elsewhere (hub rows are summed with fp32 atomics in arrival order:
cancel_ok); dcomps / db within 1e-4 relative for fp32 parameters, 2^-8 for bf16 ones; gradient dtypes = parameter dtypes."""
import copy

import numpy as np
import pytest
import torch
from torch_rgcn import routes  # noqa: E402

from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
BF16_TAGS = ("fbasis_tile_fwd_bf16", "gather_rows_sum4_bf16", "fbasis_tile_bwd_bf16")
FP32_TILE_TAGS = ("fbasis_tile_fwd", "fbasis_tile_bwd")


def _bits(t):
    return t.contiguous().view(torch.int16).to(torch.int32)


def assert_rounded(a, ref32, name, cancel_ok=False):
    """a (bf16) = ref32 rounded to bf16, up to one ulp in at most 0.1 % of the elements (tests/test_gpu_bf16.py)"""
    assert a.dtype == BF and a.shape == ref32.shape, (name, a.dtype, a.shape, ref32.shape)
    r = ref32.to(BF)
    same = (a == r) | (torch.isnan(a) & torch.isnan(r))
    frac = same.float().mean().item()
    ulp = (_bits(a) - _bits(r)).abs()
    cancel = ((a.float() - ref32).abs() <= 2 ** -16 * float(ref32.abs().max())) & cancel_ok
    assert frac >= 0.999, f"{name}: {100 * frac:.3f} % equal to the rounded fp32 result"
    assert bool(((ulp <= 1) | same | cancel).all()), f"{name}: more than one bf16 ulp off (max {int(ulp.max())})"


def rel(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).abs().max() / max(float(b.abs().max()), 1e-30))


def _graph(N, R0, E, seed, hub=True):
    """run_layer_vs_oracle's hub pattern: node 1 the subject of E / 5 triples (a hub destination whose row is cut into shared units, and a hub
    source through the inverse messages), a run of duplicate triples"""
    T = oracle.synthetic_triples(N, R0, E, seed=seed)
    if hub and E > 50:
        T[: E // 5, 0] = 1
        T[E // 5: E // 4] = T[0]
    return oracle.add_inverse_and_self(T, N, R0), 2 * R0 + 1


def _fl(tp, N, R, B, d, bias=True, seed=0):
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.manual_seed(seed)
    layer = RelationalGraphConvolutionNC(triples=torch.from_numpy(tp), num_nodes=N, num_relations=R, in_features=None, out_features=d,
                                         bias=bias, decomposition={"type": "basis", "num_bases": B}).to(DEV)
    if bias:
        with torch.no_grad():
            layer.bias.normal_()
    return layer


def _run(layer, G, relu=None):
    """(out, {param: grad}) of one forward / backward with upstream gradient G; relu: None, or the `private` flag of forward_activated"""
    layer.zero_grad(set_to_none=True)
    out = layer() if relu is None else layer.forward_activated(None, "relu", private=relu)
    out.backward(G.to(out.dtype))
    return out.detach(), {n: p.grad.clone() for n, p in layer.named_parameters()}


def _compare(layer, G, relu=None, expect=BF16_TAGS, forbid=FP32_TILE_TAGS, cancel_ok=True, sample=None):
    """the layer (bf16 bases) against a copy of it in fp32 on the fp32 tile route; expect / forbid: profile tags of the bf16 run"""
    from torch_rgcn import _native
    ref = copy.deepcopy(layer).float()
    _native.profile_start()
    out, grads = _run(layer, G, relu)
    torch.cuda.synchronize()
    tags = set(_native.profile_stop())
    with routes.override(fbasis_inplace_mb="0"):
        out32, grads32 = _run(ref, G.float(), relu)
    assert out.dtype == BF
    assert_rounded(out, out32, "out", cancel_ok)
    for n, p in layer.named_parameters():
        assert grads[n].dtype == p.dtype, (n, grads[n].dtype, p.dtype)
        if n == "bases":
            a, b = (grads[n], grads32[n]) if sample is None else (grads[n][:, sample], grads32[n][:, sample])
            assert_rounded(a, b, "dbases", cancel_ok)
        else:
            assert rel(grads[n].float(), grads32[n].float()) <= (1e-4 if p.dtype == torch.float32 else 2 ** -8), n
    for t in expect:
        assert t in tags, (t, sorted(tags))
    for t in forbid:
        assert t not in tags, (t, sorted(tags))
    return out, grads, tags


SHAPES = [(3000, 40, 10), (3001, 40, 10), (2999, 30, 16), (1000, 4, 4), (777, 7, 3), (4000, 13, 8), (16, 5, 10)]


@pytest.mark.parametrize("mode", ["ranges", "nodes", "nodes2"])
@pytest.mark.parametrize("N,B,d", SHAPES)
def test_tile_kernels_each_mode(mode, N, B, d):
    """the bf16 tile kernels in every mode on the shapes of test_featureless_basis_tile_kernels_vs_oracle: node counts off the 16-node grid, N d
    off the 4-element grid (scalar staging), a hub source and a hub destination (shared units: the fp32 scratch and the rounding launch)"""
    tp, R = _graph(N, 6, 10 * N, seed=B * 37 + d)
    layer = _fl(tp, N, R, B, d, seed=B + d)
    layer.bases.data = layer.bases.data.to(BF)
    if N >= 777:
        assert layer._graph_on(torch.device(DEV)).fbasis_plan().units_dst[2] > 0, "no shared destination units"
    G = torch.randn(N, d, device=DEV)
    with routes.override(fbasis_tile=mode):
        _compare(layer, G.to(BF))


def test_tile_refused_shape_takes_the_upcast_route():
    """(B, d) = (64, 11) in ranges mode: two tiles of doubles exceed the LDS -- the fp32 route on the widened parameters, output rounded"""
    N, B, d = 3000, 64, 11
    tp, R = _graph(N, 6, 10 * N, seed=B * 37 + d)
    layer = _fl(tp, N, R, B, d, seed=1).to(BF)
    G = torch.randn(N, d, device=DEV).to(BF)
    with routes.override(fbasis_tile="ranges"):
        _compare(layer, G, expect=(), forbid=BF16_TAGS)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("params", ["bases_only", "all"])
def test_parameter_mixes(params, bias):
    """bf16 bases with fp32 comps and bias, and a fully .bfloat16() layer; with and without a bias"""
    N, B, d = 3000, 40, 10
    tp, R = _graph(N, 6, 10 * N, seed=5)
    layer = _fl(tp, N, R, B, d, bias=bias, seed=2)
    if params == "all":
        layer = layer.to(BF)
    else:
        layer.bases.data = layer.bases.data.to(BF)
    _compare(layer, torch.randn(N, d, device=DEV).to(BF))


@pytest.mark.parametrize("private", [False, True])
def test_relu(private):
    """forward_activated(None, "relu"): the ReLU before the one rounding (= after it); the gradient through the mask (threshold_backward on
    bf16, exact)"""
    N, B, d = 3000, 40, 10
    tp, R = _graph(N, 6, 10 * N, seed=6)
    layer = _fl(tp, N, R, B, d, seed=3).to(BF)
    out, grads, _ = _compare(layer, torch.randn(N, d, device=DEV).to(BF), relu=private)
    assert bool((out >= 0).all()) and bool((out == 0).any())
    ref = copy.deepcopy(layer).float()
    with torch.no_grad(), routes.override(fbasis_inplace_mb="0"):
        plain32 = ref()
    assert_rounded(out, torch.relu(plain32), "relu(out)", cancel_ok=True)


@pytest.mark.parametrize("case", ["deterministic", "B65", "d17", "fbasis_tile0"])
def test_upcast_routes(case):
    """RGCN_DETERMINISTIC=1 (bit-reproducible), B = 65, d = 17, fbasis_tile=0: the fp32 route on the widened parameters, no bf16 tile tag"""
    from torch_rgcn import _native
    N = 2000
    B, d = {"B65": (65, 8), "d17": (8, 17)}.get(case, (40, 10))
    tp, R = _graph(N, 6, 10 * N, seed=7)
    ov = {"deterministic": dict(deterministic="1"), "fbasis_tile0": dict(fbasis_tile="0")}.get(case, {})
    with routes.override(**ov):
        layer = _fl(tp, N, R, B, d, seed=4).to(BF)
        G = torch.randn(N, d, device=DEV).to(BF)
        _native.profile_start()
        a = _run(layer, G)
        tags = set(_native.profile_stop())
        assert not (set(BF16_TAGS) & tags), sorted(tags)
        ref = copy.deepcopy(layer).float()
        out32, g32 = _run(ref, G.float())
        if case == "deterministic":
            b = _run(layer, G)
    assert_rounded(a[0], out32, "out", cancel_ok=True)
    for n in a[1]:
        assert a[1][n].dtype == BF and rel(a[1][n].float(), g32[n].to(BF).float()) <= 2 ** -7, n
    if case == "deterministic":
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
        for n in a[1]:
            assert torch.equal(a[1][n].view(torch.int16), b[1][n].view(torch.int16)), n


def test_errors():
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    N = 500
    tp, R = _graph(N, 3, 2000, seed=8)
    tpt = torch.from_numpy(tp)
    fl = RelationalGraphConvolutionNC(triples=tpt, num_nodes=N, num_relations=R, in_features=None, out_features=8).to(DEV).to(BF)
    with pytest.raises(TypeError, match="float32"):
        fl()
    blk = RelationalGraphConvolutionNC(triples=tpt, num_nodes=N, num_relations=R, in_features=None, out_features=8,
                                       decomposition={"type": "block", "num_blocks": 2}).to(DEV).to(BF)
    with pytest.raises(TypeError, match="float32"):
        blk()
    mix = _fl(tp, N, R, 4, 8)
    mix.comps.data = mix.comps.data.to(BF)
    with pytest.raises(TypeError, match="bases"):
        mix()
    half = _fl(tp, N, R, 4, 8).half()
    with pytest.raises(TypeError):
        half()
    vert = RelationalGraphConvolutionNC(triples=tpt, num_nodes=N, num_relations=R, in_features=None, out_features=8, vertical_stacking=True,
                                        decomposition={"type": "basis", "num_bases": 4}).to(DEV).to(BF)
    with pytest.raises(RuntimeError):
        vert()


def test_small_case_vs_oracle():
    """out, dbases, dcomps and db within 2^-8 relative of the C oracle evaluated on the widened parameters (tile route)"""
    from torch_rgcn import _native
    N, B, d = 3000, 30, 16
    tp, R = _graph(N, 5, 30_000, seed=9, hub=False)
    layer = _fl(tp, N, R, B, d, seed=5).to(BF)
    G = torch.randn(N, d, device=DEV).to(BF)
    _native.profile_start()
    out, grads = _run(layer, G)
    tags = set(_native.profile_stop())
    assert set(BF16_TAGS) <= tags, sorted(tags)
    params = {"bases": layer.bases.detach().float().cpu().numpy(), "comps": layer.comps.detach().float().cpu().numpy()}
    ref = oracle.nc_layer(tp, N, R, None, params, "basis", layer.bias.detach().float().cpu().numpy(), False, G.float().cpu().numpy())
    assert rel(out.float().cpu(), torch.from_numpy(ref["out"])) <= 2 ** -8
    for n in ("bases", "comps"):
        assert rel(grads[n].float().cpu(), torch.from_numpy(ref["grads"][n])) <= 2 ** -8, n
    assert rel(grads["bias"].float().cpu(), torch.from_numpy(ref["db"])) <= 2 ** -8


def _model(shape, B, nhid, nclass, seed):
    from torch_rgcn.models import NodeClassifier
    T = oracle.synthetic_triples(shape["N"], shape["R0"], shape["E"], seed=seed)
    torch.manual_seed(seed)
    return NodeClassifier(triples=torch.from_numpy(T), nnodes=shape["N"], nrel=shape["R0"], nfeat=None, nhid=nhid, nclass=nclass,
                          decomposition={"type": "basis", "num_bases": B}).to(DEV)


def _step(model):
    model.zero_grad(set_to_none=True)
    out = model()
    loss = out.float().pow(2).mean()
    loss.backward()
    return out.detach().float(), [p.grad.float() for p in model.parameters()]


MUTAG = dict(N=23_644, R0=23, E=74_227)
AM10 = dict(N=166_676, R0=133, E=598_832)


@pytest.mark.parametrize("shape,B,nhid,nclass", [(MUTAG, 30, 16, 2), (AM10, 40, 10, 11)], ids=["mutag", "am_tenth"])
def test_models(shape, B, nhid, nclass):
    """NodeClassifier(nfeat=None, basis).to(bfloat16): layer 1 on the new route, layer 2 on the featured bf16 route; logits and every parameter
    gradient against the fp32 model on the widened parameters"""
    from torch_rgcn import _native
    model = _model(shape, B, nhid, nclass, seed=11).to(BF)
    ref = copy.deepcopy(model).float()
    _native.profile_start()
    out, gr = _step(model)
    tags = set(_native.profile_stop())
    assert set(BF16_TAGS) <= tags, sorted(tags)
    assert {"spmm_bf16", "spmm_blk_bf16"} & tags, sorted(tags)
    out32, gr32 = _step(ref)
    assert rel(out, out32) <= 2e-2
    for (n, _), a, b in zip(model.named_parameters(), gr, gr32):
        assert rel(a, b) <= 2e-2, n


def test_capture_mutag_model():
    """one bf16 forward + backward of the MUTAG-shaped model captured with torch.cuda.graph after eager warm-up: the replay agrees with eager
    (within 2e-2: the LDS double adds are not bit-reproducible)"""
    model = _model(MUTAG, 30, 16, 2, seed=12).to(BF)
    out_e, gr_e = _step(model)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            _step(model)
    torch.cuda.current_stream().wait_stream(s)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out_c = model()
        out_c.float().pow(2).mean().backward()
    for p in model.parameters():
        p.grad.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert rel(out_c.float(), out_e) <= 2e-2
    for (n, p), b in zip(model.named_parameters(), gr_e):
        assert rel(p.grad.float(), b) <= 2e-2, n


def test_full_size_am_layer1():
    """AM as shipped, layer 1 (N = 1,666,764, R = 267, basis 40, hidden 10: a 1.33 GB bf16 table): one bf16 forward + backward against the fp32
    layer on the widened bases -- the whole output, and the dbases rows of 2,000 sampled nodes"""
    N, R0, E = 1_666_764, 133, 5_988_321
    T = oracle.synthetic_triples(N, R0, E, seed=2)
    tp = oracle.add_inverse_and_self(T, N, R0)
    layer = _fl(tp, N, 2 * R0 + 1, 40, 10, seed=13)
    layer.bases.data = layer.bases.data.to(BF)
    G = torch.randn(N, 10, device=DEV).to(BF)
    sample = torch.from_numpy(np.random.default_rng(2).choice(N, 2000, replace=False)).to(DEV)
    _compare(layer, G, sample=sample)
