"""ComplEx without a GPU: the C surface binds like DistMult's, the argument rules raise before anything touches a device, the model
reads decoder.model, and the float64 reference of the GPU tests (tests/complex_reference.py) agrees with itself."""
import ctypes
import inspect
import warnings

import numpy as np
import pytest
import torch

import complex_reference as cr

TWINS = {"rgcn_complex_fwd_f32": "rgcn_distmult_fwd_f32", "rgcn_complex_fwd_bf16": "rgcn_distmult_fwd_bf16",
         "rgcn_complex_bwd_nodes_f32": "rgcn_distmult_bwd_nodes_f32", "rgcn_complex_bwd_nodes_bf16": "rgcn_distmult_bwd_nodes_bf16",
         "rgcn_complex_bwd_rel_f32": "rgcn_distmult_bwd_rel_bf16", "rgcn_complex_bwd_rel_bf16": "rgcn_distmult_bwd_rel_bf16"}


def test_the_six_entries_bind_like_their_distmult_twins():
    from torch_rgcn import _native
    L = _native.lib()
    raw = ctypes.CDLL(_native._LIB_PATH)
    for name, twin in TWINS.items():
        assert hasattr(raw, name), name
        fn, tw = getattr(L, name), getattr(L, twin)
        assert fn.restype is tw.restype is ctypes.c_int, name
        assert fn.argtypes is not None and list(fn.argtypes) == list(tw.argtypes), (name, fn.argtypes, tw.argtypes)
    assert (_native.QUERY_COMPLEX, _native.DECODERS) == (2, ("distmult", "complex"))


def test_the_header_names_the_query_forms():
    from torch_rgcn import _native
    text = open(_native._HEADER_PATH).read()
    for line in ("#define RGCN_QUERY_TAIL 0", "#define RGCN_QUERY_HEAD 1", "#define RGCN_QUERY_COMPLEX 2"):
        assert text.count(line) == 1, line
    assert "head != 0" not in text


def test_an_odd_width_in_c_is_an_argument_error_with_a_message():
    """NULL tables are never read: the width is refused first where the other arguments are in order"""
    from torch_rgcn import _native
    L = _native.lib()
    one = (ctypes.c_int64 * 3)(0, 0, 0)
    buf = (ctypes.c_float * 16)()
    p, t = ctypes.addressof(buf), ctypes.addressof(one)
    assert L.rgcn_complex_fwd_f32(t, 1, p, p, None, None, None, p, 1, 1, 3, None, None, None, None) == 1
    assert b"even width" in L.rgcn_last_error()
    assert L.rgcn_complex_bwd_nodes_f32(p, p, p, p, p, p, 1, 5, None) == 1 and b"even width" in L.rgcn_last_error()
    assert L.rgcn_complex_bwd_rel_bf16(t, 1, p, p, p, p, None, None, None, 1, 1, 7, None) == 1 and b"even width" in L.rgcn_last_error()


def test_argument_errors_come_before_any_device():
    """CPU tensors: a RuntimeError ("must live on a GPU") would mean the check came too late"""
    from torch_rgcn import functional as F_
    from torch_rgcn.layers import ComplEx
    batch = torch.zeros(2, 3, dtype=torch.long)
    even, odd = (torch.zeros(4, 6), torch.zeros(3, 6)), (torch.zeros(4, 5), torch.zeros(3, 5))
    calls = {"score_all": lambda n, r, **kw: F_.distmult_score_all(batch, False, n, r, **kw),
             "rank_all": lambda n, r, **kw: F_.distmult_rank_all(batch, True, n, r, **kw),
             "topk_all_index": lambda n, r, **kw: F_.distmult_topk_all_index(batch, False, n, r, k=2, filt=None, **kw),
             "softmax_loss": lambda n, r, **kw: F_.distmult_softmax_loss(batch, False, n, r, **kw),
             }
    for name, call in calls.items():
        for bad in ("ComplEx", "transe", None, 2):
            with pytest.raises(ValueError, match="decoder must be one of"):
                call(*even, decoder=bad)
        with pytest.raises(ValueError, match="even"):
            call(*odd, decoder="complex")
    # distmult_topk_all and distmult_bce_loss keep the parameter lists existing tests pin: their ComplEx forms are siblings of the same lists
    for sibling, twin in ((F_.complex_topk_all, F_.distmult_topk_all), (F_.complex_bce_loss, F_.distmult_bce_loss)):
        assert str(inspect.signature(sibling)) == str(inspect.signature(twin))
        with pytest.raises(ValueError, match="even"):
            sibling(batch, False, *odd)
        with pytest.raises(RuntimeError, match="GPU"):
            sibling(batch, False, *even)
    with pytest.raises(ValueError, match="even"):
        F_.complex_score(batch, *odd)
    with pytest.raises(ValueError, match="even"):
        ComplEx(3, 5, 4, 3)
    # an even width and a known decoder pass the rule and stop at the device requirement
    with pytest.raises(RuntimeError, match="GPU"):
        F_.complex_score(batch, *even)
    with pytest.raises(RuntimeError, match="GPU"):
        ComplEx(3, 6, 4, 3)(batch, even[0])


def _predictor(decoder_config, nemb=8):
    from torch_rgcn.models import LinkPredictor
    enc = dict(node_embedding=nemb, hidden1_size=nemb, num_layers=1, weight_init="glorot-normal", bias_init="zeros",
               decomposition=dict(type="basis", num_bases=2), edge_dropout=dict(general=0.0, self_loop=0.0, self_loop_type="schlichtkrull-dropout"))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return LinkPredictor(nnodes=10, nrel=3, encoder_config=enc, decoder_config=decoder_config)


def test_the_model_reads_the_decoder_key():
    from torch_rgcn.layers import ComplEx, DistMult
    for value in ("complex", "Complex", "COMPLEX"):
        m = _predictor(dict(model=value, weight_init="standard-normal"))
        assert type(m.scoring_function) is ComplEx and m.scoring_function.decoder == "complex"
    for cfg in (dict(model="distmult"), dict(), dict(model="transe"), dict(model=None), None):
        m = _predictor(cfg)
        assert type(m.scoring_function) is DistMult and m.scoring_function.decoder == "distmult"
    with pytest.raises(AssertionError, match="even"):
        _predictor(dict(model="complex"), nemb=7)
    assert issubclass(ComplEx, DistMult)


def test_a_state_dict_loads_either_way():
    from torch_rgcn.layers import ComplEx, DistMult
    for b_init in (None, "zeros"):
        a, b = DistMult(3, 6, 4, 3, b_init=b_init), ComplEx(3, 6, 4, 3, b_init=b_init)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb) and all(sa[k].shape == sb[k].shape for k in sa)
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in b.named_parameters()]
        b.load_state_dict(sa)
        a.load_state_dict(b.state_dict())
        assert torch.equal(a.relations, b.relations)


def test_the_configurations_differ_from_their_parents_in_the_decoder_alone():
    import os
    import yaml
    from conftest import PKG
    for child, parent in (("lp-WN18-complex.yaml", "lp-WN18.yaml"), ("lp-WN18-1n-complex.yaml", "lp-WN18-1n.yaml")):
        c = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", child)))
        p = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", parent)))
        assert c["decoder"].pop("model") == "complex" and p["decoder"].pop("model") == "distmult"
        assert c == p and c["encoder"]["node_embedding"] == 200
        assert "EXTENSION" in open(os.path.join(PKG, "configs", "rgcn", child)).readline()


# ----------------------------------------------------------------------------- the reference against itself
def _f64_case(d, seed):
    rng = np.random.default_rng(seed)
    N, Q = 7, 9
    nodes, rel = torch.tensor(rng.standard_normal((N, d))), torch.tensor(rng.standard_normal((cr.R0, d)))
    bias = [torch.tensor(rng.standard_normal(n)) for n in (N, cr.R0, N)]
    triples = np.stack([rng.integers(0, N, Q), rng.integers(0, cr.R0, Q), rng.integers(0, N, Q)], 1)
    return nodes, rel, bias, triples


@pytest.mark.parametrize("d", [2, 6, 8])
def test_reference_complex_form_is_the_expanded_real_form(d):
    nodes, rel, bias, triples = _f64_case(d, d)
    a, b = cr.triple_scores(triples, nodes, rel), cr.expanded_real_scores(triples, nodes, rel)
    assert (a - b).abs().max() <= 1e-12 * b.abs().max()
    with_b = cr.triple_scores(triples, nodes, rel, bias)
    s, p, o = (torch.as_tensor(triples[:, k]) for k in range(3))
    assert (with_b - (a + bias[0][s] + bias[1][p] + bias[2][o])).abs().max() <= 1e-12


@pytest.mark.parametrize("head", [False, True])
@pytest.mark.parametrize("d", [2, 6])
def test_reference_query_vectors_reproduce_the_scores(d, head):
    """Re(e_s r conj(e_o)) = Re(z_tail conj(e_o)) = Re(e_s conj(z_head)): every candidate's score is a plain dot product with qv"""
    nodes, rel, bias, batch = _f64_case(d, 10 + d)
    qv = cr.query_vectors(batch, head, nodes, rel)
    want = cr.all_scores(batch, head, nodes, rel)
    assert ((qv @ nodes.T) - want).abs().max() <= 1e-12 * want.abs().max()
    # and the cell of a query's own target is the triple's score, biases included
    cells = cr.all_scores(batch, head, nodes, rel, bias)[torch.arange(len(batch)), torch.as_tensor(batch[:, 0 if head else 2])]
    assert (cells - cr.triple_scores(batch, nodes, rel, bias)).abs().max() <= 1e-12 * want.abs().max()
    # the expanded forms the header states, term by term
    h = d // 2
    a, r = nodes[batch[:, 2 if head else 0]], rel[batch[:, 1]]
    a_re, a_im, r_re, r_im = a[:, :h], a[:, h:], r[:, :h], r[:, h:]
    stated = torch.cat((r_re * a_re + r_im * a_im, r_re * a_im - r_im * a_re) if head else
                       (a_re * r_re - a_im * r_im, a_re * r_im + a_im * r_re), 1)
    assert (stated - qv).abs().max() <= 1e-12


def test_reference_gradient_identities_hold_against_autograd():
    nodes, rel, _, triples = _f64_case(6, 3)
    triples = triples[:1]
    s, p, o = (int(v) for v in triples[0])
    if s == o:
        o = (s + 1) % nodes.shape[0]
        triples[0, 2] = o
    n, r = nodes.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    cr.triple_scores(triples, n, r).sum().backward()
    zs, zr, zo = cr.cplx(nodes[s]), cr.cplx(rel[p]), cr.cplx(nodes[o])
    for got, want in ((n.grad[s], zr.conj() * zo), (n.grad[o], zs * zr), (r.grad[p], zs.conj() * zo)):
        assert (got - cr.halves(want)).abs().max() <= 1e-12
    # the chain rule of the query vectors: tail da = g conj(r), dr = g conj(a); head da = r g, dr = a conj(g)
    g = torch.tensor(np.random.default_rng(5).standard_normal((1, 6)))
    for head in (False, True):
        n, r = nodes.clone().requires_grad_(True), rel.clone().requires_grad_(True)
        (cr.query_vectors(triples, head, n, r) * g).sum().backward()
        za, zg = cr.cplx(nodes[o if head else s]), cr.cplx(g[0])
        da, dr = (zr * zg, za * zg.conj()) if head else (zg * zr.conj(), zg * za.conj())
        assert (n.grad[o if head else s] - cr.halves(da)).abs().max() <= 1e-12
        assert (r.grad[p] - cr.halves(dr)).abs().max() <= 1e-12


@pytest.mark.parametrize("head", [False, True])
def test_the_torch_helpers_of_functional_follow_the_reference(head):
    """functional._query_vectors / _query_vectors_grad in float64 on the CPU: the forms the all-candidate backward composes"""
    from torch_rgcn import functional as F_
    nodes, rel, _, batch = _f64_case(6, 21)
    anchor, p = torch.as_tensor(batch[:, 2 if head else 0]), torch.as_tensor(batch[:, 1])
    n32, r32 = nodes.float(), rel.float()
    qv = F_._query_vectors(n32, r32, anchor, p, head, "complex")
    assert qv.dtype == torch.float32 and (qv.double() - cr.query_vectors(batch, head, n32.double(), r32.double())).abs().max() <= 1e-5
    assert torch.equal(F_._query_vectors(n32, r32, anchor, p, head, "distmult"), n32[anchor] * r32[p])
    g = torch.tensor(np.random.default_rng(6).standard_normal(qv.shape))
    n, r = nodes.clone().requires_grad_(True), rel.clone().requires_grad_(True)
    (cr.query_vectors(batch, head, n, r) * g).sum().backward()
    da = torch.zeros_like(nodes).index_add_(0, anchor, F_._query_vectors_grad(g, rel[p], head, "complex", "anchor"))
    dr = torch.zeros_like(rel).index_add_(0, p, F_._query_vectors_grad(g, nodes[anchor], head, "complex", "relation"))
    assert (da - n.grad).abs().max() <= 1e-12 and (dr - r.grad).abs().max() <= 1e-12
    assert torch.equal(F_._query_vectors_grad(g, rel[p], head, "distmult", "anchor"), g * rel[p])
