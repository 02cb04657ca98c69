"""Host side of the filter block of the all-candidate entry points (no GPU): one entry point per role and storage, each taking the
filter as lists or as an index in the same seven arguments behind obias; the binding hands every one of them the block its caller's
arguments describe, under the profile tag of that role, filter form and storage."""
import types

import pytest
import torch

from test_cabi_symbols import declared_prototypes
from torch_rgcn import _native

ROLES = ["rank_fused", "topk", "lse", "lse_smooth", "softmax_grad", "softmax_grad_smooth"]
FILTERED = [f"rgcn_distmult_{role}_{st}" for role in ROLES + ["bce_sums", "bce_grad"] for st in ("f32", "bf16")]
BLOCK = ["const int32_t *filt_q", "const int32_t *filt_n", "int64_t F", "const int64_t *fkeys", "const int64_t *fptr", "const int32_t *fvals",
         "int64_t K"]


def test_the_header_declares_one_entry_point_per_role_and_storage():
    protos = declared_prototypes()
    for role in ROLES:
        for st in ("f32", "bf16"):
            assert f"rgcn_distmult_{role}_index_{st}" not in protos
            assert f"rgcn_distmult_{role}_{st}" in protos
    assert not [n for n in protos if n.startswith("rgcn_distmult_") and "_index_" in n]
    assert "rgcn_distmult_softmax_grad_bf16_workspace_bytes" not in protos
    assert protos["rgcn_distmult_softmax_grad_workspace_bytes"][1] == ["int64_t Q", "int64_t c_count", "int32_t d", "int32_t bf16"]


@pytest.mark.parametrize("name", FILTERED)
def test_the_filter_block_sits_directly_behind_obias(name):
    params = declared_prototypes()[name][1]
    at = params.index("const float *obias") + 1
    assert at == 8 and params[at:at + 7] == BLOCK, (name, params)
    assert sum(p.split()[-1].lstrip("*") in ("filt_q", "filt_n", "F", "fkeys", "fptr", "fvals", "K") for p in params) == 7       # and only there


# ----------------------------------------------------------------------------- the binding: tags and blocks, on CPU tensors
class FakeLib:
    """stands where _native.lib() does: every entry point records its arguments and returns OK, every size is 16 bytes"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *a: 16

        def entry(*args):
            self.calls.append((name, args))
            return _native.OK
        return entry


class Tag:
    def __init__(self, tags, name):
        tags.append(name)

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


@pytest.fixture
def bound(monkeypatch):
    fake, tags = FakeLib(), []
    monkeypatch.setattr(_native, "lib", lambda: fake)
    monkeypatch.setattr(_native, "_timed", lambda name: Tag(tags, name))
    monkeypatch.setattr(_native, "_req", lambda *a, **k: None)              # the one requirement CPU tensors miss: a device
    monkeypatch.setattr(_native, "_stream", lambda device: 0)
    return fake, tags


N, D, Q = 10, 8, 2
BATCH = torch.tensor([[0, 1, 2], [3, 2, 4]])
REL = torch.randn(3, D)
FQ, FN = torch.tensor([0, 1], dtype=torch.int32), torch.tensor([5, 6], dtype=torch.int32)
KEYS, PTR, VALS = torch.tensor([12, 24]), torch.tensor([0, 1, 2]), torch.tensor([5, 6], dtype=torch.int32)
INDEX = types.SimpleNamespace(num_nodes=N, device=BATCH.device, tables=[(KEYS, PTR, VALS), (KEYS, PTR, VALS)])


def filter_kwargs(form, lists=("filt_q", "filt_n"), index="filt"):
    """-> (keyword arguments of the wrapper, the block the entry point must receive)"""
    if form == "lists":
        return {lists[0]: FQ, lists[1]: FN}, (FQ.data_ptr(), FN.data_ptr(), 2, None, None, None, 0)
    if form == "index":
        return {index: INDEX}, (None, None, 0, KEYS.data_ptr(), PTR.data_ptr(), VALS.data_ptr(), 2)
    return {}, (None, None, 0, None, None, None, 0)


def strip_roles(nodes, kw):
    lse, g = torch.zeros(Q), torch.ones(1)
    keep, uni = torch.full((1,), 0.75), torch.full((Q,), 0.025)
    grad = (BATCH, True, nodes, REL, None, None, None, kw.get("filt_q"), kw.get("filt_n"), lse, g, Q, 0, N)
    return [("rank_fused", "rank_fused", lambda: _native.distmult_rank_fused(BATCH, True, nodes, REL, **kw)),
            ("topk_fused", "topk", lambda: _native._distmult_topk(BATCH, True, nodes, REL, None, None, None, 3, kw.get("filt_q"),
                                                                   kw.get("filt_n"), 0, kw.get("filt"), "distmult")),
            ("lse_fused", "lse", lambda: _native.distmult_lse(BATCH, True, nodes, REL, **kw)),
            ("lse_smooth", "lse_smooth", lambda: _native.distmult_lse_smooth(BATCH, True, nodes, REL, **kw)),
            ("softmax_grad", "softmax_grad", lambda: _native.distmult_softmax_grad(*grad, filt=kw.get("filt"))),
            ("softmax_grad_smooth", "softmax_grad_smooth", lambda: _native.distmult_softmax_grad(*grad, filt=kw.get("filt"), keep=keep, uni=uni))]


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("form", ["none", "lists", "index"])
def test_every_filtered_wrapper_passes_the_block_under_the_composed_tag(bound, form, bf16):
    fake, tags = bound
    nodes = torch.randn(N, D).to(torch.bfloat16 if bf16 else torch.float32)
    kw, block = filter_kwargs(form)
    for tag, role, call in strip_roles(nodes, kw):
        del fake.calls[:], tags[:]
        call()
        assert tags == [tag + ("_index" if form == "index" else "") + ("_bf16" if bf16 else "")]
        (name, args), = fake.calls
        assert name == f"rgcn_distmult_{role}_{'bf16' if bf16 else 'f32'}"
        assert args[8:15] == block, (name, args)
        assert len(args) == len(declared_prototypes()[name][1])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("form", ["none", "lists", "index"])
def test_the_bce_wrappers_pass_the_same_block(bound, form, bf16):
    """their tags carry no filter form: bce_sums[_bf16], bce_grad[_bf16]"""
    fake, tags = bound
    nodes = torch.randn(N, D).to(torch.bfloat16 if bf16 else torch.float32)
    kw, block = filter_kwargs(form, lists=("lab_q", "lab_n"), index="labels")
    _native.distmult_bce_sums(BATCH, True, nodes, REL, **kw)
    _native.distmult_bce_grad(BATCH, True, nodes, REL, None, None, None, kw.get("lab_q"), kw.get("lab_n"), torch.ones(1), Q, 0, N,
                              labels=kw.get("labels"))
    sfx = "_bf16" if bf16 else ""
    assert tags == ["bce_sums" + sfx, "bce_grad" + sfx]
    assert [name for name, _ in fake.calls] == [f"rgcn_distmult_bce_{r}_{'bf16' if bf16 else 'f32'}" for r in ("sums", "grad")]
    for name, args in fake.calls:
        assert args[8:15] == block, (name, args)


def test_an_index_beside_the_lists_is_refused_by_the_wrapper(bound):
    nodes = torch.randn(N, D)
    with pytest.raises(AssertionError, match="a FilterIndex or the filter lists, not both"):
        _native.distmult_lse(BATCH, True, nodes, REL, filt_q=FQ, filt_n=FN, filt=INDEX)
    with pytest.raises(AssertionError, match="a FilterIndex or the filter lists, not both"):
        _native.distmult_bce_sums(BATCH, True, nodes, REL, lab_q=FQ, lab_n=FN, labels=INDEX)
    assert not bound[0].calls
