"""The checks the DistMult all-candidate routes (score_all, rank_fused, topk, lse, softmax_grad) share, each stated once (no GPU, CPU
tensors only): the immediate range check of the triples, the range check of the filter lists, and the widening of bf16-side parameters.
The helpers ask for no device themselves -- that requirement is `_native._req`'s, checked at the end."""
import pytest
import torch

from torch_rgcn import _native, functional

N, N_REL = 10, 3
OK = torch.tensor([[0, 2, 9], [9, 0, 0]], dtype=torch.int64)
RAISES = ((False, AssertionError), (True, IndexError))          # storage (bf16?) -> what its out-of-range triples raise


def with_cell(row, col, value):
    batch = OK.clone()
    batch[row, col] = value
    return batch


@pytest.mark.parametrize("bf16", (False, True))
def test_triples_in_range_pass(bf16):
    assert _native._triples_in_range(OK, N, N_REL, bf16) is None


@pytest.mark.parametrize("bf16,exc", RAISES)
@pytest.mark.parametrize("row,col,value", ((0, 1, N_REL), (1, 1, N_REL), (0, 0, N), (1, 0, N), (0, 2, N), (1, 2, N),
                                           (0, 0, -1), (1, 1, -1), (0, 2, -1)))
def test_a_triple_out_of_range_raises_by_storage(bf16, exc, row, col, value):
    with pytest.raises(exc):
        _native._triples_in_range(with_cell(row, col, value), N, N_REL, bf16)


@pytest.mark.parametrize("bf16", (False, True))
def test_an_empty_batch_passes_untouched(bf16):
    class Untouchable:
        shape = (0, 3)

        def __getattr__(self, name):
            raise AssertionError(f"an empty batch was asked for .{name}")

    assert _native._triples_in_range(Untouchable(), N, N_REL, bf16) is None
    assert _native._triples_in_range(torch.empty(0, 3, dtype=torch.int64), N, N_REL, bf16) is None


def lists(q, n):
    return torch.tensor(q, dtype=torch.int32), torch.tensor(n, dtype=torch.int32)


def test_filter_lists_in_range_pass():
    assert _native._filter_lists_in_range(*lists([0, 1, 1], [0, 9, 4]), 2, N) is None
    assert _native._filter_lists_in_range(None, None, 2, N) is None                      # no filter
    assert _native._filter_lists_in_range(*lists([], []), 2, N) is None                  # an empty one


@pytest.mark.parametrize("q,n", (([0, 2], [1, 1]), ([-1, 0], [1, 1]), ([0, 1], [1, N]), ([0, 1], [-1, 1])))
def test_a_filter_entry_out_of_range_raises_index_error(q, n):
    with pytest.raises(IndexError):
        _native._filter_lists_in_range(*lists(q, n), 2, N)


def test_checked_queries_runs_both_checks_eagerly():
    fq, fn = lists([0, 1], [3, 4])
    assert _native.checked_queries(OK, N, N_REL, fq, fn, False) is OK
    with pytest.raises(AssertionError):
        _native.checked_queries(with_cell(0, 1, N_REL), N, N_REL, None, None, False)
    with pytest.raises(IndexError):
        _native.checked_queries(with_cell(0, 1, N_REL), N, N_REL, None, None, True)
    with pytest.raises(IndexError):
        _native.checked_queries(OK, N, N_REL, *lists([0, 2], [3, 4]), False)


def params(dtype, bias_dtype=None):
    nodes, rel = torch.zeros(N, 4, dtype=dtype), torch.zeros(N_REL, 4, dtype=dtype)
    if bias_dtype is None:
        return nodes, rel, None, None, None
    return nodes, rel, torch.zeros(N, dtype=bias_dtype), torch.zeros(N_REL, dtype=bias_dtype), torch.zeros(N, dtype=bias_dtype)


def test_widen_leaves_fp32_parameters_alone():
    for p in (params(torch.float32), params(torch.float32, torch.float32)):
        out = functional._widen_query_params(*p)
        assert len(out) == 4 and all(a is b for a, b in zip(out, p[1:]))


def test_widen_makes_bf16_parameters_fp32():
    nodes, rel, sb, pb, ob = params(torch.bfloat16, torch.bfloat16)
    rel.fill_(1.5)
    out = functional._widen_query_params(nodes, rel, sb, pb, ob)
    assert [t.dtype for t in out] == [torch.float32] * 4 and torch.equal(out[0], rel.float())
    assert nodes.dtype == torch.bfloat16                                                  # the entity table is not this function's
    rel32 = rel.float()                                                                   # fp32 parameters beside bf16 nodes: unchanged
    same = functional._widen_query_params(nodes, rel32, None, None, None)
    assert same[0] is rel32 and same[1:] == (None, None, None)


@pytest.mark.parametrize("which", ("relations", "sbias", "pbias", "obias"))
def test_widen_names_a_parameter_of_another_type(which):
    p = dict(zip(("nodes", "relations", "sbias", "pbias", "obias"), params(torch.bfloat16, torch.float32)))
    p[which] = p[which].to(torch.float16)
    with pytest.raises(TypeError, match=f"{which} must be torch.float32 or torch.bfloat16, got torch.float16"):
        functional._widen_query_params(**p)


def test_the_device_requirement_stays_with_req():
    nodes, rel, sb, pb, ob = params(torch.float32, torch.float32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _native._req_queries(OK, nodes, rel, sb, pb, ob, False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                            # before any assert: the widths differ here
        _native._req_queries(OK, nodes, rel[:, :2], None, None, None, False)
