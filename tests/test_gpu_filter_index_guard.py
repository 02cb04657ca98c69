"""The device-resident filter index under guard bands (tests/guard_bands.py): keys, ptr, vals, the mask and the workspaces sit between
poisoned bands at N = 33 (the second mask word holds one column), Q = 3, with one hub key that lists every entity.  Nothing may be stored
outside a buffer, and no band value -- NaN as a float, -1 as an integer -- may reach a result: the results are compared exactly."""
import numpy as np
import pytest
import torch

import guard_bands as gb

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
N, Q, DIM, R0 = 33, 3, 8, 5


def scenario():
    """tail queries with anchors and relations of their own (the backward's last sums then add one row per destination: one answer):
    (0, 1, ?) is the hub key, every entity a known tail; (5, 2, ?) has two known tails, one of them its target; (9, 3, ?) has none"""
    rng = np.random.default_rng(33)
    batch = np.array([[0, 1, 32], [5, 2, 7], [9, 3, 4]])
    known = np.array([(0, 1, c) for c in range(N)] + [(5, 2, 7), (5, 2, 31), (5, 2, 31), (8, 3, 4), (9, 4, 4)])
    nodes = rng.standard_normal((N, DIM)).astype(np.float32)
    rel = rng.standard_normal((R0, DIM)).astype(np.float32)
    bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)]
    return batch, known, nodes, rel, bias


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def index_is_guarded(guard, index):
    for table in index.tables:
        for t in table:
            assert guard._inside(t.data_ptr()), "an index tensor is outside the guarded allocations"


def test_mask_entry_point_under_guard_bands(monkeypatch):
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    from utils.misc import _FilterIndex, generate_true_dict
    batch, known, *_ = scenario()
    true = generate_true_dict(known)
    lists_index = _FilterIndex(true, N)
    got = {}
    with gb.Guard(monkeypatch) as guard:
        index = FilterIndex(true, N, DEV)                                      # uploaded under the guard: between bands
        index_is_guarded(guard, index)
        batch_t = guard.home(to_dev(batch))
        for head in (True, False):
            for keep_target in (False, True):
                for c_first, c_count in ((0, N), (0, 32), (32, 1)):
                    mask = _native.filter_mask_index(batch_t, head, index, keep_target, c_first, c_count)
                    assert guard._inside(mask.data_ptr())
                    got[head, keep_target, c_first, c_count] = mask.cpu().numpy().view(np.uint32)
        problems = guard.problems(f"filter mask N={N} Q={Q}")
    assert not problems, "\n".join(problems)
    for (head, keep_target, c_first, c_count), mask in got.items():
        rows, cols = lists_index.lists(batch, head, keep_target=keep_target)
        sel = (cols >= c_first) & (cols < c_first + c_count)
        want = np.zeros((Q, (c_count + 31) // 32), np.uint32)
        np.bitwise_or.at(want, (rows[sel].astype(np.int64), (cols[sel] - c_first) >> 5), np.uint32(1) << ((cols[sel] - c_first) & 31).astype(np.uint32))
        assert np.array_equal(mask, want), (head, keep_target, c_first, c_count, mask, want)
    assert got[False, True, 0, N][0].tolist() == [0xFFFFFFFF, 1] and got[False, False, 0, N][0].tolist() == [0xFFFFFFFF, 0]
    assert got[False, False, 0, N][1].tolist() == [1 << 31, 0] and not got[False, True, 0, N][2].any()


def test_softmax_loss_through_autograd_under_guard_bands(monkeypatch):
    from torch_rgcn import functional
    from torch_rgcn.functional import FilterIndex
    from utils.misc import _FilterIndex, generate_true_dict
    batch, known, nodes, rel, bias = scenario()
    true = generate_true_dict(known)
    rows, cols = _FilterIndex(true, N).lists(batch, False)

    def run(put, **filt):
        nt, rt = put(to_dev(nodes)).requires_grad_(True), put(to_dev(rel)).requires_grad_(True)
        bt = [put(to_dev(b)).requires_grad_(True) for b in bias]
        loss = functional.distmult_softmax_loss(put(to_dev(batch)), False, nt, rt, *bt, reduction="none", chunk_bytes=1, **filt)
        loss.mean().backward()
        return [loss.detach().cpu()] + [t.grad.cpu() for t in [nt, rt] + bt]

    want = run(lambda t: t, filt_q=to_dev(rows), filt_n=to_dev(cols))          # the list form, unguarded
    with gb.Guard(monkeypatch) as guard:
        index = FilterIndex(true, N, DEV)
        index_is_guarded(guard, index)
        assert torch.isnan(torch.empty(3, device=DEV)).all()
        got = run(guard.home, filt=index)
        problems = guard.problems(f"filtered softmax loss with an index N={N} Q={Q} d={DIM}")
    assert not problems, "\n".join(problems)
    assert want[0][0] == 0.0 and (want[0][1:] > 0).all()                       # the hub query keeps its target alone: lse == tscore
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.isfinite(g).all() and torch.equal(g, w), (k, g, w)
