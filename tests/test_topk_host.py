"""Host side of top-k link prediction (no GPU): the workspace-size function of the C ABI (which asks no device), the filter lists with
and without the queries' own targets, and the sort key of the materialised fallback of utils.misc.predict."""
import inspect

import numpy as np
import pytest
import torch

from torch_rgcn import _native
from utils import misc

INF = float("inf")


# ----------------------------------------------------------------------------- rgcn_distmult_topk_workspace_bytes
@pytest.mark.parametrize("bf16", [False, True])
def test_workspace_bytes_are_zero_for_bad_arguments(bf16):
    size = _native.topk_workspace_bytes
    assert size(10, 10, 8, 10, 0, bf16) > 0
    assert size(-1, 10, 8, 10, 0, bf16) == 0 and size(10, 0, 8, 10, 0, bf16) == 0 and size(10, 10, 0, 10, 0, bf16) == 0
    assert size(10, 10, 8, 0, 0, bf16) == 0 and size(10, 10, 8, -3, 0, bf16) == 0 and size(10, 10, 8, 10, -1, bf16) == 0
    assert size(10, 10, 8, _native.TOPK_MAX, 0, bf16) > 0 and size(10, 10, 8, _native.TOPK_MAX + 1, 0, bf16) == 0
    assert _native.TOPK_MAX == 32


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("strips", [0, 1, 3, 64])
def test_workspace_bytes_grow_with_q_n_d_and_k(bf16, strips):
    size = _native.topk_workspace_bytes
    Qs = [1, 2, 127, 128, 129, 257, 1_000, 5_000, 131_072, 1_000_000]
    Ns = [1, 31, 32, 33, 127, 128, 129, 700, 40_943, 1_000_000]
    ds = [1, 24, 200, 500]
    ks = [1, 2, 10, 31, 32]
    t = np.array([[[[size(Q, N, d, k, strips, bf16) for k in ks] for d in ds] for N in Ns] for Q in Qs], dtype=np.int64)
    assert (t > 0).all() and (t % 16 == 0).all()
    for axis in range(4):
        assert (np.diff(t, axis=axis) >= 0).all(), axis
    # strictly, from end to end of every axis
    assert (t[-1] > t[0]).all() and (t[:, -1] > t[:, 0]).all() and (t[:, :, -1] > t[:, :, 0]).all() and (t[..., -1] > t[..., 0]).all()
    # the mask is inside, and with explicit strips so are 2 strips Q k keys of 8 bytes
    for qi, Q in enumerate(Qs):
        for ni, N in enumerate(Ns):
            for ki, k in enumerate(ks):
                assert t[qi, ni, 0, ki] >= 4 * Q * ((N + 31) // 32) + 16 * strips * Q * k, (Q, N, k)


@pytest.mark.parametrize("bf16", [False, True])
def test_workspace_at_k_1_holds_what_the_evaluator_holds_besides_its_partials(bf16):
    """one key of 8 bytes per (strip half, query) is the size of the evaluator's (greater, equal) pair: query vectors, bias terms and the
    mask are laid out alike"""
    for Q, N, d in ((1, 1, 1), (130, 700, 24), (5_000, 40_943, 200), (257, 1_000_000, 50)):
        for s in (1, 2, 7, 64):
            rank = _native.rank_fused_workspace_bytes(Q, N, d, s, bf16)
            partials = -(-2 * s * Q * 8 // 16) * 16
            assert _native.topk_workspace_bytes(Q, N, d, 1, s, bf16) >= rank - partials, (Q, N, d, s)


def test_topk_batch_keeps_the_workspace_within_its_budget():
    assert misc._topk_batch(300, 4_099, 24, 10) == 300
    for k in (1, 10, 32):
        q = misc._topk_batch(10_000, 1_000_000, 200, k)
        assert q >= 64
        for bf16 in (False, True):
            assert _native.topk_workspace_bytes(q, 1_000_000, 200, k, 0, bf16) <= misc._FUSED_BYTES, (k, bf16)
    assert misc._topk_batch(1_000, 10 ** 10, 200, 10) == 64


# ----------------------------------------------------------------------------- _FilterIndex.lists
def _lists_before_keep_target(index, batch, head):
    """the method as it stood before it took `keep_target`, restated on the index's own tables"""
    b = np.asarray(batch, np.int64)
    keys, ptr, vals = index.tables[0 if head else 1]
    want_r, want_c = [], []
    for i, (s, p, o) in enumerate(b.tolist()):
        key = p * index.n + (o if head else s)
        at = np.searchsorted(keys, key)
        if at < len(keys) and keys[at] == key:
            for v in vals[ptr[at]:ptr[at + 1]].tolist():
                if v != (s if head else o):
                    want_r.append(i)
                    want_c.append(v)
    return np.array(want_r, np.int32), np.array(want_c, np.int32)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_filter_lists_with_and_without_the_targets(seed):
    rng = np.random.default_rng(seed)
    N, R = 30 + 7 * seed, 3 + seed
    known = np.stack([rng.integers(0, N, 400), rng.integers(0, R, 400), rng.integers(0, N, 400)], 1)
    known = np.concatenate([known, known[:25]])                          # duplicates are kept by generate_true_dict
    batch = np.concatenate([known[rng.permutation(len(known))[:40]],     # queries whose target is a known completion ...
                            np.stack([rng.integers(0, N, 20), rng.integers(0, R, 20), rng.integers(0, N, 20)], 1)])      # ... and random ones
    index = misc._FilterIndex(misc.generate_true_dict(known), N)
    for head in (True, False):
        rows, cols = index.lists(batch, head)
        want = _lists_before_keep_target(index, batch, head)
        assert rows.dtype == cols.dtype == np.int32
        assert np.array_equal(rows, want[0]) and np.array_equal(cols, want[1])
        again = index.lists(batch, head, keep_target=False)
        assert np.array_equal(again[0], rows) and np.array_equal(again[1], cols)
        # keep_target=True: the same lists plus exactly the target cells, as often as the dictionaries hold them
        all_r, all_c = index.lists(batch, head, keep_target=True)
        assert all_r.dtype == all_c.dtype == np.int32
        target = batch[:, 0 if head else 2]
        on_target = all_c == target[all_r]
        assert on_target.any() and not (cols == target[rows]).any()
        assert np.array_equal(all_r[~on_target], rows) and np.array_equal(all_c[~on_target], cols)
        table = misc.generate_true_dict(known)[0 if head else 1]
        for i, (s, p, o) in enumerate(batch.tolist()):
            held = table.get((p, o) if head else (s, p), [])
            assert int((on_target & (all_r == i)).sum()) == held.count(s if head else o), i
    assert "keep_target" in inspect.signature(misc._FilterIndex.lists).parameters
    assert inspect.signature(misc._FilterIndex.lists).parameters["keep_target"].default is False


# ----------------------------------------------------------------------------- the fallback's sort key
def test_fallback_sort_key_on_a_hand_written_matrix():
    scores = torch.tensor([[1.0, 3.0, 3.0, -INF, 2.0, 3.0],              # ties at 3: ids 1, 2, 5 in that order; one filtered cell
                           [0.0, -0.0, -1.0, 0.0, -INF, -INF],           # +0 and -0 are one value: ids 0, 1, 3
                           [-INF, -INF, -INF, -INF, -INF, -INF],         # everything filtered
                           [5.0, 4.0, 3.0, 2.0, 1.0, 0.5],
                           [7.0, -INF, 7.0, -INF, 7.0, -INF]])
    ids, s = misc._topk_of_scores(scores, 4)
    assert ids.dtype == torch.int64 and s.dtype == torch.float32 and ids.shape == s.shape == (5, 4)
    assert ids.tolist() == [[1, 2, 5, 4], [0, 1, 3, 2], [-1, -1, -1, -1], [0, 1, 2, 3], [0, 2, 4, -1]]
    assert s.tolist() == [[3, 3, 3, 2], [0, 0, 0, -1], [-INF] * 4, [5, 4, 3, 2], [7, 7, 7, -INF]]
    # k > N: every candidate in order, then the padding
    ids, s = misc._topk_of_scores(scores, 8)
    assert ids.shape == s.shape == (5, 8)
    assert ids.tolist() == [[1, 2, 5, 4, 0, -1, -1, -1], [0, 1, 3, 2, -1, -1, -1, -1], [-1] * 8, [0, 1, 2, 3, 4, 5, -1, -1],
                            [0, 2, 4, -1, -1, -1, -1, -1]]
    assert s[0].tolist() == [3, 3, 3, 2, 1, -INF, -INF, -INF] and s[2].tolist() == [-INF] * 8
    assert s[3].tolist() == [5, 4, 3, 2, 1, 0.5, -INF, -INF]
    # k = 1, and the input is left as it was
    ids, s = misc._topk_of_scores(scores, 1)
    assert ids.tolist() == [[1], [0], [-1], [0], [0]] and s.tolist() == [[3], [0], [-INF], [5], [7]]
    assert scores[1, 1].item() == 0 and np.signbit(scores[1, 1].item())


def test_fallback_sort_key_equals_lexsort():
    rng = np.random.default_rng(5)
    sc = rng.integers(-3, 4, (40, 57)).astype(np.float32)
    sc[rng.random(sc.shape) < 0.3] = -np.inf
    sc[3] = -np.inf
    for k in (1, 10, 57, 60):
        ids, s = misc._topk_of_scores(torch.from_numpy(sc), k)
        for q in range(len(sc)):
            order = np.lexsort((np.arange(sc.shape[1]), -sc[q]))
            order = order[sc[q][order] > -np.inf][:k]
            want = np.full(k, -1)
            want[:len(order)] = order
            assert ids[q].tolist() == want.tolist(), (k, q)
            assert s[q, :len(order)].tolist() == sc[q][order].tolist() and (s[q, len(order):] == -INF).all()


# ----------------------------------------------------------------------------- the public call
def test_predict_signature_and_models_it_refuses():
    p = inspect.signature(misc.predict).parameters
    assert list(p) == ["model", "graph", "queries", "num_nodes", "k", "head", "true_triples", "fused"]
    assert p["k"].default == 10 and p["head"].default is False and p["true_triples"].default is None and p["fused"].default is None
    with pytest.raises(TypeError):
        misc.predict(torch.nn.Linear(2, 2), None, [[0, 0, 1]], 2)
    f = inspect.signature(_native.distmult_topk).parameters
    assert list(f) == ["batch", "head", "nodes", "rel", "sbias", "pbias", "obias", "k", "filt_q", "filt_n", "strips"]
    from torch_rgcn import functional
    g = inspect.signature(functional.distmult_topk_all).parameters
    assert list(g) == ["batch", "head", "nodes", "relations", "sbias", "pbias", "obias", "k", "filt_q", "filt_n", "strips"]
    assert g["k"].default == 10 and g["strips"].default == 0
