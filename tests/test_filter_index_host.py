"""The numpy stage of functional.FilterIndex -- the key -> completions tables a kernel searches on the device -- against
utils.misc._FilterIndex, whose host lists are what every filtered route took before; the configuration that trains with it.  No GPU."""
import os
import sys

import numpy as np
import pytest
import yaml

from conftest import PKG
from torch_rgcn.functional import FilterIndex
from utils.misc import _FilterIndex, generate_true_dict
import utils.misc

N, R = 23, 4


def random_triples(seed, n_triples=400):
    """few entities and relations: most keys are shared by several triples; a fifth of the triples are repeated outright"""
    rng = np.random.default_rng(seed)
    t = np.stack([rng.integers(0, N, n_triples), rng.integers(0, R, n_triples), rng.integers(0, N, n_triples)], 1)
    return np.concatenate([t, t[rng.integers(0, n_triples, n_triples // 5)]])


def expand(table, batch, head, n):
    """the (row, col) pairs the device walk produces from one direction's tables: key of the query, binary search, the key's span"""
    keys, ptr, vals = table
    out = set()
    for q, (s, p, o) in enumerate(batch.tolist()):
        key = p * n + (o if head else s)
        k = int(np.searchsorted(keys, key))
        if k < len(keys) and keys[k] == key:
            out.update((q, int(v)) for v in vals[ptr[k]:ptr[k + 1]])
    return out


def test_is_reexported_from_utils_misc():
    assert utils.misc.FilterIndex is FilterIndex


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("head", [True, False])
def test_expansion_matches_the_host_lists(seed, head):
    triples = random_triples(seed)
    true = generate_true_dict(triples)
    assert any(len(v) != len(set(v)) for v in true[0].values())                 # duplicates are in the dictionaries
    tables = FilterIndex.host_tables(true, N)
    rng = np.random.default_rng(100 + seed)
    # queries: known triples (their key hits), the same one twice, and random ones (most keys of the 4 * 23 exist; some do not)
    batch = np.concatenate([triples[:40], triples[:1], np.stack([rng.integers(0, N, 60), rng.integers(0, R, 60), rng.integers(0, N, 60)], 1)])
    rows, cols = _FilterIndex(true, N).lists(batch, head, keep_target=True)
    want = set(zip(rows.tolist(), cols.tolist()))
    got = expand(tables[0 if head else 1], batch, head, N)
    assert got == want and len(want) > 100
    assert len(rows) > len(want)                                                # the lists repeat a duplicate triple, the index does not


@pytest.mark.parametrize("seed", [0, 1])
def test_keys_strictly_ascending_values_ascending_and_unique(seed):
    triples = random_triples(seed)
    for keys, ptr, vals in FilterIndex.host_tables(generate_true_dict(triples), N):
        assert keys.dtype == np.int64 and ptr.dtype == np.int64 and vals.dtype == np.int32
        assert len(ptr) == len(keys) + 1 and ptr[0] == 0 and ptr[-1] == len(vals)
        assert (np.diff(keys) > 0).all() and (np.diff(ptr) > 0).all()
        for k in range(len(keys)):
            assert (np.diff(vals[ptr[k]:ptr[k + 1]]) > 0).all()
        assert vals.min() >= 0 and vals.max() < N
    heads, tails = FilterIndex.host_tables(generate_true_dict(triples), N)
    assert set(heads[0].tolist()) == {p * N + o for _, p, o in triples.tolist()}
    assert set(tails[0].tolist()) == {p * N + s for s, p, _ in triples.tolist()}


def test_an_empty_triple_set_gives_no_keys():
    for keys, ptr, vals in FilterIndex.host_tables(generate_true_dict(np.zeros((0, 3), np.int64)), N):
        assert len(keys) == 0 and ptr.tolist() == [0] and len(vals) == 0
        assert keys.dtype == np.int64 and ptr.dtype == np.int64 and vals.dtype == np.int32


@pytest.mark.parametrize("bad", [(N, 1, 2), (2, 1, N), (-1, 1, 2), (2, 1, -1), (2, -1, 3)])
def test_a_bad_triple_raises_index_error(bad):
    triples = np.concatenate([random_triples(0, 50), np.array([bad])])
    with pytest.raises(IndexError):
        FilterIndex.host_tables(generate_true_dict(triples), N)
    with pytest.raises(IndexError):                                             # the constructor validates before it uploads anything
        FilterIndex(generate_true_dict(triples), N, "cpu")


def test_the_constructor_only_uploads():
    true = generate_true_dict(random_triples(3))
    idx = FilterIndex(true, N, "cpu")
    assert idx.num_nodes == N and idx.device.type == "cpu"
    for (keys, ptr, vals), host in zip(idx.tables, FilterIndex.host_tables(true, N)):
        assert not (keys.requires_grad or ptr.requires_grad or vals.requires_grad)
        for t, a in zip((keys, ptr, vals), host):
            assert np.array_equal(t.numpy(), a) and str(t.dtype).endswith(str(a.dtype))


def test_the_filtered_configuration_is_the_1n_one_plus_its_key():
    plain = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n.yaml")))
    filtered = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-filtered.yaml")))
    assert filtered["training"].pop("filtered") is True
    assert "filtered" not in plain["training"] and filtered == plain


def test_training_filtered_needs_the_1n_objective():
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-filtered.yaml")))
    for objective in ("negative-sampling", None):
        if objective is None:
            cfg["training"].pop("objective")
        else:
            cfg["training"]["objective"] = objective
        with pytest.raises(ValueError, match="filtered"):
            predict_links.run(cfg, quiet=True, synthetic=True)
