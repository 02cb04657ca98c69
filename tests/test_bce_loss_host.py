"""Host side of the 1-N multi-label BCE loss of DistMult (no GPU): the six entry points are exported and bound from the header, the two
workspace sizes (which ask no device), the argument errors that must come before anything touches a device, the experiment key and the
new configuration."""
import ctypes
import inspect
import os
import sys

import pytest
import torch
import yaml

from conftest import PKG
from torch_rgcn import _native, functional

SYMBOLS = ["rgcn_distmult_bce_sums_f32", "rgcn_distmult_bce_sums_bf16", "rgcn_distmult_bce_grad_f32", "rgcn_distmult_bce_grad_bf16",
           "rgcn_distmult_bce_sums_workspace_bytes", "rgcn_distmult_bce_grad_workspace_bytes"]


def align16(b):
    return (b + 15) // 16 * 16


def test_the_six_symbols_are_exported_and_bind():
    raw = ctypes.CDLL(_native._LIB_PATH)
    L = _native.lib()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes, name                                # declared from the header
    assert L.rgcn_distmult_bce_sums_workspace_bytes.restype is ctypes.c_int64 and L.rgcn_distmult_bce_grad_workspace_bytes.restype is ctypes.c_int64
    assert len(L.rgcn_distmult_bce_sums_workspace_bytes.argtypes) == 5 and len(L.rgcn_distmult_bce_grad_workspace_bytes.argtypes) == 4
    # both forms of the positives in one call: lists (filt_q, filt_n, F) and index (fkeys, fptr, fvals, K)
    assert len(L.rgcn_distmult_bce_sums_f32.argtypes) == len(L.rgcn_distmult_bce_sums_bf16.argtypes) == 24
    assert len(L.rgcn_distmult_bce_grad_f32.argtypes) == len(L.rgcn_distmult_bce_grad_bf16.argtypes) == 27
    for name in ("distmult_bce_sums", "distmult_bce_grad", "bce_sums_workspace_bytes", "bce_grad_workspace_bytes"):
        assert callable(getattr(_native, name)), name


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("strips", [0, 1, 3, 64])
def test_bce_sums_workspace_bytes(bf16, strips):
    """the layout of the smoothed log-sum-exp route (four floats per cell of the partials), and it grows with the ceil(N / 32) * Q words
    of the label mask, which this route always fills"""
    size = _native.bce_sums_workspace_bytes
    Qs = [1, 2, 127, 128, 129, 257, 1_000, 5_000, 131_072, 1_000_000]
    Ns = [1, 31, 32, 33, 127, 128, 129, 700, 4_099, 40_943, 1_000_000]
    for d in (1, 24, 200):
        table = [[size(Q, N, d, strips, bf16) for N in Ns] for Q in Qs]
        for qi, Q in enumerate(Qs):
            for ni, N in enumerate(Ns):
                b = table[qi][ni]
                words = Q * ((N + 31) // 32)
                assert b > 0 and b % 16 == 0 and b >= 4 * words, (Q, N, d)
                assert b == _native.lse_smooth_workspace_bytes(Q, N, d, strips, bf16), (Q, N, d)
                assert qi == 0 or b >= table[qi - 1][ni], ("Q", Q, N, d)
                assert ni == 0 or b >= table[qi][ni - 1], ("N", Q, N, d)
                if strips:
                    # the mask is the one term that depends on N: query vectors + bias terms + partials + align16(4 * words)
                    assert b - size(Q, 1, d, strips, bf16) == align16(4 * words) - align16(4 * Q), (Q, N, d)
    assert size(-1, 10, 8, 0, bf16) == 0 and size(10, 0, 8, 0, bf16) == 0 and size(10, 10, 0, 0, bf16) == 0 and size(10, 10, 8, -1, bf16) == 0


@pytest.mark.parametrize("bf16", [False, True])
def test_bce_grad_workspace_bytes(bf16):
    size = _native.bce_grad_workspace_bytes
    for d in (1, 24, 200):
        for Q in (1, 129, 5_000):
            prev = 0
            for C in (1, 32, 33, 128, 700, 40_943):
                b = size(Q, C, d, bf16)
                words = Q * ((C + 31) // 32)
                assert b > 0 and b % 16 == 0 and b >= 4 * words and b >= prev, (Q, C, d)
                assert b == _native.softmax_grad_workspace_bytes(Q, C, d, bf16), (Q, C, d)
                assert b - size(Q, 1, d, bf16) == align16(4 * words) - align16(4 * Q), (Q, C, d)
                prev = b
    assert size(-1, 10, 8, bf16) == 0 and size(10, 0, 8, bf16) == 0 and size(10, 10, 0, bf16) == 0


def test_arguments_are_validated_before_any_device_work():
    batch = torch.tensor([[0, 1, 2]])
    nodes, rel = torch.randn(4, 8), torch.randn(3, 8)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1", True):
        with pytest.raises(ValueError, match="label_smoothing"):
            functional.distmult_bce_loss(batch, False, nodes, rel, label_smoothing=bad)
    with pytest.raises(ValueError, match="reduction"):
        functional.distmult_bce_loss(batch, False, nodes, rel, reduction="sum")
    with pytest.raises(ValueError, match="bf16_backward"):
        functional.distmult_bce_loss(batch, False, nodes, rel, bf16_backward="widen")
    for good in (0.0, 0.5):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            functional.distmult_bce_loss(batch, False, nodes, rel, label_smoothing=good)
    from torch_rgcn.layers import DistMult
    names = list(inspect.signature(functional.distmult_bce_loss).parameters)
    assert names == ["batch", "head", "nodes", "relations", "sbias", "pbias", "obias", "lab_q", "lab_n", "labels", "reduction", "strips",
                     "chunk_bytes", "bf16_backward", "label_smoothing"]
    assert inspect.signature(DistMult.bce_loss).parameters["label_smoothing"].default == 0.0


def test_lists_and_index_are_mutually_exclusive_and_the_index_belongs_to_the_table():
    index = functional.FilterIndex(({(1, 2): [0, 3]}, {(0, 1): [2]}), 4, "cpu")
    batch = torch.tensor([[0, 1, 2]])
    nodes, rel = torch.randn(4, 8), torch.randn(3, 8)
    lists = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="mutually exclusive"):
        functional.distmult_bce_loss(batch, False, nodes, rel, lab_q=lists, lab_n=lists, labels=index)
    with pytest.raises(TypeError, match="labels must be a FilterIndex"):
        functional.distmult_bce_loss(batch, False, nodes, rel, labels={(1, 2): [0]})
    with pytest.raises(ValueError, match="built for 4 entities"):
        functional.distmult_bce_loss(batch, False, torch.randn(5, 8), rel, labels=index)


def test_training_filtered_does_not_combine_with_the_objective():
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-bce.yaml")))
    cfg["training"]["filtered"] = True
    with pytest.raises(ValueError, match="1-n-bce"):
        predict_links.run(cfg, epochs=1, quiet=True, synthetic=True)


def test_the_configuration_is_the_wn18_one_with_the_objective_and_smoothing():
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-bce.yaml")))
    plain = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18.yaml")))
    assert cfg["training"]["objective"] == "1-n-bce" and cfg["training"]["label_smoothing"] == 0.1
    del cfg["training"]["objective"], cfg["training"]["label_smoothing"]
    assert cfg == plain
