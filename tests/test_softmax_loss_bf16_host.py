"""Host side of the native bf16 backward of the 1-N softmax loss (no GPU): the C entry points exist and bind from the header, the
workspace-size function (which asks no device), the bf16 configuration, and the argument errors raised before anything touches a device."""
import ctypes
import os
import sys

import pytest
import torch
import yaml

from conftest import PKG
from torch_rgcn import _native, functional

NEW = ("rgcn_distmult_softmax_grad_workspace_bytes", "rgcn_distmult_softmax_grad_bf16", "rgcn_distmult_softmax_grad_smooth_bf16")


def test_the_library_exports_and_the_header_binds_the_new_entry_points():
    raw = ctypes.CDLL(_native._LIB_PATH)
    L = _native.lib()
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(L, name).argtypes is not None, name
    size = L.rgcn_distmult_softmax_grad_workspace_bytes
    assert size.restype is ctypes.c_int64 and size.argtypes == [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int32]
    # the signatures of the fp32 forms (every pointer is a void pointer to the binder: `const uint16_t *nodes` for `const float *nodes`)
    assert L.rgcn_distmult_softmax_grad_bf16.argtypes == L.rgcn_distmult_softmax_grad_f32.argtypes
    assert L.rgcn_distmult_softmax_grad_smooth_bf16.argtypes == L.rgcn_distmult_softmax_grad_smooth_f32.argtypes
    header = open(_native._HEADER_PATH).read()
    for name in NEW[1:]:
        decl = header[header.index(f"RGCN_API int {name}("):]
        assert "const uint16_t *nodes" in decl[:decl.index(";")], name


def pad32(d):
    return (d + 31) // 32 * 32


def test_bf16_gradient_workspace_bytes():
    def size(Q, c_count, d):
        return _native.lib().rgcn_distmult_softmax_grad_workspace_bytes(Q, c_count, d, 1)

    assert size(-1, 128, 8) == 0 and size(10, 0, 8) == 0 and size(10, -1, 8) == 0 and size(10, 128, 0) == 0 and size(10, 128, -3) == 0
    Qs = [0, 1, 2, 127, 128, 129, 5_000, 131_072]
    Cs = [1, 31, 32, 33, 127, 128, 129, 1_000, 40_943, 1_000_000]
    Ds = [1, 8, 24, 31, 32, 33, 50, 200, 500]
    table = {(Q, c, d): size(Q, c, d) for Q in Qs for c in Cs for d in Ds}
    for (Q, c, d), b in table.items():
        assert b % 16 == 0 and b >= 3 * Q * pad32(d) * 2 + 8 * Q + 4 * Q * ((c + 31) // 32), (Q, c, d, b)
        assert Q == 0 or b > 0
    for axis, values in enumerate((Qs, Cs, Ds)):                             # non-decreasing in Q, c_count and d
        for key, b in table.items():
            k = values.index(key[axis])
            if k:
                below = list(key)
                below[axis] = values[k - 1]
                assert b >= table[tuple(below)], (axis, key)
    # the mask of a chunk, not of the whole table
    assert size(5_000, 128, 200) < 8 * 2 ** 20
    # the fp32 form keeps its values: fp32 query vectors where this one holds three bf16 terms
    f32 = _native.lib().rgcn_distmult_softmax_grad_workspace_bytes(5_000, 128, 200, 0)
    assert f32 - 5_000 * 200 * 4 == size(5_000, 128, 200) - 3 * 5_000 * 224 * 2


def test_the_bf16_configuration_is_the_one_to_n_configuration_plus_one_key():
    base = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n.yaml")))
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-bf16.yaml")))
    assert cfg["training"]["bf16"] is True and "bf16" not in base["training"]
    del cfg["training"]["bf16"]
    assert cfg == base


@pytest.mark.parametrize("objective", [None, "negative-sampling"])
def test_training_bf16_needs_the_one_to_n_objective(objective):
    """refused while the configuration is read: before the data is loaded and before any device is touched"""
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-bf16.yaml")))
    if objective is None:
        del cfg["training"]["objective"]
    else:
        cfg["training"]["objective"] = objective
    with pytest.raises(ValueError, match="training.bf16"):
        predict_links.run(cfg, epochs=1, quiet=True, synthetic=True)


def test_bf16_backward_is_checked_before_any_device_work():
    batch = torch.tensor([[0, 1, 2]])
    nodes, rel = torch.randn(4, 8), torch.randn(3, 8)
    for value in ("fast", "", None, "Native"):
        with pytest.raises(ValueError, match="bf16_backward"):
            functional.distmult_softmax_loss(batch, False, nodes, rel, bf16_backward=value)
        with pytest.raises(ValueError, match="bf16_backward"):
            functional.distmult_softmax_loss(batch, False, nodes.bfloat16().requires_grad_(True), rel, bf16_backward=value)
    for value in ("upcast", "native"):                                      # a valid value gets as far as the device check
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            functional.distmult_softmax_loss(batch, False, nodes, rel, bf16_backward=value)
