"""Host side of label smoothing in the 1-N softmax loss (no GPU): the workspace size of the smoothed strip pass (which asks no device),
the validation of label_smoothing before anything touches a device, the experiment key and the new configuration."""
import os
import sys

import pytest
import torch
import yaml

from conftest import PKG
from torch_rgcn import _native, functional


def align16(b):
    return (b + 15) // 16 * 16


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("strips", [0, 1, 3, 64])
def test_lse_smooth_workspace_bytes(bf16, strips):
    size, plain = _native.lse_smooth_workspace_bytes, _native.lse_workspace_bytes
    Qs = [1, 2, 127, 128, 129, 257, 1_000, 5_000, 20_466, 131_072, 1_000_000]
    Ns = [1, 31, 32, 33, 127, 128, 129, 700, 4_099, 40_943, 1_000_000]
    for d in (1, 24, 200):
        table = [[size(Q, N, d, strips, bf16) for N in Ns] for Q in Qs]
        for qi, Q in enumerate(Qs):
            for ni, N in enumerate(Ns):
                b = table[qi][ni]
                assert b > 0 and b % 16 == 0 and b >= 4 * Q * ((N + 31) // 32), (Q, N, d)
                assert qi == 0 or b >= table[qi - 1][ni], ("Q", Q, N, d)
                assert ni == 0 or b >= table[qi][ni - 1], ("N", Q, N, d)
                assert b >= plain(Q, N, d, strips, bf16), (Q, N, d)
                if strips:
                    # four floats per (strip half, query) where the unsmoothed layout has two, everything else as it is
                    assert b - plain(Q, N, d, strips, bf16) == align16(2 * strips * Q * 16) - align16(2 * strips * Q * 8), (Q, N, d)
                    assert b >= 2 * strips * Q * 16 + 4 * Q * ((N + 31) // 32), (Q, N, d)
                else:
                    # the default: room for every strip the library may choose -- never more of them than tiles
                    assert b - plain(Q, N, d, 0, bf16) > 0 and b <= size(Q, N, d, (N + 127) // 128, bf16), (Q, N, d)
    assert size(-1, 10, 8, 0, bf16) == 0 and size(10, 0, 8, 0, bf16) == 0 and size(10, 10, 0, 0, bf16) == 0 and size(10, 10, 8, -1, bf16) == 0


def test_label_smoothing_is_validated_before_any_device_work():
    batch = torch.tensor([[0, 1, 2]])
    nodes, rel = torch.randn(4, 8), torch.randn(3, 8)
    for bad in (-0.1, 1.0, 1.5, float("nan"), "0.1"):
        with pytest.raises(ValueError, match="label_smoothing"):
            functional.distmult_softmax_loss(batch, False, nodes, rel, label_smoothing=bad)
    for good in (0.0, 0.5):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            functional.distmult_softmax_loss(batch, False, nodes, rel, label_smoothing=good)
    from torch_rgcn.layers import DistMult
    import inspect
    assert inspect.signature(DistMult.softmax_loss).parameters["label_smoothing"].default == 0.0
    assert inspect.signature(functional.distmult_softmax_loss).parameters["label_smoothing"].default == 0.0


def test_label_smoothing_needs_the_1n_objective():
    sys.path.insert(0, os.path.join(PKG, "experiments"))
    import predict_links
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18.yaml")))
    assert "objective" not in cfg["training"]
    cfg["training"]["label_smoothing"] = 0.1
    with pytest.raises(ValueError, match="label_smoothing"):
        predict_links.run(cfg, epochs=1, quiet=True, synthetic=True)


def test_the_smoothed_configuration_is_the_1n_one_plus_the_key():
    cfg = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n-smoothed.yaml")))
    plain = yaml.safe_load(open(os.path.join(PKG, "configs", "rgcn", "lp-WN18-1n.yaml")))
    assert cfg["training"]["label_smoothing"] == 0.1 and "label_smoothing" not in plain["training"]
    del cfg["training"]["label_smoothing"]
    assert cfg == plain
