"""The relation-owner backward (rgcn_bwd_own_f32) where its accumulator selection and its bias-gradient stream can go wrong, exactly.

The kernel keeps a wave's K = 8 dW accumulators as separate register quads and picks one per chunk with wave-uniform branches on the chunk's
local unit number; the bias gradient (column sums of G) is read one float4 per thread at every tile boundary, and a loop after the last
tile reads what is left.  The existing exact cases run this kernel on 11 relations and one tile per workgroup: two or three of the eight
accumulators, one boundary.  Here:

  * 121 relations (every accumulator of at least one wave in use) on 40-row tiles: 1000 tiles, three or four per workgroup on 256 CUs, an
    uneven count across the workgroups (the ones with a tile fewer finish their share of G in the loop after the tiles), waves with an odd
    number of chunks in a tile (the second chunk of the last pair is a repeat of the last chunk with val = 0);
  * 11 relations: the large ones are cut into owned parts, several units -- of several waves -- add into one dW_r;
  * the ReLU-masked form on a two-layer step;
  * node counts off every grid (40 003), one tile per workgroup (33 000 at the default tile height), and the whole case between guard bands.

All inputs are those of tests/exact_inputs.py: every sum is exact in fp32 in any order, so dX, dW and db EQUAL the float64 oracle."""
import functools

import numpy as np
import pytest
import torch
from torch_rgcn import routes

import exact_inputs as ex
import guard_bands as gb
import test_gpu_exact as tex
from oracle import oracle

pytestmark = pytest.mark.gpu
DEV = tex.DEV

# (N, R0, groups per relation, hub_log2, seed) in the table of test_gpu_exact.fixture.  1000 groups of 1 .. 16 messages per relation: ~6 200
# messages per relation and direction, 6 per (40-row tile, relation) bucket -- one chunk per bucket, ~8 chunks per wave and tile
FIXTURES = {
    "own_r60": (40_000, 60, 1000, None, 201),
    "own_r5": (40_000, 5, 12_000, None, 202),
    "own_r60_n40003": (40_003, 60, 1000, None, 203),
    "own_r5_n33000": (33_000, 5, 10_000, None, 204),
}
for _name, _fix in FIXTURES.items():
    assert tex.FIX.setdefault(_name, _fix) == _fix, _name

SHORT_TILES = dict(softwin="1", sparse_path="0", own_rows_cap="50")      # 40 000 nodes on 256 CUs: 40-row tiles, 1000 of them
ONE_TILE = dict(softwin="1", sparse_path="0")                            # the default cap (767 rows): 33 000 nodes give 129-row tiles, one per CU


@functools.lru_cache(maxsize=None)
def owner_plan_facts(fix, switches):
    """what the owner plan of the fixture looks like under the route switches, from a layer on zeros (no oracle): None when the backward
    would not take the relation-owner kernel, else a dict of the properties the cases below assert before they run"""
    from torch_rgcn import _native
    from torch_rgcn import functional as F_
    fx = tex.fixture(fix)
    shapes = tex._param_shapes(fx["R"], fx["N"], 16, 16, "none", False, 3, 2, False)
    params = {n: np.zeros(shape, np.float32) for n, shape in shapes.items()}
    layer = tex.make_layer(fx, params, params.pop("bias"), 16, 16, "none", False, False, 3, 2, False)
    with routes.override(**dict(switches)), torch.no_grad():
        layer(torch.zeros(fx["N"], 16, device=DEV))
        name, plan = F_._backward_route(layer._graph, 16, 16)
        if name != "own":
            return None
        nw, per_wave, _ = _native.bwd_own_geometry()
        n_cu = torch.cuda.get_device_properties(DEV).multi_processor_count
        chunks = (plan.own_ptr[1:] - plan.own_ptr[:-1]).view(plan.n_tiles, nw).cpu().numpy()
        units = (plan.unit_rel.view(nw, per_wave) >= 0).sum(1).cpu().numpy()
        unit_rel = plan.unit_rel.cpu().numpy()
        return dict(n_tiles=int(plan.n_tiles), tile_rows=int(plan.tile_rows), n_cu=n_cu, per_wave=per_wave, units_per_wave=units,
                    chunks=chunks, units_per_relation=np.bincount(unit_rel[unit_rel >= 0], minlength=fx["R"]),
                    waves_per_relation=[len({u // per_wave for u in np.flatnonzero(unit_rel == r)}) for r in range(fx["R"])])


def need_owner_plan(fix, switches, min_tiles_per_wg):
    facts = owner_plan_facts(fix, tuple(sorted(switches.items())))
    if facts is None:
        pytest.skip("the backward of this graph does not take the relation-owner kernel on this device")
    if facts["n_tiles"] < min_tiles_per_wg * facts["n_cu"]:
        pytest.skip(f"{facts['n_tiles']} tiles on {facts['n_cu']} CUs: fewer than {min_tiles_per_wg} per workgroup")
    print(f"[own] {fix}: {facts['n_tiles']} tiles of {facts['tile_rows']} rows on {facts['n_cu']} CUs, units per wave {facts['units_per_wave'].tolist()}, "
          f"chunks per (tile, wave) {facts['chunks'].min()} .. {facts['chunks'].max()}")
    return facts


def ran_on_owner_plan(layer):
    from torch_rgcn import _native
    graph = layer._graph
    assert graph._plans.get(("win", "bwd_own", _native.bwd_own_rows(graph.num_nodes))) is not None, "the relation-owner backward did not run"


def many_tiles_all_accumulators(fix):
    """the assertions that keep the 121-relation cases from passing vacuously; skips on a device where the shape does not give them"""
    facts = need_owner_plan(fix, SHORT_TILES, 3)
    if facts["n_tiles"] % facts["n_cu"] == 0:
        pytest.skip("every workgroup walks the same number of tiles on this device")
    assert facts["units_per_wave"].max() == facts["per_wave"], "no wave uses all of its accumulators"
    assert (facts["chunks"] % 2 == 1).any(), "no wave has an odd chunk count in any tile"
    return facts


# ----------------------------------------------------------------------------- 1, 2: the accumulator selection
@tex.BOTH
def test_every_accumulator_many_tiles_per_workgroup(vertical):
    """R = 121 on 40-row tiles: three or four tiles per workgroup, every accumulator case of at least one wave, odd chunk counts"""
    many_tiles_all_accumulators("own_r60")
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact("own_r60", 16, 16, vertical=vertical, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_owner_plan(layer)


@tex.BOTH
def test_units_of_several_waves_add_into_one_relation(vertical):
    """R = 11: the large relations are cut into owned parts, the parts of one relation sit in several waves and flush into one dW_r"""
    facts = need_owner_plan("own_r5", SHORT_TILES, 3)
    assert facts["units_per_relation"].max() > 1 and max(facts["waves_per_relation"]) > 1, (facts["units_per_relation"], facts["waves_per_relation"])
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact("own_r5", 16, 16, vertical=vertical, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_owner_plan(layer)


# ----------------------------------------------------------------------------- 3: the ReLU mask of the epilogue
def test_relu_masked_two_layer_step(monkeypatch):
    """l2(l1.forward_activated(X, "relu", private=True)) on the 121-relation shape: layer 2's backward runs the masked kernel (dX BEFORE
    layer 1's ReLU).  Layer 1 is the identity -- the self-loop relation's weight is I (its val is 1), every other weight and the bias 0 -- so
    its output is X, layer 2's input relu(X) is integer-valued, and X.grad is layer 2's masked dX itself: compared with the oracle's dX of
    layer 2 at relu(X), zeroed where X <= 0.  dW and db of layer 2 are exact too"""
    from torch_rgcn import _native
    many_tiles_all_accumulators("own_r60")
    fx = tex.fixture("own_r60")
    N, R, tp, val = fx["N"], fx["R"], fx["tp"], fx["val"][False]
    params, bias, X, g, _, _ = tex.exact_case("own_r60", False, 16, 16, "none", False, False, False, 3, 2, 2, 0.5, 0)
    W2 = params["weights"]
    A = np.maximum(X, 0)
    ex.assert_provably_exact(tp, val, N, R, A, params, "none", bias, g)
    dA, dW2, db2 = oracle.rgcn_backward(tp, val, N, R, A, W2, g, True)
    want_dX = dA * (X > 0)
    self_rel = int(tp[-1, 1])
    assert (tp[tp[:, 1] == self_rel][:, 0] == tp[tp[:, 1] == self_rel][:, 2]).all() and (val[tp[:, 1] == self_rel] == 1).all()
    W1 = np.zeros_like(W2)
    W1[self_rel] = np.eye(16, dtype=np.float32)

    masks = []
    inner = _native.bwd_own
    monkeypatch.setattr(_native, "bwd_own", lambda *a, relu=False, **kw: (masks.append(relu), inner(*a, relu=relu, **kw))[1])
    with routes.override(**SHORT_TILES):
        l1 = tex.make_layer(fx, {"weights": W1}, np.zeros(16, np.float32), 16, 16, "none", False, False, 3, 2, False)
        l2 = tex.make_layer(fx, params, bias, 16, 16, "none", False, False, 3, 2, False)
        Xd = tex._dev(X).requires_grad_(True)
        a = l1.forward_activated(Xd, "relu", private=True)
        out = l2(a)
        out.backward(tex._dev(g))
        ran_on_owner_plan(l2)
    assert masks == [True, False], masks                        # layer 2 masked with its input, layer 1 plain
    ex.assert_equal_exact(a, A, "relu(layer 1)")
    ex.assert_equal_exact(Xd.grad, want_dX, "dX (layer 2, masked)", fx["deg_o"])
    ex.assert_equal_exact(l2.weights.grad, dW2, "dW2")
    ex.assert_equal_exact(l2.bias.grad, db2, "db2")
    assert (want_dX != dA).any(), "the mask changes nothing on these inputs"


# ----------------------------------------------------------------------------- 4: the bias-gradient stream
def test_bias_stream_node_count_off_every_grid():
    """N = 40 003: G ends 3 rows = 12 float4 past a multiple of the stream's stride; db exact (with everything else)"""
    need_owner_plan("own_r60_n40003", SHORT_TILES, 3)
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact("own_r60_n40003", 16, 16, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_owner_plan(layer)


def test_bias_stream_one_tile_per_workgroup():
    """the default tile height at N = 33 000: one tile per workgroup, one boundary -- what it does not cover is the loop's"""
    facts = need_owner_plan("own_r5_n33000", ONE_TILE, 1)
    assert facts["n_tiles"] <= facts["n_cu"], facts["n_tiles"]
    with routes.override(**ONE_TILE):
        _, layer = tex.run_exact("own_r5_n33000", 16, 16, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_owner_plan(layer)


@pytest.mark.parametrize("fix", ["own_r60", "own_r60_n40003"])
def test_between_guard_bands(monkeypatch, fix):
    """G, X, the parameters, dX and dW / db in guarded allocations: no store outside them, and a load outside them meets NaN"""
    need_owner_plan(fix, SHORT_TILES, 3)
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact(fix, 16, 16, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), guard=gb.Guard(monkeypatch))
        ran_on_owner_plan(layer)
