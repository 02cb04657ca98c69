"""The shared chunk queue of the relation-owner backward (rgcn_bwd_own_f32 / _bf16 on a plan of own_relations(shared=True)), exactly.

The relation with the most messages belongs to no wave: its chunks are one more group per tile, and every wave that keeps an accumulator
for it (local number K - 1) takes them two at a time from a counter in LDS once its own range is done; the counter is reset at every tile
boundary, a pair past the end of the range repeats the last chunk with val = 0, and the waves' sums of the shared relation leave the
workgroup through the scratch and one wave's atomics.  What can go wrong there -- a chunk dealt twice or never, a stale counter, a sum
flushed twice or not at all -- changes dW of the shared relation or dX by whole messages, so every case compares with the float64 oracle
on the inputs of tests/exact_inputs.py (every sum exact in fp32 in any order): EQUAL, not close.

Each case asserts from the plan that the shared range is not empty and that the relation-owner kernel ran."""
import functools

import numpy as np
import pytest
import torch
from torch_rgcn import routes

import exact_inputs as ex
import guard_bands as gb
import test_gpu_exact as tex
import test_gpu_own_static as static
from oracle import oracle
from test_softwin_plan import random_messages

pytestmark = pytest.mark.gpu
DEV = tex.DEV

# own_sh_r5: 140 000 nodes give 547-row tiles, one per workgroup on 256 CUs: the self loops (35 chunks per tile) are five times any other
# relation (~25 000 messages per relation and direction: 6 or 7 chunks per bucket, cut into owned parts)
FIXTURES = {"own_sh_r5": (140_000, 5, 3000, None, 205)}
for _name, _fix in FIXTURES.items():
    assert tex.FIX.setdefault(_name, _fix) == _fix, _name

SHORT_TILES, ONE_TILE = static.SHORT_TILES, static.ONE_TILE
U = 2                                                        # chunks a wave takes from the queue at a time


@functools.lru_cache(maxsize=None)
def shared_plan_facts(fix, switches):
    """the owner plan of the fixture under the switches, from a layer on zeros: None when the backward would not take the relation-owner
    kernel, else what the cases assert before they run"""
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
        shared = None
        if plan.shared_ptr is not None:
            sp = plan.shared_ptr.cpu().numpy()
            shared = sp[:, 1] - sp[:, 0]
        unit_rel = plan.unit_rel.cpu().numpy().reshape(nw, per_wave)
        return dict(n_tiles=int(plan.n_tiles), tile_rows=int(plan.tile_rows), n_cu=torch.cuda.get_device_properties(DEV).multi_processor_count,
                    shared=shared, shared_rel=plan.shared_rel, shared_local=plan.shared_local, takers=int((unit_rel[:, per_wave - 1] == plan.shared_rel).sum()),
                    units_per_relation=np.bincount(unit_rel[unit_rel >= 0], minlength=fx["R"]),
                    counts=np.bincount(fx["tp"][:, 1], minlength=fx["R"]))


def need_shared_plan(fix, switches, min_tiles_per_wg):
    facts = shared_plan_facts(fix, tuple(sorted(switches.items())))
    if facts is None:
        pytest.skip("the backward of this graph does not take the relation-owner kernel on this device")
    if facts["n_tiles"] < min_tiles_per_wg * facts["n_cu"]:
        pytest.skip(f"{facts['n_tiles']} tiles on {facts['n_cu']} CUs: fewer than {min_tiles_per_wg} per workgroup")
    assert facts["shared"] is not None and facts["shared"].max() > 0, "the plan has no shared group"
    assert facts["takers"] >= 1 and facts["shared_rel"] == int(np.argmax(facts["counts"])), facts
    print(f"[own shared] {fix}: {facts['n_tiles']} tiles of {facts['tile_rows']} rows on {facts['n_cu']} CUs, relation {facts['shared_rel']} shared by "
          f"{facts['takers']} waves, {facts['shared'].min()} .. {facts['shared'].max()} chunks per tile")
    return facts


def ran_on_shared_plan(layer):
    static.ran_on_owner_plan(layer)
    plan = layer._graph.win_plan("bwd_own")
    assert plan.group_ptr is not None and plan.shared_rel >= 0 and int((plan.shared_ptr[:, 1] - plan.shared_ptr[:, 0]).max()) > 0


def odd_range_many_tiles(fix):
    """121 relations on 40-row tiles: the 40 self loops of a tile are 3 shared chunks (the second pair repeats the third chunk with val = 0),
    three or four tiles per workgroup (the counter is reset between them); 120 other relations leave 8 of the 128 slots: 8 waves take"""
    facts = need_shared_plan(fix, SHORT_TILES, 3)
    assert (facts["shared"] % U == 1).any() and facts["shared"].max() == 3, facts["shared"]
    assert 1 <= facts["takers"] < 16, facts["takers"]
    return facts


@tex.BOTH
def test_odd_shared_range_many_tiles_per_workgroup(vertical):
    odd_range_many_tiles("own_r60")
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact("own_r60", 16, 16, vertical=vertical, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_shared_plan(layer)


@tex.BOTH
def test_long_shared_range_beside_owned_parts(vertical):
    """R = 11, the shared relation five times the others, which are cut into owned parts; the shared range of a tile is longer than one pair
    per wave, so the queue hands some wave more than an even split of it (which wave: whichever is done first)"""
    facts = need_shared_plan("own_sh_r5", ONE_TILE, 1)
    others = np.delete(facts["units_per_relation"], facts["shared_rel"])
    assert others.max() > 1, facts["units_per_relation"]
    assert facts["takers"] == 16 and facts["shared"].max() > 16 * U, (facts["takers"], facts["shared"].max())
    assert facts["counts"][facts["shared_rel"]] > 3 * np.delete(facts["counts"], facts["shared_rel"]).max()
    with routes.override(**ONE_TILE):
        _, layer = tex.run_exact("own_sh_r5", 16, 16, vertical=vertical, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_shared_plan(layer)


def _direct(R, rows, n_tiles, shared_tiles, seed):
    """_native.bwd_own on a hand-built message list: relation 0 has 3 * rows messages into each of the first shared_tiles tiles and none into
    the others, the other relations rows / 2 messages into every tile; small integers: every sum exact"""
    from torch_rgcn import _native
    rng = np.random.default_rng(seed)
    N = rows * n_tiles
    nw, per_wave, _ = _native.bwd_own_geometry()
    dst = [rng.integers(0, rows * shared_tiles, 3 * rows * shared_tiles)] + [rng.integers(0, N, rows // 2 * n_tiles) for _ in range(R - 1)]
    rel = np.concatenate([np.full(len(d), r) for r, d in enumerate(dst)])
    dst = np.concatenate(dst)
    src = rng.integers(0, N, len(dst))
    val = rng.choice([0.5, 1.0, 2.0], len(dst))
    t32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(DEV)                                  # noqa: E731
    plan = _native.build_softwin_plan(t32(dst), t32(src), t32(rel), torch.from_numpy(val.astype(np.float32)).to(DEV), None, N, N, R, rows,
                                      own_waves=nw, own_per_wave=per_wave, own_shared=True)
    assert plan.shared_rel == 0 and plan.group_ptr is not None
    sp = plan.shared_ptr.cpu().numpy()
    assert (sp[:shared_tiles, 1] > sp[:shared_tiles, 0]).all() and (sp[shared_tiles:, 1] == sp[shared_tiles:, 0]).all(), sp
    G, X, W = (rng.integers(-2, 3, s).astype(np.float64) for s in ((N, 16), (N, 16), (R, 16, 16)))
    dX, dW = np.zeros((N, 16)), np.zeros((R, 16, 16))
    np.add.at(dX, dst, val[:, None] * np.einsum("mo,mio->mi", G[src], W[rel]))
    np.add.at(dW, rel, val[:, None, None] * X[dst][:, :, None] * G[src][:, None, :])
    f32 = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)                                # noqa: E731
    got = _native.bwd_own(f32(G), f32(X), f32(W), plan, want_db=True)
    torch.cuda.synchronize()
    for name, g, w in zip(("dX", "dW", "db"), got, (dX, dW, G.sum(0))):
        assert np.array_equal(g.cpu().numpy().astype(np.float64), w), f"{name} differs from the float64 sums"


def test_direct_call_empty_shared_range_in_the_last_tile():
    """the shared relation has no message in the last tile: its range there is empty and no wave takes anything from the counter"""
    _direct(R=5, rows=64, n_tiles=5, shared_tiles=4, seed=11)


def test_direct_call_shared_relation_is_the_only_one():
    """one relation: no wave owns anything, every chunk comes from the queue (the first pair of a tile is not requested a tile ahead)"""
    _direct(R=1, rows=64, n_tiles=5, shared_tiles=4, seed=12)


def test_relu_masked_two_layer_step(monkeypatch):
    """test_gpu_own_static's two-layer step (layer 1 the identity, layer 2's backward masked with its input) on the shared plan"""
    from torch_rgcn import _native
    odd_range_many_tiles("own_r60")
    fx = tex.fixture("own_r60")
    N, R, tp, val = fx["N"], fx["R"], fx["tp"], fx["val"][False]
    params, bias, X, g, _, _ = tex.exact_case("own_r60", False, 16, 16, "none", False, False, False, 3, 2, 2, 0.5, 0)
    W2 = params["weights"]
    A = np.maximum(X, 0)
    ex.assert_provably_exact(tp, val, N, R, A, params, "none", bias, g)
    dA, dW2, db2 = oracle.rgcn_backward(tp, val, N, R, A, W2, g, True)
    want_dX = dA * (X > 0)
    self_rel = int(tp[-1, 1])
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
        ran_on_shared_plan(l2)
    assert masks == [True, False], masks
    ex.assert_equal_exact(a, A, "relu(layer 1)")
    ex.assert_equal_exact(Xd.grad, want_dX, "dX (layer 2, masked)", fx["deg_o"])
    ex.assert_equal_exact(l2.weights.grad, dW2, "dW2")
    ex.assert_equal_exact(l2.bias.grad, db2, "db2")
    assert (want_dX != dA).any(), "the mask changes nothing on these inputs"


def test_node_count_off_every_grid():
    """N = 40 003: the last tile has 3 rows -- one shared chunk of 3 self loops"""
    facts = need_shared_plan("own_r60_n40003", SHORT_TILES, 3)
    assert facts["shared"][-1] == 1, facts["shared"][-4:]
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact("own_r60_n40003", 16, 16, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), counts={"bwd_fused": 1})
        ran_on_shared_plan(layer)


def test_between_guard_bands(monkeypatch):
    """the plan's arrays (group_ptr among them), G, X, the parameters, dX and dW / db in guarded allocations"""
    need_shared_plan("own_r60", SHORT_TILES, 3)
    with routes.override(**SHORT_TILES):
        _, layer = tex.run_exact("own_r60", 16, 16, expect=("spmm_blk", "bwd_fused"), forbid=("spmm",), guard=gb.Guard(monkeypatch))
        ran_on_shared_plan(layer)


@pytest.mark.parametrize("masked,R,N,M,rows,level", [(False, 20, 1000, 30000, 128, False), (True, 101, 1000, 60000, 128, False),
                                                     (True, 101, 1000, 60000, 128, True), (False, 121, 1000, 30000, 64, False),
                                                     (True, 1, 900, 30000, 128, False)])
def test_device_built_shared_plan_equals_torch_built(masked, R, N, M, rows, level):
    """rgcn_softwin_fill with waves + 1 groups per tile and the torch-op builder (stable sorts) give the same plan, array for array"""
    from torch_rgcn import _native
    nw, per_wave, _ = _native.bwd_own_geometry()
    dst, src, rel, val, alive = random_messages(N, R, M, masked, 7)
    g = [t if t is None else t.to(DEV) for t in (dst, src, rel, val, alive)]
    kw = dict(own_waves=nw, own_per_wave=per_wave, own_level=level, own_shared=True)
    p = _native.build_softwin_plan(*g, N, N, R, rows, **kw)
    with routes.override(softwin_build="torch"):
        q = _native.build_softwin_plan(*g, N, N, R, rows, **kw)
    assert p.group_ptr is not None and p.group_ptr.shape[0] == p.n_tiles * (nw + 1) + 1 and p.own_ptr.shape[0] == p.n_tiles * nw + 1
    assert (q.m_pad, q.n_chunks, q.n_messages, q.shared_rel, q.shared_local) == (p.m_pad, p.n_chunks, p.n_messages, p.shared_rel, p.shared_local)
    for name in ("group_ptr", "own_ptr", "shared_ptr", "tile_ptr", "unit_rel", "chunk_rel"):
        assert torch.equal(getattr(q, name).cpu(), getattr(p, name).cpu()), name
    assert torch.equal(q.src.cpu()[:p.m_pad], p.src.cpu()[:p.m_pad])


def test_f32_entry_rejects_tables_beyond_32_bit_offsets():
    """the records address G rows as src << 6 in 32 bits: rgcn_bwd_own_f32 refuses n_src >= 2^26 before it launches anything (as the bf16
    entry does), and a shared relation without its group pointers"""
    from torch_rgcn import _native
    f = torch.zeros(4096, device=DEV)
    i = torch.zeros(256, dtype=torch.int32, device=DEV)
    dp, L = _native._dp, _native.lib()
    call = lambda group_ptr, shared_rel, n_src: L.rgcn_bwd_own_f32(dp(f), dp(f), dp(f), dp(f), dp(f), dp(f), dp(i), group_ptr, shared_rel, dp(i), 1, 64, 64, 1,    # noqa: E731
                                                                    0, None, n_src, _native._stream(f.device))
    assert call(None, -1, 1 << 26) != 0 and call(None, -1, 0) != 0
    assert call(None, 0, 64) != 0 and call(dp(i), -1, 64) != 0 and call(dp(i), 1, 64) != 0
