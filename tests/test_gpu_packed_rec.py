"""The packed chunk records (96 bytes per chunk + a val dictionary) on the GPU: the native packer writes the bytes of its
torch twin, and rgcn_spmm_blk_* / rgcn_bwd_own_* return on packed records EXACTLY what they return on the wide ones.

The inputs are those of tests/exact_inputs.py -- small integers, vals that are multiples of one power of two q, every sum bounded by
2^23 q (asserted below from the message list, before a kernel runs) -- so every sum is exact in fp32 in any order and two launches of a
kernel that adds in arrival order return identical tensors; a difference between the two record formats is then a wrong field."""
import types

import numpy as np
import pytest
import torch
from torch_rgcn import _native, routes

import exact_inputs as ex
import guard_bands as gb
import test_gpu_exact as tex
import test_gpu_own_static as town       # noqa: F401  (registers the own_* fixtures in tex.FIX)
import test_packed_rec_host as host

pytestmark = pytest.mark.gpu
DEV = tex.DEV
VMAX = 2
WIDE = dict(packed_rec="0")


# ----------------------------------------------------------------------------- message lists
def fixture_messages(name):
    """(dst, src, rel, val, N, R, q) of a pow2 fixture under horizontal stacking: out[s] += val X[o] W_p"""
    fx = tex.fixture(name)
    tp, val = fx["tp"], fx["val"][False]
    return tp[:, 0].astype(np.int32), tp[:, 2].astype(np.int32), tp[:, 1].astype(np.int32), val.astype(np.float32), fx["N"], fx["R"], float(val.min())


def random_messages(N, R, M, vals, q, seed):
    rng = np.random.default_rng(seed)
    vals = np.asarray(vals, np.float32)
    return (rng.integers(0, N, M).astype(np.int32), rng.integers(0, N, M).astype(np.int32), rng.integers(0, R, M).astype(np.int32),
            vals[rng.integers(0, len(vals), M)], N, R, q)


def full_bucket_messages(n_tiles, rows, per_tile, v):
    """one relation, every (tile, relation) bucket a multiple of 16 messages: a plan without pads and with ONE val"""
    assert per_tile % 16 == 0
    rng = np.random.default_rng(9)
    N = n_tiles * rows
    tile = np.repeat(np.arange(n_tiles), per_tile)
    a = (tile * rows + rng.integers(0, rows, len(tile))).astype(np.int32)
    b = (tile * rows + rng.integers(0, rows, len(tile))).astype(np.int32)       # sources in the same tile: the transposed plan has full buckets too
    return a, b, np.zeros(len(tile), np.int32), np.full(len(tile), v, np.float32), N, 1, float(v)


def assert_sums_exact(dst, src, rel, val, N, R, q):
    """every val is a multiple of q, and sum|terms| / q <= 2^23 for every output row, every gradient row, every relation's dW and db, with
    |X|, |W|, |G|, |bias| <= VMAX: a term of out / dX is val x (16 products), a term of dW val x (one product)"""
    k = val.astype(np.float64) / q
    assert np.array_equal(k, np.rint(k)) and q == 2.0 ** round(np.log2(q)), "vals are not multiples of a power of two"
    lim = 2.0 ** ex.MAX_BITS
    row_term = 16 * VMAX * VMAX
    assert (np.bincount(dst, k, N).max() * row_term + VMAX / q) <= lim
    assert np.bincount(src, k, N).max() * row_term <= lim
    assert np.bincount(rel, k, R).max() * VMAX * VMAX <= lim
    assert N * VMAX <= lim


def reference(dst, src, rel, val, N, R, X, W, bias, G, relu):
    """float64 numpy: out, dX (masked with X > 0 when relu: X is then the ReLU's output), dW, db"""
    f = np.float64
    X, W, G, v = X.astype(f), W.astype(f), G.astype(f), val.astype(f)[:, None]
    out = np.zeros((N, 16), f)
    np.add.at(out, dst, v * np.einsum("mi,mio->mo", X[src], W[rel]))
    out += bias.astype(f)
    dX = np.zeros((N, 16), f)
    np.add.at(dX, src, v * np.einsum("mo,mio->mi", G[dst], W[rel]))
    dW = np.zeros((R, 16, 16), f)
    np.add.at(dW, rel, (v * X[src])[:, :, None] * G[dst][:, None, :])
    return (np.maximum(out, 0) if relu else out), (dX * (X > 0) if relu else dX), dW, G.sum(0)


# ----------------------------------------------------------------------------- plans and inputs
def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def plans(msgs, rows):
    """(forward plan, relation-owner plan of the transposed list) on `rows`-row tiles, built on the device"""
    dst, src, rel, val, N, R, _ = msgs
    d, s, r, v = t32(dst), t32(src), t32(rel), t32(val)
    nw, per_wave, max_rows = _native.bwd_own_geometry()
    fwd = _native.build_softwin_plan(d, s, r, v, None, N, N, R, rows)
    own = _native.build_softwin_plan(s, d, r, v, None, N, N, R, rows, own_waves=nw, own_per_wave=per_wave, own_shared=True)
    assert fwd is not None and own is not None and rows <= max_rows
    return fwd, own


def inputs(N, R, seed, dtype=torch.float32):
    rng = np.random.default_rng(seed)
    X, G = ex.ints((N, 16), -VMAX, VMAX, 0.7, rng), ex.ints((N, 16), -VMAX, VMAX, 0.7, rng)
    W, bias = ex.ints((R, 16, 16), -VMAX, VMAX, 1.0, rng), ex.ints((16,), -VMAX, VMAX, 1.0, rng)
    return X, G, W, bias, t32(X).to(dtype), t32(G).to(dtype), t32(W), t32(bias)


def same(a, b, name):
    assert (a is None) == (b is None), name
    if a is not None:
        assert a.dtype == b.dtype and a.shape == b.shape and not torch.isnan(a.float()).any(), name
        assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} elements differ between packed and wide records"


def both_formats(msgs, rows, seed, bf16=False, expect="packed"):
    """forward (relu off / on) and owner backward (relu off / on, with and without db) under the default and under packed_rec=0"""
    _, _, _, _, N, R, _ = msgs
    assert_sums_exact(*msgs)
    fwd, own = plans(msgs, rows)
    assert _native.blk_rec_format(fwd) == expect and _native.blk_rec_format(own, owner=True) == expect
    with routes.override(**WIDE):
        assert _native.blk_rec_format(fwd) == "wide" and _native.blk_rec_format(own, owner=True) == "wide"
    X, G, W, bias, Xd, Gd, Wd, bd = inputs(N, R, seed, torch.bfloat16 if bf16 else torch.float32)
    spmm = _native.spmm_blk_bf16 if bf16 else _native.spmm_blk
    bwd = _native.bwd_own_bf16 if bf16 else _native.bwd_own
    res = {}
    for relu in (False, True):
        got = spmm(Xd, Wd, bd, fwd, relu=relu)
        with routes.override(**WIDE):
            same(got, spmm(Xd, Wd, bd, fwd, relu=relu), f"out (relu={relu})")
        res["out", relu] = got
    Xr = torch.relu(Xd)
    for relu in ((False,) if bf16 else (False, True)):       # (rgcn_bwd_own_bf16 has no masked form)
        for want_db in (False, True):
            xin = Xr if relu else Xd
            got = bwd(Gd, xin, Wd, own, relu=relu, want_db=want_db)
            with routes.override(**WIDE):
                ref = bwd(Gd, xin, Wd, own, relu=relu, want_db=want_db)
            for name, a, b in zip(("dX", "dW", "db"), got, ref):
                same(a, b, f"{name} (relu={relu}, db={want_db})")
            res["bwd", relu, want_db] = got
    assert getattr(fwd, "_blk_rec_pk", None) is not None or expect == "wide"
    return fwd, own, res, (X, G, W, bias)


def against_reference(msgs, res, arrays):
    """the small cases: the packed results against float64 numpy as well"""
    dst, src, rel, val, N, R, _ = msgs
    X, G, W, bias = arrays
    for relu in (False, True):
        out, dX, dW, db = reference(dst, src, rel, val, N, R, np.maximum(X, 0) if relu else X, W, bias, G, relu)
        if not relu:
            ex.assert_equal_exact(res["out", False], out, "out")
        else:
            ex.assert_equal_exact(res["out", True], reference(dst, src, rel, val, N, R, X, W, bias, G, True)[0], "relu(out)")
        got = res["bwd", relu, True]
        ex.assert_equal_exact(got[0], dX, f"dX (relu={relu})")
        ex.assert_equal_exact(got[1], dW, f"dW (relu={relu})")
        ex.assert_equal_exact(got[2], db, f"db (relu={relu})")


# ----------------------------------------------------------------------------- 4: the native packer writes the twin's bytes
def test_device_record_equals_the_torch_twin():
    p = host.small_plan()
    want = _native.pack_rec_torch(p.src, p.dst, p.val, p.chunk_rel, host.ROWS, host.N)
    d = _native.packed_rec_dictionary(p.dst[:p.m_pad], p.val[:p.m_pad])
    on_dev = types.SimpleNamespace(src=p.src.to(DEV), dst=p.dst.to(DEV), val=p.val.to(DEV), chunk_rel=p.chunk_rel.to(DEV), pack=None,
                                   tile_rows=host.ROWS, n_src=host.N)
    d_dev = _native.packed_rec_dictionary(on_dev.dst[:p.m_pad], on_dev.val[:p.m_pad])
    assert torch.equal(d_dev.cpu(), d)
    got = _native._blk_rec(on_dev, d_dev).cpu()
    assert got.numel() == want.numel() == 1024 + 96 * p.n_chunks
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ, the first at {int((got != want).nonzero()[0])}"


def test_torch_description_equals_the_wide_record():
    """rec_fields_torch -- the reference of the CPU round trip and the first stage of the torch packer -- against the bytes
    rgcn_bwd_blk_prepare_f32 writes for the same plan: 16 x {src << 6, val}, 16 x u16 row << 6, the relation word"""
    p = host.small_plan()
    src, row, bits, rel, unit = _native.rec_fields_torch(p.src, p.dst, p.val, p.chunk_rel, host.ROWS)
    on_dev = types.SimpleNamespace(src=p.src.to(DEV), dst=p.dst.to(DEV), val=p.val.to(DEV), chunk_rel=p.chunk_rel.to(DEV), pack=None,
                                   tile_rows=host.ROWS, n_src=host.N)
    wide = _native._blk_rec(on_dev).cpu()[:176 * p.n_chunks].view(p.n_chunks, 176)
    slots = wide[:, :128].contiguous().view(torch.int32).view(p.n_chunks, 16, 2)
    assert torch.equal(slots[:, :, 0].reshape(-1), src << 6) and torch.equal(slots[:, :, 1].reshape(-1), bits)
    assert torch.equal(wide[:, 128:160].contiguous().view(torch.int16).to(torch.int32).reshape(-1), row << 6)
    assert torch.equal(wide[:, 160:164].contiguous().view(torch.int32).reshape(-1), rel | (unit << 16))


# ----------------------------------------------------------------------------- 5: exact parity
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_parity_121_relations_many_tiles(bf16):
    """N = 40 003, R = 121 on 40-row tiles: every accumulator case, 3-4 tiles per workgroup, odd chunk counts, a ragged last tile"""
    msgs = fixture_messages("own_r60_n40003")
    fwd, own, _, _ = both_formats(msgs, 40, 1, bf16=bf16)
    nw = _native.bwd_own_geometry()[0]
    assert fwd.n_tiles == 1001 and msgs[4] % 40 != 0
    per_wave = (own.unit_rel.view(nw, -1) >= 0).sum(1)
    assert int(per_wave.max()) == _native.bwd_own_geometry()[1], "no wave uses all of its accumulators"
    chunks = (own.group_ptr[1:] - own.group_ptr[:-1]).view(own.n_tiles, nw + 1)[:, :nw]
    assert bool((chunks % 2 == 1).any()), "no wave has an odd chunk count in any tile"


def test_parity_11_relations_shared_group():
    msgs = fixture_messages("own_r5")
    _, own, _, _ = both_formats(msgs, 40, 2)
    assert own.group_ptr is not None and own.shared_rel >= 0, "the plan has no shared self-loop group"


def test_parity_one_relation():
    msgs = random_messages(12_000, 1, 30_000, [1.0, 0.5, 0.25], 0.25, 3)
    _, _, res, arrays = both_formats(msgs, 40, 3)
    against_reference(msgs, res, arrays)


def test_parity_one_val_no_pads():
    msgs = full_bucket_messages(300, 40, 32, 0.5)
    fwd, own, res, arrays = both_formats(msgs, 40, 4)
    assert not bool((fwd.dst[:fwd.m_pad] < 0).any()) and not bool((own.dst[:own.m_pad] < 0).any()), "the plan has pads"
    assert fwd._pk_dict.tolist() == [0x3F000000] and own._pk_dict.tolist() == [0x3F000000]
    against_reference(msgs, res, arrays)


def test_parity_256_vals():
    """vals (k + 1) / 256, k < 256, on a plan WITHOUT pads (the pads' +0.0f would be a 257th pattern): multiples of 2^-8"""
    dst, src, rel, _, N, R, _ = full_bucket_messages(300, 40, 32, 1.0)
    val = ((np.arange(len(dst)) % 256 + 1) / 256.0).astype(np.float32)
    msgs = (dst, src, rel, val, N, R, 2.0 ** -8)
    fwd, own, res, arrays = both_formats(msgs, 40, 5)
    assert fwd._pk_dict.numel() == 256 and own._pk_dict.numel() == 256
    against_reference(msgs, res, arrays)


# ----------------------------------------------------------------------------- 6: what packed does not take runs on wide records
def test_fallback_257_vals():
    dst, src, rel, _, N, R, _ = full_bucket_messages(300, 40, 48, 1.0)
    val = ((np.arange(len(dst)) % 257 + 1) / 512.0).astype(np.float32)
    msgs = (dst, src, rel, val, N, R, 2.0 ** -9)
    fwd, own, res, arrays = both_formats(msgs, 40, 6, expect="wide")
    assert fwd._pk_dict is False and own._pk_dict is False and getattr(fwd, "_blk_rec_pk", None) is None
    against_reference(msgs, res, arrays)


def test_fallback_per_call_plan():
    """a plan built without host statistics (the per-call graphs of the LP layer, sync-free): wide records, no look at its vals"""
    msgs = random_messages(12_000, 3, 30_000, [1.0, 0.5, 0.25], 0.25, 7)
    dst, src, rel, val, N, R, _ = msgs
    assert_sums_exact(*msgs)
    plan = _native.build_plan_device(t32(dst), t32(src), t32(rel), t32(val), None, N, N, R, 128, len(dst), want_runs=True, sync_free=True)
    assert plan.units_host is None
    X, G, W, bias, Xd, _, Wd, bd = inputs(N, R, 7)
    assert _native.blk_rec_format(plan) == "wide"
    out = _native.spmm_blk(Xd, Wd, bd, plan)
    assert getattr(plan, "_blk_rec_pk", None) is None and getattr(plan, "_pk_dict", None) is False
    ex.assert_equal_exact(out, reference(dst, src, rel, val, N, R, X, W, bias, G, False)[0], "out")


# ----------------------------------------------------------------------------- 7: guard bands
def test_between_guard_bands(monkeypatch):
    """plan arrays, the packed record buffer (dictionary + records: exactly rgcn_bwd_blk_packed_rec_bytes, NO slack -- a lane reads 4 or
    8 bytes inside its chunk's 96, chunks past a range re-read the range's last chunk, the workgroup reads the dictionary's 1024 bytes),
    the dictionary handed to the packer, inputs and outputs in guarded allocations through one forward and one backward: no band is
    damaged, and a load outside would have met NaN -- the results equal the unguarded ones."""
    msgs = fixture_messages("own_r5")
    _, _, _, _, N, R, _ = msgs
    fwd0, own0 = plans(msgs, 40)
    _, _, _, _, Xd, Gd, Wd, bd = inputs(N, R, 8)
    want_out = _native.spmm_blk(Xd, Wd, bd, fwd0, relu=True)
    want = _native.bwd_own(Gd, Xd, Wd, own0, relu=False, want_db=True)
    with gb.Guard(monkeypatch) as guard:
        fwd, own = plans(msgs, 40)
        for p, owner in ((fwd, False), (own, True)):
            assert _native.blk_rec_format(p, owner=owner) == "packed"
            p._pk_dict = guard.home(p._pk_dict)
        Xg, Gg, Wg, bg = (guard.home(t) for t in (Xd, Gd, Wd, bd))
        out = _native.spmm_blk(Xg, Wg, bg, fwd, relu=True)
        got = _native.bwd_own(Gg, Xg, Wg, own, relu=False, want_db=True)
        for p in (fwd, own):
            assert guard._inside(p._blk_rec_pk.data_ptr()) and p._blk_rec_pk.numel() == 1024 + 96 * p.chunk_rel.shape[0]
        problems = guard.problems("packed records")
    assert not problems, "\n".join(problems)
    same(out, want_out, "out")
    for name, a, b in zip(("dX", "dW", "db"), got, want):
        same(a, b, name)
