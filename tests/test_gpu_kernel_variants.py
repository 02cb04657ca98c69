"""Every kernel instantiation the launchers of rgcn_kernels.hip, rgcn_bwd.hip and rgcn_gemm.hip can select, run on exact inputs.

Most launchers choose a template instantiation at launch time from a tuning option (spmm_u, wgrad_rg, wgrad_u, bwd_nw) or from the padded
width, and the rest of the suite only ever runs the default.  Here the `_native` wrappers are called directly on hand-built message lists
whose plan geometry is chosen (tests/kernel_variants.py: chunk counts 0, 1, U - 1, U, U + 1, 2U, 2U + 1 per work unit, pads inside
chunks, full last chunks, hub pieces cut at no multiple of U, ragged relation groups, ragged last tiles and workgroups), options are set
with routes.patch, and every result is compared with the float64 reference under assert_equal_exact: no tolerance anywhere.  The
conditions that make that legitimate (exactness bound, plan geometry, the table against the kernel census) are checked on the CPU in
tests/test_kernel_variants_host.py.  The GEMM forms are run by tests/test_gpu_gemm.py (kernel_variants.gemm_coverage)."""
import functools

import numpy as np
import pytest
import torch
from torch_rgcn import routes

import exact_inputs as ex
import kernel_variants as kv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV).to(dtype)


@functools.lru_cache(maxsize=None)
def _plan(case_fn, args, **kw):
    """device plan of a case, built once per geometry (read-only: kernels only read plans)"""
    from torch_rgcn import _native
    case = case_fn(*args)
    return case, _native.DevicePlan(case.plan(**kw), DEV)


@functools.lru_cache(maxsize=None)
def _forward_ref(case_fn, args, d_in, d_out, bias, relu):
    case = case_fn(*args)
    X, W, b, _ = case.inputs(d_in, d_out, bias=bias)
    kv.assert_exact(case, X, W, b)
    return X, W, b, kv.reference(case, X, W, b, relu=relu)["out"]


def _check_forward(fn, case_fn, args, plan, d_in, d_out, bias, relu, xdtype=torch.float32):
    X, W, b, ref = _forward_ref(case_fn, args, d_in, d_out, bias, relu)
    out = fn(_dev(X, xdtype), _dev(W), _dev(b), plan, relu=relu)
    assert out.dtype == xdtype
    deg = np.bincount(case_fn(*args).dst, minlength=plan.n_dst)
    ex.assert_equal_exact(out, ref, f"out {d_in}x{d_out} bias={bias} relu={relu} n_split={plan.n_split}", deg)


# ----------------------------------------------------------------------------- hidden-16 forward: every (U, packed)
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("U", kv.SPMM_U)
def test_spmm_d16(monkeypatch, U, packed):
    """spmm_d16_kernel<U, PACKED>: unit chunk counts 0, 1, U - 1, U, U + 1, 2U, 2U + 1 on the plan of whole tiles; the same plan cut into
    pieces of 3 chunks (boundaries at no multiple of U) with a bias, which only the FIRST piece may add, and without; relu on whole tiles"""
    from torch_rgcn import _native
    routes.patch(monkeypatch, "spmm_u", U)
    case, whole = _plan(kv.spmm16_case, (), want_pack=packed)
    _, pieces = _plan(kv.spmm16_case, (), want_pack=packed, max_unit_chunks=kv.SPMM16_PIECE)
    assert whole.n_split == 0 and pieces.n_split > 0 and (whole.pack is not None) == packed
    for plan, bias, relu in ((whole, True, False), (whole, True, True), (whole, False, False), (pieces, True, False), (pieces, False, False)):
        _check_forward(_native.spmm, kv.spmm16_case, (), plan, 16, 16, bias, relu)


# ----------------------------------------------------------------------------- wide and generic forward
WIDE_PAIRS = [(a, b) for a in kv.WIDTHS16 for b in kv.WIDTHS16]


@pytest.mark.parametrize("d_in,d_out", [p for p in WIDE_PAIRS if p != (16, 16)], ids=lambda v: str(v))
def test_spmm_wide(d_in, d_out):
    """spmm_wide_kernel<NI, NJ, U, 0>, every width pair but 16 x 16 (which is spmm_d16_kernel's): packed, bias and relu; hub pieces with bias"""
    from torch_rgcn import _native
    _, whole = _plan(kv.wide_case, (), want_pack=True)
    _, pieces = _plan(kv.wide_case, (), want_pack=True, max_unit_chunks=kv.WIDE_PIECE)
    assert whole.pack is not None and whole.n_split == 0 and pieces.n_split > 0
    _check_forward(_native.spmm, kv.wide_case, (), whole, d_in, d_out, True, True)
    _check_forward(_native.spmm, kv.wide_case, (), pieces, d_in, d_out, True, False)


@pytest.mark.parametrize("d_in,d_out", WIDE_PAIRS, ids=lambda v: str(v))
def test_spmm_bf16(d_in, d_out):
    """rgcn_spmm_bf16, all 16 width pairs: without hub pieces (BF = 3: bf16 rows out of the kernel, relu fused) and with them (BF = 1: fp32
    scratch, then round4_bf16_kernel); 16 x 16 is spmm_d16_kernel<4, true, BF>.  The result is the exact sum rounded once."""
    from torch_rgcn import _native
    _, whole = _plan(kv.wide_case, (), want_pack=True)
    _, pieces = _plan(kv.wide_case, (), want_pack=True, max_unit_chunks=kv.WIDE_PIECE)
    _check_forward(_native.spmm_bf16, kv.wide_case, (), whole, d_in, d_out, True, True, BF)
    _check_forward(_native.spmm_bf16, kv.wide_case, (), pieces, d_in, d_out, True, False, BF)


@pytest.mark.parametrize("d_in,d_out", kv.GENERIC_WIDTHS, ids=lambda v: str(v))
def test_spmm_generic(d_in, d_out):
    """spmm_generic_kernel<1 | 2 | 4 | 8> (d_out <= 16, 32, 64, above) on an unpacked plan of 24-row tiles (132 padded columns fit the tile budget)"""
    from torch_rgcn import _native
    _, whole = _plan(kv.wide_case, (24,))
    _, pieces = _plan(kv.wide_case, (24,), max_unit_chunks=kv.WIDE_PIECE)
    assert whole.pack is None and whole.n_split == 0 and pieces.n_split > 0
    _check_forward(_native.spmm, kv.wide_case, (24,), whole, d_in, d_out, True, True)
    _check_forward(_native.spmm, kv.wide_case, (24,), pieces, d_in, d_out, True, False)


# ----------------------------------------------------------------------------- weight gradients
@functools.lru_cache(maxsize=None)
def _wgrad_ref(case_fn, args, d_in, d_out):
    case = case_fn(*args)
    X, W, _, G = case.inputs(d_in, d_out, bias=False)
    kv.assert_exact(case, X, W, None, G)
    return X, G, kv.reference(case, X, W, None, G)["dW"]


@pytest.mark.parametrize("U", kv.WGRAD_U)
@pytest.mark.parametrize("RG", kv.WGRAD_RG)
def test_wgrad_tiled(monkeypatch, RG, U):
    """wgrad_tiled_d16_kernel<RG, U> over (relations, tiles, tiles per item): ragged last relation group (R = 19), the chunk_rel lookup of
    RG > 1, chunk_at across the runs of an item (runs of up to 5 chunks), items of 0, 1, U, U + 1 chunks, fewer blocks than work lists,
    and 12 tiles per item, which the launcher clamps to the 8 the kernel holds"""
    from torch_rgcn import _native
    routes.patch(monkeypatch, "wgrad_rg", RG)
    routes.patch(monkeypatch, "wgrad_u", U)
    for R, n_tiles, tpi in kv.WGRAD_TILED_COMBOS:
        _, plan = _plan(kv.wgrad_tiled_case, (R, n_tiles), want_runs=True)
        X, G, ref = _wgrad_ref(kv.wgrad_tiled_case, (R, n_tiles), 16, 16)
        dW = _native.wgrad_tiled(_dev(X), _dev(G), plan, R, tiles_per_item=tpi)
        ex.assert_equal_exact(dW, ref, f"dW R={R} n_tiles={n_tiles} tiles_per_item={tpi}")


@pytest.mark.parametrize("max_item_chunks", [64, 4])
@pytest.mark.parametrize("d_in,d_out", kv.WGRAD_WIDTHS, ids=lambda v: str(v))
def test_wgrad(d_in, d_out, max_item_chunks):
    """wgrad_d16_kernel<4> (items of 1, 4, 5, 3 chunks: its 4-way unrolled loop with and without a tail) and wgrad_generic_kernel<1, 1>, <2, 4>"""
    from torch_rgcn import _native
    case, plan = _plan(kv.relmajor_case, (), tile_rows=100, max_item_chunks=max_item_chunks)
    X, G, ref = _wgrad_ref(kv.relmajor_case, (), d_in, d_out)
    ex.assert_equal_exact(_native.wgrad(_dev(X), _dev(G), plan, case.R), ref, "dW")


@pytest.mark.parametrize("max_item_chunks", [64, 4])
@pytest.mark.parametrize("d_in,d_out", kv.WGRAD_BF16_WIDTHS, ids=lambda v: str(v))
def test_wgrad_bf16(d_in, d_out, max_item_chunks):
    """the bf16 instantiations: bf16 X and G (small integers: exact), fp32 dW"""
    from torch_rgcn import _native
    case, plan = _plan(kv.relmajor_case, (), tile_rows=100, max_item_chunks=max_item_chunks)
    X, G, ref = _wgrad_ref(kv.relmajor_case, (), d_in, d_out)
    ex.assert_equal_exact(_native.wgrad_bf16(_dev(X, BF), _dev(G, BF), plan, case.R), ref, "dW")


# ----------------------------------------------------------------------------- lean backward
@functools.lru_cache(maxsize=None)
def _lean_ref(n_tiles, relu):
    case = kv.lean_case(n_tiles)
    X, W, _, G = case.inputs(16, 16, bias=False)
    kv.assert_exact(case, X, W, None, G)
    ref = kv.reference(case, X, W, None, G, relu_input=relu)
    return X, W, G, ref["dX"], ref["dW"]


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
@pytest.mark.parametrize("atomic", [True, False], ids=["atomic", "deterministic"])
@pytest.mark.parametrize("nw", kv.LEAN_NW)
def test_bwd_lean(monkeypatch, nw, atomic, relu):
    """bwd_lean_d16_kernel<16, 3, ...> and <8, 1, ...>: 1, NW - 1, NW, NW + 1 and 2 NW + 3 tiles (a lone wave, a workgroup short of one
    wave, full, one wave over, three workgroups with a ragged last one) and 2100 tiles, where the deterministic reduction runs in S > 1
    slabs.  Deterministic mode twice: bitwise equal."""
    from torch_rgcn import _native
    routes.patch(monkeypatch, "bwd_kernel", "lean")
    routes.patch(monkeypatch, "bwd_nw", nw)
    for n_tiles in kv.lean_tiles(nw) + (kv.LEAN_BIG_TILES,):
        case, plan = _plan(kv.lean_case, (n_tiles,), want_pack=True, want_runs=True)
        assert _native.bwd_fused_ok(plan) and not _native._bwd_blk_plan(plan)
        X, W, G, dX_ref, dW_ref = _lean_ref(n_tiles, relu)
        Xd, Wd, Gd = _dev(X), _dev(W), _dev(G)
        dX, dW = _native.bwd_fused(Gd, Xd, Wd, plan, atomic=atomic, relu=relu)
        deg = np.bincount(case.src, minlength=case.n_src)
        ex.assert_equal_exact(dX, dX_ref, f"dX n_tiles={n_tiles}", deg)
        ex.assert_equal_exact(dW, dW_ref, f"dW n_tiles={n_tiles}")
        if not atomic:
            dX2, dW2 = _native.bwd_fused(Gd, Xd, Wd, plan, atomic=False, relu=relu)
            assert torch.equal(dX, dX2) and torch.equal(dW, dW2), f"n_tiles={n_tiles}: two deterministic runs differ"


@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_bwd_scatter_dw(relu):
    """bwd_scatter_dw_d16_kernel<4, RELU> on the relation-major plan of the transposed graph, items of 1, 4, 5 and 3 chunks: the item's
    share of dW, and the transformed row of every live slot, Y[slot] = val G[plan src] W_r^T (masked with X[plan dst] > 0), which the
    second pass sums per row"""
    from torch_rgcn import _native
    base = kv.relmajor_case()
    # the transposed graph: plan rows = the forward sources.  Same buckets, read as (src <- dst)
    case = kv.Case("relmajor_t", base.tiles, base.tile_rows, base.n_rows, base.n_cols, base.R, seed=base.seed, side="src")
    hp = case.plan(tile_rows=case.n_rows)
    plan = _native.DevicePlan(hp, DEV)
    X, W, _, G = case.inputs(16, 16, bias=False)
    kv.assert_exact(case, X, W, None, G)
    ref = kv.reference(case, X, W, None, G)
    Xd, Wd, Gd = _dev(X), _dev(W), _dev(G)
    Wtp = _native.pack_w16t(Wd)
    Y = torch.zeros((hp.m_pad, 16), device=DEV)
    dW = torch.empty_like(Wd)
    _native._check(_native.lib().rgcn_bwd_scatter_dw_f32(Gd.data_ptr(), Xd.data_ptr(), Wtp.data_ptr(), Y.data_ptr(), dW.data_ptr(), plan.src.data_ptr(),
                                                         plan.dst.data_ptr(), plan.val.data_ptr(), plan.chunk_rel.data_ptr(), plan.items.data_ptr(),
                                                         plan.n_items, case.R, 16, _native.F_RELU if relu else 0, _native._stream(Gd.device)), "bwd_scatter_dw")
    ex.assert_equal_exact(dW, ref["dW"], "dW")
    # per slot: plan.src = row of G (forward destination), plan.dst = row of X (forward source; < 0: pad, never written)
    ps, pd, pv = hp.src[:hp.m_pad].astype(np.int64), hp.dst[:hp.m_pad].astype(np.int64), hp.val[:hp.m_pad].astype(np.float64)
    rel = np.repeat(hp.chunk_rel[:hp.n_chunks], 16)
    Yref = np.zeros((hp.m_pad, 16))
    live = pd >= 0
    Yref[live] = pv[live, None] * np.einsum("mo,mio->mi", G[ps[live]].astype(np.float64), W[rel[live]].astype(np.float64))
    if relu:
        Yref[live] *= X[pd[live]] > 0
    ex.assert_equal_exact(Y, Yref, "Y (transformed rows per slot)")
    dX = np.zeros((case.n_src, 16))
    np.add.at(dX, pd[live], Yref[live])
    np.testing.assert_array_equal(dX, kv.reference(case, X, W, None, G, relu_input=relu)["dX"])      # the slots' rows are the reference's messages


def test_single_order_weight_packs():
    """rgcn_pack_w16_f32 / rgcn_pack_w16t_f32: the single-order packs of the C ABI (the wrappers pack both orders in one launch with
    rgcn_pack_w16_pair_f32): the same fragments as the pair's halves"""
    from torch_rgcn import _native
    W = _dev(ex.ints((5, 16, 16), -9, 9, 1.0, 3))
    Wp, Wtp = _native._packed_w16(W)
    a, b = torch.empty_like(W), torch.empty_like(W)
    _native._check(_native.lib().rgcn_pack_w16_f32(W.data_ptr(), a.data_ptr(), 5, _native._stream(W.device)), "pack_w16")
    _native._check(_native.lib().rgcn_pack_w16t_f32(W.data_ptr(), b.data_ptr(), 5, _native._stream(W.device)), "pack_w16t")
    assert torch.equal(a, Wp) and torch.equal(b, Wtp)
    w, got = W.cpu().numpy(), a.cpu().numpy().reshape(5, 4, 16, 4)          # Wp[r][k][o][c] = W[r][4k + c][o]
    np.testing.assert_array_equal(got, w.reshape(5, 4, 4, 16).transpose(0, 1, 3, 2))
    gott = b.cpu().numpy().reshape(5, 4, 16, 4)                             # Wtp[r][k][f][c] = W[r][f][4k + c]
    np.testing.assert_array_equal(gott, w.reshape(5, 16, 4, 4).transpose(0, 2, 1, 3))


# ----------------------------------------------------------------------------- the other launcher forms of rgcn_kernels.hip / rgcn_gemm.hip
@pytest.mark.parametrize("n,d,bf", [(1000, 16, False), (1000, 10, False), (1000, 16, True), (1000, 10, True), (300, 500, False)],
                         ids=["vec4", "scalar", "vec4-bf16", "scalar-bf16", "wide"])
def test_colsum(n, d, bf):
    """colsum_a_kernel<VEC4, BF> + colsum_b_kernel, and the wide pair: integer rows, the column sums exact"""
    from torch_rgcn import _native
    G = ex.ints((n, d), -3, 3, 1.0, n + d)
    got = _native.colsum_bf16(_dev(G, BF)) if bf else _native.colsum(_dev(G))
    ex.assert_equal_exact(got, G.astype(np.float64).sum(0), "db")


OTHER = {
    # id: (routes, run_exact arguments, kernel tags that must run)
    "two-pass": (dict(sparse_path="1", spmm_csr="0"), dict(fix="plain", d_in=16, d_out=16, relu=True), ("spmm_scatter", "bwd_scatter_dw", "segment_sum")),
    "two-pass-hub": (dict(sparse_path="1", spmm_csr="0"), dict(fix="hub10", d_in=16, d_out=16, split="csr"), ("spmm_scatter", "segment_sum")),
    "two-pass-scatter": (dict(sparse_path="1", spmm_csr="0", twopass="scatter"), dict(fix="plain", d_in=16, d_out=16), ("spmm_scatter", "segment_sum")),
    "diag": (dict(), dict(fix="wide", d_in=32, d_out=32, mode="diag"), ("diag_spmm", "diag_wgrad")),
    "diag-30": (dict(), dict(fix="wide", d_in=30, d_out=30, mode="diag"), ("diag_spmm", "diag_wgrad")),
    "diag-bf16": (dict(), dict(fix="wide", d_in=32, d_out=32, mode="diag", dtype=BF), ("diag_spmm_bf16", "diag_wgrad_bf16")),
    "diag-bf16-30": (dict(), dict(fix="wide", d_in=30, d_out=30, mode="diag", dtype=BF), ("diag_spmm_bf16", "diag_wgrad_bf16")),
    "diag-bf16-hub": (dict(), dict(fix="widehub10", d_in=32, d_out=32, mode="diag", dtype=BF, split="csr"), ("diag_spmm_bf16",)),
    "featureless-csr": (dict(featureless_csr="1"), dict(fix="plain", d_in=None, d_out=16, featureless=True), ("featureless_csr_fwd", "featureless_csr_wgrad")),
    "featureless-tile": (dict(featureless_csr="0"), dict(fix="plain", d_in=None, d_out=16, featureless=True), ("featureless_fwd", "featureless_wgrad")),
    "wide-two-pass-48x80": (dict(), dict(fix="wide", d_in=48, d_out=80, vmax=1), ("rel_rows", "segment_sum_wide", "rel_wgrad")),
    "wide-two-pass-7x130": (dict(), dict(fix="wide", d_in=7, d_out=130, vmax=1), ("rel_rows", "segment_sum_wide", "rel_wgrad")),
}


@pytest.mark.parametrize("case", sorted(OTHER))
def test_other_entry_points(monkeypatch, case):
    """the launcher forms of the two files that no tuning option selects -- they depend on a route or on the width alone: one exact layer
    (tests/test_gpu_exact.py's run_exact: forward and backward against the float64 oracle, equality) per form"""
    from test_gpu_exact import run_exact
    switches, kw, expect = OTHER[case]
    for k, v in switches.items():
        routes.patch(monkeypatch, k, v)
    kw = dict(kw)
    run_exact(kw.pop("fix"), kw.pop("d_in"), kw.pop("d_out"), expect=expect, **kw)


@pytest.mark.parametrize("d", [50, 52], ids=["scalar", "vec4"])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_distmult_forms(monkeypatch, storage, bwd, d):
    """distmult_fwd_kernel, distmult_bwd_kernel and the ten distmult_bwd_all_kernel forms: sides 1 and 2 with the relation table (csr),
    both sides without it (split), element loads (d = 50) and quarter-row loads (52), fp32 and bf16 entity tables"""
    if storage == "fp32":
        from test_gpu_exact import distmult_exact
        distmult_exact(monkeypatch, bwd, d, True)
    else:
        from test_gpu_bf16_lp import distmult_bf16_exact
        distmult_bf16_exact(monkeypatch, bwd, d, (), gmax=2)
