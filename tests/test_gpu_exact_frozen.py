"""Exact-arithmetic parity with part of the inputs FROZEN: every autograd function of torch_rgcn/functional.py branches on
ctx.needs_input_grad, and the branches pick other kernels (the fused backward kernels run only when X and W both want a gradient; the
featureless basis kernels get a null output pointer for the frozen side; the tile launcher replaces its fused kernel by a stand-alone one).

The gradient of a tensor does not depend on which OTHER tensors are frozen, so a frozen case has the reference of the all-trainable case:
the same cached exact_case of tests/test_gpu_exact.py, compared by equality.  run_exact(frozen=...) switches requires_grad off before the
forward and asserts afterwards that every frozen tensor has .grad None and that every other result equals the oracle.  Profile tags
(expect / forbid) and launch counts (counts: the forward and the feature gradient share a tag) are derived from functional.py and
_native.py, not from a run.  Fixtures and sizes are those of test_gpu_exact.py.

Autograd function -> tests (each differentiable input frozen at least once):
    _RelationalMP              test_relational_wave_owned, test_relational_sparse_buckets, test_relational_soft_window_big,
                               test_relational_block_tile_backward, test_relational_relu_frozen_features, test_relational_other_widths,
                               test_lp_layer_frozen
    _MatmulMFMA                test_dense_weights_from_decomposition (A, B), test_lp_layer_frozen (block-80: A = X, B = blocks_self)
    _BasisMP                   test_basis_aggregate_then_gemm
    _BlockMP                   test_block_kernels_frozen, test_lp_layer_frozen
    _DiagMP                    test_diagonal_kernels_frozen
    _FeaturelessMP             test_featureless_frozen
    _FeaturelessBasisMP        test_featureless_basis_source_major_frozen, test_featureless_basis_tile_frozen,
                               test_featureless_basis_small_blocks_frozen
    _RelationalMPBF16          test_bf16_wave_owned_frozen, test_bf16_native_frozen
    _BlockMPBF16               test_bf16_block_frozen
    _DiagMPBF16                test_bf16_diagonal_frozen
    _BlockSelfMPBF16           test_bf16_lp_block_self_frozen
    _FeaturelessBasisMPBF16    test_bf16_featureless_basis_tile_frozen
    _TripleScore               test_distmult_frozen, test_distmult_all_frozen_scores_only
    (wrapper flags no layer reaches: test_wrappers_without_bias_gradient)
Out of scope: _ShardedRelationalMP (needs a process group), _MaskedCE and _BCEWithLogits (one differentiable input), the two-layer
ReLU-token chain (its hidden activation is not integer-valued)."""
import pytest
import torch
from torch_rgcn import routes

import exact_inputs as ex
from test_gpu_exact import (BF, DEV, FORBID16, FP32_TAGS, NATIVE16, TWO_PASS_BWD, WAVE16, _dev, distmult_exact, exact_case,
                            fixture, make_layer, run_exact)

pytestmark = pytest.mark.gpu


def ids(sets):
    return pytest.mark.parametrize("frozen", sets, ids=["+".join(s) for s in sets])


# ----------------------------------------------------------------------------- _RelationalMP, width 16
REL_SETS = [("X",), ("weights",), ("bias",), ("X", "weights")]


def _rel16_tags(frozen, fwd, dx, dw, fused, fused_has_db=False):
    """expect / forbid / counts of a width-16 _RelationalMP case.  fwd, dx: the tags of the forward and of the stand-alone feature gradient
    (the same kernel on the transposed plan; a tuple of tags, one launch each per pass); dw: the tag of the stand-alone weight gradient; fused:
    the tags of the route's one-walk backward (() where the all-trainable case has none: hub-split plans); fused_has_db: that kernel sums the
    bias gradient on the side (no colsum launch)"""
    fz = set(frozen)
    both = "X" not in fz and "weights" not in fz
    runs_fused = both and bool(fused)
    expect, forbid, counts = list(fwd), [], {}
    passes = {t: 1 for t in fwd}
    if runs_fused:
        expect += fused
        forbid += [dw] + [t for t in dx if t not in fwd and t not in fused]
    else:
        forbid += [t for t in ("bwd_fused", "bwd_scatter_dw") if t not in fwd]
        if "X" not in fz:
            for t in dx:
                passes[t] = passes.get(t, 0) + 1
            expect += dx
        else:
            forbid += [t for t in dx if t not in fwd]
        if "weights" not in fz:
            expect.append(dw)
            counts[dw] = 1
        else:
            forbid.append(dw)
    for t, n in passes.items():
        if t not in fused or not runs_fused:
            counts[t] = n
    if "bias" in fz or (runs_fused and fused_has_db):
        forbid.append("colsum")
    else:
        expect.append("colsum")
        counts["colsum"] = 1
    return dict(expect=tuple(expect), forbid=tuple(forbid), counts=counts)


@ids(REL_SETS)
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub12", "plan")])
def test_relational_wave_owned(monkeypatch, fix, split, frozen):
    """sparse_path=0: rgcn_spmm_f32 forward.  All trainable on plain: bwd_fused (lean kernel, colsum on the side).  X or W frozen: the fused
    kernel must NOT run -- spmm on the transposed plan alone, or wgrad / wgrad_tiled (both tagged wgrad) alone; {X, weights}: colsum only.
    hub12: the hub-split plan has no fused backward either way (spmm + wgrad), freezing only drops launches"""
    routes.patch(monkeypatch, "sparse_path", "0")
    kw = _rel16_tags(frozen, ("spmm",), ("spmm",), "wgrad", ("bwd_fused",) if split is None else ())
    kw["forbid"] += ("spmm_csr", "spmm_scatter", "spmm_blk")
    run_exact(fix, 16, 16, frozen=frozen, split=split, **kw)


@ids(REL_SETS)
@pytest.mark.parametrize("csr", ["1", "0"], ids=["one-pass-csr", "two-pass"])
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub10", "csr")])
def test_relational_sparse_buckets(monkeypatch, fix, split, csr, frozen):
    """sparse_path=1: all trainable runs bwd_two_pass_fused (bwd_scatter_dw + segment_sum).  X frozen: wgrad alone; W frozen: the two-pass
    spmm on the transposed graph (spmm_scatter + segment_sum) alone; in neither case rgcn_bwd_scatter_dw_f32"""
    routes.patch(monkeypatch, "sparse_path", "1")
    routes.patch(monkeypatch, "spmm_csr", csr)
    fwd = ("spmm_csr",) if csr == "1" else ("spmm_scatter", "segment_sum")
    kw = _rel16_tags(frozen, fwd, ("spmm_scatter", "segment_sum"), "wgrad", TWO_PASS_BWD)
    kw["forbid"] += ("spmm", "bwd_fused") + (("spmm_csr",) if csr == "0" else ())
    if set(frozen) == {"bias"}:               # the fused two-pass backward: its segment_sum comes on top of the forward's
        kw["counts"]["segment_sum"] = 1 + (csr == "0")
        kw["counts"]["bwd_scatter_dw"] = 1
    run_exact(fix, 16, 16, frozen=frozen, split=split, **kw)


@ids(REL_SETS)
def test_relational_soft_window_big(frozen):
    """the soft-window forward (spmm_blk).  All trainable: the relation-owner backward (tag bwd_fused, db on the side).  X or W frozen: it
    must not run, and the layer never asks the graph for its plan; dX is rgcn_spmm_f32 on the transposed plan, dW wgrad"""
    from torch_rgcn import _native
    kw = _rel16_tags(frozen, ("spmm_blk",), ("spmm",), "wgrad", ("bwd_fused",), fused_has_db=True)
    _, layer = run_exact("big", 16, 16, frozen=frozen, **kw)
    graph = layer._graph
    own = graph._plans.get(("win", "bwd_own", _native.bwd_own_rows(graph.num_nodes)))
    assert (own is not None) == (set(frozen) == {"bias"}), "the relation-owner plan is built exactly when its kernel runs"


@ids(REL_SETS)
def test_relational_block_tile_backward(monkeypatch, frozen):
    """bwd_kernel=blk, bwd_own=0 on big_r9: all trainable runs rgcn_bwd_blk_f32 (tag bwd_fused, db on the side); frozen X or W: never"""
    routes.patch(monkeypatch, "bwd_kernel", "blk")
    routes.patch(monkeypatch, "sparse_path", "0")
    routes.patch(monkeypatch, "bwd_own", "0")
    fz = set(frozen)
    fused = fz == {"bias"}
    expect = ("bwd_fused",) if fused else (() if "weights" in fz else ("wgrad",)) + (() if "X" in fz else ("spmm",))
    forbid = ("wgrad", "colsum") if fused else ("bwd_fused",) + (("wgrad",) if "weights" in fz else ())
    run_exact("big_r9", 16, 16, frozen=frozen, expect=expect + (() if "bias" in fz or fused else ("colsum",)), forbid=forbid)


@pytest.mark.parametrize("vertical", [False, True], ids=["horizontal", "vertical"])
def test_relational_relu_frozen_features(monkeypatch, vertical):
    """relu=True with X frozen: the upstream gradient is masked with the stored output BEFORE the stand-alone weight gradient and colsum
    (the vertical case of this group)"""
    routes.patch(monkeypatch, "sparse_path", "0")
    run_exact("plain", 16, 16, relu=True, vertical=vertical, frozen=("X",), expect=("spmm", "wgrad", "colsum"), forbid=("bwd_fused",),
              counts={"spmm": 1, "wgrad": 1})


@ids([("X",), ("weights",)])
@pytest.mark.parametrize("d_in,d_out", [(10, 11), (48, 80)], ids=lambda v: str(v))
def test_relational_other_widths(monkeypatch, d_in, d_out, frozen):
    """(10, 11): padded to 16 x 16 (all trainable: bwd_fused), resize3 back with and without db; (48, 80): the gather-GEMM alone
    (rel_rows + segment_sum_wide for dX) or rgcn_rel_wgrad_f32 alone"""
    x = "X" in frozen
    if max(d_in, d_out) > 64:
        counts = {"rel_rows": 1 if x else 2, "segment_sum_wide": 1 if x else 2, "rel_wgrad": 1 if x else 0, "colsum": 1}
        run_exact("wide", d_in, d_out, vmax=1, frozen=frozen, expect=("rel_rows", "segment_sum_wide"), forbid=() if x else ("rel_wgrad",),
                  counts=counts, seed=d_in + d_out)
    else:
        routes.patch(monkeypatch, "sparse_path", "0")
        run_exact("plain", d_in, d_out, frozen=frozen, expect=("spmm", "colsum"), forbid=("bwd_fused",) + (() if x else ("wgrad",)),
                  counts={"spmm": 1 if x else 2, "wgrad": 1 if x else 0, "colsum": 1}, seed=d_in + d_out)


# ----------------------------------------------------------------------------- dense weights assembled from a decomposition
@pytest.mark.parametrize("mode,frozen", [("basis", ("comps",)), ("basis", ("bases",)), ("block", ("blocks",))], ids=lambda v: str(v))
def test_dense_weights_from_decomposition(monkeypatch, mode, frozen):
    """16 x 16.  basis: W = matmul_mfma(comps, bases) feeds relational_mp -- W still wants its gradient (bwd_fused), _MatmulMFMA returns
    dA (comps) or dB (bases) as None: two gemm launches (forward + one adjoint) instead of three.  block, 4 x 4 blocks frozen: W = block_diag()
    needs no gradient -- spmm on the transposed plan alone"""
    routes.patch(monkeypatch, "sparse_path", "0")
    if mode == "basis":
        run_exact("plain", 16, 16, mode="basis", num_bases=3, vmax=1, frozen=frozen, expect=("gemm", "spmm", "bwd_fused"), forbid=("wgrad",),
                  counts={"gemm": 2, "spmm": 1})
    else:
        run_exact("plain", 16, 16, mode="block", num_blocks=4, vmax=1, frozen=frozen, expect=("spmm", "colsum"),
                  forbid=("bwd_fused", "wgrad", "block_spmm"), counts={"spmm": 2})


# ----------------------------------------------------------------------------- _BasisMP
@ids([("X",), ("bases",), ("comps",), ("X", "comps"), ("X", "bases", "comps")])
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
def test_basis_aggregate_then_gemm(fix, split, frozen):
    """64 x 64, B = 3.  Launches: basis_aggregate forward (+ dX), gemm forward (+ d_ag when X or comps want a gradient, + dbases),
    basis_dcomps for comps.  {X, comps}: d_ag is not formed; {X, bases, comps}: bias only"""
    fz = set(frozen)
    x, b, c = "X" not in fz, "bases" not in fz, "comps" not in fz
    counts = {"basis_aggregate": 1 + x, "gemm": 1 + (x or c) + b, "basis_dcomps": int(c), "colsum": 1}
    run_exact(fix, 64, 64, mode="basis", vmax=1, num_bases=3, frozen=frozen, expect=("basis_aggregate", "gemm", "colsum"),
              forbid=() if c else ("basis_dcomps", "basis_dcomps_csr"), counts=counts, split=split)


# ----------------------------------------------------------------------------- _BlockMP, _DiagMP
@pytest.mark.parametrize("nb,b,relu,frozen", [(20, 4, False, ("X",)), (20, 4, False, ("blocks",)), (20, 4, True, ("X",)), (20, 4, True, ("blocks",)),
                                               (100, 5, False, ("X",)), (100, 5, False, ("blocks",))], ids=lambda v: str(v))
def test_block_kernels_frozen(nb, b, relu, frozen):
    """block_path=2: X frozen -- one block_spmm (the forward) and block_wgrad; blocks frozen -- two block_spmm, no block_wgrad"""
    x = "X" in frozen
    with routes.override(block_path="2"):
        run_exact("narrow" if nb == 100 else "wide", nb * b, nb * b, mode="block", num_blocks=nb, relu=relu, vmax=1, frozen=frozen,
                  expect=("block_spmm", "colsum"), forbid=("spmm", "rel_rows") + (() if x else ("block_wgrad",)),
                  counts={"block_spmm": 1 if x else 2, "block_wgrad": 1 if x else 0})


@ids([("X",), ("weights",)])
@pytest.mark.parametrize("fix,split", [("wide", None), ("widehub10", "csr")])
def test_diagonal_kernels_frozen(fix, split, frozen):
    x = "X" in frozen
    run_exact(fix, 30, 30, mode="diag", frozen=frozen, expect=("diag_spmm",), forbid=("spmm",) + (() if x else ("diag_wgrad",)),
              counts={"diag_spmm": 1 if x else 2, "diag_wgrad": 1 if x else 0}, split=split)


# ----------------------------------------------------------------------------- featureless layers
@ids([("weights",), ("bias",)])
@pytest.mark.parametrize("route", ["1", "0"], ids=["csr", "tile"])
def test_featureless_frozen(monkeypatch, route, frozen):
    """the weight table frozen: bias only (colsum, no table gradient kernel); the bias frozen: no colsum"""
    routes.patch(monkeypatch, "featureless_csr", route)
    fwd, wg = ("featureless_csr_fwd", "featureless_csr_wgrad") if route == "1" else ("featureless_fwd", "featureless_wgrad")
    other = ("featureless_fwd", "featureless_wgrad") if route == "1" else ("featureless_csr_fwd", "featureless_csr_wgrad")
    w = "weights" in frozen
    run_exact("plain", None, 16, featureless=True, frozen=frozen, expect=(fwd, "colsum") if w else (fwd, wg),
              forbid=other + ((wg,) if w else ("colsum",)))


FB_SETS = [("bases",), ("comps",), ("bases", "comps")]


SM_SETS = [(s, "0") for s in FB_SETS + [("bias",)]] + [(s, "1") for s in FB_SETS]      # (the deterministic kernels differ in the table gradients only)


@pytest.mark.parametrize("frozen,det", SM_SETS, ids=["+".join(s) + ("-deterministic" if det == "1" else "") for s, det in SM_SETS])
@pytest.mark.parametrize("B,d", [(4, 10), (30, 16)])
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub10", "fbasis")])
def test_featureless_basis_source_major_frozen(monkeypatch, fix, split, B, d, frozen, det):
    """the source-major kernels of rgcn_basis.hip.  {bases}: rgcn_fbasis_bwd_dc_f32 (deterministic: rgcn_fbasis_bwd_f32 + the row sum of T) with
    a null dbases; {comps}: rgcn_fbasis_bwd_f32 with a null T and no row sum; {bases, comps}: no launch at all -- this call used to raise
    'fbasis_bwd: bad argument' (both output pointers null) in the backward of a layer whose bias still trains; {bias}: no colsum"""
    if det == "1":
        routes.patch(monkeypatch, "deterministic", "1")
    fz = set(frozen)
    none = fz == {"bases", "comps"}
    run_exact(fix, None, d, mode="basis", featureless=True, num_bases=B, vmax=1, frozen=frozen,
              expect=("fbasis_fwd",) + (() if none else ("fbasis_bwd",)) + (() if "bias" in fz else ("colsum",)),
              forbid=("fbasis_tile_fwd", "fbasis_tile_bwd", "fbasis_small_bwd") + (("fbasis_bwd",) if none else ()) + (("colsum",) if "bias" in fz else ()),
              counts={} if none else {"fbasis_bwd": 1}, split=split)


@ids(FB_SETS)
@pytest.mark.parametrize("mode", ["ranges", "nodes"])
@pytest.mark.parametrize("fix,B,d", [("n3001", 40, 10), ("n16", 5, 10)])
def test_featureless_basis_tile_frozen(monkeypatch, fix, B, d, mode, frozen):
    """the tile kernels (fbasis_inplace_mb=0).  The launcher starts a kernel only for a gradient that is wanted: mode nodes with one side
    frozen runs the stand-alone fbn_dbases_kernel / fbn_dcomps_kernel where the all-trainable call runs the fused fbn_bwd_kernel (asserted
    below from the launcher's own predicate; the tag is the same); {bases, comps}: the wrapper returns before any launch"""
    from torch_rgcn import _native
    routes.patch(monkeypatch, "fbasis_inplace_mb", "0")
    routes.patch(monkeypatch, "fbasis_tile", mode)
    none = set(frozen) == {"bases", "comps"}
    _, layer = run_exact(fix, None, d, mode="basis", featureless=True, num_bases=B, vmax=1, frozen=frozen,
                         expect=("fbasis_tile_fwd", "colsum") + (() if none else ("fbasis_tile_bwd",)),
                         forbid=("fbasis_fwd", "fbasis_bwd") + (("fbasis_tile_bwd",) if none else ()), split="fbasis" if fix == "n3001" else None)
    if mode == "nodes" and fix == "n3001":        # (n16's B = 5 is below the fused kernel's 16 bases: two kernels there in any case)
        assert _native.lib().rgcn_fbasis_tile_bwd_fused_gn(layer.num_relations, B, d, layer.num_nodes) > 0, \
            "the all-trainable call of this shape does not take the fused kernel: freezing one side changes no kernel here"


@ids([("bases",), ("comps",)])
@pytest.mark.parametrize("fix", ["plain", "hub10"])
def test_featureless_basis_small_blocks_frozen(monkeypatch, fix, frozen):
    """B = 2, d = 16, away from the source-major route: rgcn_fbasis_small_bwd_f32 computes both gradients in one walk; the function hands
    back None for the frozen one"""
    routes.patch(monkeypatch, "fbasis", "csr")
    run_exact(fix, None, 16, mode="basis", featureless=True, num_bases=2, vmax=1, frozen=frozen,
              expect=("basis_aggregate", "fbasis_small_bwd", "colsum"), forbid=("fbasis_fwd", "fbasis_bwd", "fbasis_tile_bwd", "basis_dcomps"),
              counts={"basis_aggregate": 1, "fbasis_small_bwd": 1})


# ----------------------------------------------------------------------------- bf16 twins
@ids([("X",), ("weights",), ("bias",)])
@pytest.mark.parametrize("d_in,d_out", [(16, 16), (10, 16)], ids=lambda v: str(v))
@pytest.mark.parametrize("fix,split", [("plain", None), ("hub12", "plan")])
def test_bf16_wave_owned_frozen(fix, split, d_in, d_out, frozen):
    """rgcn_spmm_bf16 forward (+ dX), rgcn_wgrad_bf16, rgcn_colsum_bf16: one launch each, for what is wanted"""
    fz = set(frozen)
    counts = {"spmm_bf16": 1 + ("X" not in fz), "wgrad_bf16": int("weights" not in fz), "colsum_bf16": int("bias" not in fz)}
    run_exact(fix, d_in, d_out, dtype=BF, frozen=frozen, expect=tuple(t for t, n in counts.items() if n),
              forbid=FP32_TAGS + NATIVE16 + tuple(t for t, n in counts.items() if not n), counts=counts, split=split, seed=5)


@ids([("X",), ("weights",), ("bias",)])
def test_bf16_native_frozen(frozen):
    """rgcn_spmm_blk_bf16 / rgcn_bwd_own_bf16: the kernel computes dX and dW in any case, the function hands back None for the frozen one;
    the bias frozen: the kernel gets a null db (its column sum is guarded by the pointer)"""
    run_exact("big", 16, 16, dtype=BF, frozen=frozen, expect=NATIVE16, forbid=FP32_TAGS + WAVE16, counts={"spmm_blk_bf16": 1, "bwd_own_bf16": 1},
              seed=6)


@ids([("X",), ("blocks",)])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_bf16_block_frozen(relu, frozen):
    x = "X" in frozen
    run_exact("wide", 80, 80, mode="block", num_blocks=20, relu=relu, dtype=BF, vmax=1, frozen=frozen, expect=("block_spmm_bf16", "colsum_bf16"),
              forbid=FORBID16 + (() if x else ("block_wgrad_bf16",)), counts={"block_spmm_bf16": 1 if x else 2, "block_wgrad_bf16": 1 if x else 0})


@ids([("X",), ("weights",)])
def test_bf16_diagonal_frozen(frozen):
    x = "X" in frozen
    run_exact("wide", 32, 32, mode="diag", dtype=BF, frozen=frozen, expect=("diag_spmm_bf16",), forbid=FORBID16 + (() if x else ("diag_wgrad_bf16",)),
              counts={"diag_spmm_bf16": 1 if x else 2, "diag_wgrad_bf16": 1 if x else 0})


@ids([("X",), ("blocks",), ("blocks_self",), ("bias",)])
@pytest.mark.parametrize("fix", ["plain", "hub10"])
def test_bf16_lp_block_self_frozen(fix, frozen):
    """_BlockSelfMPBF16 (the LP layer's block-80-bf16 case): block kernels + the dense self-loop product on rgcn_gemm_f32.  gemm launches:
    the forward, g blocks_self^T for dX, X^T g for blocks_self"""
    fz = set(frozen)
    x, b, s = "X" not in fz, "blocks" not in fz, "blocks_self" not in fz
    counts = {"block_spmm_bf16": 1 + x, "block_wgrad_bf16": int(b), "gemm": 1 + x + s, "colsum_bf16": int("bias" not in fz)}
    run_exact(fix, 80, 80, mode="block", num_blocks=20, vmax=1, dtype=BF, lp=True, seed=9, frozen=frozen,
              expect=tuple(t for t, n in counts.items() if n), forbid=FORBID16 + tuple(t for t, n in counts.items() if not n), counts=counts)


@ids(FB_SETS)
@pytest.mark.parametrize("mode", ["ranges", "nodes", "nodes2"])
@pytest.mark.parametrize("fix,B,d", [("n3001", 40, 10), ("n16", 5, 10)])
def test_bf16_featureless_basis_tile_frozen(fix, B, d, mode, frozen):
    """bf16 bases table on the tile kernels: one side frozen -- the stand-alone kernel of the other; both -- no backward launch"""
    none = set(frozen) == {"bases", "comps"}
    with routes.override(fbasis_tile=mode):
        run_exact(fix, None, d, mode="basis", featureless=True, num_bases=B, vmax=1, param_dtypes={"bases": BF}, frozen=frozen,
                  expect=("fbasis_tile_fwd_bf16", "colsum_bf16") + (() if none else ("fbasis_tile_bwd_bf16",)),
                  forbid=("fbasis_tile_fwd", "fbasis_tile_bwd") + (("fbasis_tile_bwd_bf16",) if none else ()),
                  split="fbasis" if fix == "n3001" else None)


# ----------------------------------------------------------------------------- LP layer, eval mode, fp32
@pytest.mark.parametrize("case,frozen", [("none-16", ("X",)), ("none-20x128", ("X",)), ("block-80", ("X",)), ("block-80", ("blocks_self",))],
                         ids=lambda v: str(v))
@pytest.mark.parametrize("fix", ["plain", "hub10"])
def test_lp_layer_frozen(fix, case, frozen):
    """per-call graphs.  none-16: spmm + bwd_fused when all train, X frozen: wgrad alone.  none-20x128: rel_wgrad alone.  block-80: block_mp plus
    matmul_mfma(X, blocks_self) -- X frozen: one block_spmm, block_wgrad, gemm forward + X^T g; blocks_self frozen: gemm forward + g B^T"""
    mode, dims = case.split("-")
    d_in, d_out = (int(dims), int(dims)) if "x" not in dims else map(int, dims.split("x"))
    kw = dict(mode="block", num_blocks=20, vmax=1) if mode == "block" else {}
    x = "X" in frozen
    expect, forbid, counts = {
        "none-16": (("spmm", "wgrad", "colsum"), ("bwd_fused",) + WAVE16, {"spmm": 1, "wgrad": 1}),
        "none-20x128": (("rel_rows", "segment_sum_wide", "rel_wgrad", "colsum"), ("spmm",), {"rel_rows": 1, "segment_sum_wide": 1, "rel_wgrad": 1}),
        "block-80": (("block_spmm", "block_wgrad", "gemm", "colsum"), ("spmm", "rel_rows"), {"block_spmm": 1 if x else 2, "block_wgrad": 1, "gemm": 2}),
    }[case]
    run_exact(fix, d_in, d_out, lp=True, seed=9, frozen=frozen, expect=expect, forbid=forbid, counts=counts, **kw)


# ----------------------------------------------------------------------------- DistMult
DM_SETS = [("nodes",), ("relations",), ("biases",), ("relations", "biases")]


@ids(DM_SETS)
@pytest.mark.parametrize("d", [50, 300])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_distmult_frozen(monkeypatch, bwd, d, frozen):
    """the backward kernels compute every gradient whatever is frozen (the tag set of the all-trainable case, asserted in distmult_exact);
    frozen tensors keep .grad None, the others equal the oracle.  The ranks are counted by the scoring kernel whenever one input wants a
    gradient and the route walks the CSRs"""
    distmult_exact(monkeypatch, bwd, d, True, frozen=frozen)


@pytest.mark.parametrize("d", [50, 300])
@pytest.mark.parametrize("bwd", ["csr", "split", "atomic"])
def test_distmult_all_frozen_scores_only(monkeypatch, bwd, d):
    """nodes, relations and biases frozen: the forward builds no ranks, the scores are exact, nothing runs backward"""
    distmult_exact(monkeypatch, bwd, d, True, frozen=("nodes", "relations", "biases"))


# ----------------------------------------------------------------------------- wrapper flags no layer reaches
@pytest.mark.parametrize("kernel", ["bwd_own", "bwd_own_bf16", "bwd_fused-blk", "bwd_fused-lean"])
def test_wrappers_without_bias_gradient(monkeypatch, kernel):
    """_RelationalMP._backward always asks the fp32 kernels for db; want_db=False (a null db pointer in the relation-owner and block-tile kernels) is
    reached only by calling the wrappers: on the layer's own plan, dX and dW equal to the oracle and no db returned"""
    from torch_rgcn import _native
    fix = {"bwd_own": "big", "bwd_own_bf16": "big", "bwd_fused-blk": "big_r9", "bwd_fused-lean": "plain"}[kernel]
    if kernel.startswith("bwd_fused"):
        routes.patch(monkeypatch, "bwd_kernel", "blk")
        routes.patch(monkeypatch, "bwd_own", "0")
    fx = fixture(fix)
    params, bias, X, g, ref, bits = exact_case(fix, False, 16, 16, "none", False, False, False, 3, 2, 2, 0.5, 0)
    layer = make_layer(fx, params, bias, 16, 16, "none", False, False, 3, 2, False)
    graph = layer._graph_on(torch.device(DEV))
    dtype = BF if kernel == "bwd_own_bf16" else torch.float32
    Xd, gd, W = _dev(X, dtype), _dev(g, dtype), layer.weights.detach().contiguous()
    if graph.perm is not None:          # plans on locality-relabelled ids (as the layer does)
        Xd, gd = Xd.index_select(0, graph.inv).contiguous(), gd.index_select(0, graph.inv).contiguous()
    _native.profile_start()
    if kernel.startswith("bwd_own"):
        plan = graph.win_plan("bwd_own")
        assert plan is not None and not _native._blk_units(plan)[2]
        res = (_native.bwd_own_bf16 if dtype == BF else _native.bwd_own)(gd, Xd, W, plan, want_db=False)
        assert len(res) == 3 and res[2] is None, "want_db=False returned a bias gradient"
    else:
        plan = graph.bwd_blk_plan() if kernel == "bwd_fused-blk" else graph.bwd_plan(16)
        assert plan is not None and bool(_native._bwd_blk_plan(plan)) == (kernel == "bwd_fused-blk") and _native.bwd_fused_ok(plan)
        res = _native.bwd_fused(gd, Xd, W, plan, atomic=True, want_db=False)
        assert len(res) == 2, "want_db=False returned a bias gradient"
    tags = set(_native.profile_stop())
    dX, dW = res[0], res[1]
    if graph.perm is not None:
        dX = dX.index_select(0, graph.perm)
    print(f"[exact] {fix} 16x16 {kernel} want_db=False: tags {sorted(tags)} | proof bits dX {bits['dX']:.1f} weights {bits['weights']:.1f}")
    assert tags == {"bwd_own_bf16" if dtype == BF else "bwd_fused"}, sorted(tags)
    assert dX.dtype == dtype and dW.dtype == torch.float32
    ex.assert_equal_exact(dX, ref["dX"], "dX", fx["deg_o"])
    ex.assert_equal_exact(dW, ref["grads"]["weights"], "dweights")
