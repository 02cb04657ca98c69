"""CPU checks of tests/kernel_variants.py: what tests/test_gpu_kernel_variants.py relies on holds before any kernel runs.

  * `reference` (float64 numpy from a message list) equals the float64 oracle on a fixture of tests/test_gpu_exact.py;
  * the exactness condition (sum|terms| / q <= 2^23) holds for every case at every width the GPU file runs it with;
  * every plan has the geometry its case claims: chunks per tile, unit chunk counts, hub pieces, pads, full last chunks, straddling runs,
    item chunk totals of the tiled weight gradient, item sizes of the relation-major plan;
  * VARIANTS has exactly the census names of the three kernel files (tools/kernel_census.py);
  * every `unreachable` row names a line of its launcher."""
import importlib.util
import os

import numpy as np
import pytest

import exact_inputs as ex
import kernel_variants as kv
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-rgcn_amd", "csrc")


def _census_tool():
    spec = importlib.util.spec_from_file_location("kernel_census", os.path.join(ROOT, "tools", "kernel_census.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ----------------------------------------------------------------------------- the reference
def test_reference_equals_the_oracle_on_an_exact_fixture():
    """out, dX, dW and db of oracle.nc_layer on the message list of test_gpu_exact.py's `plain` fixture (2000 nodes, 7 relations, val = the
    layer's own normalisation: powers of two), with bias and with the ReLU mask"""
    N, R0, groups, hub, seed = 2000, 3, 1000, None, 101                  # FIX["plain"] of tests/test_gpu_exact.py
    tp = oracle.add_inverse_and_self(ex.pow2_triples(N, R0, groups, hub_log2=hub, seed=seed), N, R0)
    R = 2 * R0 + 1
    val = oracle.nc_edge_norm(tp, N, R, False)

    class Msgs:
        dst, src, rel = tp[:, 0], tp[:, 2], tp[:, 1]
        n_dst = n_src = N
    Msgs.val, Msgs.R = val, R
    rng = np.random.default_rng(5)
    X, W, b, g = ex.ints((N, 16), -2, 2, 0.5, rng), ex.ints((R, 16, 16), -2, 2, 1.0, rng), ex.ints((16,), -2, 2, 1.0, rng), ex.ints((N, 16), -2, 2, 0.5, rng)
    ex.assert_provably_exact(tp, val, N, R, X, {"weights": W}, "none", b, g)
    want = oracle.nc_layer(tp, N, R, X, {"weights": W}, "none", b, False, g)
    got = kv.reference(Msgs, X, W, b, g)
    ex.assert_equal_exact(got["out"], want["out"], "out")
    ex.assert_equal_exact(got["dX"], want["dX"], "dX")
    ex.assert_equal_exact(got["dW"], want["grads"]["weights"], "dW")
    ex.assert_equal_exact(got["db"], want["db"], "db")
    # the layer's ReLU: the oracle is handed the masked gradient (tests/test_gpu_exact.py: exact_case)
    want = oracle.nc_layer(tp, N, R, X, {"weights": W}, "none", b, False, g * (want["out"] > 0))
    got = kv.reference(Msgs, X, W, b, g, relu=True)
    ex.assert_equal_exact(got["out"], np.maximum(want["out"], 0), "relu out")
    ex.assert_equal_exact(got["dX"], want["dX"], "relu dX")
    ex.assert_equal_exact(got["dW"], want["grads"]["weights"], "relu dW")


# ----------------------------------------------------------------------------- exactness of every case
def _all_cases():
    """(case, d_in, d_out, with G) for everything tests/test_gpu_kernel_variants.py launches"""
    out = [(kv.spmm16_case(), 16, 16, False)]
    out += [(kv.wide_case(), a, b, False) for a in kv.WIDTHS16 for b in kv.WIDTHS16]
    out += [(kv.wide_case(24), a, b, False) for a, b in kv.GENERIC_WIDTHS]
    out += [(kv.wgrad_tiled_case(R, nt), 16, 16, True) for R, nt in sorted({(R, nt) for R, nt, _ in kv.WGRAD_TILED_COMBOS})]
    out += [(kv.relmajor_case(), a, b, True) for a, b in kv.WGRAD_WIDTHS + kv.WGRAD_BF16_WIDTHS]
    out += [(kv.lean_case(nt), 16, 16, True) for nt in sorted({n for nw in kv.LEAN_NW for n in kv.lean_tiles(nw)} | {kv.LEAN_BIG_TILES})]
    return out


def test_every_case_is_provably_exact():
    worst = {}
    for case, d_in, d_out, with_g in _all_cases():
        X, W, b, G = case.inputs(d_in, d_out, bias=not with_g)
        bits = kv.assert_exact(case, X, W, b, G if with_g else None)
        assert np.isin(case.val, kv.VALS).all() and set(np.unique(case.val)) == set(kv.VALS.tolist()), case.name
        for k, v in bits.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("[kernel variants] worst proof bits:", {k: round(v, 1) for k, v in worst.items()})
    assert max(worst.values()) <= ex.MAX_BITS


# ----------------------------------------------------------------------------- geometry
def _check_tiles(case, plan):
    got = np.diff(plan.tile_ptr[:plan.n_tiles + 1]).tolist()
    want = case.L + [0] * (case.n_tiles - len(case.L))
    assert plan.n_tiles == case.n_tiles and got == want, (case.name, got, want)
    assert plan.n_messages == len(case.rows) and plan.n_chunks == sum(want)


@pytest.mark.parametrize("make,piece,units_want", [(kv.spmm16_case, kv.SPMM16_PIECE, {0, 1, 2, 3}), (kv.wide_case, kv.WIDE_PIECE, {0, 1, 2, 3}),
                                                   (lambda: kv.wide_case(24), kv.WIDE_PIECE, {0, 1, 2, 3})], ids=["spmm16", "wide32", "wide24"])
def test_forward_plans_have_the_claimed_geometry(make, piece, units_want):
    case = make()
    for packed in (True, False):
        whole = case.plan(want_pack=packed)
        _check_tiles(case, whole)
        assert (whole.pack is not None) == packed and whole.n_split == 0 and whole.n_units == case.n_tiles
        assert (whole.units[:whole.n_units, 2] - whole.units[:whole.n_units, 1]).tolist() == case.unit_chunks(1 << 20)[0]
        pieces = case.plan(want_pack=packed, max_unit_chunks=piece)
        want, ns = case.unit_chunks(piece)
        u = pieces.units[:pieces.n_units]
        assert (u[:, 2] - u[:, 1]).tolist() == want and pieces.n_split == ns > 0 and set(want) == units_want
        first = u[(u[:, 3] & 2) != 0]
        assert len(first) == len({int(t) for t in u[(u[:, 3] & 1) != 0, 0]}), "one FIRST piece per hub tile"
        # piece boundaries inside a tile at no multiple of 2 chunks from the tile's first chunk: every unrolled form meets a ragged piece
        assert any((int(a) - int(pieces.tile_ptr[t])) % 2 for t, a, _, f in u if f & 1), "no piece starts at an odd chunk"
    p = case.plan()
    dst = p.dst[:p.m_pad].reshape(-1, 16)
    assert (dst < 0).any() and case.n_rows % case.tile_rows, "pads inside chunks, a ragged last tile"
    assert 0 in case.L[1:-1] and case.L[-1] == 0 and len(case.L) == p.n_tiles, "an empty tile in the middle and at the end"
    for t in range(p.n_tiles):                       # the last chunk of every tile that has one is full of real messages
        if p.tile_ptr[t + 1] > p.tile_ptr[t]:
            assert (dst[p.tile_ptr[t + 1] - 1] >= 0).all(), t
    # a destination whose messages of one relation run across a chunk boundary
    same = (dst[1:, 0] == dst[:-1, 15]) & (dst[1:, 0] >= 0) & (p.chunk_rel[1:p.n_chunks] == p.chunk_rel[:p.n_chunks - 1])
    assert same.any(), "no run straddles a chunk boundary"
    cnt = np.bincount(case.dst.astype(np.int64) * case.R + case.rel, minlength=case.n_dst * case.R)
    assert cnt.max() >= 16, "no destination with 16 messages of one relation"


def test_spmm16_unit_chunk_counts_cover_every_unrolled_form():
    L = set(kv.spmm16_case().L)
    for U in kv.SPMM_U:
        assert {0, 1, U - 1, U, U + 1, 2 * U, 2 * U + 1} <= L, (U, sorted(L))
    for U in (1, 2):                                 # the wide kernels unroll by 1 or 2
        assert {0, 1, U - 1, U, U + 1, 2 * U, 2 * U + 1} <= set(kv.wide_case().L), U


def test_wgrad_tiled_plans_cover_every_item_shape():
    for R, nt in sorted({(R, nt) for R, nt, _ in kv.WGRAD_TILED_COMBOS}):
        case = kv.wgrad_tiled_case(R, nt)
        plan = case.plan(want_runs=True)
        _check_tiles(case, plan)
        assert plan.run_ptr is not None and case.n_rows % case.tile_rows
    assert {R for R, _, _ in kv.WGRAD_TILED_COMBOS} == {1, 16, 19} and {t for _, t, _ in kv.WGRAD_TILED_COMBOS} == {1, 7, 9, 65}
    assert {t for _, _, t in kv.WGRAD_TILED_COMBOS} == {1, 3, 8, 12}
    blocks = {-(-nt // min(tpi, 8)) for _, nt, tpi in kv.WGRAD_TILED_COMBOS}
    assert any(b < 8 for b in blocks) and any(b > 8 and b % 8 for b in blocks), blocks
    for RG in kv.WGRAD_RG:
        totals, longest = set(), 0
        for R, nt, tpi in kv.WGRAD_TILED_COMBOS:
            case = kv.wgrad_tiled_case(R, nt)
            t, run = kv.wgrad_tiled_item_totals(case, case.plan(want_runs=True), RG, tpi)
            totals |= t
            longest = max(longest, run)
        for U in kv.WGRAD_U:
            assert {0, 1, U, U + 1} <= totals, (RG, U, sorted(totals))
        assert longest >= 3, "no (tile, relation) run of 3 chunks: chunk_at never walks inside a run"
        if RG > 1:
            assert 19 % RG, "R = 19 must leave a ragged last relation group"


def test_relation_major_plan_has_the_claimed_items():
    case = kv.relmajor_case()
    for mic, want in ((64, [1, 4, 5, 3]), (4, [1, 4, 4, 1, 3])):
        p = case.plan(tile_rows=case.n_rows, max_item_chunks=mic)
        assert p.n_tiles == 1 and (p.items[:p.n_items, 1] - p.items[:p.n_items, 0]).tolist() == want
    dst = p.dst[:p.m_pad].reshape(-1, 16)
    rel1 = np.flatnonzero(p.chunk_rel[:p.n_chunks] == 1)
    assert len(rel1) == 4 and (dst[rel1] >= 0).all(), "the 4-chunk relation is whole chunks of real messages"


def test_lean_plans_have_the_claimed_geometry():
    from torch_rgcn import _native
    for nw in kv.LEAN_NW:
        assert kv.lean_tiles(nw) == (1, nw - 1, nw, nw + 1, 2 * nw + 3)
        assert -(-kv.LEAN_BIG_TILES // nw) >= 128, "the deterministic reduction needs n_blocks >= 128 for S > 1"
    for nt in sorted({n for nw in kv.LEAN_NW for n in kv.lean_tiles(nw)} | {kv.LEAN_BIG_TILES}):
        case = kv.lean_case(nt)
        p = case.plan(want_pack=True, want_runs=True)
        _check_tiles(case, p)
        assert p.pack is not None and p.n_split == 0 and p.n_units == p.n_tiles == nt and case.n_rows % case.tile_rows
        assert _native.lib().rgcn_bwd_lean_supported(p.tile_rows)
        run = p.run_ptr.reshape(nt, case.R + 1)
        assert (run[:, 0] == p.tile_ptr[:nt]).all() and (run[:, -1] == p.tile_ptr[1:nt + 1]).all()
    assert -(-kv.LEAN_R // 4) == 3, "three window groups: more than the 8-wave form's one slot group"


# ----------------------------------------------------------------------------- the table
def test_gemm_rows_are_reached_by_the_gemm_tests_shapes():
    """the launcher model against the test it points to: the shapes of test_gemm_layouts_and_edges are the ones listed here"""
    import ast
    src = open(os.path.join(ROOT, "tests", "test_gpu_gemm.py")).read()
    fn = next(n for n in ast.walk(ast.parse(src)) if isinstance(n, ast.FunctionDef) and n.name == "test_gemm_layouts_and_edges")
    marks = {d.args[0].value: ast.literal_eval(d.args[1]) for d in fn.decorator_list}
    assert marks["M,N,K"] == kv.GEMM_TEST_SHAPES and marks["bm"] == ["128", "64", "0"] and len(marks["ta,tb"]) == 4
    cov = kv.gemm_coverage()
    assert len([n for n in cov if n.startswith("gemm_kernel<")]) == 16 and len([n for n in cov if n.startswith("gemm_panel_kernel<")]) == 16


def test_variants_table_equals_the_kernel_census():
    tool = _census_tool()
    try:
        census = {f: tool.census(os.path.splitext(f)[0]) for f in kv.FILES}
    except (tool.ToolMissing, FileNotFoundError) as e:
        pytest.skip(f"no kernel census on this machine: {e}")
    for f in kv.FILES:
        table = kv.names_of(f)
        assert table == census[f], (f, sorted(set(table) - set(census[f])), sorted(set(census[f]) - set(table)))
    for name, row in kv.VARIANTS.items():
        assert ("unreachable" in row) != ("test" in row), name
        if "test" in row:
            assert row["entry"] and row["wrapper"], name


def test_unreachable_rows_name_a_launcher_line():
    rows = kv.unreachable()
    assert rows == sorted(f"spmm_wide_kernel<1, 1, 2, {bf}>" for bf in (0, 1, 3))
    for name in rows:
        row = kv.VARIANTS[name]
        assert kv.launcher_has_line(CSRC, row), (name, row["launcher_line"])
        # and the launcher holds no second way to the form: the wide dispatch sits in the `else` of that line
        text = open(os.path.join(CSRC, row["file"])).read()
        body = text[text.index(f'extern "C" int {row["entry"]}('):]
        body = body[:body.find('extern "C"', 1)]
        assert body.index("if (d_in == 16 && d_out == 16) {") < body.index("switch (d_in / 16)"), name


def test_new_tests_named_in_the_table_exist():
    import ast
    defs = {}
    for f in ("test_gpu_kernel_variants.py", "test_gpu_gemm.py"):
        tree = ast.parse(open(os.path.join(ROOT, "tests", f)).read())
        defs[f] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
    for name, row in kv.VARIANTS.items():
        if "test" in row:
            f, t = row["test"].split("::")
            assert t.split("[")[0] in defs[f], (name, row["test"])
