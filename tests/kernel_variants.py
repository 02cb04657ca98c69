"""Every kernel instantiation the launchers of rgcn_kernels.hip, rgcn_bwd.hip and rgcn_gemm.hip can select: how to reach it, hand-built
message lists whose PLAN GEOMETRY is chosen (not drawn), and a float64 reference straight from the message list.

Many launchers pick a template instantiation at launch time from a tuning option (spmm_u, wgrad_rg, wgrad_u, bwd_nw, gemm_bm) or from
the padded width; `routes.py` says they all "compute the same result".  tests/test_gpu_kernel_variants.py runs each of them on the cases
below and compares with `assert_equal_exact`; tests/test_kernel_variants_host.py checks this file on the CPU (the table against the
kernel census of the device code, the exactness condition of every case, the claimed geometry of every plan).

    VARIANTS          census name -> how to reach it (entry point, wrapper, options, widths, plan properties, the test that runs it) or
                      `unreachable` with the launcher line that shows it
    bucket_messages   messages (rows, cols, rel, val) from a per-tile list of (relation, messages, repeat) buckets
    Case              a message list in forward terms (dst, src, rel, val) and the claims about its plan; .plan(...) builds it with
                      _native.build_plan_host (tile_rows, max_item_chunks, want_runs, want_pack, max_unit_chunks): nothing is patched
    reference         out / dX / dW in float64 numpy from the message list
    exact_bits        the condition of exact_inputs.py, sum|terms| / q <= 2^23 per element, from |inputs| (q = the smallest val: 1/4)

Inputs: val in {1, 1/2, 1/4}, everything else small integers (exact_inputs.ints), so every partial sum in any order is exact in fp32 and
every comparison is equality; a bf16 result is the exact value rounded once."""
import functools
import itertools

import numpy as np

import exact_inputs as ex

VALS = np.array([1.0, 0.5, 0.25], np.float32)
Q = 0.25                       # the grid: the smallest val
CHUNK = 16


# ----------------------------------------------------------------------------- message lists with a chosen geometry

def bucket_messages(tiles, tile_rows, n_rows, n_cols, seed):
    """tiles[t] = [(relation, messages, repeat), ...]: bucket (t, relation) gets `messages` messages; their rows walk the tile's rows
    cyclically from a bucket-specific start, `repeat` messages per row (the plan sorts a bucket by row, so a row's messages are one run).
    cols are drawn, val from VALS; the list is shuffled.  -> rows, cols, rel, val"""
    rng = np.random.default_rng(seed)
    rows, rel = [], []
    for t, buckets in enumerate(tiles):
        row0 = t * tile_rows
        nr = min(tile_rows, n_rows - row0)
        assert not buckets or nr > 0, f"tile {t} lies past row {n_rows}"
        assert len({b[0] for b in buckets}) == len(buckets), f"tile {t}: a relation twice"
        for r, n, rep in buckets:
            start = (5 * r + 3 * t) % nr
            rows.append(row0 + (start + np.arange(n) // rep) % nr)
            rel.append(np.full(n, r, np.int64))
    rows = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    rel = np.concatenate(rel) if rel else np.zeros(0, np.int64)
    M = len(rows)
    cols = rng.integers(0, n_cols, M)
    val = VALS[rng.integers(0, len(VALS), M)]
    order = rng.permutation(M)
    return rows[order].astype(np.int32), cols[order].astype(np.int32), rel[order].astype(np.int32), val[order]


def tile_chunks(buckets):
    return sum(-(-n // CHUNK) for _, n, _ in buckets)


def tile_spec(L, t=0, R=3, rep_last=3):
    """a tile of exactly L chunks: buckets whose size is no multiple of 16 (pads inside chunks) FOLLOWED by a bucket of whole chunks of
    real messages -- the last chunk of the tile is full, so a tail guard that counts it twice shows.  Relations rotate with the tile."""
    rels = sorted((t + i) % R for i in range(min(3, R)))
    if L == 0:
        return []
    if L == 1 or len(rels) == 1:
        return [(rels[-1], CHUNK * L, rep_last)]
    if L == 2 or len(rels) == 2:
        return [(rels[0], CHUNK * (L - 1) - 5, 1), (rels[-1], CHUNK, rep_last)]
    a = (L - 1) // 2
    return [(rels[0], CHUNK * a - 5, 1), (rels[1], 7, 2), (rels[2], CHUNK * (L - a - 1), rep_last)]


class Case:
    """messages in forward terms: out[dst] += val X[src] W[rel].  side: which end the plan tiles -- "dst" (forward plans: spmm, wgrad) or
    "src" (the transposed plan of the feature-gradient kernels: plan rows = src, plan columns = dst)."""

    def __init__(self, name, tiles, tile_rows, n_rows, n_cols, R, seed, side="dst"):
        self.name, self.tiles, self.tile_rows, self.n_rows, self.n_cols, self.R, self.side = name, tiles, tile_rows, n_rows, n_cols, R, side
        rows, cols, rel, val = bucket_messages(tiles, tile_rows, n_rows, n_cols, seed)
        self.rows, self.cols, self.rel, self.val = rows, cols, rel, val
        self.dst, self.src = (rows, cols) if side == "dst" else (cols, rows)
        self.n_dst, self.n_src = (n_rows, n_cols) if side == "dst" else (n_cols, n_rows)
        self.L = [tile_chunks(b) for b in tiles]          # the claim: chunks per tile
        self.seed = seed
        for a in (self.rows, self.cols, self.rel, self.val):
            a.flags.writeable = False

    @property
    def n_tiles(self):
        return -(-self.n_rows // self.tile_rows)

    def plan(self, want_pack=False, want_runs=False, max_unit_chunks=1 << 20, max_item_chunks=64, tile_rows=None):
        """the host plan over `rows` (tile_rows: another height -- n_rows gives the relation-major plan of one tile)"""
        from torch_rgcn import _native
        return _native.build_plan_host(self.rows, self.cols, self.rel, self.val, self.n_rows, self.n_cols, self.R, tile_rows or self.tile_rows,
                                       max_item_chunks=max_item_chunks, want_runs=want_runs, want_pack=want_pack, max_unit_chunks=max_unit_chunks)

    def unit_chunks(self, max_unit_chunks):
        """the claim: chunk counts of the work units when tiles above max_unit_chunks are cut (rgcn_plan_units_host) -> (list, n_split)"""
        out, ns = [], 0
        for L in self.L + [0] * (self.n_tiles - len(self.L)):
            if L <= max_unit_chunks:
                out.append(L)
            else:
                pieces = [min(max_unit_chunks, L - c) for c in range(0, L, max_unit_chunks)]
                out += pieces
                ns += len(pieces)
        return out, ns

    def inputs(self, d_in, d_out, seed=0, bias=True, vmax=2):
        """X [n_src, d_in], W [R, d_in, d_out], bias [d_out], G [n_dst, d_out]: small integers, read-only"""
        rng = np.random.default_rng(1000 * self.seed + 17 * d_in + d_out + seed)
        X = ex.ints((self.n_src, d_in), -vmax, vmax, 1.0, rng)
        W = ex.ints((self.R, d_in, d_out), -vmax, vmax, 1.0, rng)
        b = ex.ints((d_out,), -vmax, vmax, 1.0, rng) if bias else None
        G = ex.ints((self.n_dst, d_out), -vmax, vmax, 1.0, rng)
        for a in (X, W, b, G):
            if a is not None:
                a.flags.writeable = False
        return X, W, b, G


# ----------------------------------------------------------------------------- the float64 reference

def reference(case, X, W, bias=None, G=None, relu=False, relu_input=False):
    """float64, straight from the message list.  out[dst] += val X[src] @ W[rel] (+ bias, relu).  With G: dX[src] += val G[dst] @ W[rel]^T,
    dW[rel] += val X[src]^T G[dst]; relu: G is masked with out > 0 first (the layer's own ReLU); relu_input: X is the output of a ReLU
    and dX is wanted before it -- rows masked with X > 0 (the fused backward kernels' RELU form).  -> dict"""
    dst, src, rel, val = case.dst.astype(np.int64), case.src.astype(np.int64), case.rel.astype(np.int64), case.val.astype(np.float64)
    X64, W64 = np.asarray(X, np.float64), np.asarray(W, np.float64)
    d_out = W64.shape[2]
    out = np.zeros((case.n_dst, d_out))
    for r in range(case.R):
        ix = np.flatnonzero(rel == r)
        if len(ix):
            np.add.at(out, dst[ix], val[ix, None] * (X64[src[ix]] @ W64[r]))
    if bias is not None:
        out += np.asarray(bias, np.float64)
    res = {"out": np.maximum(out, 0) if relu else out}
    if G is None:
        return res
    G64 = np.asarray(G, np.float64) * (out > 0) if relu else np.asarray(G, np.float64)
    dX = np.zeros_like(X64)
    dW = np.zeros_like(W64)
    for r in range(case.R):
        ix = np.flatnonzero(rel == r)
        if len(ix):
            np.add.at(dX, src[ix], val[ix, None] * (G64[dst[ix]] @ W64[r].T))
            dW[r] = (val[ix, None] * X64[src[ix]]).T @ G64[dst[ix]]
    res.update(dX=dX * (X64 > 0) if relu_input else dX, dW=dW, db=G64.sum(0))
    return res


def exact_bits(case, X, W, bias=None, G=None):
    """log2 of max(sum|terms| / q) per tensor: the reference on |inputs|, q = 1/4 (the smallest val; db has no val: q = 1).  Sums that a
    mask or a ReLU shortens are bounded by the unmasked ones."""
    assert np.isin(case.val, VALS).all()
    for a in (X, W, bias, G):
        assert a is None or (np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 256), "inputs must be small integers"
    A = reference(case, np.abs(X), np.abs(W), None if bias is None else np.abs(bias), None if G is None else np.abs(G))
    return {k: (float(np.log2(max(v.max() / (1.0 if k == "db" else Q), 1.0))) if v.size else 0.0) for k, v in A.items()}


def assert_exact(case, X, W, bias=None, G=None):
    bits = exact_bits(case, X, W, bias, G)
    bad = {k: round(v, 2) for k, v in bits.items() if v > ex.MAX_BITS}
    assert not bad, f"{case.name}: not provably exact in fp32 (more than {ex.MAX_BITS} bits): {bad}"
    return bits


# ----------------------------------------------------------------------------- the cases

SPMM_U = (1, 2, 4, 8)
SPMM16_L = [1, 2, 3, 0, 4, 5, 7, 8, 9, 16, 17, 0]      # chunks per tile: 0, 1, U - 1, U, U + 1, 2U, 2U + 1 for U in 1, 2, 4, 8
SPMM16_PIECE = 3                                       # max_unit_chunks of the plan with hub pieces: cuts at no multiple of 2, 4, 8


@functools.lru_cache(maxsize=None)
def spmm16_case():
    """hidden-16 forward: twelve 64-row tiles (the last 37 rows tall), an empty tile in the middle and at the end, pads inside chunks,
    every tile's last chunk full, and in the 17-chunk tile rows with 20 messages of one relation (runs across chunk boundaries)"""
    tiles = [tile_spec(L, t, rep_last=20 if L == 17 else 3) for t, L in enumerate(SPMM16_L)]
    return Case("spmm16", tiles, 64, 11 * 64 + 37, 500, 3, seed=11)


WIDE_L = [1, 2, 3, 0, 5, 4, 0]
WIDE_PIECE = 3
WIDTHS16 = (16, 32, 48, 64)
GENERIC_WIDTHS = ((5, 7), (16, 20), (33, 50), (7, 130))     # spmm_generic_kernel<1>, <2>, <4>, <8>


@functools.lru_cache(maxsize=None)
def wide_case(tile_rows=32):
    """wide (U = 1, 2) and generic (no unrolling) forward: seven tiles, one empty in the middle, the last empty and 11 rows tall; tile_rows 32 keeps 4 waves x 32 rows x 64
    floats inside the 64 KB tile budget, 24 rows do for 132 padded columns"""
    tiles = [tile_spec(L, t, rep_last=20 if L == 5 else 3) for t, L in enumerate(WIDE_L)]
    return Case(f"wide{tile_rows}", tiles, tile_rows, (len(WIDE_L) - 1) * tile_rows + 11, 300, 3, seed=12)


WGRAD_RG = (1, 2, 4, 8, 16)
WGRAD_U = (1, 2, 4)
WGRAD_TILE_ROWS = 16
# (R, n_tiles, tiles_per_item): R = 19 is ragged for every RG > 1; n_blocks = ceil(n_tiles / min(tiles_per_item, 8)) is 1, 3, 7, 9, 22:
# below 8 and no multiple of 8, so some of the eight interleaved work lists run out early; 12 tiles per item must behave as 8
WGRAD_TILED_COMBOS = ((19, 9, 3), (19, 65, 8), (19, 65, 12), (16, 7, 1), (1, 9, 3), (1, 1, 1), (19, 1, 8), (16, 65, 3), (19, 7, 8), (1, 65, 1))


def _wgrad_tile(t, R):
    """bucket sizes of tile t: blocks of 8 tiles alternate between a dense pattern and nearly empty stretches whose chunk totals are 1, 2,
    0, 3, 4, 5 -- with 8 tiles per item and 16 relations per group those are whole items"""
    blk, pos = divmod(t, 8)
    sparse = {1: {1: [(0, 5)]}, 2: {1: [(1, 20)]}, 3: {}, 4: {1: [(0, 40)]}, 5: {1: [(2, 16)], 2: [(0, 40)]}, 6: {1: [(0, 40)], 2: [(1, 20)]}}
    if blk in sparse:
        got = {}
        for r, n in sparse[blk].get(pos, []):
            got[r % R] = got.get(r % R, 0) + n
        return [(r, n, 2) for r, n in sorted(got.items())]
    size = {0: 0, 1: 0, 2: 5, 3: 16, 4: 0, 5: 20, 6: 0, 7: 40, 8: 0, 9: 64, 10: 0, 11: 72, 12: 0}
    return [(r, size[(5 * t + 3 * r + 7) % 13], 2) for r in range(R) if size[(5 * t + 3 * r + 7) % 13]]


@functools.lru_cache(maxsize=None)
def wgrad_tiled_case(R, n_tiles):
    tiles = [_wgrad_tile(t, R) for t in range(n_tiles)]
    return Case(f"wgrad_tiled_R{R}_T{n_tiles}", tiles, WGRAD_TILE_ROWS, n_tiles * WGRAD_TILE_ROWS - 5, 200, R, seed=13 + R + n_tiles)


def wgrad_tiled_item_totals(case, plan, RG, tiles_per_item):
    """chunk totals of the work items (relation group, tile block) as the launcher forms them, and the longest (tile, relation) run"""
    R, nt = case.R, case.n_tiles
    run = plan.run_ptr.reshape(nt, R + 1)
    tpi = min(tiles_per_item, 8)
    totals = set()
    for t0 in range(0, nt, tpi):
        for r0 in range(0, R, RG):
            r1 = min(R, r0 + RG)
            totals.add(int((run[t0:t0 + tpi, r1] - run[t0:t0 + tpi, r0]).sum()))
    return totals, int(np.diff(run, axis=1).max())


WGRAD_WIDTHS = ((16, 16), (8, 8), (48, 80))         # wgrad_d16_kernel<4, false>, wgrad_generic_kernel<1, 1, false>, <2, 4, false>
WGRAD_BF16_WIDTHS = ((16, 16), (32, 64))            # wgrad_d16_kernel<4, true>, wgrad_generic_kernel<2, 4, true>


@functools.lru_cache(maxsize=None)
def relmajor_case():
    """one tile (the relation-major plan): relations of 1, 4, 5 and 3 chunks -- with max_item_chunks = 4 the 5-chunk relation is two items.
    The 4-chunk relation is whole chunks of real messages (a tail that re-reads the last chunk counts them twice)."""
    return Case("relmajor", [[(0, 16, 1), (1, 64, 3), (2, 75, 2), (3, 40, 1)]], 100, 100, 150, 4, seed=14)


LEAN_NW = (16, 8)
LEAN_TILE_ROWS = 64
LEAN_R = 9                     # three window groups of 4 relations; the 8-wave form keeps ONE of them in its window, the 16-wave form all three
LEAN_BIG_TILES = 2100          # n_blocks = 132 (16 waves), 263 (8 waves): >= 128, so dw_reduce_a_kernel runs with S = 2 and S = 4


def lean_tiles(nw):
    return (1, nw - 1, nw, nw + 1, 2 * nw + 3)


@functools.lru_cache(maxsize=None)
def lean_case(n_tiles):
    """the transposed plan of the lean backward: tiles of 64 source rows, chunk counts cycling through SPMM16_L (empty tiles included),
    relations rotating with the tile; the large case is sparse (0 .. 2 chunks per tile)"""
    if n_tiles >= 1000:
        tiles = [tile_spec((1, 0, 2, 1)[t % 4], t, LEAN_R) for t in range(n_tiles)]
    else:
        tiles = [tile_spec(SPMM16_L[(t + 4) % len(SPMM16_L)], t, LEAN_R) for t in range(n_tiles)]
    return Case(f"lean_T{n_tiles}", tiles, LEAN_TILE_ROWS, n_tiles * LEAN_TILE_ROWS - 27, 300, LEAN_R, seed=15 + n_tiles, side="src")


# ----------------------------------------------------------------------------- the GEMM launcher's choice, as rgcn_gemm_f32 makes it

GEMM_TEST_SHAPES = [(1, 1, 1), (7, 5, 3), (128, 128, 16), (130, 127, 33), (400, 200, 513), (37, 256, 200), (300, 2, 64), (16, 400, 40),
                    (257, 129, 4), (404, 200, 400), (200, 400, 204), (1000, 16, 36), (68, 100, 52), (132, 144, 20), (64, 208, 16), (60, 212, 24)]
GEMM_TEST = "test_gpu_gemm.py::test_gemm_layouts_and_edges"


def gemm_form(M, N, K, ta, tb, bm, split_k=1):
    """the kernel rgcn_gemm_f32 launches for contiguous, 16-byte aligned operands (what _native.gemm passes): lda = A.shape[1], ldb = B.shape[1]"""
    GT, GK = 128, 16
    tiles_m, tiles_n = -(-M // GT), -(-N // GT)
    S = min(split_k, max(1, -(-K // GK)))
    kps = -(-(-(-K // S)) // GK) * GK
    S = -(-K // kps) if K > 0 else 1
    t128, t64 = tiles_m * tiles_n * S, -(-M // 64) * tiles_n * S
    half = (bm == 64) if bm else (-(-t64 // 256) < 2 * -(-t128 // 256) and t128 > 256)
    vec = (M if ta else K) % 4 == 0 and (K if tb else N) % 4 == 0
    b = lambda v: "true" if v else "false"
    if vec and not bm and M >= 4 and N >= 4 and K >= 4:
        nt = -(-N // 16)
        n_panels = (nt + 12) // 13
        need = -(-nt // n_panels)
        nb = 4 if need <= 4 else 7 if need <= 7 else 10 if need <= 10 else 13
        if n_panels * nb * 16 * 100 < tiles_n * GT * 95:
            return f"gemm_panel_kernel<{b(ta)}, {b(tb)}, {nb}>"
    return f"gemm_kernel<{b(ta)}, {b(tb)}, {b(vec)}, {64 if half else 128}>"


def gemm_coverage():
    """form -> the first parameter set of test_gemm_layouts_and_edges that launches it"""
    seen = {}
    for (M, N, K), ta, tb, bm in itertools.product(GEMM_TEST_SHAPES, (False, True), (False, True), (128, 64, 0)):
        for split_k in (1, 5):
            seen.setdefault(gemm_form(M, N, K, ta, tb, bm, split_k), dict(M=M, N=N, K=K, trans_a=ta, trans_b=tb, gemm_bm=bm, split_k=split_k))
    return seen


# ----------------------------------------------------------------------------- the table

NEW = "test_gpu_kernel_variants.py::"


def _reach(file, entry, wrapper, test, **how):
    return dict(file=file, entry=entry, wrapper=wrapper, test=test, **how)


def _unreachable(file, entry, reason, launcher_line):
    return dict(file=file, entry=entry, unreachable=reason, launcher_line=launcher_line)


def _wide_u(ni, nj):
    return 2 if (nj == 1 or (nj == 2 and ni <= 2)) else 1


def _build_variants():
    K, B, G = "rgcn_kernels.hip", "rgcn_bwd.hip", "rgcn_gemm.hip"
    v = {}
    # hidden-16 forward
    for U in SPMM_U:
        for packed in (True, False):
            v[f"spmm_d16_kernel<{U}, {'true' if packed else 'false'}, 0>"] = _reach(
                K, "rgcn_spmm_f32", "_native.spmm", NEW + "test_spmm_d16", options={"spmm_u": U}, widths=(16, 16),
                plan=dict(packed=packed, tile_rows=64, n_split=(0, "> 0 with max_unit_chunks = 3")))
    for bf, split in ((3, False), (1, True)):
        v[f"spmm_d16_kernel<4, true, {bf}>"] = _reach(K, "rgcn_spmm_bf16", "_native.spmm_bf16", NEW + "test_spmm_bf16", widths=(16, 16),
                                                     plan=dict(packed=True, tile_rows=32, n_split="> 0" if split else 0))
    # wide forward
    for ni, nj in itertools.product(range(1, 5), repeat=2):
        for bf in (0, 1, 3):
            name = f"spmm_wide_kernel<{ni}, {nj}, {_wide_u(ni, nj)}, {bf}>"
            if (ni, nj) == (1, 1):
                entry = "rgcn_spmm_f32" if bf == 0 else "rgcn_spmm_bf16"
                v[name] = _unreachable(K, entry, f"16 x 16 never reaches the wide dispatch: {entry} sends it to spmm_d16_kernel first",
                                       "if (d_in == 16 && d_out == 16) {")
            elif bf == 0:
                v[name] = _reach(K, "rgcn_spmm_f32", "_native.spmm", NEW + "test_spmm_wide", widths=(16 * ni, 16 * nj),
                                 plan=dict(packed=True, tile_rows=32, n_split=(0, "> 0")))
            else:
                v[name] = _reach(K, "rgcn_spmm_bf16", "_native.spmm_bf16", NEW + "test_spmm_bf16", widths=(16 * ni, 16 * nj),
                                 plan=dict(packed=True, tile_rows=32, n_split="> 0" if bf == 1 else 0))
    v["round4_bf16_kernel"] = _reach(K, "rgcn_spmm_bf16", "_native.spmm_bf16", NEW + "test_spmm_bf16", plan=dict(n_split="> 0"))
    for njt, (di, do) in zip((1, 2, 4, 8), GENERIC_WIDTHS):
        v[f"spmm_generic_kernel<{njt}>"] = _reach(K, "rgcn_spmm_f32", "_native.spmm", NEW + "test_spmm_generic", widths=(di, do),
                                                  plan=dict(packed=False, tile_rows=24, n_split=(0, "> 0")))
    v["pack_w_blocks_kernel"] = _reach(K, "rgcn_pack_w_blocks_f32", "_native.pack_w_blocks", NEW + "test_spmm_wide")
    v["pack_w16_kernel"] = _reach(K, "rgcn_pack_w16_f32", "lib().rgcn_pack_w16_f32 (the wrappers pack both orders with rgcn_pack_w16_pair_f32)",
                                  NEW + "test_single_order_weight_packs")
    # weight gradients
    for RG in WGRAD_RG:
        for U in WGRAD_U:
            v[f"wgrad_tiled_d16_kernel<{RG}, {U}>"] = _reach(K, "rgcn_wgrad_tiled_f32", "_native.wgrad_tiled", NEW + "test_wgrad_tiled",
                                                             options={"wgrad_rg": RG, "wgrad_u": U}, widths=(16, 16),
                                                             plan=dict(want_runs=True, tile_rows=WGRAD_TILE_ROWS, combos=WGRAD_TILED_COMBOS))
    v["wgrad_d16_kernel<4, false>"] = _reach(K, "rgcn_wgrad_f32", "_native.wgrad", NEW + "test_wgrad", widths=(16, 16), plan=dict(relation_major=True))
    v["wgrad_generic_kernel<1, 1, false>"] = _reach(K, "rgcn_wgrad_f32", "_native.wgrad", NEW + "test_wgrad", widths=(8, 8), plan=dict(relation_major=True))
    v["wgrad_generic_kernel<2, 4, false>"] = _reach(K, "rgcn_wgrad_f32", "_native.wgrad", NEW + "test_wgrad", widths=(48, 80), plan=dict(relation_major=True))
    v["wgrad_d16_kernel<4, true>"] = _reach(K, "rgcn_wgrad_bf16", "_native.wgrad_bf16", NEW + "test_wgrad_bf16", widths=(16, 16), plan=dict(relation_major=True))
    v["wgrad_generic_kernel<2, 4, true>"] = _reach(K, "rgcn_wgrad_bf16", "_native.wgrad_bf16", NEW + "test_wgrad_bf16", widths=(32, 64), plan=dict(relation_major=True))
    v["zero_fill_kernel"] = _reach(K, "zero_async (every launcher that clears its output)", "_native.wgrad", NEW + "test_wgrad")
    # the rest of rgcn_kernels.hip: one launcher form each, run through the layers on the exact fixtures of test_gpu_exact.py
    other = NEW + "test_other_entry_points"
    for vec in (True, False):
        for bf in (False, True):
            v[f"colsum_a_kernel<{'true' if vec else 'false'}, {'true' if bf else 'false'}>"] = _reach(
                K, "rgcn_colsum_bf16" if bf else "rgcn_colsum_f32", "_native.colsum_bf16" if bf else "_native.colsum", NEW + "test_colsum",
                widths=(("d % 4 == 0" if bf else "d % 4 == 0 and d < 128") if vec else "d % 4 != 0",))
    v["colsum_b_kernel"] = _reach(K, "rgcn_colsum_f32", "_native.colsum", NEW + "test_colsum")
    v["colsum_wide_a_kernel"] = _reach(K, "rgcn_colsum_f32", "_native.colsum", NEW + "test_colsum", widths=("d % 4 == 0 and d >= 128",))
    v["colsum_wide_b_kernel"] = _reach(K, "rgcn_colsum_f32", "_native.colsum", NEW + "test_colsum", widths=("d % 4 == 0 and d >= 128",))
    v["diag_csr_kernel<false>"] = _reach(K, "rgcn_diag_spmm_f32", "_native.diag_spmm", other + "[diag]")
    v["diag_csr_kernel<false, unsigned short*>"] = _reach(K, "rgcn_diag_spmm_bf16", "_native.diag_spmm_bf16", other + "[diag-bf16]")
    v["diag_csr_kernel<true>"] = _reach(K, "rgcn_featureless_csr_fwd_f32", "_native.featureless_csr_fwd", other + "[featureless-csr]")
    v["round_shared_rows_bf16_kernel<16>"] = _reach(K, "rgcn_diag_spmm_bf16", "_native.diag_spmm_bf16", other + "[diag-bf16-hub]", plan=dict(n_split="> 0"))
    for vec in (True, False):
        for bf in (False, True):
            v[f"diag_wgrad_kernel<{'true' if vec else 'false'}, {'true' if bf else 'false'}>"] = _reach(
                K, "rgcn_diag_wgrad_bf16" if bf else "rgcn_diag_wgrad_f32", "_native.diag_wgrad_bf16" if bf else "_native.diag_wgrad",
                other + ("[diag-bf16]" if bf else "[diag]"), widths=("d % 4 == 0" if vec else "d % 4 != 0",))
    v["featureless_fwd_kernel"] = _reach(K, "rgcn_featureless_fwd_f32", "_native.featureless_fwd", other + "[featureless-tile]")
    v["featureless_wgrad_kernel"] = _reach(K, "rgcn_featureless_wgrad_f32", "_native.featureless_wgrad", other + "[featureless-tile]")
    v["featureless_csr_wgrad_kernel"] = _reach(K, "rgcn_featureless_csr_wgrad_f32", "_native.featureless_csr_wgrad", other + "[featureless-csr]")
    v["spmm_scatter_d16_kernel<4>"] = _reach(K, "rgcn_spmm_scatter_f32", "_native.spmm_two_pass", other + "[two-pass]")
    v["segment_sum_d16_kernel"] = _reach(K, "rgcn_segment_sum_f32", "_native.spmm_two_pass", other + "[two-pass-scatter]", routes={"twopass": "scatter"})
    v["segment_gather_sum_d16_kernel"] = _reach(K, "rgcn_segment_gather_sum_f32", "_native.spmm_two_pass", other + "[two-pass]")
    v["segment_gather_sum_units_d16_kernel"] = _reach(K, "rgcn_segment_gather_sum_units_f32", "_native.spmm_two_pass", other + "[two-pass-hub]")
    for bf in (False, True):
        t = "true" if bf else "false"
        v[f"distmult_fwd_kernel<{t}>"] = _reach(K, "rgcn_distmult_fwd_bf16" if bf else "rgcn_distmult_fwd_f32", "_native.distmult_fwd" + ("_bf16" if bf else ""), NEW + "test_distmult_forms")
        v[f"distmult_bwd_kernel<{t}>"] = _reach(K, "rgcn_distmult_bwd_rel_bf16" if bf else "rgcn_distmult_bwd_f32", "_native.distmult_bwd" + ("_rel_bf16" if bf else ""), NEW + "test_distmult_forms")
    for sides, vec, table, bf in ((1, False, True, False), (1, True, True, False), (2, False, True, False), (2, True, True, False), (3, False, False, False),
                                  (3, False, False, True), (3, False, True, True), (3, True, False, False), (3, True, False, True), (3, True, True, True)):
        b = lambda x: "true" if x else "false"
        entry = {(True, False): "rgcn_distmult_bwd_all_f32", (False, False): "rgcn_distmult_bwd_nodes_f32", (True, True): "rgcn_distmult_bwd_all_bf16",
                 (False, True): "rgcn_distmult_bwd_nodes_bf16"}[(table, bf)]
        v[f"distmult_bwd_all_kernel<{sides}, {b(vec)}, {b(table)}, {b(bf)}>"] = _reach(K, entry, "_native." + entry[5:].replace("_f32", ""), NEW + "test_distmult_forms",
                                                                                      widths=("d % 4 == 0" if vec else "d % 4 != 0",))
    # rgcn_bwd.hip
    for nw, ng in ((16, 3), (8, 1)):
        for atomic in (True, False):
            for relu in (True, False):
                v[f"bwd_lean_d16_kernel<{nw}, {ng}, {'true' if atomic else 'false'}, {'true' if relu else 'false'}, 0>"] = _reach(
                    B, "rgcn_bwd_lean_f32", "_native.bwd_fused", NEW + "test_bwd_lean", options={"bwd_nw": nw}, routes={"bwd_kernel": "lean"}, widths=(16, 16),
                    plan=dict(packed=True, want_runs=True, tile_rows=LEAN_TILE_ROWS, n_split=0, n_tiles=lean_tiles(nw) + (LEAN_BIG_TILES,)), atomic=atomic, relu=relu)
    v["bwd_lean_prep_kernel"] = _reach(B, "rgcn_bwd_lean_prepare_f32", "_native.bwd_fused", NEW + "test_bwd_lean")
    v["dw_reduce_a_kernel"] = _reach(B, "rgcn_bwd_lean_f32", "_native.bwd_fused", NEW + "test_bwd_lean", atomic=False, plan=dict(n_tiles=LEAN_BIG_TILES, S=(2, 4)))
    v["dw_reduce_b_kernel"] = _reach(B, "rgcn_bwd_lean_f32", "_native.bwd_fused", NEW + "test_bwd_lean", atomic=False)
    for relu in (True, False):
        v[f"bwd_scatter_dw_d16_kernel<4, {'true' if relu else 'false'}>"] = _reach(B, "rgcn_bwd_scatter_dw_f32", "lib().rgcn_bwd_scatter_dw_f32 (the wrapper "
                                                                                  "_native.bwd_two_pass_fused needs a device-built CSR)", NEW + "test_bwd_scatter_dw",
                                                                                  widths=(16, 16), plan=dict(relation_major=True, item_chunks=(1, 4, 5, 3)), relu=relu)
    v["pack_w16_pair_kernel"] = _reach(B, "rgcn_pack_w16_pair_f32", "_native.pack_w16 / pack_w16t", NEW + "test_bwd_lean")
    v["pack_w16t_kernel"] = _reach(B, "rgcn_pack_w16t_f32", "lib().rgcn_pack_w16t_f32 (the wrappers pack both orders with rgcn_pack_w16_pair_f32)",
                                   NEW + "test_single_order_weight_packs")
    v[("zero_fill_kernel", B)] = _reach(B, "zero_async", "_native.bwd_fused", NEW + "test_bwd_lean", atomic=True)
    # rgcn_gemm.hip: the shapes tests/test_gpu_gemm.py runs reach every form (gemm_form models the launcher; asserted on the CPU)
    for name, how in sorted(gemm_coverage().items()):
        v[name] = _reach(G, "rgcn_gemm_f32", "_native.gemm", GEMM_TEST, options={"gemm_bm": how["gemm_bm"]},
                         shape=(how["M"], how["N"], how["K"]), trans=(how["trans_a"], how["trans_b"]), split_k=how["split_k"])
    v["sum_slices_kernel"] = _reach(G, "rgcn_gemm_f32", "_native.gemm", GEMM_TEST, split_k=5)
    for vec in (True, False):
        t = "true" if vec else "false"
        w = (48, 80) if vec else (33, 50)
        v[f"rel_rows_kernel<{t}>"] = _reach(G, "rgcn_rel_rows_f32", "_native.spmm_wide_two_pass", other + f"[wide-two-pass-{w[0]}x{w[1]}]", widths=w)
        v[f"rel_wgrad_kernel<{t}>"] = _reach(G, "rgcn_rel_wgrad_f32", "_native.wgrad_wide", other + f"[wide-two-pass-{w[0]}x{w[1]}]", widths=w)
    v["segment_gather_sum_wide_kernel"] = _reach(G, "rgcn_segment_gather_sum_wide_f32", "_native.spmm_wide_two_pass", other + "[wide-two-pass-48x80]")
    v[("zero_fill_kernel", G)] = _reach(G, "zero_async", "_native.wgrad_wide", other + "[wide-two-pass-48x80]")
    return v


VARIANTS = _build_variants()
FILES = ("rgcn_kernels.hip", "rgcn_bwd.hip", "rgcn_gemm.hip")


def names_of(file):
    """the table's census names of one source file (zero_fill_kernel lives in every file: its rows are keyed (name, file))"""
    return sorted((k if isinstance(k, str) else k[0]) for k, row in VARIANTS.items() if row["file"] == file)


def unreachable():
    return sorted(k for k, row in VARIANTS.items() if "unreachable" in row)


def launcher_has_line(csrc_dir, row):
    """an `unreachable` row names a line in the body of its launcher (compared without the macros' line continuations and surrounding
    blanks), ahead of the launch it keeps the form away from"""
    import os
    text = open(os.path.join(csrc_dir, row["file"])).read()
    start = text.index(f'extern "C" int {row["entry"]}(')
    nxt = text.find('extern "C"', start + 1)
    body = text[start:nxt if nxt > 0 else len(text)].splitlines()
    norm = lambda ln: ln.rstrip().rstrip("\\").strip()
    hits = [i for i, ln in enumerate(body) if norm(ln) == norm(row["launcher_line"])]
    return bool(hits)
