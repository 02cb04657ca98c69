"""autograd bindings of the HIP kernels.

`relational_mp`  : out = sum_e val_e X[o_e] W[p_e] + b      (featured layers)
`featureless_mp` : out = sum_e val_e W[p_e, o_e, :] + b     (X = I)

Both are the custom-Function form of what the reference leaves to autograd
(torch_rgcn/layers.py:286-306; duals in SURVEY.md 8 a-9).  backward runs on the
autograd engine's thread and launches on that thread's current HIP stream; it uses
nothing but the tensors saved on ctx and the immutable RelGraph.
"""
import numbers

import numpy as np
import torch

from . import _native, routes


def _wgrad_tiles(plan):
    """destination tiles per work item of the tile-major weight gradient: more tiles amortise the item's set-up and its
    256 atomics (8 measured best at S1), fewer keep small graphs parallel"""
    env = routes.get("wgrad_tiles")
    return int(env) if env else (8 if plan.n_tiles >= 4096 else 4)


def _sparse_buckets(graph, d_in, d_out):
    """hidden 16 and (tile, relation) buckets so small that the 16-slot chunks are mostly padding"""
    if d_in != 16 or d_out != 16 or graph._dev is None or graph.sync_free or graph.per_call:
        return False            # (the two-pass path sizes its scratch by a message count read back from the device)
    mode = routes.get("sparse_path", "auto")
    if mode != "auto":
        return mode == "1"
    fp = graph.fwd_plan(16)
    if not (fp.m_pad > 0 and fp.n_messages < 0.5 * fp.m_pad):
        return False
    # pass 2 walks a destination's messages with 4 lanes: keep mega-hubs on the tile path (which splits them)
    return graph.max_degree() <= 4096


def _hub_free(plan):
    """a plan of tall tiles, none of them cut into hub pieces (what the relation-owner backward and a ReLU epilogue need)"""
    return plan is not None and not _native._blk_units(plan)[2]


def _tall_plan(plan, relu):
    """a forward plan of tall tiles for rgcn_spmm_blk_f32 / _bf16 as it is, or None: no such plan, or the ReLU epilogue on tiles cut into hub pieces"""
    return plan if plan is not None and (not relu or _hub_free(plan)) else None


def _forward_route(graph, R, d_in, d_out, relu=False, blocks4=False):
    """(name, plan) of the forward of _RelationalMP at the padded shape [R, d_in, d_out]; relu: the ReLU epilogue is
    wanted; blocks4: W = block_diag(4 x 4 blocks) at width 16 and the caller holds the blocks.  Builds forward plans only."""
    # spmm_csr=0 asks for the two-pass forward: it turns every one-launch kernel of width 16 off -- the CSR kernel, and with it both plans of
    # tall tiles (_native.spmm_blk_rows gives them no rows then: graph.fwd_blk_plan() and graph.win_plan("fwd") are None)
    one_launch = routes.get("spmm_csr", "1") != "0"
    if _sparse_buckets(graph, d_in, d_out):
        csr = graph.csr("fwd")
        if blocks4 and routes.get("block_fwd", "1") != "0":
            # W = block_diag(blocks), 4 x 4 blocks, sparse buckets (AM): the forward reads the blocks themselves on the CSR
            # kernel (block table in LDS; one gather per message, no transformed-row buffer): 0.46 ms against 0.65 ms for the
            # two passes below.  The backward stays on the dense W (dX rows + dW from one relation-major walk; autograd
            # through block_diag() picks the blocks' gradient out of dW).
            return "block_csr", csr
        if one_launch and _native.spmm_csr_d16_ok(csr, R):
            # sparse buckets, up to 120 relations: ONE pass over the destination-major CSR, messages of mixed relations, W in LDS
            return "csr", csr
        # sparse buckets, more relations than the CSR kernel's LDS holds (AM as shipped, layer 2: R = 267): the forward plan cut into
        # tall workgroup-owned tiles (31 messages per (tile, relation) bucket instead of ~2), one launch, no [M, 16] intermediate
        # (not in deterministic mode: the tile is summed in arrival order)
        plan = _tall_plan(graph.fwd_blk_plan(), relu) if one_launch and not deterministic() else None
        return ("blk", plan) if plan is not None else ("two_pass", None)
    if d_in == 16 and d_out == 16 and one_launch:
        # dense buckets on a large static graph (S1): tall workgroup-owned tiles walked in soft-window order -- the whole chip gathers
        # from a few MB of X at any time (0.33 ms against 0.42 on the wave-owned tiles, tools/softwin_probe.py)
        plan = _tall_plan(graph.win_plan("fwd"), relu)
        if plan is not None:
            return "win", plan
    return "tiles", None


def _pad_blocks(X, W, bias, graph=None):
    """Widths up to 64 run on the MFMA block kernels (hidden-16 scheme over blocks of 16 features) with operands
    zero-padded to multiples of 16: a 40-byte row costs the same 128-byte fabric request as a 64-byte one, and these
    kernels (packed slots, pre-swizzled weight fragments, DPP folds) are several times faster than the generic-width
    one (AM: 10 -> 11 layer 2.9 -> 0.9 ms per launch, 32 -> 32 layer 7.5 -> 2.2 ms).
    -> (X', W', bias', (d_in, d_out)) or the inputs unchanged and None."""
    d_in, d_out = W.shape[1], W.shape[2]
    pi, po = -d_in % 16, -d_out % 16
    if max(d_in, d_out) > _BLOCKED_MAX or (pi == 0 and po == 0) or \
            (graph is not None and _wide_gemm_path(graph, d_in, d_out)):       # (the gather-GEMM takes ragged widths as they are)
        return X, W, bias, None
    # one launch for W and the bias together (torch.nn.functional.pad: a fill and a copy each)
    if pi and _zero_padded_rows(X, d_in + pi):
        Xp = torch.as_strided(X, (X.shape[0], d_in + pi), (d_in + pi, 1))      # the producer wrote the padded rows already: no copy
    else:
        Xp = X if pi == 0 else _native.resize3(dense(X), (X.shape[0], d_in + pi))
    if bias is None:
        Wp, bp = _native.resize3(dense(W), (d_in + pi, d_out + po)), None
    else:
        Wp, bp = _native.resize3(dense(W), (d_in + pi, d_out + po), dense(bias), d_out + po)
    return Xp, Wp, bp, (d_in, d_out)


_BLOCKED_MAX = 512     # widest layer that is cut into 64-wide blocks of the MFMA block kernel


def _wide_gemm_path(graph, d_in, d_out):
    """undecomposed weights above width 64: relation-grouped gather-GEMM on the matrix cores + per-destination row sum
    (csrc/rgcn_gemm.hip); needs the device-side graph and host-known message counts (not the sync-free per-call build)"""
    return max(d_in, d_out) > 64 and graph._dev is not None and not graph.sync_free


def _spmm_blocked(X, W, bias, plan_of, relu=False, graph=None, kind="fwd"):
    """spmm for any width.  Up to 64 x 64 it is one launch of the block kernels.  Above (undecomposed weights at d = 100,
    200, ...): relation-grouped gather-GEMM (X gathered once per message, every W_r through LDS once per 128 messages) + row
    sum; graphs without a device-side build keep round 1's (d_in / 64) x (d_out / 64) launches of the block kernel."""
    d_in, d_out = W.shape[1], W.shape[2]
    if graph is not None and _wide_gemm_path(graph, d_in, d_out):
        return _native.spmm_wide_two_pass(X, W, bias, graph.scatter_plan(kind, 8), graph.csr(kind), relu=relu)
    if max(d_in, d_out) <= 64 or d_in % 16 or d_out % 16 or max(d_in, d_out) > _BLOCKED_MAX:
        return _native.spmm(X, W, bias, plan_of(d_out), relu=relu and max(d_in, d_out) <= 64)
    xs = [X[:, i:i + 64].contiguous() for i in range(0, d_in, 64)]
    cols = []
    for j in range(0, d_out, 64):
        wj = min(64, d_out - j)
        acc = None
        for bi, i in enumerate(range(0, d_in, 64)):
            part = _native.spmm(xs[bi], W[:, i:i + 64, j:j + wj].contiguous(),
                                bias[j:j + wj].contiguous() if (bias is not None and bi == 0) else None, plan_of(wj))
            acc = part if acc is None else acc.add_(part)
        cols.append(acc)
    return torch.cat(cols, dim=1)


def _zero_padded_rows(t, wide):
    """t = the first columns of a contiguous, 16-byte aligned [N, wide] buffer whose other columns are ZERO (the producer said so)?"""
    if not (getattr(t, "_rgcn_zero_padded", False) and _rows16(t) and t.stride(0) == wide):
        return False
    # the mark is a Python attribute: it survives set_() / resize_() / .data swaps of the tensor object -- the storage must still hold the rows
    return t.untyped_storage().nbytes() >= (t.storage_offset() + t.shape[0] * wide) * t.element_size()


def _padded_grad(g, dims):
    """the upstream gradient of a layer whose widths _pad_blocks padded (dims), dense, at the padded output width"""
    if dims is not None and dims[1] % 16:
        wide = dims[1] + (-dims[1] % 16)
        if _zero_padded_rows(g, wide):
            g = torch.as_strided(g, (g.shape[0], wide), (wide, 1))       # MaskedCrossEntropy wrote the zero-padded rows already
        else:
            g = _native.resize3(dense(g), (g.shape[0], wide))
    return dense(g)


def _unpad_blocks(dims, dX, dW, db, dx_view=False):
    if dims is None:
        return dX, dW, db
    d_in, d_out = dims
    if dX is not None and dX.shape[1] != d_in:
        if dx_view:       # X was an intermediate that arrived as the first columns of zero-padded rows: its gradient goes back the same way
            dX = dX[:, :d_in]                                  # (the padded columns of dX are exact zeros: W's padding rows are)
            dX._rgcn_zero_padded = True
        else:
            dX = _native.resize3(dense(dX), (dX.shape[0], d_in))
    if dW is not None and (dW.shape[1] != d_in or dW.shape[2] != d_out):      # contiguous gradients in one launch (a sliced view costs
        if db is not None:                                                     # AccumulateGrad a strided copy per tensor)
            dW, db = _native.resize3(dense(dW), (d_in, d_out), dense(db), d_out)
        else:
            dW = _native.resize3(dense(dW), (d_in, d_out))
    elif db is not None and db.shape[0] != d_out:
        db = db[:d_out]
    return dX, dW, db


def deterministic():
    """RGCN_DETERMINISTIC=1: bit-reproducible gradients.  The hidden-16 backward then runs the lean window kernel on 64-row tiles
    (wave-owned dX tiles: a fixed summation order), writes its per-workgroup dW partials with plain stores and two small kernels
    sum them in a fixed order (+0.1-0.15 ms per layer at S1) -- instead of the block-tile kernel, whose waves add to the shared
    dX tile, to dW and to the bias gradient in arrival order (fp32 sums differ in the last bits from run to run).  Outputs are
    reproducible either way."""
    return routes.get("deterministic", "0") == "1"


def _dense_buckets(plan):
    return plan.m_pad > 0 and plan.n_messages >= 0.5 * plan.m_pad


def dense(t):
    """contiguous AND 16-byte aligned (what the C ABI asks for): a contiguous view at an odd storage offset is copied"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _ReluToken:
    """Links a layer whose kernel applied ReLU in its epilogue (the producer of H = relu(pre)) with the layer that consumes
    H.  The consumer's fused backward can mask its feature gradient with H > 0 in the kernel's epilogue -- that IS the ReLU's
    backward -- and then records here WHICH tensor it returned; the producer's backward skips its own masking launch
    (aten.threshold_backward) only when the gradient it receives is that very tensor object, unmodified (same Python object
    through a weak reference, same version counter).  Anything else -- H had other consumers and autograd summed their
    gradients (a new tensor, or an in-place add that bumps the version), a hook replaced the tensor, the consumer took
    another route -- falls back to masking, which is idempotent on the pre-masked part: always exact.

    OPT-IN (round 5).  What the consumer hands autograd for H is then dL/d(pre-activation), not dL/dH -- they differ exactly where
    H == 0 -- and `torch.autograd.grad(loss, H)` (or a grad_fn pre-hook) reads that value without leaving any trace the backward could
    see.  So the consumer pre-masks only when the PRODUCER was told that H is private: `layer.forward_activated(x, "relu",
    private=True)` = "H goes into layers of this library and nobody asks autograd for its gradient" (models.py, whose hidden
    activation never leaves forward(), and bench.py do).  A bare `l2(l1.forward_activated(x, "relu"))` -- like the reference's
    `F.relu(self.rgc1(...))` -- returns the exact dL/dH; the producer masks in its own backward (one elementwise launch)."""
    __slots__ = ("ref", "version", "consumer_input", "private")

    def __init__(self, private=False):
        self.ref, self.version, self.consumer_input, self.private = None, -1, None, bool(private)

    def observed(self):
        """someone can SEE the gradient that arrives at H -- H.retain_grad() or a tensor hook on H: then it has to be dL/dH, not the
        pre-masked dL/d(pre-activation), and the consumer leaves the masking to the producer.  (torch.autograd.grad(loss, H) cannot
        be seen from here: it returns the pre-masked gradient, which differs from dL/dH exactly where H == 0.)"""
        h = self.consumer_input() if self.consumer_input is not None else None
        return h is None or h.retains_grad or bool(getattr(h, "_backward_hooks", None))

    def mark(self, dX):
        import weakref
        self.ref, self.version = weakref.ref(dX), dX._version

    def premasked(self, g):
        return self.ref is not None and self.ref() is g and g._version == self.version


def _backward_route(graph, d_in, d_out, need_x=True, need_w=True, diag4=False, sparse=None):
    """(name, plan) of the backward of _RelationalMP at the padded widths, from the routes table as it is NOW.
    own / blk / lean: hidden 16, both gradients wanted -- ONE walk of a transposed plan gathers G[s] once per message and produces dX and dW
    together (blk_forced: the block-tile kernel on the wave-owned plan of a forced tile height, RGCN_TILE_ROWS, never with diag4); scatter: the same on the relation-major plan of sparse buckets; split: a kernel per gradient (X or W frozen, other widths,
    RGCN_BWD=split, plans no fused kernel takes: hub-split tiles, unpacked slots) -- and then no fused-backward plan is asked for.
    diag4: W = block_diag(4 x 4 blocks) and only dW's diagonal blocks are wanted (block-tile kernel only).  sparse: the sparse-bucket test
    where the caller has its answer (the relation-sharded layer: never)."""
    if not (need_x and need_w) or d_in != 16 or d_out != 16 or routes.get("bwd", "fused") == "split":
        return "split", None
    if sparse is None:
        sparse = _sparse_buckets(graph, d_in, d_out)
    if not diag4 and not sparse and routes.get("bwd_own", "1") != "0" and _native.bwd_route() == "blk":
        # large static graph with dense buckets (S1): tall tiles in soft-window order, every relation's dW in the registers of its owner wave
        op = graph.win_plan("bwd_own")
        if _hub_free(op):
            return "own", op
    # sparse (tile, relation) buckets normally leave the tile plan -- except on a graph the block-tile kernel takes: its tall tiles
    # (128 .. 512 rows) hold several messages per bucket where a 64-row tile holds one or two, and dW of all relations (block-diagonal
    # weights: its diagonal blocks) fits the workgroup's LDS.  One launch instead of the two-pass backward's three.
    rows = _native.bwd_blk_rows(graph.num_nodes, graph.num_rels, deterministic(), graph.device, diag4, sparse)
    if rows or not sparse:
        bp = graph.bwd_blk_plan(rows=rows)                  # tall tiles, one per workgroup -- or the wave-owned 64-row plan
        # (a plan the kernel takes without diag4 it takes with it -- the diagonal blocks need less LDS --, so one question settles both)
        name = "blk" if bp is not None and _native._bwd_blk_plan(bp, diag4) else "lean"
        if name == "lean":
            bp = graph.bwd_plan(16)
            if _native._bwd_blk_plan(bp):                   # (64 rows: no; a forced tile height, RGCN_TILE_ROWS, may be taller)
                name = "blk_forced"
        if _native.bwd_fused_ok(bp, blk=name != "lean"):
            return name, bp
    if sparse and routes.get("twopass", "gather") == "gather" and not deterministic():
        # sparse buckets: relation-major walk, G[s] and X[o] gathered once each for dX's rows and dW together
        return "scatter", graph.scatter_plan("bwd")
    return "split", None


def _weight_gradient(X, W, g, graph):
    if _wide_gemm_path(graph, W.shape[1], W.shape[2]):
        # (the same 128-slot work items as the row GEMM: longer items flush fewer partial blocks but leave too few
        # workgroups on small per-call graphs -- measured 0.104 -> 0.184 ms at FB15k-237 shape -- and cost a second plan)
        return _native.wgrad_wide(X, g, graph.scatter_plan("fwd", 8), W.shape[0])
    fp = graph.fwd_plan(min(W.shape[2], 64))
    # tile-major walk (one random gather per message) unless a (tile, relation) run is so long that
    # one wave would serialise it (hub nodes): then the relation-major kernel with bounded work items
    # and unless the (tile, relation) buckets are so sparse that a work item is a fraction of a chunk
    tiled_ok = W.shape[1] == 16 and W.shape[2] == 16 and fp.max_run_chunks <= 64 and _dense_buckets(fp)
    if tiled_ok and routes.get("wgrad", "tiled") == "tiled":
        return _native.wgrad_tiled(X, g, fp, W.shape[0], _wgrad_tiles(fp))
    return _native.wgrad(X, g, graph.wgt_plan(), W.shape[0])


class _RelationalMP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, W, bias, graph, relu=False, blocks=None, in_token=None):
        ctx.in_token = in_token                      # X = relu(...) of a layer that fused the activation (see _ReluToken)
        # H itself, kept alive until the backward: at padded widths (AM: hidden 10) the tensor saved below is the [N, 16] buffer behind it, the
        # caller's H is a temporary, and _ReluToken.observed() must still be able to ask it whether anybody watches its gradient
        ctx.h_ref = X if in_token is not None else None
        ctx.out_token = _ReluToken(private=relu == "private") if relu else None
        relu = bool(relu)
        x_padded_view = W.shape[1] % 16 != 0 and _zero_padded_rows(X, W.shape[1] + (-W.shape[1] % 16))
        X, W, bias, ctx.dims = _pad_blocks(X, W, bias, graph)
        # the feature gradient of such an input returns as a view of the padded rows too (no crop launch) -- to an intermediate only: a
        # leaf's .grad stays a dense tensor of its own shape
        ctx.dx_view = bool(x_padded_view and ctx.dims is not None and routes.get("pad16_view", "1") != "0")
        X = dense(X)
        W = dense(W)
        b = None if bias is None else dense(bias)
        fused_relu = relu and (max(W.shape[1], W.shape[2]) <= 64 or _wide_gemm_path(graph, W.shape[1], W.shape[2]))   # kernel epilogues
        # W = block_diag(4 x 4 blocks) at width 16: the backward may keep only dW's diagonal blocks (block-tile kernel, R <= 447)
        ctx.diag4 = blocks is not None and ctx.dims is None and tuple(blocks.shape[2:]) == (4, 4) and W.shape[1] == 16 and W.shape[2] == 16
        route, plan = _forward_route(graph, *W.shape, relu=fused_relu, blocks4=ctx.diag4)
        with _native.w16_scope() as w16:        # [R,16,16] weights: both fragment orders packed once, handed to the backward below
            if route == "block_csr":
                out = _native.block_spmm(X, blocks.detach().contiguous(), b, plan, relu=fused_relu)
            elif route == "csr":
                out = _native.spmm_csr_d16(X, W, b, plan, relu=fused_relu)
            elif route in ("blk", "win"):
                out = _native.spmm_blk(X, W, b, plan, relu=fused_relu)
            elif route == "two_pass":
                out = _native.spmm_two_pass(X, W, b, graph.scatter_plan("fwd"), graph.csr("fwd"), relu=fused_relu)
            else:
                out = _spmm_blocked(X, W, b, graph.fwd_plan, relu=fused_relu, graph=graph, kind="fwd")
        ctx.w16 = w16.pair(W)
        if relu and not fused_relu:
            out = torch.relu_(out)
        ctx.graph = graph
        ctx.has_bias = bias is not None
        ctx.relu = relu
        if relu:
            ctx.save_for_backward(X, W, out)
        else:
            ctx.save_for_backward(X, W)
        if ctx.dims is None or out.shape[1] == ctx.dims[1]:
            return out
        if routes.get("pad16_view", "1") != "0":
            return out[:, :ctx.dims[1]]       # the first columns of the padded rows, no copy (MaskedCrossEntropy reads them in place)
        return _native.resize3(out, (out.shape[0], ctx.dims[1]))

    @staticmethod
    def backward(ctx, g):
        X, W = ctx.saved_tensors[:2]
        with _native.w16_scope(seed=(W, ctx.w16)):
            return _RelationalMP._backward(ctx, g, X, W)

    @staticmethod
    def _backward(ctx, g, X, W):
        graph = ctx.graph
        g = _padded_grad(g, ctx.dims)
        if ctx.relu and not ctx.out_token.premasked(g):     # out = relu(pre): the gradient passes where the stored output is positive
            g = torch.ops.aten.threshold_backward(g, ctx.saved_tensors[2], 0.0)
        dX = dW = db = None
        sparse = _sparse_buckets(graph, W.shape[1], W.shape[2])
        route, plan = _backward_route(graph, W.shape[1], W.shape[2], ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.diag4, sparse)
        # X is the output of a ReLU whose producer left the masking to this layer (_ReluToken): dX is wanted BEFORE it, masked with X > 0 in
        # the fused kernel's epilogue (scatter: the mask rides on the transformed rows, at any input width)
        masked = route != "split" and ctx.in_token is not None and ctx.in_token.private and not ctx.in_token.observed() and \
            (route == "scatter" or ctx.dims is None or ctx.dims[0] % 16 == 0)
        if route == "own":
            dX, dW, db = _native.bwd_own(g, X, W, plan, relu=masked, want_db=True)
        elif route in ("blk", "blk_forced", "lean"):
            dX, dW, db = _native.bwd_fused(g, X, W, plan, atomic=not deterministic(), relu=masked, want_db=True, diag4=route == "blk" and ctx.diag4)
        elif route == "scatter":
            dX, dW = _native.bwd_two_pass_fused(g, X, W, plan, graph.csr("bwd"), relu=masked)
        else:
            if ctx.needs_input_grad[0]:
                Wt = W.transpose(1, 2).contiguous()
                if sparse:
                    dX = _native.spmm_two_pass(g, Wt, None, graph.scatter_plan("bwd"), graph.csr("bwd"))
                else:
                    dX = _spmm_blocked(g, Wt, None, graph.bwd_plan, graph=graph, kind="bwd")
            if ctx.needs_input_grad[1]:
                dW = _weight_gradient(X, W, g, graph)
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        db = (db if db is not None else _native.colsum(g)) if want_db else None      # (the relation-owner and block-tile kernels sum G's columns on the side)
        res = _unpad_blocks(ctx.dims, dX, dW, db, getattr(ctx, "dx_view", False))
        if masked:
            ctx.in_token.mark(res[0])                 # the tensor autograd is handed (a view or a crop of dX for padded widths) already is the
        return (*res, None, None, None, None)         # gradient BEFORE the producer's ReLU


# ----------------------------------------------------------------------------- bf16 storage
# A featured layer called with bf16 features returns bf16; every product and sum is fp32 and the result is rounded to bf16 once.  The weights
# arrive here as the dense fp32 W (bf16 parameters are widened by the layer, once per call; nothing here rounds a weight).


def _bf16_native_plans(graph, d_in, d_out, relu):
    """the native bf16 route at padded widths (d_in, d_out) <= 64, or None (RGCN_DETERMINISTIC=1, wider layers, plans without packed slots:
    the upcast route).  ("win", forward plan, owner plan): S1-shaped graphs at width 16 -- the soft-window forward (rgcn_spmm_blk_bf16) and the
    relation-owner backward (rgcn_bwd_own_bf16: dX, dW and db in one walk).  ("wave", forward plan, transposed plan): every other graph
    (host-built, device-built, per-call LP graphs, hub-split plans; RGCN_SOFTWIN=0, RGCN_BWD_OWN=0) -- rgcn_spmm_bf16 forward and dX,
    rgcn_wgrad_bf16 on the relation-major plan, rgcn_colsum_bf16."""
    if max(d_in, d_out) > 64 or deterministic():
        return None
    if d_in == 16 and d_out == 16 and routes.get("bwd_own", "1") != "0":
        fp = _tall_plan(graph.win_plan("fwd"), relu)
        op = graph.win_plan("bwd_own") if fp is not None else None
        if _hub_free(op):
            return "win", fp, op
    fp, bp = graph.fwd_plan(d_out), graph.bwd_plan(d_in)
    if fp.pack is None or bp.pack is None or fp.n_src >= (1 << 24) or bp.n_src >= (1 << 24):
        return None
    return "wave", fp, bp


def _pad16(t, rows_last2):
    """zero-pad the trailing dimensions of t to multiples of 16 (bf16 or fp32; a torch pad, as _pad_blocks' resize3 for fp32)"""
    pads = []
    for n in reversed(rows_last2):
        pads += [0, -n % 16]
    return torch.nn.functional.pad(t, pads) if any(pads) else t


class _RelationalMPBF16(torch.autograd.Function):
    """relational_mp on bf16 features, native routes (see _bf16_native_plans): X and the upstream gradient are gathered as bf16 rows, W
    and the bias are fp32, out and dX are rounded to bf16 once, dW and db are fp32 sums returned in W's / the bias's dtype"""

    @staticmethod
    def forward(ctx, X, W, bias, graph, relu, plans):
        d_in, d_out = W.shape[1], W.shape[2]
        ctx.dims, ctx.plans, ctx.relu, ctx.has_bias = (d_in, d_out), plans, bool(relu), bias is not None
        ctx.w_dtype, ctx.b_dtype = W.dtype, None if bias is None else bias.dtype
        Xp = dense(_pad16(X, (d_in,)))
        Wp = dense(_pad16(W.detach().float(), (d_in, d_out)))
        bp = None if bias is None else dense(_pad16(bias.detach().float(), (d_out,)))
        ctx.graph = graph
        if plans[0] == "win":
            out = _native.spmm_blk_bf16(Xp, Wp, bp, plans[1], relu=bool(relu))
        else:
            out = _native.spmm_bf16(Xp, Wp, bp, plans[1], relu=bool(relu))
        ctx.save_for_backward(Xp, Wp, out if relu else None)
        return out if out.shape[1] == d_out else out[:, :d_out].contiguous()

    @staticmethod
    def backward(ctx, g):
        Xp, Wp, out = ctx.saved_tensors
        d_in, d_out = ctx.dims
        g = dense(_pad16(g.to(torch.bfloat16), (d_out,)))
        if ctx.relu:
            g = torch.ops.aten.threshold_backward(g, out, 0.0)        # a mask: exact in bf16
        want_db = ctx.has_bias and ctx.needs_input_grad[2]
        if ctx.plans[0] == "win":
            dX, dW, db = _native.bwd_own_bf16(g, Xp, Wp, ctx.plans[2], want_db=want_db)
        else:
            dX = _native.spmm_bf16(g, Wp.transpose(1, 2).contiguous(), None, ctx.plans[2]) if ctx.needs_input_grad[0] else None
            dW = _native.wgrad_bf16(Xp, g, ctx.graph.wgt_plan(), Wp.shape[0]) if ctx.needs_input_grad[1] else None
            db = _native.colsum_bf16(g) if want_db else None
        if dX is not None and dX.shape[1] != d_in:
            dX = dX[:, :d_in].contiguous()
        dW = dW[:, :d_in, :d_out].to(ctx.w_dtype) if (ctx.needs_input_grad[1] and dW is not None) else None
        db = db[:d_out].to(ctx.b_dtype) if db is not None else None
        return (dX if ctx.needs_input_grad[0] else None), dW, db, None, None, None


def relational_mp_bf16(features, weights, bias, graph, relu=False, group=None, n_slabs=0, comm="allreduce"):
    """relational_mp for bf16 features: weights [R, d_in, d_out] and bias in fp32 (the layer widened bf16 parameters) -> bf16 [N, d_out].
    Native HIP route where it applies (_bf16_native_plans); the rest -- widths above 64, relation-sharded layers (group),
    RGCN_DETERMINISTIC=1 -- runs the fp32 route on the widened features and rounds its output: CORRECTNESS ONLY, no speed-up (autograd
    carries the casts)."""
    if features.dtype != torch.bfloat16:
        raise TypeError(f"relational_mp_bf16: features must be torch.bfloat16, got {features.dtype}")
    if weights.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise TypeError("relational_mp_bf16: weights and bias are widened to torch.float32 by the caller")
    d16 = lambda n: n + (-n % 16)
    plans = None if group is not None else _bf16_native_plans(graph, d16(weights.shape[1]), d16(weights.shape[2]), relu)
    if plans is not None:
        return _RelationalMPBF16.apply(features, weights, bias, graph, relu, plans)
    if group is not None:
        out = sharded_relational_mp(features.float(), weights, bias, graph, group, n_slabs, comm)
        return (torch.relu(out) if relu else out).to(torch.bfloat16)
    return relational_mp(features.float(), weights, bias, graph, relu=relu).to(torch.bfloat16)


def _join_shards(partial, group, mode="allreduce"):
    """Sum the ranks' partial N x d matrices (in place; returns the tensor to use).  mode (an argument -- the sharded
    layer's transport, torch_rgcn.dist.set_transport -- not process-global state):
      allreduce (default)  one RCCL all-reduce of the whole matrix
      rs_ag                reduce-scatter of row blocks + all-gather (the two halves of an all-reduce as separate
                           collectives: lets RCCL pick its direct algorithms per half; same bytes on every link)
      a2a                  direct exchange: all-to-all of the row blocks (every rank sends block j straight to rank j: on the
                           fully connected xGMI mesh all 7 links carry 1/8 of the matrix at once, a ring carries 7/8 of it
                           through every link in turn), local sum of the world_size received blocks, all-gather"""
    import torch.distributed as dist
    assert mode in ("allreduce", "rs_ag", "a2a"), f"unknown transport {mode!r}"
    if mode == "a2a":
        world = dist.get_world_size(group)
        n, d = partial.shape
        rows = -(-n // world)
        buf = partial if rows * world == n else torch.nn.functional.pad(partial, (0, 0, 0, rows * world - n))
        recv = torch.empty_like(buf)                         # recv[j] = rank j's partial of MY row block
        dist.all_to_all_single(recv, buf, group=group)
        shard = recv.view(world, rows * d).sum(dim=0).view(rows, d)      # fixed order: rank 0 .. world-1
        dist.all_gather_into_tensor(buf, shard, group=group)
        return buf if rows * world == n else buf[:n].contiguous()
    if mode == "rs_ag":
        world = dist.get_world_size(group)
        n, d = partial.shape
        rows = -(-n // world)
        buf = partial if rows * world == n else torch.nn.functional.pad(partial, (0, 0, 0, rows * world - n))
        shard = torch.empty((rows, d), device=partial.device, dtype=partial.dtype)
        dist.reduce_scatter_tensor(shard, buf, group=group)
        dist.all_gather_into_tensor(buf, shard, group=group)
        return buf if rows * world == n else buf[:n].contiguous()
    dist.all_reduce(partial, group=group)
    return partial


def _all_ranks_agree(mine, graph, group, key, device):
    """A route whose collectives differ from the fallback's (other row ranges, other slab cuts) may only be taken when EVERY rank of the
    group can take it: hub pieces, for one, exist on the rank that owns a hub relation and nowhere else (ranks deciding on their
    own would post mismatched all-reduces -- a hang or silently wrong dX).  One MIN all-reduce of the local eligibility per (graph, route),
    cached on the graph: every rank reaches this call on its first backward (the conditions in front of it are rank-invariant)."""
    import torch.distributed as dist
    cache = graph.__dict__.setdefault("_group_routes", {})
    if key not in cache:
        flag = torch.tensor([1 if mine else 0], device=device, dtype=torch.int32)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=group)
        cache[key] = bool(int(flag.item()))
    return cache[key]


class _ShardedRelationalMP(torch.autograd.Function):
    """Relation shard of the featured layer.  Features and upstream gradient are replicated; every rank computes the
    partial output (and, in backward, the partial feature gradient) of ITS relations and the partials are summed over
    the group; rank 0 alone adds the bias (it is summed once).  n_slabs > 0: the partial is produced slab by slab and
    every finished slab is all-reduced asynchronously (RCCL on its own stream) while the next slab's kernels run --
    pays when the kernels are long against the collective (weak scaling); n_slabs = 0: one collective after the kernel
    (strong scaling at 8 GPUs: the kernel is ~8x shorter than the collective, nothing to hide behind)."""

    @staticmethod
    def forward(ctx, X, W, bias, graph, group, n_slabs, comm="allreduce"):
        import torch.distributed as dist
        X, W, bias, ctx.dims = _pad_blocks(X, W, bias)
        X, W = dense(X), dense(W)
        rank = dist.get_rank(group)
        b = dense(bias) if (bias is not None and rank == 0) else None
        with _native.w16_scope() as w16:
            if n_slabs > 0 and comm == "allreduce":
                works = []
                out = _native.spmm_slabs(X, W, b, graph.fwd_plan(W.shape[2]), n_slabs,
                                         lambda o, r0, r1: works.append(dist.all_reduce(o[r0:r1], group=group, async_op=True)))
                for w in works:
                    w.wait()
            else:
                out = _join_shards(_native.spmm(X, W, b, graph.fwd_plan(W.shape[2])), group, comm)
        ctx.w16 = w16.pair(W)
        ctx.graph, ctx.group, ctx.n_slabs, ctx.has_bias, ctx.comm = graph, group, n_slabs, bias is not None, comm
        ctx.save_for_backward(X, W)
        return out if ctx.dims is None else out[:, :ctx.dims[1]]

    @staticmethod
    def backward(ctx, g):
        X, W = ctx.saved_tensors
        with _native.w16_scope(seed=(W, ctx.w16)):
            return _ShardedRelationalMP._backward(ctx, g, X, W)

    @staticmethod
    def _backward(ctx, g, X, W):
        import torch.distributed as dist
        graph = ctx.graph
        g = _padded_grad(g, ctx.dims)
        dX = dW = db = None
        works = []
        slabbed = ctx.n_slabs > 0 and ctx.comm == "allreduce"
        both = None
        joined = False
        if ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and slabbed and not deterministic() and routes.get("bwd", "fused") != "split":
            # the fused backward slab by slab (round 5): the all-reduce of slab k's dX rows -- RCCL on its own stream -- runs under slab
            # k + 1's kernel; dW (owner-local rows) keeps adding across the slabs.  Plans with hub pieces keep the unfused slab path below.
            bp = graph.bwd_blk_plan()
            mine = bp is not None and W.shape[1] == 16 and W.shape[2] == 16 and _native.bwd_fused_slabs_ok(bp)
            if _all_ranks_agree(mine, graph, ctx.group, ("bwd_fused_slabs", ctx.n_slabs), g.device):
                dX, dW, _ = _native.bwd_fused_slabs(g, X, W, bp, ctx.n_slabs,
                                                    lambda o, r0, r1: works.append(dist.all_reduce(o[r0:r1], group=ctx.group, async_op=True)))
                both, joined = (dX, dW), True
        if not slabbed:         # (a rank's share of the relations never takes the sparse-bucket routes)
            route, plan = _backward_route(graph, W.shape[1], W.shape[2], ctx.needs_input_grad[0], ctx.needs_input_grad[1], sparse=False)
            if route != "split":
                both = _native.bwd_own(g, X, W, plan, want_db=True) if route == "own" else \
                    _native.bwd_fused(g, X, W, plan, atomic=not deterministic(), want_db=True)
        if both is not None:
            dX, dW = both[:2]
        else:
            if ctx.needs_input_grad[0]:
                Wt = W.transpose(1, 2).contiguous()
                if slabbed:
                    dX = _native.spmm_slabs(g, Wt, None, graph.bwd_plan(W.shape[1]), ctx.n_slabs,
                                            lambda o, r0, r1: works.append(dist.all_reduce(o[r0:r1], group=ctx.group, async_op=True)))
                else:
                    dX = _native.spmm(g, Wt, None, graph.bwd_plan(W.shape[1]))
            if ctx.needs_input_grad[1]:   # owner-local: runs while the last slabs are still being reduced
                dW = _weight_gradient(X, W, g, graph)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _native.colsum(g)
        if dX is not None and not slabbed and not joined:
            dX = _join_shards(dX, ctx.group, ctx.comm)
        for w in works:
            w.wait()
        return (*_unpad_blocks(ctx.dims, dX, dW, db), None, None, None, None)


def sharded_relational_mp(features, weights, bias, graph, group, n_slabs=0, comm="allreduce"):
    return _ShardedRelationalMP.apply(features, weights, bias, graph, group, n_slabs, comm)


def _featureless_csr(graph, width):
    """the featureless layer's route: destination-major CSR kernels (one lane group per message) when the (tile, relation) buckets
    of the tile plan are mostly padding (AIFB: 91 relations on 8-row tiles, 23 slots per message) and the graph is static"""
    if graph._dev is None or graph.sync_free or graph.per_call or routes.get("featureless_csr", "auto") == "0":
        return False
    if routes.get("featureless_csr", "auto") == "1":
        return True
    fp = graph.fwd_plan(width)
    return not _dense_buckets(fp) and graph.max_degree() <= 4096


def _relu_epilogue(ctx, res, relu):
    """res: what a native forward returned for relu=True -- (out, applied in the kernel's epilogue) -- or the plain output; finishes the
    activation where the kernel could not, and keeps what the backward needs (see _ReluToken)"""
    ctx.relu = bool(relu)
    ctx.out_token = _ReluToken(private=relu == "private") if relu else None
    if not relu:
        return res
    out, applied = res if isinstance(res, tuple) else (res, False)
    return out if applied else torch.relu_(out)


def _relu_backward(ctx, g, out):
    """the gradient before the fused ReLU: masked here unless the consumer's backward kernel already did it (_ReluToken)"""
    if ctx.relu and not ctx.out_token.premasked(g):
        g = torch.ops.aten.threshold_backward(g, out, 0.0)
    return g


class _FeaturelessMP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, bias, graph, relu=False):
        table = dense(table)
        b = None if bias is None else dense(bias)
        ctx.csr = _featureless_csr(graph, table.shape[2])
        if ctx.csr:
            out = _relu_epilogue(ctx, _native.featureless_csr_fwd(table, b, graph.csr("fwd"), relu=bool(relu)), relu)
        else:
            out = _relu_epilogue(ctx, _native.featureless_fwd(table, b, graph.fwd_plan(table.shape[2])), relu)
        if relu:
            ctx.save_for_backward(out)
        ctx.graph = graph
        ctx.has_bias = bias is not None
        ctx.num_rels = table.shape[0]
        ctx.n_src = table.shape[1]
        ctx.width = table.shape[2]
        return out

    @staticmethod
    def backward(ctx, g):
        g = dense(g)
        if ctx.relu:
            g = _relu_backward(ctx, g, ctx.saved_tensors[0])
        dT = db = None
        if ctx.needs_input_grad[0]:
            if ctx.csr:
                dT = _native.featureless_csr_wgrad(g, ctx.graph.csr("fwd"), ctx.num_rels, ctx.n_src)
            else:
                dT = _native.featureless_wgrad(g, ctx.graph.fwd_plan(ctx.width), ctx.num_rels)
        if ctx.has_bias and ctx.needs_input_grad[1]:
            db = _native.colsum(g)
        return dT, db, None, None


class _BlockMP(torch.autograd.Function):
    """Block-diagonal per-relation weights without expanding them (reference layers.py:243-244 / :520-527 build
    block_diag(blocks) and run the dense path): out = sum_r A_r X blockdiag(B_r) + b on the CSR kernels of csrc/rgcn_block.hip.
    Relations past blocks.shape[0] (the LP layer's dense self-loop relation) are skipped -- the caller adds them."""

    @staticmethod
    def forward(ctx, X, blocks, bias, graph, relu):
        X, blocks = dense(X), dense(blocks)
        b = None if bias is None else dense(bias)
        out = _native.block_spmm(X, blocks, b, graph.csr("fwd"), relu=relu)
        ctx.save_for_backward(X, blocks, out if relu else None)
        ctx.graph = graph
        ctx.has_bias = bias is not None
        ctx.relu = relu
        return out

    @staticmethod
    def backward(ctx, g):
        X, blocks, out = ctx.saved_tensors
        g = dense(g)
        if ctx.relu:
            g = torch.ops.aten.threshold_backward(g, out, 0.0)
        graph = ctx.graph
        dX = dB = db = None
        if ctx.needs_input_grad[0]:
            dX = _native.block_spmm(g, blocks, None, graph.csr("bwd"), transposed=True)
        if ctx.needs_input_grad[1]:
            dB = _native.block_wgrad(X, g, graph.wgt_plan(), tuple(blocks.shape))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _native.colsum(g)
        return dX, dB, db, None, None


def block_mp(features, blocks, bias, graph, relu=False):
    """features [N, nb * bi], blocks [R', nb, bi, bo] -> [N, nb * bo]"""
    return _BlockMP.apply(features, blocks, bias, graph, relu)


def use_block_path(graph, blocks):
    """The block kernels need the device-side graph build (CSR + relation-major plan) and blocks of at most 8 x 8.  At
    width 16 the expanded 16 x 16 weights on the matrix-core kernels are faster (AM shape, 4 x 4 blocks: 1.96 ms per layer
    forward + backward against 2.43 -- every message re-reads its blocks from L2, 4x the bytes of its feature row), so
    RGCN_BLOCK_PATH=1 (default) takes the block kernels only above width 16; 2 = whenever supported; 0 = never."""
    mode = routes.get("block_path", "1")
    if mode == "0" or graph._dev is None or not _native.block_supported(blocks.shape[2], blocks.shape[3]):
        return False
    wide = blocks.shape[1] * blocks.shape[2] > 16 or blocks.shape[1] * blocks.shape[3] > 16
    return wide or mode == "2"


class _DiagMP(torch.autograd.Function):
    """Diagonal per-relation weights (reference layers.py:289-292): out = sum_r A_r (X * w_r) + b, backward
    dX = sum_r A_r^T (G * w_r) (the same kernel on the transposed plan), dw_r = sum over the messages of r of val X[src] * G[dst]."""

    @staticmethod
    def forward(ctx, X, w, bias, graph):
        X, w = dense(X), dense(w)
        b = None if bias is None else dense(bias)
        out = _native.diag_spmm(X, w, b, graph.csr("fwd"))
        ctx.save_for_backward(X, w)
        ctx.graph = graph
        ctx.has_bias = bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        X, w = ctx.saved_tensors
        g = dense(g)
        graph = ctx.graph
        dX = dw = db = None
        if ctx.needs_input_grad[0]:
            dX = _native.diag_spmm(g, w, None, graph.csr("bwd"))
        if ctx.needs_input_grad[1]:
            dw = _native.diag_wgrad(X, g, graph.wgt_plan(), w.shape[0])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _native.colsum(g)
        return dX, dw, db, None


def diag_mp(features, w, bias, graph):
    """features [N, d], w [R, d] -> [N, d]"""
    return _DiagMP.apply(features, w, bias, graph)


def use_diag_path(graph, d):
    """the diagonal kernels need the device-side graph build (CSR + relation-major plan)"""
    return graph._dev is not None and routes.get("diag_path") != "0"


# bf16 storage of the two structured decompositions: storage twins of _BlockMP / _DiagMP.  X and the upstream gradient
# are gathered as bf16 rows, the parameters arrive widened to fp32 by the layer (autograd carries the cast back: a bf16 parameter gets a bf16
# gradient), out and dX are fp32 sums rounded once, the parameter gradients fp32.  Nothing of size R x d x d is built.


class _BlockMPBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, blocks, bias, graph, relu):
        X, blocks = dense(X), dense(blocks)
        b = None if bias is None else dense(bias)
        out = _native.block_spmm_bf16(X, blocks, b, graph.csr("fwd"), relu=relu)
        ctx.save_for_backward(X, blocks, out if relu else None)
        ctx.graph, ctx.has_bias, ctx.relu = graph, bias is not None, relu
        return out

    @staticmethod
    def backward(ctx, g):
        X, blocks, out = ctx.saved_tensors
        g = dense(g.to(torch.bfloat16))              # (exact when it comes from a bf16 consumer)
        if ctx.relu:
            g = torch.ops.aten.threshold_backward(g, out, 0.0)        # a mask: exact in bf16
        graph = ctx.graph
        dX = dB = db = None
        if ctx.needs_input_grad[0]:
            dX = _native.block_spmm_bf16(g, blocks, None, graph.csr("bwd"), transposed=True)
        if ctx.needs_input_grad[1]:
            dB = _native.block_wgrad_bf16(X, g, graph.wgt_plan(), tuple(blocks.shape))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _native.colsum_bf16(g)
        return dX, dB, db, None, None


def _check_bf16_args(name, features, *params):
    if features.dtype != torch.bfloat16:
        raise TypeError(f"{name}: features must be torch.bfloat16, got {features.dtype}")
    if any(p is not None and p.dtype != torch.float32 for p in params):
        raise TypeError(f"{name}: the parameters are widened to torch.float32 by the caller")


def block_mp_bf16(features, blocks, bias, graph, relu=False):
    """block_mp for bf16 features [N, nb * bi]: blocks [R', nb, bi, bo] and bias fp32 -> bf16 [N, nb * bo] (csrc/rgcn_block.hip, bf16 forms)"""
    _check_bf16_args("block_mp_bf16", features, blocks, bias)
    return _BlockMPBF16.apply(features, blocks, bias, graph, bool(relu))


class _BlockSelfMPBF16(torch.autograd.Function):
    """The LP layer with block decomposition on bf16 features: out = round(block part + self-loop part), ONE rounding.  The block part
    (relations 0 .. R-2) is gathered as bf16 and left as unrounded fp32 sums (the fp32 output mode of rgcn_block_spmm_bf16); the self-loop
    relation has a dense weight and one message per node, X.float() @ blocks_self on rgcn_gemm_f32, masked by the node keep-mask or by
    the schlichtkrull dropout exactly as the fp32 route does (torch.native_dropout: what nn.functional.dropout dispatches to on the GPU, so
    a seeded run draws the same mask in both dtypes).  dX likewise: transposed block spmm (fp32 output mode) + g @ blocks_self^T, rounded once."""

    @staticmethod
    def forward(ctx, X, blocks, blocks_self, bias, graph, node_mask, self_drop):
        X, blocks, blocks_self = dense(X), dense(blocks), dense(blocks_self)
        b = None if bias is None else dense(bias)
        acc = _native.block_spmm_bf16(X, blocks, b, graph.csr("fwd"), out_f32=True)
        own = _native.gemm(X.float(), blocks_self)
        drop_mask = None
        if self_drop is not None:
            own, drop_mask = torch.native_dropout(own, self_drop, True)
        elif node_mask is not None:
            own = own * node_mask[:, None].to(own.dtype)
        ctx.save_for_backward(X, blocks, blocks_self, drop_mask, node_mask)
        ctx.graph, ctx.has_bias, ctx.self_drop = graph, bias is not None, self_drop
        return acc.add_(own).to(torch.bfloat16)

    @staticmethod
    def backward(ctx, g):
        X, blocks, blocks_self, drop_mask, node_mask = ctx.saved_tensors
        g = dense(g.to(torch.bfloat16))
        graph = ctx.graph
        g_own = g.float()                            # the gradient of the self-loop messages
        if drop_mask is not None:
            g_own = torch.ops.aten.native_dropout_backward(g_own, drop_mask, 1.0 / (1.0 - ctx.self_drop))
        elif node_mask is not None:
            g_own = g_own * node_mask[:, None].to(g_own.dtype)
        dX = dB = dS = db = None
        if ctx.needs_input_grad[0]:
            acc = _native.block_spmm_bf16(g, blocks, None, graph.csr("bwd"), transposed=True, out_f32=True)
            dX = acc.add_(_native.gemm(g_own, blocks_self, trans_b=True)).to(torch.bfloat16)
        if ctx.needs_input_grad[1]:
            dB = _native.block_wgrad_bf16(X, g, graph.wgt_plan(), tuple(blocks.shape))
        if ctx.needs_input_grad[2]:
            X32 = X.float()
            dS = _native.gemm(X32, g_own, trans_a=True, split_k=_split_k(X32.shape[0], X32.shape[1], g_own.shape[1]))
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = _native.colsum_bf16(g)
        return dX, dB, dS, db, None, None, None


def block_self_mp_bf16(features, blocks, blocks_self, bias, graph, node_mask=None, self_drop=None):
    """the LP layer's block decomposition for bf16 features: block_mp over `blocks` plus the dense self-loop relation features @ blocks_self
    (rows masked by node_mask [N] where given, or dropped out with probability self_drop), rounded to bf16 once.  Parameters fp32."""
    _check_bf16_args("block_self_mp_bf16", features, blocks, blocks_self, bias)
    return _BlockSelfMPBF16.apply(features, blocks, blocks_self, bias, graph, node_mask, self_drop)


class _DiagMPBF16(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, w, bias, graph):
        X, w = dense(X), dense(w)
        b = None if bias is None else dense(bias)
        out = _native.diag_spmm_bf16(X, w, b, graph.csr("fwd"))
        ctx.save_for_backward(X, w)
        ctx.graph, ctx.has_bias = graph, bias is not None
        return out

    @staticmethod
    def backward(ctx, g):
        X, w = ctx.saved_tensors
        g = dense(g.to(torch.bfloat16))
        graph = ctx.graph
        dX = dw = db = None
        if ctx.needs_input_grad[0]:
            dX = _native.diag_spmm_bf16(g, w, None, graph.csr("bwd"))
        if ctx.needs_input_grad[1]:
            dw = _native.diag_wgrad_bf16(X, g, graph.wgt_plan(), w.shape[0])
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _native.colsum_bf16(g)
        return dX, dw, db, None


def diag_mp_bf16(features, w, bias, graph):
    """diag_mp for bf16 features [N, d]: w [R, d] and bias fp32 -> bf16 [N, d] (diag_csr_kernel / diag_wgrad_kernel, bf16 forms)"""
    _check_bf16_args("diag_mp_bf16", features, w, bias)
    return _DiagMPBF16.apply(features, w, bias, graph)


def _split_k(K, M, N):
    """slices of the K dimension so that a skinny product (K = number of nodes, M x N = a weight matrix) still fills the chip"""
    tiles = -(-M // 128) * -(-N // 128)
    # (at most 64 slices: past that the partial products' round trip through HBM costs more than the extra workgroups buy --
    # tools/splitk_probe.py, WN18's dbases = ag^T g, K = 40,943: 64 slices 122.7 us, the former choice of 79 133.7, 128 142.0)
    # short K (the weight assembly's adjoint: K = relations, a few hundred) is ONE workgroup's serial loop of K / 16 steps, each a global
    # round trip with nothing to overlap it (32 us for K = 267): slices of at least three steps
    # slice length: 48 steps of K for short products, growing to 512 for long ones -- continuous in K (K // 48 below 8192 and K // 512
    # from there on gave K = 8191 64 slices and K = 8192 16)
    return int(max(1, min(64, (4 * 256) // max(tiles, 1), K // max(48, min(512, K // 16)))))


class _MatmulMFMA(torch.autograd.Function):
    """A @ B on rgcn_gemm_f32 (the weight assembly einsum('rb,bio->rio') of layers.py:241-242 as an [R, B] x [B, d_i d_o]
    product, and the other small dense products of the path): no rocBLAS."""

    @staticmethod
    def forward(ctx, A, B):
        A, B = dense(A), dense(B)
        ctx.save_for_backward(A, B)
        return _native.gemm(A, B)

    @staticmethod
    def backward(ctx, g):
        A, B = ctx.saved_tensors
        g = dense(g)
        dA = _native.gemm(g, B, trans_b=True) if ctx.needs_input_grad[0] else None          # g B^T
        # A^T g: K = the rows of A (nodes) -- split so that a small M x N output still fills the chip (fixed-order reduction)
        dB = _native.gemm(A, g, trans_a=True, split_k=_split_k(A.shape[0], A.shape[1], g.shape[1])) \
            if ctx.needs_input_grad[1] else None
        return dA, dB


def matmul_mfma(A, B):
    return _MatmulMFMA.apply(A, B)


class _BasisMP(torch.autograd.Function):
    """W_r = sum_b comps[r,b] bases[b] at large width: aggregate per basis, then contract (B d_in) x d_out on the matrix
    cores -- never touches an R x d x d weight tensor (reference: layers.py:241-242, :468-469).  Forward: aggregation
    kernel + hand-written MFMA GEMM (rgcn_gemm_f32; 57 TFLOP/s at WN18 size, rocBLAS addmm 50).  Backward:
    d_ag = g flat^T and dbases = ag^T g on rgcn_gemm_f32, dX by the same aggregation on the source-major CSR, dcomps by the
    relation-major dot-product kernel."""

    @staticmethod
    def forward(ctx, X, bases, comps, bias, graph):
        X, bases, comps = dense(X), dense(bases), dense(comps)
        B, d_in, d_out = bases.shape
        b = None if bias is None else dense(bias)
        ag = _native.basis_aggregate(X, comps, graph.csr("fwd"), B, d_in, 1)          # [N, B*d_in]
        out = _native.gemm(ag, bases.view(B * d_in, d_out), bias=b)
        ctx.graph, ctx.has_bias = graph, bias is not None
        ctx.save_for_backward(X, bases, comps, ag)
        return out

    @staticmethod
    def backward(ctx, g):
        X, bases, comps, ag = ctx.saved_tensors
        B, d_in, d_out = bases.shape
        g = dense(g)
        flat = bases.view(B * d_in, d_out)
        dX = dB = dC = db = None
        d_ag = _native.gemm(g, flat, trans_b=True) if (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]) else None   # [N, B*d_in]
        if ctx.needs_input_grad[1]:
            dB = _native.gemm(ag, g, trans_a=True, split_k=_split_k(ag.shape[0], B * d_in, d_out)).view(B, d_in, d_out)
        if ctx.needs_input_grad[0]:
            dX = _native.basis_aggregate(d_ag, comps, ctx.graph.csr("bwd"), B, d_in, B)
        if ctx.needs_input_grad[2]:
            if ctx.graph.per_call and not deterministic() and _native.basis_dcomps_csr_ok(comps.shape[0], B, d_in):
                # per-step (LP) graphs: on the CSR the forward walked -- building a relation-major plan for this one kernel costs a dozen launches
                dC = _native.basis_dcomps_csr(X, d_ag, ctx.graph.csr("fwd"), comps.shape[0], B, d_in)
            else:
                dC = _native.basis_dcomps(X, d_ag, ctx.graph.wgt_plan(), comps.shape[0], B, d_in)
        if ctx.has_bias and ctx.needs_input_grad[3]:
            db = _native.colsum(g)
        return dX, dB, dC, db, None


class _FeaturelessBasisMP(torch.autograd.Function):
    """Featureless layer with basis decomposition WITHOUT the R x N x d_out weight table the reference
    materialises (layers.py:242 + :288; 17.8 GB for AM):  out[s] = sum_e val_e sum_b comps[r_e,b] bases[b,o_e,:]."""

    @staticmethod
    def forward(ctx, bases, comps, bias, graph, relu=False):
        out = _FeaturelessBasisMP._forward(ctx, bases, comps, bias, graph, relu)
        ctx.out_padded = bool(getattr(out, "_rgcn_zero_padded", False))     # (the saved copy comes back as another Python object)
        to_save = ctx.to_save
        del ctx.to_save
        ctx.save_for_backward(*to_save, *((out,) if relu else ()))
        return out

    @staticmethod
    def _forward(ctx, bases, comps, bias, graph, relu):
        B, N, d = bases.shape
        ctx.src_major = _native.fbasis_supported(B, d) and routes.get("fbasis", "src") == "src"
        # Layout of the table the source-major kernels walk.  Node-major [N, B, d] (a transposed copy per step, and a transposed
        # gradient back): a node's B rows are ONE contiguous run -- what a table far beyond the caches needs (AM as shipped: 2.7 GB,
        # rows of 40 bytes: reading them in place, 40 half-used lines per node, cost 33.5 ms per step against 24).  Basis-major
        # [B, N, d] = the parameter itself, no copies: wins while the table stays cache-resident (MUTAG: 45 MB, step 0.56 -> 0.51 ms).
        # Round 4: tables beyond the caches are walked in place too, by the tile kernels (rgcn_fbasis_tile.hip: 16 source nodes per tile,
        # staged through LDS with aligned 16-byte accesses, software-pipelined) -- no transposed copy, no transposed gradient.  They also
        # beat the wave-per-node kernels on a cache-resident table of MUTAG's size (45 MB: forward 42 -> 40 us, backward 65 -> 49 us), hence
        # the 32 MB threshold -- which only holds where the tile kernels can take over: a shape or mode they refuse (deterministic mode,
        # B > 64 ...) keeps round 3's 256 MB before it pays for the transposed copy.
        tile_ok, tile_mode = _native.fbasis_tile_ok(comps.shape[0], B, d, N, graph.fbasis_plan().max_src_degree) if ctx.src_major else (False, 0)
        limit_mb = int(routes.get("fbasis_inplace_mb")) if routes.is_set("fbasis_inplace_mb") else (32 if tile_ok else 256)
        ctx.in_place = ctx.src_major and B * N * d * 4 <= limit_mb << 20
        tiled, ctx.tile_mode = (tile_ok, tile_mode) if (ctx.src_major and not ctx.in_place) else (False, 0)
        ctx.tile_bwd = tiled
        if tiled:
            comps, bases = dense(comps), dense(bases)
            ctx.graph, ctx.has_bias = graph, bias is not None
            ctx.in_place = True
            ctx.to_save = (bases, comps)
            return _relu_epilogue(ctx, _native.fbasis_tile_fwd(bases, comps, bias, graph.fbasis_plan(), relu=bool(relu), mode=ctx.tile_mode,
                                                               padded=routes.get("pad16_view", "1") != "0"), relu)
        if ctx.src_major and ctx.in_place:
            comps, bases = dense(comps), dense(bases)
            ctx.graph, ctx.has_bias = graph, bias is not None
            ctx.to_save = (bases, comps)
            return _relu_epilogue(ctx, _native.fbasis_fwd(bases, comps, bias, graph.fbasis_plan(), basis_major=True, relu=bool(relu)), relu)
        table = bases.permute(1, 0, 2).contiguous()                   # [N, B, d]: one contiguous block per source node
        if ctx.src_major:   # every node's B x d block is read once
            comps = dense(comps)
            ctx.graph, ctx.has_bias = graph, bias is not None
            ctx.to_save = (table, comps)
            return _relu_epilogue(ctx, _native.fbasis_fwd(table, comps, bias, graph.fbasis_plan(), relu=bool(relu)), relu)
        comps = dense(comps)
        out = _native.basis_aggregate(table.view(N, B * d), comps, graph.csr("fwd"), B, d, B)
        if bias is not None:
            out += bias
        ctx.graph, ctx.has_bias = graph, bias is not None
        # small blocks (S2: B = 2): the backward walks the sources in order and reads / writes their blocks as B sequential streams -- straight
        # from the PARAMETER's [B, N, d] layout and into a gradient of that layout (round 5: no strided view for AccumulateGrad to copy);
        # only the forward's per-message gather wants the node-major copy (one 128-byte line per message instead of B half-used ones)
        ctx.small_in_place = (not deterministic()) and _native.fbasis_small_ok(comps.shape[0], B, d)
        ctx.to_save = (dense(bases), comps) if ctx.small_in_place else (table, comps)
        return _relu_epilogue(ctx, out, relu)

    @staticmethod
    def backward(ctx, g):
        if getattr(ctx, "tile_bwd", False) and g.dim() == 2 and g.shape[1] % 16 and _zero_padded_rows(g, g.shape[1] + (-g.shape[1] % 16)):
            # the consumer handed its feature gradient back as the first columns of zero-padded [N, 16] rows: the tile kernels gather those rows
            # in place (64-byte aligned: one line per row instead of 40-byte rows straddling two), the ReLU's mask and the bias' column sum run
            # on the padded buffer (its extra columns stay zero)
            wide = g.stride(0)
            g16 = torch.as_strided(g, (g.shape[0], wide), (wide, 1))
            if ctx.relu and not ctx.out_token.premasked(g):
                out = ctx.saved_tensors[2]
                out16 = torch.as_strided(out, (out.shape[0], wide), (wide, 1)) if (ctx.out_padded and _rows16(out) and out.stride(0) == wide) else \
                    _native.resize3(dense(out), (out.shape[0], wide))
                g16 = torch.ops.aten.threshold_backward(g16, out16, 0.0)
            table, comps = ctx.saved_tensors[:2]
            dB, dC = _native.fbasis_tile_bwd(table, comps, g16[:, :g.shape[1]], ctx.graph.fbasis_plan(), ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                             mode=ctx.tile_mode)
            db = _native.colsum(g16)[:g.shape[1]].contiguous() if ctx.has_bias and ctx.needs_input_grad[2] else None
            return dB, dC, db, None, None
        g = dense(g)
        if ctx.relu:
            g = _relu_backward(ctx, g, ctx.saved_tensors[2])
        if ctx.src_major:
            table, comps = ctx.saved_tensors[:2]
            if getattr(ctx, "tile_bwd", False):
                dB, dC = _native.fbasis_tile_bwd(table, comps, g, ctx.graph.fbasis_plan(), ctx.needs_input_grad[0], ctx.needs_input_grad[1], mode=ctx.tile_mode)
            else:
                dB, dC = _native.fbasis_bwd(table, comps, g, ctx.graph.fbasis_plan(), ctx.needs_input_grad[0],
                                            ctx.needs_input_grad[1], basis_major=ctx.in_place)
            if dB is not None and not ctx.in_place:
                dB = dB.permute(1, 0, 2)      # a view: autograd accumulates it into the [B, N, d] parameter gradient
            db = _native.colsum(g) if ctx.has_bias and ctx.needs_input_grad[2] else None
            return dB, dC, db, None, None
        table, comps = ctx.saved_tensors[:2]
        dB = dC = db = None
        if getattr(ctx, "small_in_place", False):
            # small blocks (S2: B = 2, d = 16): one walk of the source-major CSR for both gradients (one gather per message), in the parameter's layout
            B, N, d = table.shape
            dB, dC = _native.fbasis_small_bwd(g, table, comps, ctx.graph.csr("bwd"), B, d, basis_major=True)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                db = _native.colsum(g)
            return (dB if ctx.needs_input_grad[0] else None), (dC if ctx.needs_input_grad[1] else None), db, None, None
        N, B, d = table.shape
        if ctx.needs_input_grad[0]:
            dB = _native.basis_aggregate(g, comps, ctx.graph.csr("bwd"), B, d, 1).view(N, B, d).permute(1, 0, 2)
        if ctx.needs_input_grad[1]:
            dC = _native.basis_dcomps(g, table.view(N, B * d), ctx.graph.wgt_plan(), comps.shape[0], B, d, swap=True)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = _native.colsum(g)
        return dB, dC, db, None, None


def featureless_basis_mp(bases, comps, bias, graph, relu=False):
    return _FeaturelessBasisMP.apply(bases, comps, bias, graph, relu)


class _FeaturelessBasisMPBF16(torch.autograd.Function):
    """featureless_basis_mp on a bf16 bases table, on the tile kernels: the table is staged as bf16 and widened, comps and the
    bias are fp32 (widened here, once per call, never rounded), out is the fp32 sum rounded to bf16 once (after the bias and the ReLU).
    Backward: the upstream gradient is gathered as bf16 rows; dbases is bf16 in the parameter's layout (the fp32 / fp64 sum rounded once),
    dcomps and db are fp32 sums returned in each parameter's dtype."""

    @staticmethod
    def forward(ctx, bases, comps, bias, graph, relu, mode):
        ctx.graph, ctx.mode, ctx.relu, ctx.has_bias = graph, mode, bool(relu), bias is not None
        ctx.c_dtype, ctx.b_dtype = comps.dtype, None if bias is None else bias.dtype
        bases, c32 = dense(bases), dense(comps.detach().float())
        b32 = None if bias is None else dense(bias.detach().float())
        out = _native.fbasis_tile_fwd_bf16(bases, c32, b32, graph.fbasis_plan(), relu=bool(relu), mode=mode)
        out = out[0] if relu else out
        ctx.save_for_backward(bases, c32, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        bases, c32, out = ctx.saved_tensors
        d = bases.shape[2]
        g = g.to(torch.bfloat16)
        if ctx.relu:
            g = torch.ops.aten.threshold_backward(g, out, 0.0)        # a mask: exact in bf16
        # zero-padded [N, 16 k] rows: 32-byte aligned gathers in the tile kernels (20-byte rows at d = 10 straddle lines), and the width
        # rgcn_colsum_bf16 wants (a multiple of 4) for the bias
        g16 = dense(_pad16(g, (d,)))
        gv = g16[:, :d] if g16.shape[1] != d else g16
        dB, dC = _native.fbasis_tile_bwd_bf16(bases, c32, gv, ctx.graph.fbasis_plan(), ctx.needs_input_grad[0], ctx.needs_input_grad[1],
                                              mode=ctx.mode)
        db = _native.colsum_bf16(g16)[:d].to(ctx.b_dtype) if ctx.has_bias and ctx.needs_input_grad[2] else None
        dC = dC.to(ctx.c_dtype) if dC is not None else None
        return dB, dC, db, None, None, None


def featureless_basis_mp_bf16(bases, comps, bias, graph, relu=False):
    """featureless_basis_mp for a bf16 bases table (comps and bias fp32 or bf16) -> bf16 [N, d].  The tile kernels whenever
    fbasis_tile_ok offers them, whatever the table's size (rgcn_basis.hip has no bf16 form); otherwise -- shapes the tile kernels refuse,
    RGCN_DETERMINISTIC=1, fbasis_tile=0, fbasis=csr -- the fp32 route on the widened parameters with its output rounded: CORRECTNESS ONLY,
    no speed-up (autograd carries the casts)."""
    if bases.dtype != torch.bfloat16:
        raise TypeError(f"featureless_basis_mp_bf16: bases must be torch.bfloat16, got {bases.dtype}")
    if any(t is not None and t.dtype not in (torch.float32, torch.bfloat16) for t in (comps, bias)):
        raise TypeError("featureless_basis_mp_bf16: comps and bias must be torch.float32 or torch.bfloat16")
    B, N, d = bases.shape
    ok, mode = False, 0
    if _native.fbasis_supported(B, d) and routes.get("fbasis", "src") == "src":
        ok, mode = _native.fbasis_tile_ok(comps.shape[0], B, d, N, graph.fbasis_plan().max_src_degree)
    if ok:
        return _FeaturelessBasisMPBF16.apply(bases, comps, bias, graph, bool(relu), mode)
    out = featureless_basis_mp(bases.float(), comps.float(), None if bias is None else bias.float(), graph, relu=bool(relu))
    return out.to(torch.bfloat16)


def basis_mp(features, bases, comps, bias, graph):
    return _BasisMP.apply(features, bases, comps, bias, graph)


def use_basis_path(num_bases, d_in, d_out, graph):
    """aggregate-then-contract pays when the per-message d_in x d_out product is large and B is small"""
    return graph._dev is not None and d_in * d_out >= 64 * 64 and num_bases <= 8


def relational_mp(features, weights, bias, graph, relu=False, blocks=None):
    """features [N, d_in], weights [R, d_in, d_out] (dense), bias [d_out] or None -> [N, d_out]; relu=True applies the
    activation in the kernel's epilogue (the backward masks the upstream gradient with the stored output), relu="private" also lets
    the layer that consumes the output mask on this layer's behalf (see _ReluToken: the caller promises that nobody asks autograd for
    the output's gradient); blocks: the
    [R, nb, bi, bo] parameter when weights = block_diag(blocks) (a hint: lets the forward skip the zero entries)"""
    # features = the output of a layer that applied ReLU in its kernel's epilogue: its backward node carries the token
    in_token = getattr(getattr(features, "grad_fn", None), "out_token", None)
    if in_token is not None:
        import weakref
        in_token.consumer_input = weakref.ref(features)     # looked at again in the backward: see _ReluToken.observed
    return _RelationalMP.apply(features, weights, bias, graph, relu, blocks, in_token)


def featureless_mp(table, bias, graph, relu=False):
    """table [R, N, d_out] -> [N, d_out]; relu: the activation the models apply right after the layer, in the kernel's epilogue"""
    return _FeaturelessMP.apply(table, bias, graph, relu)


# the _native wrappers of the scored-triples roles per (decoder, bf16 entity table): (score, all-in-one CSR walk or None, relation and bias
# gradients, entity gradients).  NAMES, looked up on the module at every call.  The ComplEx wrappers pick the storage themselves.
_TRIPLE_ROLES = {("distmult", False): ("distmult_fwd", "distmult_bwd_all", "distmult_bwd_rel", "distmult_bwd_nodes"),
                 ("distmult", True): ("distmult_fwd_bf16", "distmult_bwd_all_bf16", "distmult_bwd_rel_bf16", "distmult_bwd_nodes_bf16"),
                 ("complex", False): ("complex_fwd", None, "complex_bwd_rel", "complex_bwd_nodes"),
                 ("complex", True): ("complex_fwd", None, "complex_bwd_rel", "complex_bwd_nodes")}


class _TripleScore(torch.autograd.Function):
    """DistMult or ComplEx scores of triples on an fp32 or a bf16 entity table.  On a bf16 table the
    relations and biases arrive as fp32 (distmult_score / complex_score widened bf16 parameters); scores are fp32, dnodes has the table's
    dtype -- bf16: an fp32 sum per entity rounded once --, the parameter gradients are fp32.

    The backward walks the scored triples as two CSRs, whose counting pass rides on the scoring kernel when something needs a gradient and
    there are triples.  DistMult, by the route switch distmult_bwd: csr = every gradient from the CSR walks (fp32: two, bf16: ONE) where the
    relation table fits the LDS (WN18: 18 x 200; no predicate sort), else as split; split = the entity gradients from the CSRs, one wave
    per entity and no atomics, + the predicate-sorted kernel for relations and biases; atomic (RGCN_DISTMULT_BWD=atomic) = the
    predicate-sorted kernel also scatters the entity gradients with fp32 atomics and the scoring kernel counts nothing -- on a bf16 table
    CORRECTNESS ONLY: bf16 is never accumulated with atomics, so the fp32 scatter kernel runs on the widened table and its dnodes is rounded
    once.  ComplEx has ONE route, DistMult's split: no LDS-table and no atomic-scatter twin, the switch is ignored, `atomic` included.

    No ranks were counted = DistMult's atomic route, or no triples at all: then DistMult takes the scatter call (of no triples: its zero
    fills) and ComplEx the relation kernel's zero fills beside a zero dnodes."""

    @staticmethod
    def forward(ctx, decoder, triples, nodes, relations, sbias, pbias, obias):
        shape = triples.shape[:-1]
        tr = triples.reshape(-1, 3).contiguous()
        nodes = dense(nodes)
        relations = dense(relations)
        ctx.roles = _TRIPLE_ROLES[decoder, nodes.dtype == torch.bfloat16]
        walks = decoder == "complex" or routes.get("distmult_bwd", "csr") != "atomic"
        count = bool(any(ctx.needs_input_grad[2:]) and tr.shape[0] and walks)
        out = getattr(_native, ctx.roles[0])(tr, nodes, relations, sbias, pbias, obias, ranks=count)
        scores, ctx.ranks = out if count else (out, None)
        ctx.save_for_backward(tr, nodes, relations)
        ctx.scatter = decoder == "distmult" and not count
        ctx.with_bias = sbias is not None
        return scores.view(shape)

    @staticmethod
    def backward(ctx, gs):
        tr, nodes, relations = ctx.saved_tensors
        gs = dense(gs.reshape(-1).float())
        _, bwd_all, bwd_rel, bwd_nodes = ctx.roles
        if (bwd_all and not ctx.scatter and routes.get("distmult_bwd", "csr") != "split"
                and _native.distmult_bwd_all_supported(relations.shape[0], nodes.shape[1])):
            return (None, None) + getattr(_native, bwd_all)(tr, ctx.ranks, nodes, relations, gs, ctx.with_bias)
        order = torch.argsort(tr[:, 1], stable=True)   # predicate runs -> relation gradient accumulates in registers
        tr_p, gs_p = tr[order].contiguous(), gs[order].contiguous()
        if ctx.scatter:
            dn, dr, dsb, dpb, dob = _native.distmult_bwd(tr_p, nodes.float(), relations, gs_p, ctx.with_bias, nodes_grad=True)
            return None, None, dn.to(nodes.dtype), dr, dsb, dpb, dob
        dr, dsb, dpb, dob = getattr(_native, bwd_rel)(tr_p, nodes, relations, gs_p, ctx.with_bias)
        dn = torch.zeros_like(nodes) if ctx.ranks is None else getattr(_native, bwd_nodes)(tr, ctx.ranks, nodes, relations, gs)
        return None, None, dn, dr, dsb, dpb, dob


def _check_decoder(decoder, nodes):
    """the `decoder=` rule of the public functions, before anything touches a device: "distmult" or "complex" (an even width) -- ValueError"""
    _native.check_decoder(decoder, nodes.shape[-1])


def _complex_mul(x, y, conj_y=False):
    """x y, or x conj(y), of rows of complex features stored as real halves | imaginary halves; every element two rounded products and
    one rounded add or subtract, as the query kernels form them"""
    h = x.shape[-1] // 2
    x_re, x_im, y_re, y_im = x[..., :h], x[..., h:], y[..., :h], y[..., h:]
    if conj_y:
        return torch.cat((x_re * y_re + x_im * y_im, x_im * y_re - x_re * y_im), -1)
    return torch.cat((x_re * y_re - x_im * y_im, x_re * y_im + x_im * y_re), -1)


def _query_vectors(nodes, rel, anchor, p, head, decoder):
    """qv [Q, d] fp32, the query vectors as the query kernel of the decoder forms them, bit for bit (.float(): bf16 rows): DistMult
    nodes[anchor] * rel[p]; ComplEx [Re z | Im z] with z = a r for tail queries and z = conj(r) a for head queries"""
    a, r = nodes[anchor].float(), rel[p]
    if decoder == "distmult":
        return a * r
    if not head:
        return _complex_mul(a, r)
    h = a.shape[1] // 2                                # conj(r) a, the terms in the kernel's order
    a_re, a_im, r_re, r_im = a[:, :h], a[:, h:], r[:, :h], r[:, h:]
    return torch.cat((r_re * a_re + r_im * a_im, r_re * a_im - r_im * a_re), 1)


def _query_vectors_grad(dqv, other, head, decoder, wrt):
    """the chain rule of _query_vectors: the gradient rows [Q, d] with respect to the anchor rows (wrt="anchor", other = rel[p]) or to the
    relation rows (wrt="relation", other = nodes[anchor].float()) from g = dqv.  DistMult: g * other.  ComplEx, g read as a complex
    number: tail da = g conj(r), dr = g conj(a); head da = r g, dr = a conj(g)."""
    if decoder == "distmult":
        return dqv * other
    if not head:
        return _complex_mul(dqv, other, conj_y=True)
    return _complex_mul(other, dqv) if wrt == "anchor" else _complex_mul(other, dqv, conj_y=True)


def _widen_query_params(nodes, relations, sbias, pbias, obias):
    """-> (relations, sbias, pbias, obias) as the native DistMult calls take them.  fp32 nodes: as they are.  bf16 nodes:
    each fp32 or bf16, else TypeError; bf16 ones widened to fp32, once per call (.float() is a no-op on fp32; they are small)"""
    if nodes.dtype != torch.bfloat16:
        return relations, sbias, pbias, obias
    for name, t in (("relations", relations), ("sbias", sbias), ("pbias", pbias), ("obias", obias)):
        if t is not None and t.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"{name} must be torch.float32 or torch.bfloat16, got {t.dtype}")
    return tuple(None if t is None else t.float() for t in (relations, sbias, pbias, obias))


def distmult_score(triples, nodes, relations, sbias=None, pbias=None, obias=None):
    """DistMult scores of `triples` [..., 3].  fp32 nodes: everything fp32.  bf16 nodes: relations and biases fp32 or bf16
    -- bf16 parameters are widened here, once per call, and autograd carries the cast back --, scores fp32, dnodes bf16."""
    return _TripleScore.apply("distmult", triples, nodes, *_widen_query_params(nodes, relations, sbias, pbias, obias))


def complex_score(triples, nodes, relations, sbias=None, pbias=None, obias=None):
    """ComplEx scores of `triples` [..., 3] (Trouillon et al. 2016; an extension): nodes [N, d] and relations [R, d], d even
    (else ValueError), hold d / 2 complex features per row, real halves in columns [0, d / 2), imaginary halves behind them, and
        score(s, p, o) = Re sum_k e_s[k] r_p[k] conj(e_o[k])  (+ sbias[s] + pbias[p] + obias[o], all three or none)
    -- not symmetric in s and o.  Dtypes as in distmult_score: fp32 nodes, or bf16 nodes with fp32 or bf16 relations and biases (widened
    here), fp32 scores, dnodes in the table's dtype.  The backward always runs the CSR walk for the entities and the predicate-sorted kernel
    for relations and biases (DistMult's "split" route); the route switch distmult_bwd has no effect on it."""
    _check_decoder("complex", nodes)
    return _TripleScore.apply("complex", triples, nodes, *_widen_query_params(nodes, relations, sbias, pbias, obias))


def distmult_score_all(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, out=None, decoder="distmult"):
    """fp32 scores [Q, N] of every entity as the head (head=True) or the tail of each triple of `batch` (int64 [Q, 3] on the device), no
    autograd: the ranking evaluator's product (utils/misc.py:71-88).  fp32 nodes run the fp32 matrix instructions; bf16 nodes (DESIGN.md
    4.6) the bf16 ones on the bf16 table, with relations and biases fp32 or bf16 (widened here) -- same sums, another order.
    decoder (here and in every all-candidate function below): "distmult", or "complex" for the ComplEx scores of complex_score on the
    same kernels -- only the query vectors differ; an even width, and any other value is a ValueError."""
    _check_decoder(decoder, nodes)
    score_all = _native.distmult_score_all_bf16 if nodes.dtype == torch.bfloat16 else _native.distmult_score_all
    return score_all(batch, head, nodes, *_widen_query_params(nodes, relations, sbias, pbias, obias), out=out, decoder=decoder)


class FilterIndex:
    """The known completions of every query key, resident on the device: what the filtered routes take as `filt=` in place
    of the per-batch int32 lists (filt_q, filt_n).  true_triples: the pair utils.misc.generate_true_dict returns -- (p, o) -> known heads
    and (s, p) -> known tails.  Per direction (tables[0]: heads, tables[1]: tails) three device tensors
        keys int64 [K]      strictly ascending, key = p * num_nodes + o (heads) or p * num_nodes + s (tails),
        ptr  int64 [K + 1],
        vals int32 [ptr[K]] the completions of key k in vals[ptr[k]:ptr[k + 1]], ascending and deduplicated,
    from which a kernel fills a query batch's filter mask (one binary search per query) -- no host pass, no upload and no length F per
    call, so a filtered step has static shapes and can be captured.  Everything is validated HERE, once, on the host (`host_tables`, which
    needs no GPU): an entity outside [0, num_nodes) or a negative relation raises IndexError, and no call checks the index again.  An
    empty dictionary gives K = 0, an index that filters nothing.  The tensors never require grad; one index serves any number of calls."""

    def __init__(self, true_triples, num_nodes, device):
        self.num_nodes = int(num_nodes)
        self.tables = [tuple(torch.from_numpy(a).to(device) for a in t) for t in self.host_tables(true_triples, num_nodes)]
        self.device = self.tables[0][0].device

    @staticmethod
    def host_tables(true_triples, num_nodes):
        """-> [(keys, ptr, vals) of the heads, (keys, ptr, vals) of the tails] as numpy arrays (int64, int64, int32): the numpy stage"""
        n = int(num_nodes)
        if n < 1:
            raise IndexError("a FilterIndex needs num_nodes >= 1")
        out = []
        for table, rel_at, ent_at in ((true_triples[0], 0, 1), (true_triples[1], 1, 0)):      # heads: (p, o) -> [s]; tails: (s, p) -> [o]
            lens = np.fromiter((len(v) for v in table.values()), np.int64, len(table))
            total = int(lens.sum())
            rel = np.repeat(np.fromiter((k[rel_at] for k in table), np.int64, len(table)), lens)
            ent = np.repeat(np.fromiter((k[ent_at] for k in table), np.int64, len(table)), lens)
            comp = np.fromiter((x for v in table.values() for x in v), np.int64, total)
            if total and (rel.min() < 0 or ent.min() < 0 or ent.max() >= n or comp.min() < 0 or comp.max() >= n):
                raise IndexError(f"true triples: an entity outside [0, {n}) or a negative relation")
            if total and int(rel.max()) > (np.iinfo(np.int64).max - n) // n:
                raise IndexError("true triples: relation * num_nodes does not fit 64 bits")
            key = rel * n + ent
            order = np.lexsort((comp, key))
            key, comp = key[order], comp[order]
            first = np.ones(total, bool)
            first[1:] = (key[1:] != key[:-1]) | (comp[1:] != comp[:-1])           # a duplicate triple is one completion
            key, comp = key[first], comp[first]
            keys, counts = np.unique(key, return_counts=True)
            ptr = np.zeros(len(keys) + 1, np.int64)
            np.cumsum(counts, out=ptr[1:])
            out.append((keys.astype(np.int64), ptr, comp.astype(np.int32)))
        return out


def _filter_args(filt, filt_q, filt_n, nodes, name="filt", lists="filt_q / filt_n"):
    """the argument rules of `filt=` (and of `labels=`, under its own names): a FilterIndex or the lists, built for this entity table,
    on its device"""
    if filt is None:
        return
    if not isinstance(filt, FilterIndex):
        raise TypeError(f"{name} must be a FilterIndex, got {type(filt).__name__}")
    if filt_q is not None or filt_n is not None:
        raise ValueError(f"{name} (a FilterIndex) and {lists} (the lists) are mutually exclusive")
    if filt.device != nodes.device:
        raise ValueError(f"the FilterIndex is on {filt.device}, the entity table on {nodes.device}")
    if filt.num_nodes != nodes.shape[0]:
        raise ValueError(f"the FilterIndex was built for {filt.num_nodes} entities, the entity table has {nodes.shape[0]}")


def distmult_rank_all(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, filt_q=None, filt_n=None, strips=0, filt=None,
                      decoder="distmult"):
    """(greater, ties, tscore) [Q]: for each triple of `batch` the number of entities that score above its target as the head (head=True)
    or the tail, the number that score the same (the target included) and the target's score -- the counts `_native.rank_count` takes from
    the score matrix of distmult_score_all after `_native.rank_filter` on the int32 device lists (filt_q, filt_n), without that matrix
    (utils/misc.py:40-58, 71-99).  No autograd.  fp32 or bf16 nodes; with bf16 nodes relations and biases are fp32 or bf16
    (widened here), as in distmult_score_all.  filt: a FilterIndex in place of the lists (not both: ValueError) -- the same counts."""
    _check_decoder(decoder, nodes)
    _filter_args(filt, filt_q, filt_n, nodes)
    relations, sbias, pbias, obias = _widen_query_params(nodes, relations, sbias, pbias, obias)
    return _native.distmult_rank_fused(batch, head, nodes, relations, sbias, pbias, obias, filt_q, filt_n, strips, filt=filt, decoder=decoder)


def distmult_topk_all(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, k=10, filt_q=None, filt_n=None, strips=0):
    """(ids int64 [Q, k], scores fp32 [Q, k]): for each triple of `batch` the k entities that score best as its head (head=True) or its
    tail -- the rows of distmult_score_all after `_native.rank_filter` on the int32 device lists (filt_q, filt_n), sorted by score
    descending and id ascending and cut at k, without that matrix.  The predicted column of `batch` is ignored and every
    listed cell is excluded; rows with fewer than k candidates end in id -1, score -inf.  No autograd.  k <= _native.TOPK_MAX.  fp32 or
    bf16 nodes; with bf16 nodes relations and biases are fp32 or bf16 (widened here), as in distmult_rank_all.  With a FilterIndex in
    place of the lists: distmult_topk_all_index; over ComplEx scores: complex_topk_all (this function's parameter list is the one its
    callers know; it stays)."""
    return _topk_all(batch, head, nodes, relations, sbias, pbias, obias, k, filt_q, filt_n, strips, None, "distmult")


def complex_topk_all(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, k=10, filt_q=None, filt_n=None, strips=0):
    """distmult_topk_all over ComplEx scores (complex_score): the same kernels on ComplEx query vectors, the same
    parameter list (that one is fixed, so the decoder cannot be a keyword of it).  An odd width is a ValueError.  With a FilterIndex:
    distmult_topk_all_index(..., decoder="complex")."""
    _check_decoder("complex", nodes)
    return _topk_all(batch, head, nodes, relations, sbias, pbias, obias, k, filt_q, filt_n, strips, None, "complex")


def distmult_topk_all_index(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, k=10, filt=None, strips=0, decoder="distmult"):
    """distmult_topk_all with `filt`, a FilterIndex, in place of the lists: every known completion of a query is excluded -- the same
    rows, bit for bit, with no list built on the host.  The index must be on the tensors' device and built for nodes.shape[0] entities
    (ValueError)."""
    _check_decoder(decoder, nodes)
    if filt is None:
        raise ValueError("distmult_topk_all_index needs a FilterIndex (distmult_topk_all takes lists or no filter)")
    _filter_args(filt, None, None, nodes)
    return _topk_all(batch, head, nodes, relations, sbias, pbias, obias, k, None, None, strips, filt, decoder)


def _topk_all(batch, head, nodes, relations, sbias, pbias, obias, k, filt_q, filt_n, strips, filt, decoder):
    relations, sbias, pbias, obias = _widen_query_params(nodes, relations, sbias, pbias, obias)
    if filt is not None:
        return _native.distmult_topk_index(batch, head, nodes, relations, sbias, pbias, obias, k, filt, strips, decoder=decoder)
    if decoder == "distmult":
        return _native.distmult_topk(batch, head, nodes, relations, sbias, pbias, obias, k, filt_q, filt_n, strips)
    # (_native.distmult_topk keeps its parameter list: the list form of another decoder goes to what it wraps)
    return _native._distmult_topk(batch, head, nodes, relations, sbias, pbias, obias, k, filt_q, filt_n, strips, None, decoder)


_UNIT = {}


def unit_gradient(device):
    """the constant 1.0 to start a backward pass with -- `loss.backward(gradient=unit_gradient(loss.device))` -- instead of the ones_like()
    autograd fills per call; MaskedCrossEntropy's backward recognises it and skips the multiplication by it (two launches per step of a
    launch-bound graph).  Never written to."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _UNIT:
        _UNIT[device] = torch.ones((), device=device)
    return _UNIT[device]


def _is_unit(g):
    u = _UNIT.get(g.device)
    return u is not None and g.dim() == 0 and g.data_ptr() == u.data_ptr() and u._version == 0


def _rows16(t):
    """t = the first columns of a contiguous [N, 16 k] buffer (what a layer of fewer than 16 k outputs returns, see _RelationalMP.forward)?"""
    return t.dim() == 2 and t.stride(1) == 1 and t.stride(0) % 16 == 0 and t.stride(0) > t.shape[1] and t.storage_offset() == 0 and \
        t.data_ptr() % 16 == 0


SOFTMAX_CHUNK_BYTES = 1 << 30      # the backward's dS buffer per chunk of candidate columns: utils.misc._SCORE_BYTES, the evaluator's budget


def softmax_chunk_plan(Q, N, chunk_bytes):
    """[(c_first, c_count), ...]: the candidate columns [0, N) cut into the chunks of the 1-N softmax loss's backward.  Every c_first is
    a multiple of 128 (the tile and mask-word alignment of the gradient-cell kernel), every chunk but the last a multiple of 128 wide with
    Q * c_count * 4 <= chunk_bytes -- but never narrower than one tile column of 128 --, the last one ragged; one chunk when the whole
    [Q, N] matrix fits the budget."""
    assert Q >= 0 and N >= 1 and chunk_bytes >= 1
    if 4 * Q * N <= chunk_bytes:
        return [(0, N)]
    per = max(128, chunk_bytes // (4 * Q) // 128 * 128)
    return [(c, min(per, N - c)) for c in range(0, N, per)]


class _DistMultSoftmaxLoss(torch.autograd.Function):
    """loss[q] = log sum_{n allowed} exp(s[q, n]) - s[q, target_q] on an fp32 or a bf16 table (relations and biases fp32).  Saves lse [Q]
    and the inputs; the backward recomputes the product chunk by chunk (softmax_chunk_plan) into one reused [Q, c_count] buffer.  A bf16
    table is saved as it is and never widened as a whole: the gradient cells come from the bf16 kernel, the two contractions stay fp32
    (the chunk's rows are widened into one reused buffer), dnodes is summed in fp32 and rounded to bf16 once at the end.  filt: a
    FilterIndex in place of the lists; it is not a tensor input and is kept by reference on ctx (never written, needs no grad), so the
    head and the tail loss of a step share one index.
    smoothing = eps > 0 (label smoothing over the allowed candidates): loss[q] = lse - (1 - eps) s[q, target_q] - (eps / n_q) sum_allowed s,
    from the smoothed strip pass (lse, tscore, ssum, cnt) composed here with torch ops on the device; keep = 1 - eps [1] and
    uni = eps / cnt [Q] are saved as device floats and the backward's cells subtract them -- same chunk plan, same contractions."""

    @staticmethod
    def forward(ctx, batch, head, nodes, relations, sbias, pbias, obias, filt_q, filt_n, mean, strips, chunk_bytes, filt=None, smoothing=0.0,
                decoder="distmult"):
        batch = batch.reshape(-1, 3).contiguous()
        nodes, relations = dense(nodes), dense(relations)
        ctx.decoder = decoder
        # range-checked here, once, for the forward and the backward (under deferred checks: clamped, the error queued)
        batch = _native.checked_queries(batch, nodes.shape[0], relations.shape[0], filt_q, filt_n, nodes.dtype == torch.bfloat16)
        # (with a FilterIndex there are no lists: checked_queries takes its unfiltered path -- no read-back under deferred checks)
        ctx.head, ctx.mean, ctx.chunk_bytes, ctx.filt = bool(head), mean, chunk_bytes, filt
        if smoothing:
            lse, tscore, ssum, cnt = _native.distmult_lse_smooth(batch, head, nodes, relations, sbias, pbias, obias, filt_q, filt_n, strips,
                                                                 checked=True, filt=filt, decoder=decoder)
            keep = torch.full((1,), 1.0 - smoothing, device=lse.device, dtype=torch.float32)
            uni = smoothing / cnt.to(torch.float32)                           # cnt >= 1: the target is always allowed
            ctx.save_for_backward(batch, nodes, relations, sbias, pbias, obias, filt_q, filt_n, lse, keep, uni)
            loss = lse - keep * tscore - uni * ssum
            return loss.mean() if mean else loss
        lse, tscore = _native.distmult_lse(batch, head, nodes, relations, sbias, pbias, obias, filt_q, filt_n, strips, checked=True, filt=filt,
                                           decoder=decoder)
        ctx.save_for_backward(batch, nodes, relations, sbias, pbias, obias, filt_q, filt_n, lse)
        loss = lse - tscore
        return loss.mean() if mean else loss

    @staticmethod
    def backward(ctx, g):
        batch, nodes, rel, sbias, pbias, obias, filt_q, filt_n, lse, *smooth = ctx.saved_tensors
        keep, uni = smooth if smooth else (None, None)

        def cells(g, c_first, c_count, buf):
            return _native.distmult_softmax_grad(batch, ctx.head, nodes, rel, sbias, pbias, obias, filt_q, filt_n, lse, g,
                                                 batch.shape[0] if ctx.mean else 1, c_first, c_count, out=buf, filt=ctx.filt, keep=keep, uni=uni,
                                                 decoder=ctx.decoder)
        # sum_n dS[q, n] = 0: the query-side bias gradients are zeros
        grads = _all_candidate_backward(ctx, g, batch, nodes, rel, sbias, pbias, obias, cells, query_bias=False)
        return (None, None) + grads + (None,) * 8


def _all_candidate_backward(ctx, g, batch, nodes, rel, sbias, pbias, obias, cells, query_bias):
    """-> (dnodes, drel, dsbias, dpbias, dobias) of a loss over all candidates of every query of `batch`, from its gradient cells: the
    chunk loop the 1-N softmax loss and the 1-N BCE loss share.  cells(g, c_first, c_count, buf) -> dS fp32 [Q, c_count], the cells of
    the candidate columns [c_first, c_first + c_count) written into `buf`; ctx: head, decoder, chunk_bytes and needs_input_grad (inputs 2..6 are
    nodes, relations and the three biases).  query_bias: the rows of dS do not sum to zero, so the query-side bias gradients are real --
    dS times a column of ones per chunk, the chunks added in chunk order, then index_add_ into pbias[p] and into obias[anchor] (head) or
    sbias[anchor] (tail); without it they are zeros."""
    need_n, need_r = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
    need_b = sbias is not None and any(ctx.needs_input_grad[4:7])
    Q, (N, d), dev = batch.shape[0], nodes.shape, nodes.device
    dn = dr = dsb = dpb = dob = None
    if Q and (need_n or need_r or need_b):
        if not _is_unit(g):
            g = dense(g.to(torch.float32))
        anchor, p = batch[:, 2 if ctx.head else 0], batch[:, 1]
        bf16 = nodes.dtype == torch.bfloat16
        qv = _query_vectors(nodes, rel, anchor, p, ctx.head, ctx.decoder)  # as the query kernel forms them
        plan = softmax_chunk_plan(Q, N, ctx.chunk_bytes)
        # bf16 table: the rows of a chunk widened for the query-side product, one buffer for every chunk (the first chunk is the widest)
        wide = torch.empty(plan[0][1], d, device=dev, dtype=torch.float32) if bf16 and (need_n or need_r) else None
        buf = torch.empty(Q * plan[0][1], device=dev, dtype=torch.float32)
        dn = torch.empty(N, d, device=dev, dtype=torch.float32) if need_n else None
        # the candidate-side bias gradient is dS^T times a column of ones: a product of its own into its own [N, 1] column (beside qv
        # it would make the rows of dnodes d + 1 wide and cost a second [N, d] copy to take them apart)
        ones = torch.ones(Q, 1, device=dev) if need_b else None
        cand = torch.empty(N, 1, device=dev, dtype=torch.float32) if need_b else None
        ones_c = torch.ones(plan[0][1], 1, device=dev) if need_b and query_bias else None
        dqv = dqb = None
        for c_first, c_count in plan:
            dS = cells(g, c_first, c_count, buf)
            # both products are skinny (d wide): K is cut into slices, summed in a fixed order, where the output tiles alone would
            # leave most of the chip idle
            if dn is not None:                                            # candidate side: every row written once, nothing accumulated
                _native.gemm(dS, qv, trans_a=True, split_k=_split_k(Q, c_count, d), out=dn[c_first:c_first + c_count])
            if cand is not None:
                _native.gemm(dS, ones, trans_a=True, split_k=_split_k(Q, c_count, 1), out=cand[c_first:c_first + c_count])
            if ones_c is not None:                                        # query-side biases: the rows' sums, added in chunk order
                part = _native.gemm(dS, ones_c[:c_count], split_k=_split_k(c_count, Q, 1))
                dqb = part if dqb is None else dqb.add_(part)
            if need_n or need_r:                                          # query side: the chunks' partials added in chunk order
                rows = nodes[c_first:c_first + c_count]
                if wide is not None:
                    rows = wide[:c_count].copy_(rows)
                part = _native.gemm(dS, rows, split_k=_split_k(c_count, Q, d))
                dqv = part if dqv is None else dqv.add_(part)
        if need_n:
            dn.index_add_(0, anchor, _query_vectors_grad(dqv, rel[p], ctx.head, ctx.decoder, "anchor"))
            if bf16:
                dn = dn.to(torch.bfloat16)                                # fp32 sums, one rounding
        if need_r:
            dr = torch.zeros_like(rel).index_add_(0, p, _query_vectors_grad(dqv, nodes[anchor].float(), ctx.head, ctx.decoder, "relation"))
        if need_b:
            cand = cand.view(N)
            zeros = torch.zeros(N, device=dev)
            dpb = torch.zeros_like(pbias)
            if dqb is not None:
                dqb = dqb.view(Q)
                zeros.index_add_(0, anchor, dqb)
                dpb.index_add_(0, p, dqb)
            dsb, dob = (cand, zeros) if ctx.head else (zeros, cand)
    else:
        dn = torch.zeros_like(nodes) if need_n else None
        dr = torch.zeros_like(rel) if need_r else None
        if need_b:
            dsb, dpb, dob = torch.zeros_like(sbias), torch.zeros_like(pbias), torch.zeros_like(obias)
    return dn, dr, dsb, dpb, dob


def _loss_args(label_smoothing, reduction, bf16_backward, chunk_bytes):
    """the keyword rules the all-candidate losses share, checked before anything touches a device -> chunk_bytes (None: the default)"""
    if isinstance(label_smoothing, bool) or not isinstance(label_smoothing, numbers.Real) or not 0.0 <= label_smoothing < 1.0:
        raise ValueError(f"label_smoothing must be a real number in [0, 1), got {label_smoothing!r}")
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be 'mean' or 'none', got {reduction!r}")
    if bf16_backward not in ("upcast", "native"):
        raise ValueError(f"bf16_backward must be 'upcast' or 'native', got {bf16_backward!r}")
    if chunk_bytes is None:
        chunk_bytes = SOFTMAX_CHUNK_BYTES
    assert isinstance(chunk_bytes, int) and chunk_bytes >= 1, "chunk_bytes must be a positive int"
    return chunk_bytes


def _loss_params(nodes, relations, sbias, pbias, obias, bf16_backward):
    """-> (nodes, relations, sbias, pbias, obias) as the all-candidate losses' autograd functions take them: relations and biases widened
    for a bf16 table (_widen_query_params), and the table itself widened when it trains on the "upcast" route"""
    params = (nodes, relations, sbias, pbias, obias)
    relations, sbias, pbias, obias = _widen_query_params(nodes, relations, sbias, pbias, obias)
    if nodes.dtype == torch.bfloat16 and bf16_backward == "upcast" and torch.is_grad_enabled() and \
            any(t is not None and t.requires_grad for t in params):
        nodes = nodes.float()
    return nodes, relations, sbias, pbias, obias


def distmult_softmax_loss(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, filt_q=None, filt_n=None,
                          reduction="mean", strips=0, chunk_bytes=None, filt=None, bf16_backward="upcast", label_smoothing=0.0,
                          decoder="distmult"):
    """1-N softmax cross-entropy of DistMult (an extension: the reference trains on sampled negatives only).  For each triple of `batch`
    (int64 [Q, 3]) every entity is scored as its head (head=True) or its tail -- the cells s[q, n] of distmult_score_all -- and
        loss[q] = log sum_{n allowed} exp(s[q, n]) - s[q, target_q],
    `allowed` being every entity that is not on the int32 device lists (filt_q, filt_n); an entry on a query's own target is ignored (as in
    distmult_rank_all), so the target is always in the sum.  Returns the mean over the queries, or the vector with reduction="none".
    filt: a FilterIndex in place of the lists (not both: ValueError) -- the same loss and gradients, bit for bit, with nothing built on
    the host and nothing read back: under route deferred_checks = 1 the filtered step does not synchronise and can be captured.
    The [Q, N] logits never exist: the forward is one strip pass with a running (max, sum) per query and keeps lse [Q];
    the backward computes the product again in chunks of candidate columns (softmax_chunk_plan: Q * c_count * 4 <= chunk_bytes, default
    SOFTMAX_CHUNK_BYTES) into one reused buffer dS and contracts each chunk on the matrix cores -- dnodes[chunk] = dS^T qv, every row
    written once, and dqv += dS nodes[chunk], the chunks added in chunk order.  The one unordered sum of the route comes last:
    dnodes[anchor_q] += dqv[q] * rel[p_q] and drel[p_q] += dqv[q] * nodes[anchor_q] are index_add_ (fp32 atomics over Q rows), so two
    runs may differ in the last bits of those rows.  The query-side bias gradients (pbias, and obias if head else sbias) are
    sum_n dS[q, n] = 0 in exact arithmetic and are returned as zeros.  strips: as in distmult_rank_all.
    bf16 nodes: with nothing that requires grad the bf16 kernels run on the bf16 table -- a test-set cross-entropy.
    When something requires grad, bf16_backward chooses the route.  "upcast" (the default): the table is widened to fp32 here, the fp32
    route runs and autograd rounds dnodes once on the way back -- an fp32 copy of the whole table lives from the forward to the backward.
    "native": the table is never widened.  The forward is the bf16 strip kernel and saves the bf16 table itself; the backward takes the
    gradient cells of each chunk from the bf16 kernel (the product on the bf16 matrix instructions, from the three bf16 terms of the fp32
    query vector nodes[anchor].float() * rel[p]), contracts them in fp32 as above -- only the chunk's rows of the table are widened, into
    one reused [c_count, d] buffer --, accumulates dnodes in fp32, the anchor rows' index_add_ included, and rounds it to bf16 once.
    drel and the bias gradients are fp32.  With fp32 nodes the keyword has no effect.  Relations and biases are fp32, or bf16 with bf16
    nodes (widened here: they are small).
    label_smoothing = eps, a real number in [0, 1) (else ValueError): the target distribution is 1 - eps on the target plus eps spread
    evenly over the n_q ALLOWED candidates of the query (filtered entities are out of the problem and get no mass),
        loss[q] = lse[q] - (1 - eps) s[q, target_q] - (eps / n_q) sum_{n allowed} s[q, n],
    which without a filter is torch.nn.functional.cross_entropy(logits, target, label_smoothing=eps).  The strip pass carries the sum and
    the count of the allowed scores beside (max, sum exp) -- lse and the target score keep their bits --, the loss is composed from the
    four [Q] vectors on the device, and the gradient cells become scale_q (exp(s - lse) - (1 - eps) [n == target_q] - eps / n_q): their
    row sums are still 0, so the query-side bias gradients stay zeros.  Nothing is read back; bf16 tables go the routes above.  0 takes
    the unsmoothed path, call for call.
    decoder="complex": the same loss over ComplEx scores (complex_score) -- the strip pass and the gradient cells are the
    same kernels on ComplEx query vectors, and the last step of the backward applies their chain rule (tail queries: da = g conj(r),
    dr = g conj(a); head queries: da = r g, dr = a conj(g), g = dqv read as complex) in place of the two element-wise products."""
    _check_decoder(decoder, nodes)
    chunk_bytes = _loss_args(label_smoothing, reduction, bf16_backward, chunk_bytes)
    _filter_args(filt, filt_q, filt_n, nodes)
    nodes, relations, sbias, pbias, obias = _loss_params(nodes, relations, sbias, pbias, obias, bf16_backward)
    return _DistMultSoftmaxLoss.apply(batch, head, nodes, relations, sbias, pbias, obias, filt_q, filt_n, reduction == "mean", strips,
                                      chunk_bytes, filt, float(label_smoothing), decoder)


class _DistMultBCELoss(torch.autograd.Function):
    """loss[q] = (1 / N) sum_n (softplus(s[q, n]) - y'[q, n] s[q, n]), y' = (1 - eps) y + eps / N, on an fp32 or a bf16 table (relations
    and biases fp32): composed from the strip pass's (sp, ps) and, with eps > 0, the sum of a row's scores, which needs no kernel --
    AS[q] = qv[q] . colsum(nodes) + the bias terms.  Saves the inputs alone; the backward is the chunk loop of the 1-N softmax loss
    (_all_candidate_backward) on this loss's gradient cells, with the query-side bias gradients it owes.  labels: a FilterIndex in place
    of the lists, kept by reference on ctx as _DistMultSoftmaxLoss keeps its filter."""

    @staticmethod
    def forward(ctx, batch, head, nodes, relations, sbias, pbias, obias, lab_q, lab_n, mean, strips, chunk_bytes, labels=None, smoothing=0.0,
                decoder="distmult"):
        batch = batch.reshape(-1, 3).contiguous()
        nodes, relations = dense(nodes), dense(relations)
        ctx.decoder = decoder
        N = nodes.shape[0]
        batch = _native.checked_queries(batch, N, relations.shape[0], lab_q, lab_n, nodes.dtype == torch.bfloat16)
        ctx.head, ctx.mean, ctx.chunk_bytes, ctx.labels, ctx.smoothing = bool(head), mean, chunk_bytes, labels, smoothing
        sp, ps, _ = _native.distmult_bce_sums(batch, head, nodes, relations, sbias, pbias, obias, lab_q, lab_n, strips, checked=True, labels=labels,
                                              decoder=decoder)
        ctx.save_for_backward(batch, nodes, relations, sbias, pbias, obias, lab_q, lab_n)
        if smoothing:
            anchor, p = batch[:, 2 if head else 0], batch[:, 1]
            rows = _query_vectors(nodes, relations, anchor, p, head, decoder) @ nodes.sum(0, dtype=torch.float32)     # (the bf16 table is never widened)
            if sbias is not None:
                cbias, abias = (sbias, obias) if head else (obias, sbias)
                rows = rows + (cbias.sum() + N * (pbias[p] + abias[anchor]))
            loss = (sp - (1.0 - smoothing) * ps - (smoothing / N) * rows) / N
        else:
            loss = (sp - ps) / N
        return loss.mean() if mean else loss

    @staticmethod
    def backward(ctx, g):
        batch, nodes, rel, sbias, pbias, obias, lab_q, lab_n = ctx.saved_tensors

        def cells(g, c_first, c_count, buf):
            return _native.distmult_bce_grad(batch, ctx.head, nodes, rel, sbias, pbias, obias, lab_q, lab_n, g, batch.shape[0] if ctx.mean else 1,
                                             c_first, c_count, out=buf, labels=ctx.labels, label_smoothing=ctx.smoothing, decoder=ctx.decoder)
        grads = _all_candidate_backward(ctx, g, batch, nodes, rel, sbias, pbias, obias, cells, query_bias=True)
        return (None, None) + grads + (None,) * 8


def distmult_bce_loss(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, lab_q=None, lab_n=None, labels=None,
                      reduction="mean", strips=0, chunk_bytes=None, bf16_backward="upcast", label_smoothing=0.0):
    """1-N multi-label binary cross-entropy of DistMult ("K-vs-All", the objective ConvE introduced; an extension: the reference's
    sampled-negative BCE is this loss on a sample of the cells).  For each triple of `batch` (int64 [Q, 3]) every entity is scored as its
    head (head=True) or its tail -- the cells s[q, n] of distmult_score_all -- against the label
        y[q, n] = 1 if n is the query's own target, or (q, n) is on the int32 device lists (lab_q, lab_n), or n is a known completion of
                  the query in `labels`, a FilterIndex (lists and index are mutually exclusive: ValueError); 0 otherwise,
        loss[q] = (1 / N) sum_n (softplus(s[q, n]) - y'[q, n] s[q, n]),        y' = (1 - eps) y + eps / N,    eps = label_smoothing,
    which is torch.nn.functional.binary_cross_entropy_with_logits(s, y') row by row; the mean over the queries (its default reduction),
    or the [Q] vector with reduction="none".  Without lists and index only the target is positive (1-vs-All).  Three rules differ from
    distmult_softmax_loss: a listed target STAYS a label (there it is dropped from the filter); nothing is filtered out -- every entity
    is in every query's sum and receives a gradient, and N in eps / N is the number of entities --; and the rows of the gradient cells
    do not sum to zero, so the query-side bias gradients (pbias, and obias if head else sbias) are real.
    The [Q, N] logits and labels never exist: the label matrix is the 1-bit-per-cell mask the routes above use as a filter, filled on
    the device, and the forward is one strip pass that carries sum softplus(s) and the sum of the positive scores per query (DESIGN.md
    4.5); with eps > 0 the sum of a row's scores is qv . colsum(nodes) plus the bias terms, no kernel.  The backward is
    distmult_softmax_loss's: the product again in chunks of candidate columns (softmax_chunk_plan, chunk_bytes) into one reused buffer of
    cells scale_q (sigmoid(s) - (1 - eps) y - eps / N), contracted on the matrix cores in the same order, the same index_add_ last; the
    query-side bias gradients are dS times a column of ones, the chunks added in chunk order.  Nothing is read back: range checks go
    through checked_queries, and under route deferred_checks = 1 the call does not synchronise and can be captured.
    bf16 nodes, bf16_backward ("upcast" / "native"), strips: as in distmult_softmax_loss.  label_smoothing: a real number in [0, 1).
    Over ComplEx scores: complex_bce_loss (this function's parameter list is fixed, so the decoder cannot be a keyword of it)."""
    return _bce_loss(batch, head, nodes, relations, sbias, pbias, obias, lab_q, lab_n, labels, reduction, strips, chunk_bytes, bf16_backward,
                     label_smoothing, "distmult")


def complex_bce_loss(batch, head, nodes, relations, sbias=None, pbias=None, obias=None, lab_q=None, lab_n=None, labels=None,
                     reduction="mean", strips=0, chunk_bytes=None, bf16_backward="upcast", label_smoothing=0.0):
    """distmult_bce_loss over ComplEx scores (complex_score), the same parameter list: the strip pass and the gradient
    cells are the same kernels on ComplEx query vectors, the smoothed row sum and the last step of the backward go through the query
    vectors' own form and chain rule, as in distmult_softmax_loss(..., decoder="complex").  An odd width is a ValueError."""
    _check_decoder("complex", nodes)
    return _bce_loss(batch, head, nodes, relations, sbias, pbias, obias, lab_q, lab_n, labels, reduction, strips, chunk_bytes, bf16_backward,
                     label_smoothing, "complex")


def _bce_loss(batch, head, nodes, relations, sbias, pbias, obias, lab_q, lab_n, labels, reduction, strips, chunk_bytes, bf16_backward,
              label_smoothing, decoder):
    chunk_bytes = _loss_args(label_smoothing, reduction, bf16_backward, chunk_bytes)
    _filter_args(labels, lab_q, lab_n, nodes, name="labels", lists="lab_q / lab_n")
    nodes, relations, sbias, pbias, obias = _loss_params(nodes, relations, sbias, pbias, obias, bf16_backward)
    return _DistMultBCELoss.apply(batch, head, nodes, relations, sbias, pbias, obias, lab_q, lab_n, reduction == "mean", strips, chunk_bytes,
                                  labels, float(label_smoothing), decoder)


class _MaskedCE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, row_label, lab_rows):
        logits = logits if _rows16(logits) else dense(logits)      # the padded rows are read in place
        loss, dl, dl_full = _native.ce_head(logits, row_label, lab_rows)
        ctx.save_for_backward(dl)
        ctx.dl_full = dl_full is not None
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dl, = ctx.saved_tensors
        if not _is_unit(g):
            return dl * g, None, None
        if ctx.dl_full:      # dl = the first columns of a zero-padded [N, 16] buffer: the layer's backward takes the buffer as it is
            dl._rgcn_zero_padded = True
        return dl, None, None


class _BCEWithLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scores, labels):
        loss, ds = _native.bce_head(dense(scores.reshape(-1)), dense(labels.reshape(-1).to(torch.float32)))
        ctx.save_for_backward(ds)
        ctx.shape = scores.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        ds, = ctx.saved_tensors
        return (ds if _is_unit(g) else ds * g).view(ctx.shape), None


def bce_with_logits(scores, labels):
    """`F.binary_cross_entropy_with_logits(scores, labels)` (mean reduction; reference experiments/predict_links.py:152-153) as ONE kernel for the
    loss and its gradient instead of ATen's ~13 launches around a few hundred thousand scalars (rgcn_bce_head_f32); labels get no gradient"""
    return _BCEWithLogits.apply(scores, labels)


class MaskedCrossEntropy(torch.nn.Module):
    """`criterion(logits[idx, :], labels)` with nn.CrossEntropyLoss() (reference experiments/classify_nodes.py:107-110) for a FIXED
    set of labelled nodes, as one kernel for the loss and its gradient instead of ATen's ~13 launches (gather, log-softmax, nll,
    their backwards and an index_put through a sort): `MaskedCrossEntropy(idx, labels, num_nodes)(logits)`; idx must not repeat."""

    def __init__(self, idx, labels, num_nodes):
        super().__init__()
        idx, labels = idx.reshape(-1).long(), labels.reshape(-1).long()
        assert idx.numel() == labels.numel() and idx.numel() > 0 and torch.unique(idx).numel() == idx.numel(), "labelled nodes: one label each"
        # (one read-back at construction) the kernel indexes a row of logits with the label: checked against the class count in forward,
        # as ATen's CrossEntropyLoss device-asserts
        self._label_range = (int(labels.min().item()), int(labels.max().item()))
        row_label = torch.full((num_nodes,), -1, dtype=torch.int32, device=idx.device)
        row_label[idx] = labels.to(torch.int32)
        self.register_buffer("row_label", row_label, persistent=False)
        self.register_buffer("lab_rows", idx.to(torch.int32).contiguous(), persistent=False)

    def forward(self, logits):
        assert logits.dim() == 2 and logits.shape[0] == self.row_label.shape[0]
        assert int(logits.shape[1]) <= 64, "at most 64 classes"
        lo, hi = self._label_range
        if lo < 0 or hi >= int(logits.shape[1]):
            raise IndexError(f"MaskedCrossEntropy: labels span {lo} .. {hi} but the logits have {int(logits.shape[1])} classes")
        return _MaskedCE.apply(logits, self.row_label, self.lab_rows)
