"""Drop-in `torch_rgcn.layers` for MI355X: same class names, constructor / forward
signatures, parameter names and shapes as thiviyanT/torch-rgcn's layers.py, with
the message passing done by hand-written HIP kernels (csrc/) instead of ATen
sparse ops.

    RelationalGraphConvolutionNC   reference torch_rgcn/layers.py:101-308
    RelationalGraphConvolutionLP   reference torch_rgcn/layers.py:311-565
    DistMult                       reference torch_rgcn/layers.py:9-98
    ComplEx                        an extension: DistMult's interface over complex numbers

What is the same: the function computed, out = sum_r A_r X W_r + b with the
reference's exact per-edge normalisation (including the link-prediction
double-count), parameter inventory, initialisers, asserts.
What differs: tensors must be on a GPU (no CPU fallback -- a CPU tensor raises);
the graph layout is cached (NC) instead of being rebuilt every forward; the dense
R x N x d intermediates of the reference are never materialised for featured layers.
"""
import math
import os

import torch

from . import routes
from torch import nn
from torch.nn import Module, Parameter

from . import functional as F_
from .graph import graph_from_lp_triples, graph_from_nc_triples
from .utils import block_diag, schlichtkrull_normal_, select_b_init, select_w_init, split_spo

_RELU_GAIN = math.sqrt(2.0)  # nn.init.calculate_gain('relu')


def _unpack_decomposition(decomposition):
    d = decomposition or {}
    return d.get('type'), d.get('num_bases'), d.get('num_blocks')


def _require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f"{what} is on {t.device}: this build of torch_rgcn runs its message passing on "
                           "HIP kernels only and has no CPU path; move the module and its inputs to a GPU")


class DistMult(Module):
    """DistMult decoder: score(s,p,o) = <e_s, r_p, e_o> (+ per-entity / per-relation biases)."""

    decoder = "distmult"           # what the all-candidate functions of functional.py take as `decoder=` (ComplEx overrides it)

    def __init__(self, indim, outdim, num_nodes, num_rel, w_init='standard-normal', w_gain=False, b_init=None):
        super().__init__()
        self.w_init, self.w_gain, self.b_init = w_init, w_gain, b_init
        self.relations = Parameter(torch.empty(indim, outdim))
        if b_init:
            self.sbias = Parameter(torch.empty(num_nodes))
            self.obias = Parameter(torch.empty(num_nodes))
            self.pbias = Parameter(torch.empty(num_rel))
        else:
            for name in ('sbias', 'obias', 'pbias'):
                self.register_parameter(name, None)
        self.initialise_parameters()

    def initialise_parameters(self):
        fill = select_w_init(self.w_init)
        if self.w_gain:
            fill(self.relations, gain=_RELU_GAIN)
        else:
            fill(self.relations)
        if self.b_init:
            fill_b = select_b_init(self.b_init)
            for b in (self.sbias, self.pbias, self.obias):
                fill_b(b)

    def s_penalty(self, triples, nodes):
        """Schlichtkrull L2 penalty: mean squares of the gathered s / p / o embeddings (layers.py:77-85).

        The reference gathers three T x d operands and lets autograd scatter their gradients back (index_put with
        accumulation: 15 ms of a 20 ms WN18 training step here).  The same number is sum_n count(n) * |row_n|^2 / (T d):
        count the occurrences once (integer histogram), square-sum every row once -- the gradient is then a plain
        elementwise product and nothing is gathered or scattered."""
        s, p, o = split_spo(triples)
        s, p, o = s.reshape(-1), p.reshape(-1), o.reshape(-1)
        scale = 1.0 / (s.numel() * nodes.shape[-1])
        # counts and square sums in fp32 whatever the storage type (a bf16 count stops at 256: 256 + 1 rounds back to 256); .float() is a
        # no-op on fp32 tensors, and the result is returned in nodes.dtype
        node_sq = nodes.float().pow(2).sum(dim=-1)
        rel_sq = self.relations.float().pow(2).sum(dim=-1)
        def count(idx, n):       # occurrence histogram without torch.bincount (which reads the maximum back: a sync)
            return torch.zeros(n, device=nodes.device, dtype=torch.float32).index_add_(
                0, idx.to(nodes.device), torch.ones(idx.numel(), device=nodes.device, dtype=torch.float32))
        n_nodes, n_rel = nodes.shape[0], self.relations.shape[0]
        return (((count(s, n_nodes) * node_sq).sum() + (count(o, n_nodes) * node_sq).sum()) * scale
                + (count(p, n_rel) * rel_sq).sum() * (1.0 / (p.numel() * self.relations.shape[-1]))).to(nodes.dtype)

    def forward(self, triples, nodes):
        _require_gpu(nodes, "DistMult node embeddings")
        triples = triples.to(nodes.device)
        if self.b_init:
            return F_.distmult_score(triples, nodes, self.relations, self.sbias, self.pbias, self.obias)
        return F_.distmult_score(triples, nodes, self.relations)

    def softmax_loss(self, triples, nodes, head=False, filt_q=None, filt_n=None, reduction="mean", filt=None, bf16_backward="upcast",
                     label_smoothing=0.0):
        """1-N softmax cross-entropy of `triples` [Q, 3] against every entity as the head (head=True) or the tail, with this decoder's
        relations and biases (functional.distmult_softmax_loss: no [Q, N] logits; an extension, the reference has no counterpart).
        filt_q / filt_n: int32 device lists of (query, entity) cells left out of the denominator; filt: a functional.FilterIndex in
        their place (the known completions of every query, looked up on the device: the filtered step stays capturable).
        bf16_backward: "upcast" or "native", the route of a bf16 embedding table that trains (functional.distmult_softmax_loss; no effect
        on fp32 embeddings).  label_smoothing: eps in [0, 1), spread evenly over the candidates that are not filtered (0: none)."""
        _require_gpu(nodes, "DistMult node embeddings")
        triples = triples.to(nodes.device)
        # (without b_init the three biases are registered as None: one call serves both)
        return F_.distmult_softmax_loss(triples, head, nodes, self.relations, self.sbias, self.pbias, self.obias,
                                        filt_q=filt_q, filt_n=filt_n, reduction=reduction, filt=filt, bf16_backward=bf16_backward,
                                        label_smoothing=label_smoothing, decoder=self.decoder)

    def bce_loss(self, triples, nodes, head=False, lab_q=None, lab_n=None, labels=None, reduction="mean", bf16_backward="upcast",
                 label_smoothing=0.0):
        """1-N multi-label binary cross-entropy ("K-vs-All") of `triples` [Q, 3] against every entity as the head (head=True) or the
        tail, with this decoder's relations and biases (functional.distmult_bce_loss: no [Q, N] logits or labels; an extension).
        A query's own target is a positive label, and so is every cell on the int32 device lists lab_q / lab_n or every known
        completion in `labels`, a functional.FilterIndex (not both); everything else is a negative.  bf16_backward: as in softmax_loss.
        label_smoothing: eps in [0, 1), y' = (1 - eps) y + eps / N over ALL entities."""
        _require_gpu(nodes, "DistMult node embeddings")
        triples = triples.to(nodes.device)
        bce_loss = F_.complex_bce_loss if self.decoder == "complex" else F_.distmult_bce_loss
        return bce_loss(triples, head, nodes, self.relations, self.sbias, self.pbias, self.obias, lab_q=lab_q, lab_n=lab_n,
                        labels=labels, reduction=reduction, bf16_backward=bf16_backward, label_smoothing=label_smoothing)


class ComplEx(DistMult):
    """ComplEx decoder (Trouillon et al. 2016; an extension, the reference has DistMult only): score(s,p,o) = Re <e_s, r_p, conj(e_o)>
    (+ the same biases) -- not symmetric in s and o, so it can tell (a, hypernym, b) from (b, hypernym, a).  A row of the embeddings and
    of `relations`, `outdim` wide, holds outdim / 2 complex features: real halves in the first columns, imaginary halves behind them
    (an odd outdim: ValueError).  Constructor, parameter names and shapes are DistMult's, so a state dict loads either way; s_penalty is
    inherited (|e|^2 = re^2 + im^2); softmax_loss and bce_loss run DistMult's all-candidate kernels on ComplEx query vectors."""

    decoder = "complex"

    def __init__(self, indim, outdim, num_nodes, num_rel, w_init='standard-normal', w_gain=False, b_init=None):
        if outdim % 2:
            raise ValueError(f"ComplEx needs an even embedding width (real halves | imaginary halves), got outdim = {outdim}")
        super().__init__(indim, outdim, num_nodes, num_rel, w_init, w_gain, b_init)

    def forward(self, triples, nodes):
        _require_gpu(nodes, "ComplEx node embeddings")
        triples = triples.to(nodes.device)
        if self.b_init:
            return F_.complex_score(triples, nodes, self.relations, self.sbias, self.pbias, self.obias)
        return F_.complex_score(triples, nodes, self.relations)


class _RGCBase(Module):
    """Parameter inventory shared by the NC and LP layers."""

    def _make_weights(self, num_relations, in_dim, out_dim, lp):
        kind = self.weight_decomp
        if kind is None:
            self.weights = Parameter(torch.empty(num_relations, in_dim, out_dim))
        elif kind == 'basis':
            assert self.num_bases > 0, 'Number of bases should be set to higher than zero for basis decomposition!'
            self.bases = Parameter(torch.empty(self.num_bases, in_dim, out_dim))
            self.comps = Parameter(torch.empty(num_relations, self.num_bases))
        elif kind == 'block':
            nb = self.num_blocks
            assert nb > 0, 'Number of blocks should be set to a value higher than zero for block diagonal decomposition!'
            assert in_dim % nb == 0 and out_dim % nb == 0, \
                f'For block diagonal decomposition, input dimensions ({in_dim}, {out_dim}) must be divisible ' \
                f'by number of blocks ({nb})'
            if lp:  # the self-loop relation keeps a dense matrix of its own
                self.blocks = Parameter(torch.empty(num_relations - 1, nb, in_dim // nb, out_dim // nb))
                self.blocks_self = Parameter(torch.empty(in_dim, out_dim))
            else:
                self.blocks = Parameter(torch.empty(num_relations, nb, in_dim // nb, out_dim // nb))
        else:
            raise NotImplementedError(f'{kind} decomposition has not been implemented')

    def _dense_weights_f32(self):
        """the dense fp32 weights of the bf16 route: bf16 parameters widened once per call (autograd carries the casts back)"""
        if getattr(self, "diag_weight_matrix", False):
            return torch.diag_embed(self.weights.float())
        kind = self.weight_decomp
        if kind is None:
            return self.weights.float()
        if kind == 'basis':
            B = self.bases.size(0)
            W = F_.matmul_mfma(self.comps.float(), self.bases.float().reshape(B, -1))
            return W.view(self.comps.size(0), *self.bases.shape[1:])
        return block_diag(self.blocks.float())

    def _dense_weights(self):
        """(R, in_dim, out_dim) view of the (possibly decomposed) relation weights."""
        kind = self.weight_decomp
        if kind is None:
            return self.weights
        if kind == 'basis':
            B = self.bases.size(0)
            flat = self.bases.reshape(B, -1)
            # einsum('rb,bio->rio') as an [R, B] x [B, d_i d_o] product on the matrix cores (GPU); CPU tensors (parameter
            # inspection before .cuda()) keep torch.matmul
            W = F_.matmul_mfma(self.comps, flat) if self.comps.is_cuda else torch.matmul(self.comps, flat)
            return W.view(self.comps.size(0), *self.bases.shape[1:])
        if kind == 'block':
            return block_diag(self.blocks)
        raise NotImplementedError(f'{kind} decomposition has not been implemented')


def _check_dtypes(layer, features):
    """fp32 (the default) or bf16 features (bf16 out, fp32 arithmetic); the parameters fp32, or bf16 with bf16 features only.
    Featureless: fp32 parameters, or -- basis decomposition only -- bf16 bases (the table decides the storage) with fp32 or bf16 comps / bias"""
    pdt = {p.dtype for p in layer.parameters()}
    if features is None:
        if not pdt - {torch.float32}:
            return False
        if layer.weight_decomp != 'basis' or getattr(layer, "diag_weight_matrix", False) or layer.in_features is not None:
            raise TypeError(f"featureless layers support torch.float32 parameters only (torch.bfloat16 needs basis decomposition), "
                            f"got {sorted(map(str, pdt))}")
        if pdt - {torch.float32, torch.bfloat16}:
            raise TypeError(f"featureless basis layers take torch.float32 or torch.bfloat16 parameters, got {sorted(map(str, pdt))}")
        if layer.bases.dtype != torch.bfloat16:
            raise TypeError("torch.bfloat16 comps / bias need torch.bfloat16 bases (the bases table decides the storage; "
                            f"got bases {layer.bases.dtype})")
        return True
    if features.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"features must be torch.float32 or torch.bfloat16 (opt-in, fp32 arithmetic), got {features.dtype}")
    if pdt - {torch.float32, torch.bfloat16}:
        raise TypeError(f"parameters must be torch.float32 or torch.bfloat16, got {sorted(map(str, pdt))}")
    if features.dtype == torch.float32 and torch.bfloat16 in pdt:
        raise TypeError("torch.bfloat16 parameters need torch.bfloat16 features (fp32 features take torch.float32 parameters)")
    return features.dtype == torch.bfloat16


def _f32(t):
    return None if t is None else t.float()


class RelationalGraphConvolutionNC(_RGCBase):
    """R-GCN layer for node classification; the (already augmented) graph is fixed at construction."""

    def __init__(self, triples=None, num_nodes=None, num_relations=None, in_features=None, out_features=None,
                 edge_dropout=None, edge_dropout_self_loop=None, bias=True, decomposition=None,
                 vertical_stacking=False, diag_weight_matrix=False, reset_mode='glorot_uniform'):
        super().__init__()
        assert (triples is not None or num_nodes is not None or num_relations is not None or
                out_features is not None), \
            "The following must be specified: triples, number of nodes, number of relations and output dimension!"
        in_dim = num_nodes if in_features is None else in_features  # featureless: one-hot inputs
        self.weight_decomp, self.num_bases, self.num_blocks = _unpack_decomposition(decomposition)
        self.triples = triples
        self.num_nodes, self.num_relations = num_nodes, num_relations
        self.in_features, self.out_features = in_features, out_features
        self.vertical_stacking = vertical_stacking
        self.diag_weight_matrix = diag_weight_matrix
        self.edge_dropout, self.edge_dropout_self_loop = edge_dropout, edge_dropout_self_loop  # stored, unused (as upstream)

        if diag_weight_matrix:
            self.weights = Parameter(torch.empty(num_relations, in_features))
            self.out_features = in_features
            self.weight_decomp = None
            bias = False
        else:
            self._make_weights(num_relations, in_dim, out_features, lp=False)
        if bias:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        self._graph = None
        self._graph_key = None
        self.reset_parameters(reset_mode)

    def reset_parameters(self, reset_mode='glorot_uniform'):
        if reset_mode in ('glorot_uniform', 'schlichtkrull'):
            targets = {'block': ('blocks',), 'basis': ('bases', 'comps')}.get(self.weight_decomp, ('weights',))
            for name in targets:
                nn.init.xavier_uniform_(getattr(self, name), gain=_RELU_GAIN)
            if self.bias is not None:
                nn.init.zeros_(self.bias)
        elif reset_mode == 'uniform':
            bound = 1.0 / math.sqrt(self.weights.size(1))  # AttributeError under decomposition, as upstream
            targets = {'block': ('blocks',), 'basis': ('bases', 'comps')}.get(self.weight_decomp, ('weights',))
            for name in targets:
                getattr(self, name).data.uniform_(-bound, bound)
            if self.bias is not None:
                self.bias.data.uniform_(-bound, bound)
        else:
            raise NotImplementedError(f'{reset_mode} parameter initialisation method has not been implemented')

    # the layer is handed a CPU LongTensor and never told about .cuda(): pick the device from the
    # parameters at forward time and keep the device-resident layout until the triples change
    def _graph_on(self, device):
        t = self.triples
        key = (id(t), t._version if torch.is_tensor(t) else None, str(device), self.vertical_stacking)
        if self._graph is None or self._graph_key != key:
            # featureless layers index their R x N x d weight table by node id: no locality relabelling for them (the automatic
            # choice skips them; an explicit route `relabel` raises in forward, as before)
            relabel = "none" if (self.in_features is None and not routes.is_set("relabel")) else None
            self._graph = graph_from_nc_triples(t, self.num_nodes, self.num_relations, self.vertical_stacking, device, relabel=relabel)
            if getattr(self, "_shard_group", None) is not None and self._shard_keep == "lpt":
                from .dist import filter_graph_for_rank
                filter_graph_for_rank(self._graph, self._shard_group)
            self._graph_key = key
        return self._graph

    def forward(self, features=None):
        return self._forward_impl(features, self.__dict__.pop("_fused_activation", None), self.__dict__.pop("_fused_private", False))

    def forward_activated(self, features=None, activation=None, private=False):
        """forward() plus the activation the models apply right after this layer (reference models.py:194,235,290
        `F.relu(self.rgc1(...))`), run in the kernel's epilogue.  activation: None or "relu".  A separate method so that
        forward() keeps the reference's exact signature; it goes through nn.Module.__call__ (forward / pre-forward hooks
        registered on the layer fire exactly as for `F.relu(self.rgc1(...))`), the activation rides along as a transient
        attribute.

        private=True is a promise by the caller: the returned activation H is only fed to layers of this library and nobody asks
        autograd for ITS gradient (no torch.autograd.grad(loss, H), no grad_fn pre-hook; retain_grad() and tensor hooks are seen and
        honoured).  The consuming layer's backward kernel may then apply the ReLU's mask in its own epilogue and hand autograd
        dL/d(pre-activation) in the place of dL/dH -- one elementwise launch less per step (functional._ReluToken).  Without the
        promise (the default, and what `F.relu(layer(x))` gives) every gradient autograd can show is exact."""
        assert activation in (None, "relu"), f"unknown activation {activation!r}"
        self._fused_activation = activation
        self._fused_private = bool(private)
        try:
            return self(features=features)
        finally:
            self.__dict__.pop("_fused_activation", None)
            self.__dict__.pop("_fused_private", None)

    def _forward_impl(self, features, activation, private=False):
        assert (features is None) == (self.in_features is None), "in_features not provided!"
        assert activation in (None, "relu"), f"unknown activation {activation!r}"
        if _check_dtypes(self, features):
            if features is None:
                return self._forward_featureless_bf16(activation, private)
            return self._forward_bf16(features, activation, private)
        any_param = self.weights if (self.diag_weight_matrix or self.weight_decomp is None) else \
            (self.bases if self.weight_decomp == 'basis' else self.blocks)
        _require_gpu(any_param, "RelationalGraphConvolutionNC parameters")
        N, R, out_dim = self.num_nodes, self.num_relations, self.out_features
        in_dim = N if self.in_features is None else self.in_features
        graph = self._graph_on(any_param.device)
        relabelled = graph.perm is not None
        if relabelled:      # plans on locality-relabelled ids (RGCN_RELABEL): features in through inv, output back through perm
            if features is None:
                raise NotImplementedError("RGCN_RELABEL with a featureless layer (the R x N x d weight table is indexed by node id)")
            features = features.index_select(0, graph.inv)

        fl_basis = self.in_features is None and self.weight_decomp == 'basis' and not self.vertical_stacking and graph._dev is not None
        # block-diagonal weights: the blocks are applied as they are (csrc/rgcn_block.hip); blocks above 8 x 8, or a host-built
        # graph, are expanded to dense R x d x d weights and multiplied per message by the relation-grouped gather-GEMM of
        # csrc/rgcn_gemm.hip (hand-written MFMA).  Round 1-2 had a third route for small graphs -- einsum('nbi,rbio->rnbo') on
        # rocBLAS into an R x N x d_out message table -- removed in round 3: no path arithmetic on a vendor BLAS.
        block_path = self.in_features is not None and self.weight_decomp == 'block' and not self.diag_weight_matrix and \
            F_.use_block_path(graph, self.blocks)
        diag_path = self.diag_weight_matrix and self.in_features is not None and not self.vertical_stacking and \
            getattr(self, "_shard_group", None) is None and F_.use_diag_path(graph, in_dim)
        if self.diag_weight_matrix:
            assert self.weights.size() == (R, in_dim)
            # W_r = diag(w_r): scaled on the way into the aggregation (rgcn_diag_spmm_f32); embedded only off that path
            weights = None if diag_path else torch.diag_embed(self.weights)
        elif fl_basis:
            weights = None                                     # never materialise the R x N x d_out table
            assert self.bases.size() == (self.num_bases, in_dim, out_dim) and self.comps.size() == (R, self.num_bases)
        elif block_path:
            weights = None                                     # never expand the blocks to R x d x d
        elif self.in_features is not None and self.weight_decomp == 'basis' and \
                F_.use_basis_path(self.num_bases, in_dim, out_dim, graph):
            weights = None                                     # aggregate per basis, then contract
        else:
            weights = self._dense_weights()
            assert weights.size() == (R, in_dim, out_dim)

        if self.in_features is None:
            if self.vertical_stacking:
                raise RuntimeError("featureless message passing needs horizontal stacking "
                                   f"(mat1 and mat2 shapes cannot be multiplied: {R * N}x{N} and {R * N}x{out_dim})")
            # the models' F.relu(self.rgc1()) (reference models.py:194) in the kernel's epilogue; the consumer layer's backward masks
            fuse_act = activation == "relu" and getattr(self, "_shard_group", None) is None and ("private" if private else True)
            if fl_basis:
                local = lambda _x, b: F_.featureless_basis_mp(self.bases, self.comps, b, graph, relu=fuse_act)
            else:
                local = lambda _x, b: F_.featureless_mp(weights, b, graph, relu=fuse_act)
            if fuse_act:
                activation = None
        else:
            _require_gpu(features, "features")
            assert features.size() == (N, in_dim), f"features {tuple(features.size())} vs ({N}, {in_dim})"
            if diag_path:
                local = lambda x, b: F_.diag_mp(x, self.weights, b, graph)
            elif block_path:
                fuse_act = activation == "relu" and getattr(self, "_shard_group", None) is None
                local = lambda x, b: F_.block_mp(x, self.blocks, b, graph, relu=bool(fuse_act))
                if fuse_act:
                    activation = None
            elif self.weight_decomp == 'basis' and not self.diag_weight_matrix and weights is None:
                local = lambda x, b: F_.basis_mp(x, self.bases, self.comps, b, graph)
            else:
                fuse_act = activation == "relu" and getattr(self, "_shard_group", None) is None and ("private" if private else True)
                hint = self.blocks if (self.weight_decomp == 'block' and not self.diag_weight_matrix) else None
                local = lambda x, b: F_.relational_mp(x, weights, b, graph, relu=fuse_act, blocks=hint)
                if fuse_act:
                    activation = None
        group = getattr(self, "_shard_group", None)
        if group is None:
            output = local(features, self.bias)
        elif self.in_features is not None and weights is not None:
            # relation-sharded: partial sums joined by the layer's transport (torch_rgcn.dist.shard_layer / set_transport)
            comm, slabs = getattr(self, "_shard_transport", ("allreduce", 0))
            output = F_.sharded_relational_mp(features, weights, self.bias, graph, group, slabs, comm)
        else:  # relation-sharded: partial sums joined by an all-reduce, bias added once afterwards
            from .dist import sharded_apply
            output = sharded_apply(lambda x: local(x, None), features, group)
            if self.bias is not None:
                output = output + self.bias
        assert output.size() == (N, out_dim)
        if relabelled:
            output = output.index_select(0, graph.perm)
        return torch.relu(output) if activation == "relu" else output

    def _forward_bf16(self, features, activation, private):
        """bf16 features, bf16 output rounded once.  Block-diagonal and diagonal weights are applied as they are on the bf16
        forms of the block / diagonal kernels where the fp32 layer takes those kernels (above padded width 16; block_path / diag_path = 2:
        at any width); every other layer -- width 16, relation-sharded, RGCN_DETERMINISTIC=1, host-built graphs -- on its dense fp32 W"""
        _require_gpu(features, "features")
        N, out_dim = self.num_nodes, self.out_features
        assert features.size() == (N, self.in_features), f"features {tuple(features.size())} vs ({N}, {self.in_features})"
        any_param = next(self.parameters())
        _require_gpu(any_param, "RelationalGraphConvolutionNC parameters")
        graph = self._graph_on(any_param.device)
        if graph.perm is not None:
            features = features.index_select(0, graph.inv)
        structured = getattr(self, "_shard_group", None) is None and not F_.deterministic()
        output = None
        if structured and self.diag_weight_matrix:
            wide = self.in_features + (-self.in_features % 16) > 16 or routes.get("diag_path") == "2"
            if wide and not self.vertical_stacking and F_.use_diag_path(graph, self.in_features):
                assert self.weights.size() == (self.num_relations, self.in_features)
                output = F_.diag_mp_bf16(features, self.weights.float(), _f32(self.bias), graph)
                if activation == "relu":
                    output = torch.relu(output)
        elif structured and self.weight_decomp == 'block' and F_.use_block_path(graph, self.blocks):
            output = F_.block_mp_bf16(features, self.blocks.float(), _f32(self.bias), graph, relu=activation == "relu")
        if output is not None:
            assert output.size() == (N, out_dim)
            return output.index_select(0, graph.perm) if graph.perm is not None else output
        weights = self._dense_weights_f32()
        assert weights.size() == (self.num_relations, self.in_features, out_dim)
        relu = activation == "relu" and ("private" if private else True)
        group = getattr(self, "_shard_group", None)
        comm, slabs = getattr(self, "_shard_transport", ("allreduce", 0))
        output = F_.relational_mp_bf16(features, weights, _f32(self.bias), graph, relu=relu, group=group, n_slabs=slabs, comm=comm)
        assert output.size() == (N, out_dim)
        return output.index_select(0, graph.perm) if graph.perm is not None else output

    def _forward_featureless_bf16(self, activation, private):
        """featureless layer with basis decomposition and bf16 bases: the tile kernels on the bf16 table
        (F_.featureless_basis_mp_bf16); relation-sharded layers and host-built graphs run the fp32 route on the widened
        parameters and round the output once"""
        N, R, out_dim = self.num_nodes, self.num_relations, self.out_features
        _require_gpu(self.bases, "RelationalGraphConvolutionNC parameters")
        assert self.bases.size() == (self.num_bases, N, out_dim) and self.comps.size() == (R, self.num_bases)
        graph = self._graph_on(self.bases.device)
        if graph.perm is not None:
            raise NotImplementedError("RGCN_RELABEL with a featureless layer (the R x N x d weight table is indexed by node id)")
        if self.vertical_stacking:
            raise RuntimeError("featureless message passing needs horizontal stacking "
                               f"(mat1 and mat2 shapes cannot be multiplied: {R * N}x{N} and {R * N}x{out_dim})")
        relu = activation == "relu"
        group = getattr(self, "_shard_group", None)
        fl_basis = graph._dev is not None
        if group is None and fl_basis:
            return F_.featureless_basis_mp_bf16(self.bases, self.comps, self.bias, graph, relu=relu)
        # upcast: the fp32 routes of _forward_impl on the widened parameters, one rounding at the end
        bases, comps, bias = self.bases.float(), self.comps.float(), _f32(self.bias)
        if fl_basis:
            local = lambda: F_.featureless_basis_mp(bases, comps, None, graph)
        else:
            W = F_.matmul_mfma(comps, bases.reshape(self.num_bases, -1)).view(R, N, out_dim)
            local = lambda: F_.featureless_mp(W, None, graph)
        if group is None:
            output = local()
        else:
            from .dist import sharded_apply
            output = sharded_apply(lambda _x: local(), None, group)
        if bias is not None:
            output = output + bias
        output = torch.relu(output) if relu else output
        assert output.size() == (N, out_dim)
        return output.to(torch.bfloat16)


class RelationalGraphConvolutionLP(_RGCBase):
    """R-GCN layer for link prediction; the message graph is supplied on every call."""

    def __init__(self, num_nodes=None, num_relations=None, in_features=None, out_features=None, edge_dropout=None,
                 edge_dropout_self_loop=None, decomposition=None, vertical_stacking=False, w_init='glorot-normal',
                 w_gain=False, b_init=None):
        super().__init__()
        assert (num_nodes is not None or num_relations is not None or out_features is not None), \
            "The following must be specified: number of nodes, number of relations and output dimension!"
        in_dim = num_nodes if in_features is None else in_features
        self.weight_decomp, self.num_bases, self.num_blocks = _unpack_decomposition(decomposition)
        self.num_nodes, self.num_relations = num_nodes, num_relations
        self.in_features, self.out_features = in_dim, out_features   # never None (upstream quirk)
        self.vertical_stacking = vertical_stacking
        self.edge_dropout, self.edge_dropout_self_loop = edge_dropout, edge_dropout_self_loop
        self.w_init, self.w_gain, self.b_init = w_init, w_gain, b_init

        self._make_weights(num_relations, in_dim, out_features, lp=True)
        if b_init:
            self.bias = Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        self.initialise_weights()
        if self.bias is not None:
            self.initialise_biases()
        if torch.cuda.is_available():  # upstream creates its parameters on the GPU when there is one
            self.cuda()

    def initialise_biases(self):
        select_b_init(self.b_init)(self.bias)

    def initialise_weights(self):
        gain = _RELU_GAIN if self.w_gain else 1.0
        fill = select_w_init(self.w_init)
        if self.weight_decomp == 'block':
            fan = [(self.num_relations - 1) // 2, self.in_features // self.num_blocks]
            schlichtkrull_normal_(self.blocks, shape=fan, gain=gain)
            schlichtkrull_normal_(self.blocks_self, shape=fan, gain=gain)
        elif self.weight_decomp == 'basis':
            fill(self.bases, gain=gain)
            fill(self.comps, gain=gain)
        else:
            fill(self.weights, gain=gain)

    def forward(self, triples, features=None):
        assert (features is None) == (self.in_features is None), "in_features not given"
        N, R = self.num_nodes, self.num_relations
        in_dim, out_dim = self.in_features, self.out_features
        anchor = next(self.parameters())
        _require_gpu(anchor, "RelationalGraphConvolutionLP parameters")
        device = anchor.device
        features = features.to(device)   # upstream moves both inputs to the GPU it found
        training_dropout = self.training and self.edge_dropout["self_loop_type"] == 'schlichtkrull-dropout'
        if self.training and self.edge_dropout["self_loop_type"] != 'schlichtkrull-dropout':
            keep = 1 - self.edge_dropout["self_loop"]
        else:
            keep = 1

        if self.weight_decomp == 'block' and self.vertical_stacking:
            # upstream concatenates the 3-D block_diag(blocks) with the 2-D blocks_self and fails here
            raise RuntimeError("Tensors must have same number of dimensions: got 3 and 2 "
                               "(block decomposition is only usable with horizontal stacking)")

        with torch.no_grad():
            # The reference draws the Bernoulli mask on every call, also with keep = 1 (layers.py:481-487): the draw is kept so
            # that a seeded run consumes the generator exactly as upstream does (also inside a captured hipGraph).
            # (drawn straight into the uint8 mask the graph builder reads: the same draws as torch.bernoulli(probabilities) -- one
            # uniform per element against its probability -- without the two casts, float -> bool -> uint8, at 8 us each)
            mask = torch.empty(N, dtype=torch.uint8, device=device).bernoulli_(
                torch.full((N,), float(keep), dtype=torch.float, device=device))
            graph = graph_from_lp_triples(triples, N, R, self.vertical_stacking, mask, device)

        assert features.size() == (N, in_dim)
        bf16 = _check_dtypes(self, features)
        self_drop = None
        block_path = self.weight_decomp == 'block' and F_.use_block_path(graph, self.blocks)
        if self.weight_decomp == 'block':
            if training_dropout and self.edge_dropout["self_loop"] > 0:
                # dense dropout on the self-loop messages X @ blocks_self before aggregation (added below)
                self_drop = self.edge_dropout["self_loop"]
        if bf16:
            return self._forward_bf16(features, graph, self_drop, block_path, None if keep == 1 else mask)
        if self.weight_decomp == 'block':
            if block_path:      # blocks applied as they are; the dense self-loop relation is added below
                weights = None
            else:
                own = torch.zeros_like(self.blocks_self) if self_drop is not None else self.blocks_self
                weights = torch.cat([block_diag(self.blocks), own[None]], dim=0)
        elif self.weight_decomp == 'basis' and F_.use_basis_path(self.num_bases, in_dim, out_dim, graph):
            weights = None                                     # aggregate per basis, then contract: no R x d x d tensor
        else:
            weights = self._dense_weights()
        assert weights is None or weights.size() == (R, in_dim, out_dim)

        if self.weight_decomp == 'basis' and weights is None:
            output = F_.basis_mp(features, self.bases, self.comps, self.bias, graph)
        elif block_path:
            # relations 0 .. R-2 on the block kernels (they skip relation R-1); the self-loop relation has a dense weight
            # (layers.py:514-527), one message per node and -- horizontal stacking, one per (relation, row) -- the
            # normalisation constant 1: its messages are the rows of X @ blocks_self, for the nodes whose loop survived
            output = F_.block_mp(features, self.blocks, self.bias, graph)
            if self_drop is None:
                own = F_.matmul_mfma(features, self.blocks_self)
                output = output + (own if (mask is None or keep == 1) else own * mask[:, None].to(own.dtype))
        else:
            output = F_.relational_mp(features, weights, self.bias, graph)
        if self_drop is not None:
            # schlichtkrull-dropout keeps every self loop (keep = 1 above), each node has exactly one, and its
            # normalisation count is 1 in both stackings: the self-loop messages are added row for row
            output = output + nn.functional.dropout(F_.matmul_mfma(features, self.blocks_self), p=self_drop, training=True)
        assert output.size() == (N, out_dim)
        return output

    def _forward_bf16(self, features, graph, self_drop, block_path=False, node_mask=None):
        """bf16 features, bf16 output rounded once.  Block decomposition on the block path: the blocks as they are on the bf16
        block kernels plus the dense self-loop relation, summed in fp32 and rounded once (F_.block_self_mp_bf16); everything else on the dense
        fp32 W of its decomposition (block: block_diag(blocks) with the dense self-loop relation)"""
        if block_path and not F_.deterministic():
            return F_.block_self_mp_bf16(features, self.blocks.float(), self.blocks_self.float(), _f32(self.bias), graph,
                                         node_mask=node_mask, self_drop=self_drop)
        if self.weight_decomp == 'block':
            own = torch.zeros_like(self.blocks_self, dtype=torch.float32) if self_drop is not None else self.blocks_self.float()
            weights = torch.cat([block_diag(self.blocks.float()), own[None]], dim=0)
        else:
            weights = self._dense_weights_f32()
        assert weights.size() == (self.num_relations, self.in_features, self.out_features)
        if self_drop is None:
            return F_.relational_mp_bf16(features, weights, _f32(self.bias), graph)
        # schlichtkrull-dropout: the self-loop messages are added before the one rounding (upcast route)
        X = features.float()
        output = F_.relational_mp(X, weights, _f32(self.bias), graph)
        output = output + nn.functional.dropout(F_.matmul_mfma(X, self.blocks_self.float()), p=self_drop, training=True)
        return output.to(torch.bfloat16)
