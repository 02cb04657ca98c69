"""The float64 reference of one link-prediction training step, on the CPU, in plain differentiable torch -- what
experiments/predict_links.py::step_loss computes, written from the formulas of include/rgcn_hip.h, predict_links.py and oracle/:

    x0 = relu(node_embeddings + node_embeddings_bias)
    LP layer: out[s] = sum over the messages (s, p, o) of val * x[o] @ W[p] + bias, the message list and val from oracle.lp_augment /
              oracle.edge_norm (the calls oracle.lp_layer makes); W from `weights`, from `bases` / `comps`, or block_diag(blocks) with
              the dense blocks_self as the last relation; ReLU between two layers
    c-rgcn:   node_embeddings + decoding_layer(layers(encoding_layer(x0)))
    decoder:  DistMult sum_k e_s r_p e_o, or ComplEx (complex_reference), with or without sbias[s] + pbias[p] + obias[o]
    loss:     mean BCE-with-logits on sampled negatives | 0.5 (tail + head) of the 1-N softmax | 0.5 (tail + head) of the K-vs-All BCE
    penalty:  schlichtkrull-l2 in the GATHERED form (mean of squares of the gathered s / p / o rows) | relations.pow(2).sum()

Gradients come from float64 autograd through these functions.  bf16 cases: the parameters are the widened bf16 values and `rounded=True`
rounds where DESIGN.md 4.6 says the library does, with the identity as a rounding's derivative.  rounded="activations": the embedding
ReLU's input sum and every layer's output, once each.  rounded=True: also the gradients 4.6 names -- a layer's dX, dnodes of each loss
term, every parameter's gradient (an fp32 sum returned in the parameter's dtype) -- and the bf16 sums autograd forms where a bf16 tensor
has several readers (the encoder output and the relations: tail term, head term, penalty; the decoder biases: two terms).
rounded=False is the same evaluation without any rounding.  Also here: the case table the host test and the
GPU test share, the seeded inputs of a case, and the parameter inventory of a config.  Nothing here imports torch_rgcn or touches a GPU;
tests/test_lp_step_reference_host.py checks this module against oracle/, the golden files and central differences."""
import numpy as np
import torch

import complex_reference as cr
from oracle import oracle

F64 = torch.float64
N, R0, E, Q, RATE = 300, 4, 1500, 130, 3            # entities, relations, message triples, positives, negatives per positive


# ----------------------------------------------------------------------------- the case table
# the seed of each case's inputs is 100 k + SEEDS[k], chosen among the first hundred so that the ReLU condition holds with the widest
# room (relu_margins; the host test asserts the condition for every case)
SEEDS = (3, 50, 62, 8, 8, 2, 53, 1, 7, 91, 22, 11, 0, 0, 0)


def _enc(model="rgcn", layers=2, width=16, decomposition=None, emb=None, mode="eval"):
    """an encoder config in the schema of configs/rgcn/*.yaml.  width: of every layer (rgcn: of the embeddings too; c-rgcn: the
    bottleneck, under embeddings `emb` wide).  mode: eval | other (training, self_loop_type "other", self_loop 0.2) | sd (training,
    the shipped schlichtkrull-dropout)"""
    dropout = {"general": 0.5, "self_loop": 0.2, "self_loop_type": "schlichtkrull-dropout" if mode == "sd" else "other"}
    cfg = {"model": model, "num_layers": layers, "node_embedding": emb or width, "hidden1_size": width, "hidden2_size": width,
           "edge_dropout": dropout, "weight_init": "glorot-normal", "bias_init": "zeros"}
    if decomposition == "basis":
        cfg["decomposition"] = {"type": "basis", "num_bases": 2}
    elif decomposition == "block":
        cfg["decomposition"] = {"type": "block", "num_blocks": 4}
    return cfg


def _case(objective, decoder, biased, encoder, mode="eval", filtered=False, eps=0.0, penalty="schlichtkrull-l2", l2=0.01,
          storage="fp32", seed=0):
    dec = {"model": decoder, "l2_penalty_type": penalty, "l2_penalty": l2, "weight_init": "standard-normal"}
    if biased:
        dec["bias_init"] = "zeros"
    return dict(objective=objective, encoder=dict(encoder, edge_dropout=dict(encoder["edge_dropout"])), decoder=dec, mode=mode,
                filtered=filtered, eps=eps, storage=storage, seed=seed)


def _cases():
    c = {}
    # sampled negatives: the three penalties
    c["ns-sl2-distmult-b-none2-16"] = _case("negative-sampling", "distmult", True, _enc(width=16))
    c["ns-plain-complex-basis2-50-sd"] = _case("negative-sampling", "complex", False, _enc(width=50, decomposition="basis", mode="sd"),
                                               mode="sd", penalty="plain-l2")
    c["ns-nopen-distmult-block2-32-other"] = _case("negative-sampling", "distmult", False,
                                                   _enc(width=32, decomposition="block", mode="other"), mode="other", l2=0.0)
    c["ns-sl2-complex-b-crgcn2-50"] = _case("negative-sampling", "complex", True, _enc("c-rgcn", width=16, emb=50))
    # 1-N softmax: unfiltered, filtered, filtered and smoothed
    c["1n-distmult-none1-50"] = _case("1-n", "distmult", False, _enc(layers=1, width=50))
    c["1n-filt-complex-b-basis2-16-other"] = _case("1-n", "complex", True, _enc(width=16, decomposition="basis", mode="other"),
                                                   mode="other", filtered=True)
    c["1n-filt-smooth-distmult-b-block2-32"] = _case("1-n", "distmult", True, _enc(width=32, decomposition="block"), filtered=True,
                                                     eps=0.1, penalty="plain-l2")
    c["1n-filt-smooth-complex-crgcn1-50-other"] = _case("1-n", "complex", False, _enc("c-rgcn", layers=1, width=16, emb=50, mode="other"),
                                                        mode="other", filtered=True, eps=0.1)
    # K-vs-All BCE: eps 0 and 0.1
    c["bce-distmult-b-basis1-50"] = _case("1-n-bce", "distmult", True, _enc(layers=1, width=50, decomposition="basis"))
    c["bce-smooth-complex-block2-32-other"] = _case("1-n-bce", "complex", False, _enc(width=32, decomposition="block", mode="other"),
                                                    mode="other", eps=0.1)
    c["bce-smooth-distmult-crgcn2-50"] = _case("1-n-bce", "distmult", False, _enc("c-rgcn", width=16, emb=50), eps=0.1, penalty="plain-l2")
    c["bce-complex-b-none2-16"] = _case("1-n-bce", "complex", True, _enc(width=16), l2=0.0)
    # bf16 storage, native backward (what training.bf16 runs).  One layer: the margin of the ReLU condition below, one bf16 ulp of the
    # tensor's maximum, is 2^-8 of a few standard deviations -- about 1 % of the 4,800 pre-activations between two layers fall inside
    # it whatever the seed, while the embedding ReLU's inputs are parameters and are moved out of it by construction (case_inputs)
    c["bf16-1n-distmult-b-none1-16"] = _case("1-n", "distmult", True, _enc(layers=1, width=16), storage="bf16")
    c["bf16-1n-filt-smooth-complex-basis1-50"] = _case("1-n", "complex", False, _enc(layers=1, width=50, decomposition="basis"),
                                                       filtered=True, eps=0.1, storage="bf16")
    c["bf16-bce-smooth-distmult-b-block1-32"] = _case("1-n-bce", "distmult", True, _enc(layers=1, width=32, decomposition="block"),
                                                      eps=0.1, storage="bf16")
    for k, (name, case) in enumerate(c.items()):
        case["name"], case["seed"], case["mask_seed"] = name, 100 * k + SEEDS[k], 7000 + k
    return c


CASES = _cases()


# ----------------------------------------------------------------------------- inputs of a case
def param_shapes(case):
    """{name as in model.named_parameters(): shape} of the model the case's configs build"""
    enc, dec = case["encoder"], case["decoder"]
    emb, w, layers = enc["node_embedding"], enc["hidden1_size"], enc["num_layers"]
    R = 2 * R0 + 1
    shapes = {"node_embeddings": (N, emb), "node_embeddings_bias": (1, emb)}
    for k in range(1, layers + 1):
        kind = (enc.get("decomposition") or {}).get("type")
        if kind == "basis":
            shapes[f"rgc{k}.bases"], shapes[f"rgc{k}.comps"] = (2, w, w), (R, 2)
        elif kind == "block":
            shapes[f"rgc{k}.blocks"], shapes[f"rgc{k}.blocks_self"] = (R - 1, 4, w // 4, w // 4), (w, w)
        else:
            shapes[f"rgc{k}.weights"] = (R, w, w)
        shapes[f"rgc{k}.bias"] = (w,)
    shapes["scoring_function.relations"] = (R0, emb)
    if dec.get("bias_init"):
        shapes.update({"scoring_function.sbias": (N,), "scoring_function.obias": (N,), "scoring_function.pbias": (R0,)})
    if enc["model"] == "c-rgcn":
        shapes.update({"encoding_layer.weight": (w, emb), "encoding_layer.bias": (w,),
                       "decoding_layer.weight": (emb, w), "decoding_layer.bias": (emb,)})
    return shapes


def _scale(name, shape):
    """standard normal times this: pre-activations and scores of the order of one, every bias clearly away from zero"""
    leaf = name.split(".")[-1]
    if leaf in ("weights", "bases", "blocks_self"):
        return 0.3 / np.sqrt(shape[-2])
    if leaf == "blocks":
        return 0.3 / np.sqrt(shape[-2])
    if leaf == "weight":                             # nn.Linear [out, in]
        return 1.0 / np.sqrt(shape[-1])
    if leaf == "relations":
        return 1.0 / np.sqrt(shape[-1])
    return {"node_embeddings": 0.7, "comps": 0.7}.get(leaf, 0.3)      # every bias: 0.3


def bf16_values(a):
    """a float array rounded to bf16 (fp32 first, as the library's fp32 sums are), widened again"""
    return torch.as_tensor(np.asarray(a)).float().to(torch.bfloat16).double().numpy()


def graph_triples(rng):
    """E message triples: node 0 is the subject of a quarter of them, 5 % repeat an earlier triple"""
    fresh = E - E // 20
    T = np.stack([rng.integers(0, N, fresh), rng.integers(0, R0, fresh), rng.integers(0, N, fresh)], 1)
    T[rng.choice(fresh, E // 4, replace=False), 0] = 0
    T = np.concatenate([T, T[rng.choice(fresh, E - fresh, replace=False)]])
    return T[rng.permutation(E)].astype(np.int64)


def case_inputs(case):
    """-> dict(graph [E, 3], batch [Q, 3] or [Q (1 + RATE), 3], labels or None, positives [Q, 3], params {name: float64 array})"""
    rng = np.random.default_rng(case["seed"])
    T = graph_triples(rng)
    pos = T[rng.choice(E, Q, replace=False)]
    if case["objective"] == "negative-sampling":
        neg = np.repeat(pos, RATE, axis=0)
        heads = rng.random(len(neg)) < 0.5
        draw = rng.integers(0, N, len(neg))
        neg[heads, 0], neg[~heads, 2] = draw[heads], draw[~heads]
        batch = np.concatenate([pos, neg])
        labels = np.concatenate([np.ones(Q), np.zeros(Q * RATE)])
    else:
        batch, labels = pos, None
    params = {name: rng.standard_normal(shape) * _scale(name, shape) for name, shape in param_shapes(case).items()}
    if case["storage"] == "bf16":
        params = {k: bf16_values(v) for k, v in params.items()}
        # the embedding ReLU's inputs are parameters: those inside the margin of the ReLU condition are moved to three times the margin
        emb, bias = params["node_embeddings"], params["node_embeddings_bias"]
        z = bf16_values(emb + bias)
        margin = 2.0 ** -7 * np.abs(z).max()
        near = np.abs(z) <= 1.5 * margin
        emb[near] = bf16_values(np.where(z >= 0, 3.0, -3.0) * margin - np.broadcast_to(bias, emb.shape))[near]
    return dict(graph=T, batch=batch, labels=labels, positives=pos, params=params)


def recorded_keeps(case):
    """the self-loop keep masks of the case's two layers: every loop outside training mode "other"; there, what the generator of an
    MI355X draws after torch.manual_seed(case["mask_seed"]) -- recorded in tests/golden, so that the ReLU condition of the very step the
    GPU test runs can be checked without a GPU (the GPU test replays the draws and compares them with the record)"""
    if case["mode"] != "other":
        return (None, None)
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lp_step_keep_masks.npz")
    masks = np.load(path, allow_pickle=False)[f"seed{case['mask_seed']}"]
    return (masks[0], masks[1])


def known_completions(triples):
    """(p, o) -> set of known heads, (s, p) -> set of known tails"""
    heads, tails = {}, {}
    for s, p, o in np.asarray(triples).tolist():
        heads.setdefault((p, o), set()).add(s)
        tails.setdefault((s, p), set()).add(o)
    return heads, tails


def known_cells(batch, known, head):
    """bool [Q, N]: the known completions of every query (its own target among them)"""
    heads, tails = known
    cell = torch.zeros(len(batch), N, dtype=torch.bool)
    for q, (s, p, o) in enumerate(np.asarray(batch).tolist()):
        cell[q, sorted(heads[(p, o)] if head else tails[(s, p)])] = True
    return cell


# ----------------------------------------------------------------------------- encoder
def _to_bf16(t):
    """rounded to bf16 through fp32, the width the library sums in"""
    return t.float().to(torch.bfloat16).double()


class _BF16(torch.autograd.Function):
    """a tensor stored as bf16: its value rounded on the way forward (value=True), the gradient that arrives for it rounded on the way
    back (grad=True); the derivative of a rounding is the identity"""

    @staticmethod
    def forward(ctx, t, value, grad):
        ctx.grad = grad
        return _to_bf16(t) if value else t.clone()

    @staticmethod
    def backward(ctx, g):
        return (_to_bf16(g) if ctx.grad else g), None, None


def bf16_round(t, grad=False):
    """t rounded to bf16; grad: the gradient rounded too"""
    return _BF16.apply(t, True, grad)


def bf16_grad(t):
    """t as it is, its gradient rounded to bf16: a bf16 tensor read by one consumer"""
    return _BF16.apply(t, False, True)


def fan_out(t, n, rounded):
    """n handles of a bf16 tensor with n consumers: every consumer's gradient is rounded, and autograd adds them one by one in bf16,
    the LAST handle's first (it runs the consumers in the reverse of the order they were called in) -- ((g_n + g_n-1) + ...) + g_1"""
    if rounded is not True:
        return [t] * n
    handles = []
    for k in range(n):
        t = bf16_grad(t)                    # rounds the sum of everything that arrives below
        handles.append(bf16_grad(t) if k < n - 1 else t)
    return handles


def block_diag(blocks):
    """[R, nb, bi, bo] -> [R, nb bi, nb bo]"""
    R, nb, bi, bo = blocks.shape
    W = torch.zeros(R, nb * bi, nb * bo, dtype=blocks.dtype)
    rows = [torch.cat([blocks[:, b] if c == b else W[:, :bi, :bo] for c in range(nb)], 2) for b in range(nb)]
    return torch.cat(rows, 1)


def dense_weights(P, prefix=""):
    if prefix + "weights" in P:
        return P[prefix + "weights"]
    if prefix + "bases" in P:
        return torch.einsum("rb,bio->rio", P[prefix + "comps"], P[prefix + "bases"])
    return torch.cat([block_diag(P[prefix + "blocks"]), P[prefix + "blocks_self"][None]], 0)


def messages(triples, num_nodes, num_rels, keep=None, vertical=False):
    """the augmented message list and its normalisation constants, by the calls oracle.lp_layer makes"""
    Tp, n_self = oracle.lp_augment(triples, num_nodes, num_rels, keep)
    val = oracle.edge_norm(Tp, num_nodes, 2 * num_rels + 1, vertical, len(np.asarray(triples).reshape(-1, 3)), n_self)
    return torch.from_numpy(Tp), torch.from_numpy(val).double()


def lp_layer(msgs, X, W, bias=None):
    """out[s] = sum over the messages (s, p, o) of val * X[o] @ W[p] (+ bias): the rows gathered and summed per (relation, subject)
    first, then one product per relation"""
    Tp, val = msgs
    s, p, o = Tp[:, 0], Tp[:, 1], Tp[:, 2]
    R, n = W.shape[0], X.shape[0]
    agg = torch.zeros(R * n, X.shape[1], dtype=X.dtype).index_add(0, p * n + s, val[:, None] * X[o])
    out = torch.einsum("rni,rio->no", agg.view(R, n, -1), W)
    return out if bias is None else out + bias


def encode(P, enc, graph, keeps=(None, None), rounded=False, relu_inputs=None):
    """the encoder output x [N, emb].  keeps: the self-loop keep mask of each layer (None: every loop); relu_inputs: a list that
    receives (name, tensor) of every ReLU's input"""
    assert not (rounded and enc["model"] == "c-rgcn"), "no bf16 case runs c-rgcn: where its two nn.Linear round is not written down here"
    rnd = bf16_round if rounded else (lambda t: t)
    if rounded is True:          # every parameter is read once in here: its gradient is an fp32 sum returned as bf16; and each layer's dX
        P = {k: bf16_grad(v) for k, v in P.items()}
    dx = bf16_grad if rounded is True else (lambda t: t)

    def relu(name, t):
        if relu_inputs is not None:
            relu_inputs.append((name, t.detach()))
        return torch.relu(t)
    x = relu("embedding", rnd(P["node_embeddings"] + P["node_embeddings_bias"]))
    if enc["model"] == "c-rgcn":
        x = x @ P["encoding_layer.weight"].T + P["encoding_layer.bias"]
    x = rnd(lp_layer(messages(graph, N, R0, keeps[0]), dx(x), dense_weights(P, "rgc1."), P.get("rgc1.bias")))
    if enc["num_layers"] == 2:
        x = rnd(lp_layer(messages(graph, N, R0, keeps[1]), dx(relu("layer 1", x)), dense_weights(P, "rgc2."), P.get("rgc2.bias")))
    if enc["model"] == "c-rgcn":
        x = P["node_embeddings"] + x @ P["decoding_layer.weight"].T + P["decoding_layer.bias"]
    return x


# ----------------------------------------------------------------------------- decoder
def decoder_biases(P):
    return tuple(P.get("scoring_function." + k) for k in ("sbias", "pbias", "obias"))


def triple_scores(triples, x, rel, bias, decoder):
    if decoder == "complex":
        return cr.triple_scores(triples, x, rel, bias)
    s, p, o = (torch.as_tensor(triples[..., k]).long() for k in range(3))
    out = (x[s] * rel[p] * x[o]).sum(-1)
    return out if bias[0] is None else out + bias[0][s] + bias[1][p] + bias[2][o]


def all_scores(batch, head, x, rel, bias, decoder):
    """[Q, N]: every entity as the head (head=True) or the tail of each query"""
    if decoder == "complex":
        return cr.all_scores(batch, head, x, rel, bias)
    s, p, o = (torch.as_tensor(batch[:, k]).long() for k in range(3))
    out = (x[o] * rel[p]) @ x.T if head else (x[s] * rel[p]) @ x.T
    if bias[0] is not None:
        sb, pb, ob = bias
        out = out + ((sb[None, :] + (pb[p] + ob[o])[:, None]) if head else (ob[None, :] + (pb[p] + sb[s])[:, None]))
    return out


# ----------------------------------------------------------------------------- objectives and penalty
def softplus(s):
    return torch.clamp(s, min=0) + torch.log1p(torch.exp(-s.abs()))


def sampled_bce(scores, labels):
    """mean over the batch of softplus(s) - y s"""
    return (softplus(scores) - labels * scores).mean()


def softmax_term(scores, batch, head, known, eps):
    """mean over the queries of lse_allowed - (1 - eps) s[target] - eps mean_allowed(s): the known completions (known=None: none) other
    than the query's own target are out of the problem"""
    nq = len(batch)
    tgt = torch.as_tensor(batch[:, 0 if head else 2]).long()
    allowed = torch.ones(nq, N, dtype=torch.bool) if known is None else ~known_cells(batch, known, head)
    allowed[torch.arange(nq), tgt] = True
    lse = torch.logsumexp(scores.masked_fill(~allowed, -np.inf), 1)
    mean_allowed = (scores * allowed).sum(1) / allowed.sum(1)
    return (lse - (1 - eps) * scores[torch.arange(nq), tgt] - eps * mean_allowed).mean()


def bce_term(scores, batch, head, known, eps):
    """mean over the queries of (1 / N) sum_n softplus(s) - y' s, y = 1 on every known completion, y' = (1 - eps) y + eps / N"""
    y = known_cells(batch, known, head)
    assert bool(y[torch.arange(len(batch)), torch.as_tensor(batch[:, 0 if head else 2]).long()].all())
    ys = (1 - eps) * y.to(F64) + eps / N
    return ((softplus(scores) - ys * scores).sum(1) / N).mean()


def gathered_penalty(batch, x, rel):
    """schlichtkrull-l2 as the reference's layers.py states it: the mean of squares of the gathered s, p and o rows"""
    s, p, o = (torch.as_tensor(batch[..., k]).long().reshape(-1) for k in range(3))
    return x[s].pow(2).mean() + rel[p].pow(2).mean() + x[o].pow(2).mean()


def step_loss(case, inputs, P, keeps=(None, None), rounded=False, relu_inputs=None):
    """the scalar loss of the case's step, float64, differentiable in every tensor of P"""
    enc, dec = case["encoder"], case["decoder"]
    batch, decoder = inputs["batch"], dec["model"]
    x = encode(P, enc, inputs["graph"], keeps, rounded, relu_inputs)
    rel, bias = P["scoring_function.relations"], decoder_biases(P)
    pen = dec["l2_penalty"] != 0.0
    sl2 = pen and dec["l2_penalty_type"] == "schlichtkrull-l2"
    if case["objective"] == "negative-sampling":
        assert rounded is not True, "no bf16 case trains on sampled negatives: where that backward rounds is not written down here"
        loss = sampled_bce(triple_scores(batch, x, rel, bias, decoder), torch.as_tensor(inputs["labels"], dtype=F64))
        xs, rels = [x], [rel]
    else:
        # three readers of x and of the relations -- the tail term, the head term, the penalty -- and two of every decoder bias
        xs, rels = fan_out(x, 2 + sl2, rounded), fan_out(rel, 2 + pen, rounded)
        biases = list(zip(*[fan_out(b, 2, rounded) if b is not None else (None, None) for b in bias]))
        known = known_completions(inputs["graph"])                       # the training triples are the message graph's

        def term(head):
            scores = all_scores(batch, head, xs[head], rels[head], biases[head], decoder)
            if case["objective"] == "1-n":
                return softmax_term(scores, batch, head, known if case["filtered"] else None, case["eps"])
            return bce_term(scores, batch, head, known, case["eps"])
        loss = 0.5 * (term(False) + term(True))
    if not pen:
        return loss
    penalty = gathered_penalty(batch, xs[-1], rels[-1]) if sl2 else rels[-1].pow(2).sum()
    return loss + dec["l2_penalty"] * penalty


def leaves(params):
    return {k: torch.tensor(np.asarray(v), dtype=F64, requires_grad=True) for k, v in params.items()}


def loss_and_grads(case, inputs, keeps=(None, None), rounded=False):
    """-> (loss float, {name: float64 gradient array})"""
    P = leaves(inputs["params"])
    loss = step_loss(case, inputs, P, keeps, rounded)
    grads = torch.autograd.grad(loss, list(P.values()), allow_unused=False)
    return loss.item(), {k: g.numpy() for k, g in zip(P, grads)}


def relu_margins(case, inputs, keeps=(None, None)):
    """[(name, min |input|, required margin)] of every ReLU of the case's evaluation: fp32 cases 1e-5 max |input|; bf16 cases, on the
    rounded evaluation, one bf16 ulp of the tensor's maximum"""
    seen = []
    bf16 = case["storage"] == "bf16"
    step_loss(case, inputs, leaves(inputs["params"]), keeps, bf16, seen)
    out = []
    for name, t in seen:
        top = t.abs().max().item()
        margin = 2.0 ** (np.floor(np.log2(top)) - 7) if bf16 else 1e-5 * top
        out.append((name, t.abs().min().item(), margin))
    return out


def rel_dist(got, want, floor=0.0):
    """max |got - want| / max(max |want|, floor)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max(initial=0.0) / max(np.abs(want).max(initial=0.0), floor, 1e-300)
