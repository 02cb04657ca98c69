"""Inputs under which an R-GCN layer is computed WITHOUT round-off, and the comparison that goes with them.

Every parity test of this suite used to compare under `max|a - b| / max|b| < 1e-4`.  R-GCN divides each message by the number of
messages with the same (relation, destination), so the rows where kernels go wrong -- hub rows: cut into pieces, merged with atomics,
split over lane groups -- carry the SMALLEST numbers, and the max-norm is set by the degree-1 rows: a kernel that loses a handful of a
hub's 45 038 messages scores 8e-6 .. 3e-5 and passes.

The kernels' arithmetic allows a test without a tolerance.  Products run in exact fp32, accumulators are fp32 or fp64,
`val = 1.0f / count` is a correctly rounded division, bf16 is rounded once.  If every `val` is a power of two and every other input a small
integer, every term is a multiple of a power of two q (the row's smallest val), and as long as sum|terms| / q fits the 24-bit significand,
every partial sum, IN ANY ORDER (atomics in arrival order, split-K, pieces), is exact.  The float64 oracle and a correct kernel then agree
in every element; one lost, duplicated or misrouted message moves an element by at least q.

    pow2_triples            graphs whose normalisation constants are powers of two under both stackings and the LP layer's formula
    ints                    small integers as float32 (exactly representable in bf16 too)
    assert_provably_exact   the CONDITION above, checked on the CPU from the oracle on |inputs| (no measurement of any kernel)
    assert_equal_exact      got - ref == 0 in every element
    eval_f32                plain float32 numpy evaluation in a given message order (the self-test of the method, tests/test_exact_inputs.py)
"""
import numpy as np

from oracle import oracle

MAX_BITS = 23.0          # A / q <= 2^23: the 24-bit significand of fp32 with one bit to spare


def pow2_triples(N, R0, groups_per_relation, hub_log2=None, seed=0, max_log2=4):
    """[E, 3] base triples (s, p, o) with #{(p, s)} and #{(p, o)} a power of two for every relation p and node.

    Per relation: `groups_per_relation` group sizes 2^0 .. 2^max_log2, each group on a distinct random subject; the same multiset of sizes
    on distinct random objects; both sides expanded to stubs and matched by a random permutation.  After add_inverse_and_self both
    normalisations (vertical: 1 / #{(p, s)}; horizontal with the transpose trick: the count of the inverse message, oracle_edge_norm) are
    2^-k.  Duplicates and s == o stay.  hub_log2: relation 0 holds ONLY large groups (2^hub and three smaller ones) -- the hub in a relation
    of its own keeps the weight-gradient grid of the other relations coarse.  The triple order is shuffled."""
    rng = np.random.default_rng(seed)
    assert groups_per_relation <= N
    parts = []
    for p in range(R0):
        if hub_log2 is not None and p == 0:
            logs = np.array([hub_log2, max(hub_log2 - 3, 0), max(hub_log2 - 5, 0), max(hub_log2 - 5, 0)])
        else:
            logs = rng.integers(0, max_log2 + 1, groups_per_relation)
        sizes = np.int64(1) << logs.astype(np.int64)
        subj = rng.choice(N, len(sizes), replace=False)
        obj = rng.choice(N, len(sizes), replace=False)
        s = np.repeat(subj, sizes)
        o = rng.permutation(np.repeat(obj, rng.permutation(sizes)))
        parts.append(np.stack([s, np.full(len(s), p, np.int64), o], 1))
    T = np.concatenate(parts).astype(np.int64) if parts else np.zeros((0, 3), np.int64)
    return T[rng.permutation(len(T))]


def ints(shape, lo=-2, hi=2, density=1.0, rng=0):
    """integers of [lo, hi] as float32, a fraction `density` of them kept (the rest 0); |value| <= 256, so bf16 holds them exactly.
    rng: a seed or a numpy Generator (which then advances)"""
    assert -256 <= lo <= hi <= 256
    rng = np.random.default_rng(rng)
    a = rng.integers(lo, hi + 1, shape).astype(np.float32)
    if density < 1.0:
        a *= rng.random(shape) < density
    return a


def is_pow2(val):
    m, _ = np.frexp(np.asarray(val, np.float32))
    return bool(np.all(m == 0.5))


def _scatter_min(index, val, size):
    q = np.ones(size, np.float64)
    np.minimum.at(q, index, val.astype(np.float64))
    return q


def _bits(A, q):
    A = np.asarray(A, np.float64)
    r = A / q
    return float(np.log2(r.max())) if r.size and r.max() > 0 else 0.0


def provable_bits(tp, val, N, R, X, params, mode, bias, g):
    """-> {tensor name: log2 of max(sum|terms| / grid)} of one layer.  sum|terms| is the oracle on the absolute values of every input
    (parameter gradients through contract_weight_grads as usual); the grid is the smallest val of the messages that reach the element:
    per destination row (out), per source row (dX), per relation (gradients with a relation axis), the global minimum for gradients that
    sum over the relations (bases).  db sums the entries of g themselves (no val): its grid is 1.

    Pre-aggregates that a kernel may form (sum of val x over one (relation, destination) group, before the weights) are convex
    combinations -- the vals of a group sum to 1 -- so they are bounded by max|x| on the same grid and need no check of their own."""
    tp = np.asarray(tp, np.int64)
    val = np.asarray(val, np.float32)
    assert is_pow2(val), "not provably exact: a normalisation constant is not a power of two"
    for name, a in (("X", X), ("bias", bias), ("g", g), *params.items()):
        assert a is None or np.array_equal(a, np.rint(a)), f"not provably exact: {name} is not integer-valued (the grid is val x 1)"
    absp = {k: np.abs(v) for k, v in params.items()}
    A = oracle.layer(tp, val, N, R, None if X is None else np.abs(X), absp, mode, None if bias is None else np.abs(bias),
                     None if g is None else np.abs(g))
    s, p, o = tp[:, 0], tp[:, 1], tp[:, 2]
    bits = {"out": _bits(A["out"], _scatter_min(s, val, N)[:, None])}
    if g is None:
        return bits
    if X is not None:
        bits["dX"] = _bits(A["dX"], _scatter_min(o, val, N)[:, None])
    bits["db"] = _bits(A["db"], 1.0)
    q_rel = _scatter_min(p, val, R)
    q_all = float(val.min()) if len(val) else 1.0
    for name, a in A["grads"].items():
        if name in ("weights", "blocks", "comps"):           # first axis = relation (LP blocks: all but the self-loop relation, the last)
            bits[name] = _bits(a, q_rel[:a.shape[0]].reshape((-1,) + (1,) * (a.ndim - 1)))
        elif name == "blocks_self":                           # the LP layer's dense weight of the self-loop relation
            bits[name] = _bits(a, q_rel[R - 1])
        else:
            assert name == "bases", name                      # sums over the relations: the smallest val of the graph
            bits[name] = _bits(a, q_all)
    return bits


def assert_provably_exact(tp, val, N, R, X, params, mode, bias=None, g=None, skip=()):
    """the condition under which every partial sum of the layer is exact in fp32, in any order: asserted on the CPU before a kernel runs.
    A case that fails it gets other inputs (a smaller hub, sparser or smaller values, fewer nodes), never a tolerance.  -> the bits"""
    bits = provable_bits(tp, val, N, R, X, params, mode, bias, g)
    bad = {k: round(v, 2) for k, v in bits.items() if v > MAX_BITS and k not in skip}
    assert not bad, f"not provably exact in fp32 (more than {MAX_BITS} bits): {bad}"
    return bits


def assert_equal_exact(got, ref, name, degree=None):
    """no NaN and got - ref == 0 in every element (as values: -0.0 equals +0.0).  got: numpy or torch, fp32 or bf16 -- a bf16 result is
    compared with the reference rounded once to bf16.  degree: per-row message counts, printed for the rows that differ."""
    import torch
    ref = np.asarray(ref)
    if torch.is_tensor(got):
        got = got.detach()
        if got.dtype == torch.bfloat16:
            ref = torch.from_numpy(np.array(ref, np.float32)).to(torch.bfloat16).float().numpy()
            got = got.float()
        got = got.cpu().numpy()
    got = np.asarray(got)
    assert got.shape == ref.shape, f"{name}: shape {got.shape} against {ref.shape}"
    assert not np.isnan(got).any(), f"{name}: NaN in {int(np.isnan(got).sum())} elements"
    diff = got.astype(np.float64) - ref.astype(np.float64)
    bad = np.argwhere(diff != 0)
    if len(bad):
        lines = []
        for ix in bad[:8]:
            ix = tuple(int(i) for i in ix)
            deg = "" if degree is None or not ix else f" degree {int(degree[ix[0]])}"
            lines.append(f"  {ix}: got {got[ix]!r} ref {ref[ix]!r}{deg}")
        raise AssertionError(f"{name}: {len(bad)} of {got.size} elements differ from the exact result\n" + "\n".join(lines))


def eval_f32(tp, val, N, R, X, W, bias, g, order):
    """out, dX, dW of the dense-weight layer in plain float32 numpy, the messages added one by one in the given order"""
    tp = np.asarray(tp, np.int64)[order]
    val = np.asarray(val, np.float32)[order]
    s, p, o = tp[:, 0], tp[:, 1], tp[:, 2]
    f = np.float32
    d_in, d_out = W.shape[1], W.shape[2]
    XW = np.einsum("ni,rio->rno", X.astype(f), W.astype(f))           # small integers: exact
    GW = np.einsum("no,rio->rni", g.astype(f), W.astype(f))
    out = np.zeros((N, d_out), f)
    np.add.at(out, s, val[:, None] * XW[p, o])
    out += bias.astype(f)
    dX = np.zeros((N, d_in), f)
    np.add.at(dX, o, val[:, None] * GW[p, s])
    dW = np.zeros((R, d_in, d_out), f)
    for a in range(0, len(tp), 1 << 14):
        b = slice(a, a + (1 << 14))
        np.add.at(dW, p[b], (val[b, None] * X[o[b]].astype(f))[:, :, None] * g[s[b]].astype(f)[:, None, :])
    return {"out": out, "dX": dX, "weights": dW}
