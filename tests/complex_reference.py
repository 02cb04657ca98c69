"""The float64 reference of the ComplEx tests, on the CPU, with torch complex tensors -- another formula than the kernels' expanded real
one.  A row [.., d] holds h = d / 2 complex features, real halves in columns [0, h), imaginary halves in [h, d):

    z = torch.complex(t[..., :h], t[..., h:])          score(s, p, o) = Re sum_k z_s[k] z_r[k] conj(z_o[k])  (+ the three biases)

Gradients come from float64 autograd through these functions.  tests/test_complex_host.py checks the reference against itself: the
expanded real form, the query-vector identities and the gradient identities of DESIGN.md 4.5.  Nothing here touches a GPU."""
import numpy as np
import torch

F64 = torch.float64
R0 = 5                      # relations of every case


def cplx(t):
    h = t.shape[-1] // 2
    return torch.complex(t[..., :h], t[..., h:])


def halves(z):
    """a complex tensor read back as [Re | Im]"""
    return torch.cat((z.real, z.imag), -1)


def f64(a):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=F64)


def triple_scores(triples, nodes, rel, bias=(None, None, None)):
    """float64 [T]: Re sum_k z_s z_r conj(z_o) + sbias[s] + pbias[p] + obias[o]"""
    s, p, o = (torch.as_tensor(triples[..., k]).long() for k in range(3))
    zn, zr = cplx(nodes), cplx(rel)
    out = (zn[s] * zr[p] * zn[o].conj()).sum(-1).real
    if bias[0] is not None:
        out = out + bias[0][s] + bias[1][p] + bias[2][o]
    return out


def all_scores(batch, head, nodes, rel, bias=(None, None, None)):
    """float64 [Q, N]: every entity as the head (head=True) or the tail of each query"""
    s, p, o = (torch.as_tensor(batch[:, k]).long() for k in range(3))
    zn, zr = cplx(nodes), cplx(rel)
    if head:
        out = (zn[None, :, :] * (zr[p] * zn[o].conj())[:, None, :]).sum(-1).real
    else:
        out = ((zn[s] * zr[p])[:, None, :] * zn.conj()[None, :, :]).sum(-1).real
    if bias[0] is not None:
        sb, pb, ob = bias
        out = out + ((sb[None, :] + (pb[p] + ob[o])[:, None]) if head else (ob[None, :] + (pb[p] + sb[s])[:, None]))
    return out


def expanded_real_scores(triples, nodes, rel):
    """the same score written out over the real numbers (what the kernels multiply): for the reference's self-test only"""
    s, p, o = (torch.as_tensor(triples[..., k]).long() for k in range(3))
    h = nodes.shape[1] // 2
    sr, si, rr, ri, orr, oi = nodes[s, :h], nodes[s, h:], rel[p, :h], rel[p, h:], nodes[o, :h], nodes[o, h:]
    return ((sr * rr - si * ri) * orr + (sr * ri + si * rr) * oi).sum(-1)


def query_vectors(batch, head, nodes, rel):
    """float64 [Q, d]: qv with scores[q, n] = qv[q] . nodes[n] -- tail z = a r, head z = conj(r) a, as [Re z | Im z]"""
    s, p, o = (torch.as_tensor(batch[:, k]).long() for k in range(3))
    zn, zr = cplx(nodes), cplx(rel)
    return halves(zr[p].conj() * zn[o] if head else zn[s] * zr[p])


def make_case(N, Q, d, biased, storage="fp32", integer=False, seed=0):
    """host arrays of one case (nodes [N, d], rel [R0, d], three biases or Nones, triples [Q, 3]); bf16 storage: the table rounded to
    bf16; integer: entries in [-2, 2], biases in [-1, 1] -- every product and sum is then an integer far below 2^24"""
    rng = np.random.default_rng(100000 * seed + 1000 * N + 10 * Q + d + int(biased))
    if integer:
        nodes = rng.integers(-2, 3, (N, d)).astype(np.float32)
        rel = rng.integers(-2, 3, (R0, d)).astype(np.float32)
        bias = [rng.integers(-1, 2, n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    else:
        nodes = rng.standard_normal((N, d)).astype(np.float32)
        rel = rng.standard_normal((R0, d)).astype(np.float32)
        bias = [rng.standard_normal(n).astype(np.float32) for n in (N, R0, N)] if biased else [None] * 3
    if storage == "bf16":
        nodes = torch.from_numpy(nodes).to(torch.bfloat16).float().numpy()
    triples = np.stack([rng.integers(0, N, Q), rng.integers(0, R0, Q), rng.integers(0, N, Q)], 1)
    return rng, nodes, rel, bias, triples


def rel_err(got, want):
    """(max |got - want|, max |want|) in float64"""
    if torch.is_tensor(got):
        got = got.detach().float().cpu().numpy()
    if torch.is_tensor(want):
        want = want.detach().cpu().numpy()
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want).max(initial=0.0), np.abs(want).max(initial=0.0)


def close(got, want, what, bound=1e-4, floor=0.0):
    """max |got - want| <= bound * max |want|, the figure printed before it is asserted.  floor: a lower limit of the norm, for a
    reference that is zero up to its own rounding (the caller says what it cancels from)"""
    err, norm = rel_err(got, want)
    norm = max(norm, floor)
    print(f"[complex] {what}: max err {err:.3e}, norm {norm:.3e}, relative {err / norm if norm else 0.0:.3e} (bound {bound:.3e})")
    g = got.detach().float().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    assert np.isfinite(g).all(), what
    assert err <= bound * norm, (what, err, norm)


def equal(got, want, what):
    """exact equality with a float64 array of integers"""
    if torch.is_tensor(got):
        got = got.detach().float().cpu().numpy()
    if torch.is_tensor(want):
        want = want.detach().cpu().numpy()
    want = np.asarray(want, np.float64)
    assert np.array_equal(want, np.round(want)) and np.abs(want).max(initial=0.0) < 2 ** 24, what
    assert np.array_equal(np.asarray(got, np.float64), want), (what, np.abs(np.asarray(got, np.float64) - want).max())
