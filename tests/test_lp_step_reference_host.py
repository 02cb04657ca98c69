"""The float64 reference of the link-prediction step (tests/lp_step_reference.py) checked before a GPU is compared with it: its LP layer
against oracle.lp_layer and the g2_lp_* golden layers, its DistMult against g5_distmult, its ComplEx cells against complex_reference, the
gradient of every committed step against central differences, and the conditions the GPU test relies on -- every ReLU input away from
zero, queries that share a key.  CPU only."""
import glob
import os

import numpy as np
import pytest
import torch

import complex_reference as cr
import lp_step_reference as ref
from conftest import GOLDEN, load_golden
from oracle import oracle

F64 = torch.float64
G2 = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "g2_lp_*.npz")))
FP32_CASES = [n for n, c in ref.CASES.items() if c["storage"] == "fp32"]


def layer_with_grads(T, N, R0, X, params, bias, g, keep=None, vertical=False):
    """the reference's layer and the gradients of <out, g> -> dict(out, dX, db, grads)"""
    P = ref.leaves(params)
    Xt = torch.tensor(np.asarray(X), dtype=F64, requires_grad=True)
    bt = None if bias is None else torch.tensor(np.asarray(bias), dtype=F64, requires_grad=True)
    out = ref.lp_layer(ref.messages(T, N, R0, keep, vertical), Xt, ref.dense_weights(P), bt)
    wrt = [Xt] + list(P.values()) + ([] if bt is None else [bt])
    grads = torch.autograd.grad(out, wrt, grad_outputs=torch.as_tensor(np.asarray(g), dtype=F64))
    res = dict(out=out.detach().numpy(), dX=grads[0].numpy(), grads={k: v.numpy() for k, v in zip(P, grads[1:])})
    if bt is not None:
        res["db"] = grads[-1].numpy()
    return res


def same_layer(mine, theirs, bound):
    assert ref.rel_dist(theirs["out"], mine["out"]) < bound and ref.rel_dist(theirs["dX"], mine["dX"]) < bound
    assert ref.rel_dist(theirs["db"], mine["db"]) < bound
    assert set(mine["grads"]) == set(theirs["grads"])
    for k, v in theirs["grads"].items():
        assert ref.rel_dist(v, mine["grads"][k]) < bound, k


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", ["none", "basis", "block"])
def test_layer_equals_the_oracle_layer(mode, masked):
    """out, dX, db and every parameter gradient: the oracle returns fp32 (double sums rounded once), hence 1e-6"""
    N, R0, E, d_in, d_out = 40, 3, 200, 12, 8
    R = 2 * R0 + 1
    rng = np.random.default_rng(11)
    T = oracle.synthetic_triples(N, R0, E, seed=4)
    f32 = lambda *shape: rng.standard_normal(shape).astype(np.float32)     # noqa: E731
    params = {"none": {"weights": f32(R, d_in, d_out)}, "basis": {"bases": f32(2, d_in, d_out), "comps": f32(R, 2)},
              "block": {"blocks": f32(R - 1, 4, d_in // 4, d_out // 4), "blocks_self": f32(d_in, d_out)}}[mode]
    X, bias, g = f32(N, d_in), f32(d_out), f32(N, d_out)
    keep = (rng.random(N) < 0.7).astype(np.uint8) if masked else None
    theirs = oracle.lp_layer(T, N, R, X, params, mode, bias, False, keep, g)
    same_layer(layer_with_grads(T, N, R0, X, params, bias, g, keep), theirs, 1e-6)


@pytest.mark.parametrize("name", G2)
def test_layer_reproduces_the_golden_layers(name):
    """the layers the upstream project itself computed (fp32), at the bound test_oracle_golden.py holds the oracle to"""
    d = load_golden(name)
    N, R0 = int(d["num_nodes"]), int(d["num_rels"])
    params = {k[len("param_"):]: v for k, v in d.items() if k.startswith("param_")}
    bias = params.pop("bias", None)
    mine = layer_with_grads(d["triples"], N, R0, d["X"], params, bias, d["g"], None, bool(d["vertical"]))
    assert ref.rel_dist(mine["out"], d["out"]) < 2e-5 and ref.rel_dist(mine["dX"], d["grad_X"]) < 2e-5
    if bias is not None:
        assert ref.rel_dist(mine["db"], d["grad_bias"]) < 2e-5
    assert set(mine["grads"]) == {k[5:] for k in d if k.startswith("grad_")} - {"X", "bias"}
    for k, v in mine["grads"].items():
        assert ref.rel_dist(v, d["grad_" + k]) < 2e-5, k


def test_distmult_reproduces_the_golden_decoder():
    d = load_golden("g5_distmult")
    for tag in ("nb", "b"):
        names = ("relations", "sbias", "pbias", "obias") if tag == "b" else ("relations",)
        for nm in ("2", "3"):
            nodes = torch.tensor(d["nodes"], dtype=F64, requires_grad=True)
            P = {k: torch.tensor(d[f"{tag}_param_{k}"], dtype=F64, requires_grad=True) for k in names}
            bias = tuple(P.get(k) for k in ("sbias", "pbias", "obias"))
            sc = ref.triple_scores(d["triples" + nm], nodes, P["relations"], bias, "distmult")
            assert ref.rel_dist(sc.detach().numpy(), d[f"{tag}_scores{nm}"]) < 2e-5
            grads = torch.autograd.grad(sc, [nodes] + list(P.values()), grad_outputs=torch.as_tensor(d[f"{tag}_g{nm}"], dtype=F64))
            for k, g in zip(("nodes",) + names, grads):
                assert ref.rel_dist(g.numpy(), d[f"{tag}_grad_{k}{nm}"]) < 2e-5, (tag, nm, k)


@pytest.mark.parametrize("decoder", ["distmult", "complex"])
def test_all_candidate_cells_are_the_triple_scores(decoder):
    """ComplEx: all_scores IS complex_reference.all_scores; both decoders: the cell (q, n) is the score of the query with n put in"""
    rng = np.random.default_rng(3)
    n, d, q = 23, 6, 9
    x, rel = cr.f64(rng.standard_normal((n, d))), cr.f64(rng.standard_normal((ref.R0, d)))
    bias = tuple(cr.f64(rng.standard_normal(k)) for k in (n, ref.R0, n))
    batch = np.stack([rng.integers(0, n, q), rng.integers(0, ref.R0, q), rng.integers(0, n, q)], 1)
    for b in (bias, (None, None, None)):
        for head in (True, False):
            cells = ref.all_scores(batch, head, x, rel, b, decoder)
            if decoder == "complex":
                assert torch.equal(cells, cr.all_scores(batch, head, x, rel, b))
            every = np.repeat(batch[:, None, :], n, axis=1)
            every[:, :, 0 if head else 2] = np.arange(n)[None, :]
            assert ref.rel_dist(cells.numpy(), ref.triple_scores(every, x, rel, b, decoder).numpy()) < 1e-13


def test_gathered_penalty_counts_every_occurrence():
    """three rows, one of them gathered twice: the mean of squares by hand"""
    x = cr.f64([[1.0, 2.0], [3.0, 0.0], [0.0, 1.0]])
    rel = cr.f64([[2.0, 2.0], [1.0, 0.0]])
    batch = np.array([[0, 1, 2], [0, 0, 1]])
    want = (5 + 5) / 4 + (1 + 8) / 4 + (1 + 9) / 4
    assert abs(ref.gathered_penalty(batch, x, rel).item() - want) < 1e-15


@pytest.mark.parametrize("name", list(ref.CASES))
def test_every_relu_input_is_away_from_zero(name):
    """the condition under which a sign cannot legitimately differ on the GPU: fp32 cases 1e-5 of the tensor's maximum; bf16 cases one
    bf16 ulp of it, on the rounded evaluation.  Training mode "other": under the keep masks the GPU test's step draws (recorded)"""
    case = ref.CASES[name]
    for what, smallest, margin in ref.relu_margins(case, ref.case_inputs(case), ref.recorded_keeps(case)):
        print(f"[lp-step] {name}: ReLU '{what}' min |input| {smallest:.3e}, margin {margin:.3e}")
        assert smallest > margin, (name, what, smallest, margin)
    assert len(ref.relu_margins(case, ref.case_inputs(case))) == case["encoder"]["num_layers"]


@pytest.mark.parametrize("name", list(ref.CASES))
def test_the_inputs_reach_the_edges(name):
    """the graph has its hub and its duplicates, queries share keys (so the filter and the labels are not trivial), every bias is far
    from zero, and the parameter inventory is the config's"""
    case = ref.CASES[name]
    inp = ref.case_inputs(case)
    T, pos = inp["graph"], inp["positives"]
    assert T.shape == (ref.E, 3) and pos.shape == (ref.Q, 3)
    assert (T[:, 0] == 0).sum() >= ref.E // 4 and ref.E - len(np.unique(T, axis=0)) >= ref.E // 20
    assert ref.Q > 128 and ref.N > 256                                       # a second query tile, a third column tile
    known = ref.known_completions(T)
    for head in (True, False):
        cells = ref.known_cells(pos, known, head)
        tgt = torch.as_tensor(pos[:, 0 if head else 2])
        assert bool(cells[torch.arange(ref.Q), tgt].all())
        assert int(cells.sum()) - ref.Q >= 10, "known completions beside the targets"
        keys = [tuple(r) for r in (pos[:, 1:] if head else pos[:, :2]).tolist()]
        assert len(set(keys)) < len(keys), "no two queries share a key"
    for k, v in inp["params"].items():
        assert v.shape == ref.param_shapes(case)[k]
        if "bias" in k:
            assert np.abs(v).max() > 0.1, k
    if case["storage"] == "bf16":
        assert all(np.array_equal(v, ref.bf16_values(v)) for v in inp["params"].values())
    if inp["labels"] is not None:
        assert inp["batch"].shape == (ref.Q * (1 + ref.RATE), 3) and inp["labels"].sum() == ref.Q


def test_the_table_holds_every_listed_value():
    cases = list(ref.CASES.values())
    fp32 = [c for c in cases if c["storage"] == "fp32"]
    kind = lambda c: "c-rgcn" if c["encoder"]["model"] == "c-rgcn" else (c["encoder"].get("decomposition") or {}).get("type", "none")   # noqa: E731
    for objective in ("negative-sampling", "1-n", "1-n-bce"):
        mine = [c for c in fp32 if c["objective"] == objective]
        assert {kind(c) for c in mine} == {"none", "basis", "block", "c-rgcn"}
        assert {c["decoder"]["model"] for c in mine} == {"distmult", "complex"}
        assert any(c["decoder"].get("bias_init") for c in mine) and any(not c["decoder"].get("bias_init") for c in mine)
    ns = [c["decoder"] for c in fp32 if c["objective"] == "negative-sampling"]
    assert {(d["l2_penalty_type"], d["l2_penalty"] > 0) for d in ns} >= {("schlichtkrull-l2", True), ("plain-l2", True)}
    assert any(d["l2_penalty"] == 0.0 for d in ns)
    assert {(c["filtered"], c["eps"]) for c in fp32 if c["objective"] == "1-n"} == {(False, 0.0), (True, 0.0), (True, 0.1)}
    assert {c["eps"] for c in fp32 if c["objective"] == "1-n-bce"} == {0.0, 0.1}
    assert {c["encoder"]["num_layers"] for c in fp32} == {1, 2} and {c["mode"] for c in fp32} == {"eval", "other", "sd"}
    assert all(kind(c) == "basis" for c in fp32 if c["mode"] == "sd")
    assert {c["encoder"]["hidden1_size"] for c in fp32} == {16, 32, 50}
    bf16 = {(c["objective"], c["filtered"], c["eps"]) for c in cases if c["storage"] == "bf16"}
    assert bf16 == {("1-n", False, 0.0), ("1-n", True, 0.1), ("1-n-bce", False, 0.1)}


@pytest.mark.parametrize("name", FP32_CASES)
def test_gradient_agrees_with_central_differences(name):
    """d/dt loss(P + t D) at t = 0 from autograd against (loss(P + h D) - loss(P - h D)) / 2h, h = 1e-5, along three seeded random
    directions D of the joint parameter space (every entry a standard normal times its parameter's scale): 1e-6 relative.  In float64
    the difference's rounding error is ~1e-16 loss / h = 1e-11 and its truncation error h^2 / 6 times a third derivative"""
    case = ref.CASES[name]
    inp = ref.case_inputs(case)
    keeps = ref.recorded_keeps(case)
    _, grads = ref.loss_and_grads(case, inp, keeps)
    rng = np.random.default_rng(5)
    h = 1e-5
    for k in range(3):
        D = {n: rng.standard_normal(v.shape) * ref._scale(n, v.shape) for n, v in inp["params"].items()}
        want = sum(float((grads[n] * D[n]).sum()) for n in D)
        ends = []
        for sign in (1.0, -1.0):
            with torch.no_grad():
                P = {n: torch.as_tensor(v + sign * h * D[n], dtype=F64) for n, v in inp["params"].items()}
                ends.append(ref.step_loss(case, inp, P, keeps).item())
        got = (ends[0] - ends[1]) / (2 * h)
        print(f"[lp-step] {name} direction {k}: autograd {want:.9e}, central difference {got:.9e}, relative {abs(got - want) / abs(want):.2e}")
        assert abs(got - want) <= 1e-6 * abs(want), (name, k, got, want)
