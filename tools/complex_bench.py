"""ComplEx next to DistMult at WN18 size -- N = 40,943 entities, d = 200 (100 complex features), 5,000 queries per launch
of the all-candidate calls, 330,000 triples for the triple decoder --, fp32 and bf16 tables, one process.  Per call the two decoders
ALTERNATE launch by launch; the measurement is repeated five times and the median of the five medians is reported with their spread:

  score_all          functional.distmult_score_all into a reused [Q, N] buffer (the evaluator's launch)
  rank_all           functional.distmult_rank_all (the fused ranks)
  softmax_forward    functional.distmult_softmax_loss, reduction="none", nothing requires grad
  softmax_step       the same, mean, forward + backward (bf16: the native route)
  bce_step           functional.distmult_bce_loss / complex_bce_loss, forward + backward
  triples_step       functional.distmult_score / complex_score on the triples, forward + backward

Two readings, no threshold in either.  (b) complex_over_distmult per call.  (a) DistMult must not have paid for the query-form code: the
DistMult calls alone (--distmult-only: no ComplEx name is touched, so the mode also runs on a tree from before ComplEx, --tree DIR) are
measured on the parent commit's build before and after this one's in the same session; --parent A.json B.json --this C.json attach the
three files, and the figures to read are this_over_parent per call against parent_run_to_run, the spread between the parent's two runs.

    python tools/complex_bench.py [--steps 10 --warmup 3 --out DIR]        -> DIR/complex_bench_<csrc_sha>.json (DIR: profiles/)
    python tools/complex_bench.py --distmult-only [--tree DIR] --json FILE  -> FILE
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--out", default=None)
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose torch_rgcn is measured")
ap.add_argument("--distmult-only", action="store_true")
ap.add_argument("--json", default=None, help="--distmult-only: where the result goes")
ap.add_argument("--parent", nargs=2, default=None, metavar=("A.json", "B.json"))
ap.add_argument("--this", default=None, metavar="C.json")
ARGS = ap.parse_args() if __name__ == "__main__" else ap.parse_args([])
ROOT = os.path.abspath(ARGS.tree)
for p in (ROOT, os.path.join(ROOT, "torch-rgcn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"
N, D, Q, T, R0 = 40_943, 200, 5_000, 330_000, 18


def alternate(variants, steps, warmup):
    """{name: callable} -> {name: median ms}, the variants taking turns launch by launch"""
    for run in variants.values():
        for _ in range(warmup):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(steps):
        for k, run in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: statistics.median(t) for k, t in times.items()}


def repeated(variants, steps, warmup, repeats):
    medians = {k: [] for k in variants}
    for r in range(repeats):
        one = alternate(variants, steps, warmup if r == 0 else 1)
        for k in variants:
            medians[k].append(round(one[k], 4))
    res = {k: {"ms_medians": m, "ms_median": round(statistics.median(m), 4), "ms_spread": [min(m), max(m)]} for k, m in medians.items()}
    if "complex" in res:
        res["complex_over_distmult"] = round(res["complex"]["ms_median"] / res["distmult"]["ms_median"], 4)
    return res


def calls(storage, decoders):
    """{call: {decoder: callable}} on one case; decoders without "complex" touch no ComplEx name"""
    from torch_rgcn import _native, functional
    torch.manual_seed(0)
    nodes = torch.randn(N, D, device=DEV) * D ** -0.25            # scores of unit scale
    rel = (torch.randn(R0, D, device=DEV) * D ** -0.25).requires_grad_(True)
    nt = (nodes if storage == "fp32" else nodes.to(torch.bfloat16)).requires_grad_(True)
    nd, rd = nt.detach(), rel.detach()
    batch = torch.from_numpy(_native.synthetic_triples_host(N, R0, Q, 5)).to(DEV)
    triples = torch.from_numpy(_native.synthetic_triples_host(N, R0, T, 7)).to(DEV)
    buf = torch.empty(Q, N, device=DEV)
    gs = torch.randn(T, device=DEV)
    native = {} if storage == "fp32" else {"bf16_backward": "native"}
    out = {}

    def step(fn, *a, **kw):
        def run():
            nt.grad = rel.grad = None
            loss = fn(*a, **kw)
            loss.backward(gradient=functional.unit_gradient(loss.device))
        return run

    def triples_step(score):
        def run():
            nt.grad = rel.grad = None
            score(triples, nt, rel).backward(gs)
        return run
    for dec in decoders:
        kw = {} if dec == "distmult" else {"decoder": "complex"}
        bce = functional.distmult_bce_loss if dec == "distmult" else functional.complex_bce_loss
        score = functional.distmult_score if dec == "distmult" else functional.complex_score
        for name, run in (("score_all", lambda kw=kw: functional.distmult_score_all(batch, False, nd, rd, out=buf, **kw)),
                          ("rank_all", lambda kw=kw: functional.distmult_rank_all(batch, False, nd, rd, **kw)),
                          ("softmax_forward", lambda kw=kw: functional.distmult_softmax_loss(batch, False, nd, rd, reduction="none", **kw)),
                          ("softmax_step", step(functional.distmult_softmax_loss, batch, False, nt, rel, **native, **kw)),
                          ("bce_step", step(bce, batch, False, nt, rel, **native)),
                          ("triples_step", triples_step(score))):
            out.setdefault(name, {})[dec] = run
    return out


def measure(decoders, steps, warmup, repeats):
    res = {}
    for storage in ("fp32", "bf16"):
        res[storage] = {name: repeated(variants, steps, warmup, repeats) for name, variants in calls(storage, decoders).items()}
        print(json.dumps({storage: res[storage]}), flush=True)
        torch.cuda.empty_cache()
    return res


def against_parent(parent_files, this_file):
    """(a): per storage and call, this build's DistMult median over the parent's (the mean of its two runs' medians), beside the spread
    between the parent's two runs"""
    a, b = (json.load(open(f)) for f in parent_files)
    c = json.load(open(this_file))
    out = {"parent_csrc_sha": a["csrc_sha"], "this_csrc_sha": c["csrc_sha"], "calls": {}}
    for storage in ("fp32", "bf16"):
        for name in a["distmult"][storage]:
            pa, pb = (x["distmult"][storage][name]["distmult"]["ms_median"] for x in (a, b))
            mine = c["distmult"][storage][name]["distmult"]["ms_median"]
            out["calls"][f"{storage}/{name}"] = {"parent_ms": [pa, pb], "this_ms": mine, "parent_run_to_run": round(abs(pa - pb) / min(pa, pb), 4),
                                                 "this_over_parent": round(mine / ((pa + pb) / 2), 4)}
    return out


def main():
    if not torch.cuda.is_available():
        raise SystemExit("complex_bench: needs the GPU (no CPU fallback)")
    from torch_rgcn import _native
    out = {"tool": "tools/complex_bench.py", "csrc_sha": _native.csrc_sha(), "tree": "this" if ARGS.tree == ap.get_default("tree") else "other",
           "steps": ARGS.steps, "warmup": ARGS.warmup, "repeats": ARGS.repeats, "device": torch.cuda.get_device_name(0),
           "shape": {"N": N, "d": D, "Q": Q, "T": T, "relations": R0}}
    if ARGS.distmult_only:
        out["distmult"] = measure(("distmult",), ARGS.steps, ARGS.warmup, ARGS.repeats)
        path = ARGS.json or "complex_bench_distmult_only.json"
    else:
        out["both"] = measure(("distmult", "complex"), ARGS.steps, ARGS.warmup, ARGS.repeats)
        if ARGS.parent and ARGS.this:
            out["distmult_against_parent"] = against_parent(ARGS.parent, ARGS.this)
        folder = ARGS.out or os.path.join(ROOT, "profiles")
        os.makedirs(folder, exist_ok=True)
        path = os.path.join(folder, f"complex_bench_{_native.csrc_sha()}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
