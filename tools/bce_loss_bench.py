"""1-N multi-label BCE loss of DistMult: functional.distmult_bce_loss -- fused softplus sums forward, chunked backward,
no [Q, N] logits and no [Q, N] labels -- timed per launch of 5,000 queries at d = 200, one process.

  wn18     N = 40,943 and
  million  N = 1,000,000, each with an fp32 table and a bf16 one (native route): the forward and forward + backward of the new call, its
           labels in a FilterIndex of 150,000 synthetic known triples plus the batch and label_smoothing 0.1, against the UNSMOOTHED,
           unfiltered 1-N softmax call (functional.distmult_softmax_loss) on the same inputs -- the same product, one transcendental
           fewer per cell, no mask.  The two ALTERNATE launch by launch; the measurement is repeated five times and the median of the
           five medians is reported with their spread, plus the per-kernel times of one launch of each and the peak memory of each.
  dense    at WN18 size, fp32 only: distmult_score_all + a dense [Q, N] label matrix + ATen binary_cross_entropy_with_logits (forward),
           and the ATen autograd step (nodes[s] * rel[p]) @ nodes.T -> binary_cross_entropy_with_logits (forward + backward), with the
           peak memory of both routes -- at a million entities the logits alone would be 20 GB.
No figure is a threshold.  What is checked is that the peak of the fused route stays under the chunk budget plus the tables: it does not
grow with Q * N * 4 (peak_bytes against logits_bytes, and the 64 MiB-chunk variant at WN18 size).

    python tools/bce_loss_bench.py [--steps 10 --warmup 3 --out DIR]   -> DIR/bce_loss_bench_<csrc_sha>.json (DIR: profiles/)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-rgcn_amd"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from softmax_loss_bench import DEV, alternate, case, kernels_of, peak_of  # noqa: E402

EPS = 0.1
KNOWN = 150_000


def known_index(N, batch, R0=18):
    """-> (FilterIndex, the true-triple dictionaries) of KNOWN synthetic triples and the batch itself"""
    from torch_rgcn import _native
    from torch_rgcn.functional import FilterIndex
    from utils.misc import generate_true_dict
    known = np.concatenate([_native.synthetic_triples_host(N, R0, KNOWN, 11), batch.cpu().numpy()])
    true = generate_true_dict(known)
    return FilterIndex(true, N, DEV), true


def repeated(variants, steps, warmup, repeats):
    """alternate() `repeats` times -> {name: {ms_medians, ms_median (of the medians), ms_spread, kernels_ms, peak_bytes}}"""
    medians = {k: [] for k in variants}
    for r in range(repeats):
        one = alternate(variants, steps, warmup if r == 0 else 1)
        for k in variants:
            medians[k].append(one[k]["ms_median"])
    return {k: {"ms_medians": m, "ms_median": round(statistics.median(m), 4), "ms_spread": [min(m), max(m)]} for k, m in medians.items()}


def fused_leg(N, steps, warmup, repeats=5):
    from torch_rgcn import functional
    nodes, rel, batch = case(N)
    index, _ = known_index(N, batch)
    Q = batch.shape[0]
    res = {"shape": {"N": N, "d": nodes.shape[1], "Q": Q}, "label_smoothing": EPS, "repeats": repeats, "logits_bytes": 4 * Q * N,
           "chunks": len(functional.softmax_chunk_plan(Q, N, functional.SOFTMAX_CHUNK_BYTES))}
    for storage in ("fp32", "bf16"):
        nt = nodes if storage == "fp32" else nodes.detach().to(torch.bfloat16).requires_grad_(True)
        nd, rd = nt.detach(), rel.detach()
        kw = {} if storage == "fp32" else {"bf16_backward": "native"}

        def step_of(loss_fn, **more):
            def run():
                nt.grad = rel.grad = None
                loss = loss_fn(batch, False, nt, rel, **kw, **more)
                loss.backward(gradient=functional.unit_gradient(loss.device))
                return loss
            return run
        legs = {"forward": {"bce": lambda: functional.distmult_bce_loss(batch, False, nd, rd, labels=index, reduction="none", label_smoothing=EPS),
                            "softmax": lambda: functional.distmult_softmax_loss(batch, False, nd, rd, reduction="none")},
                "forward_backward": {"bce": step_of(functional.distmult_bce_loss, labels=index, label_smoothing=EPS),
                                     "softmax": step_of(functional.distmult_softmax_loss)}}
        res[storage] = {}
        for what, variants in legs.items():
            leg = repeated(variants, steps, warmup, repeats)
            for k, run in variants.items():
                leg[k]["kernels_ms"] = kernels_of(run)
                leg[k]["peak_bytes"] = peak_of(run)
            leg["bce_over_softmax"] = round(leg["bce"]["ms_median"] / leg["softmax"]["ms_median"], 4)
            res[storage][what] = leg
        if N < 100_000:                  # the backward's buffer follows the chunk budget, not Q * N * 4
            small = step_of(functional.distmult_bce_loss, labels=index, label_smoothing=EPS, chunk_bytes=64 << 20)
            res[storage]["forward_backward"]["bce_chunks_64MiB"] = {"peak_bytes": peak_of(small),
                                                                    "chunks": len(functional.softmax_chunk_plan(Q, N, 64 << 20))}
        res[storage]["loss"] = {k: float(run().detach()) for k, run in legs["forward_backward"].items()}
        nt.grad = rel.grad = None
    return res


def dense_leg(N, steps, warmup):
    """the route a user has without the fused call, fp32 at WN18 size: [Q, N] logits and [Q, N] labels"""
    from torch_rgcn import _native, functional
    nodes, rel, batch = case(N)
    index, true = known_index(N, batch)
    nd, rd = nodes.detach(), rel.detach()
    Q = batch.shape[0]
    bt = batch.cpu().numpy()
    cells = [(q, n) for q, (s, p, o) in enumerate(bt) for n in true[1].get((int(s), int(p)), ())]
    lq, ln = (torch.tensor(x, device=DEV, dtype=torch.long) for x in zip(*cells))

    def labels():
        y = torch.zeros(Q, N, device=DEV)
        y[lq, ln] = 1.0
        y[torch.arange(Q, device=DEV), batch[:, 2]] = 1.0
        return y * (1.0 - EPS) + EPS / N

    def dense_forward():
        return torch.nn.functional.binary_cross_entropy_with_logits(_native.distmult_score_all(batch, False, nd, rd), labels())

    def dense_step():
        nodes.grad = rel.grad = None
        logits = (nodes[batch[:, 0]] * rel[batch[:, 1]]) @ nodes.t()
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels())
        loss.backward()
        return loss

    def fused_step():
        nodes.grad = rel.grad = None
        loss = functional.distmult_bce_loss(batch, False, nodes, rel, labels=index, label_smoothing=EPS)
        loss.backward(gradient=functional.unit_gradient(loss.device))
        return loss
    legs = {"forward": {"fused": lambda: functional.distmult_bce_loss(batch, False, nd, rd, labels=index, label_smoothing=EPS),
                        "score_all_dense_labels_aten_bce": dense_forward},
            "forward_backward": {"fused": fused_step, "aten_matmul_dense_labels_bce": dense_step}}
    res = {"shape": {"N": N, "d": nodes.shape[1], "Q": Q}, "logits_bytes": 4 * Q * N, "labels_bytes": 4 * Q * N}
    for what, variants in legs.items():
        res[what] = alternate(variants, steps, warmup)
        for k, run in variants.items():
            res[what][k]["peak_bytes"] = peak_of(run)
    res["loss"] = {"fused": float(fused_step().detach())}
    g = nodes.grad.clone()
    res["loss"]["aten"] = float(dense_step().detach())
    res["dnodes_max_abs_difference_over_max"] = float((g - nodes.grad).abs().max() / nodes.grad.abs().max())
    nodes.grad = rel.grad = None
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--skip-million", action="store_true")
    ap.add_argument("--wn18-n", type=int, default=40_943)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bce_loss_bench: needs the GPU (no CPU fallback)")
    from torch_rgcn import _native
    out = {"tool": "tools/bce_loss_bench.py", "csrc_sha": _native.csrc_sha(), "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    out["wn18"] = fused_leg(args.wn18_n, args.steps, args.warmup)
    print(json.dumps({"wn18": out["wn18"]}), flush=True)
    out["dense"] = dense_leg(args.wn18_n, args.steps, args.warmup)
    print(json.dumps({"dense": out["dense"]}), flush=True)
    if not args.skip_million:
        steps = max(3, args.steps // 2)
        out["million"] = dict(fused_leg(1_000_000, steps, max(1, args.warmup // 2)), steps=steps)
        print(json.dumps({"million": out["million"]}), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"bce_loss_bench_{_native.csrc_sha()}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
