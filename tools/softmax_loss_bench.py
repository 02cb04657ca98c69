"""1-N softmax loss of DistMult: functional.distmult_softmax_loss -- fused log-sum-exp forward, chunked backward, no
[Q, N] logits -- timed per launch of 5,000 queries at d = 200, one process.

  wn18     N = 40,943.  Forward: the fused route against distmult_score_all + torch.logsumexp (the [Q, N] scores written and read back).
           Forward + backward: the fused route (default chunk budget, and 64 MiB chunks) against an ATen autograd step
           (nodes[s] * rel[p]) @ nodes.T -> F.cross_entropy, which holds the logits and their gradient.
  million  N = 1,000,000: the fused route alone (the logits would be 20 GB, with their gradient 40 GB).
  bf16     at both sizes, the table of the case rounded to bf16 and trained: forward + backward on the upcast route (the table widened
           to fp32, the fp32 kernels: the only route before bf16_backward existed) against the native route (bf16_backward="native"),
           with the bytes each holds between its forward and its backward.
The variants of a group ALTERNATE launch by launch (a drift of the shared host hits all alike); HIP events; median, minimum and quartiles
of --steps after --warmup.  Peak memory: the rise of torch.cuda.max_memory_allocated over one call of each variant from an emptied
cache.  No figure is a threshold: the fused forward recomputes nothing but writes nothing either, the fused backward computes the
product a second time -- what is bought is memory.

  --smooth EPS  the label-smoothing leg INSTEAD of the above: at both sizes, fp32 and bf16 (native route), the forward and forward +
           backward with label_smoothing=EPS against the same call without it, the two alternating launch by launch; the measurement is
           repeated five times and the median of the five medians is reported with their spread (min .. max), plus the per-kernel times
           of one launch of each (lse_fused against lse_smooth, softmax_grad against softmax_grad_smooth).

    python tools/softmax_loss_bench.py [--steps 10 --warmup 3 --out DIR]   -> DIR/softmax_loss_bench_<csrc_sha>.json (DIR: profiles/)
    python tools/softmax_loss_bench.py --smooth 0.1 [...]                  -> DIR/softmax_loss_smooth_bench_<csrc_sha>.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-rgcn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"


def alternate(variants, steps, warmup):
    """{name: callable} -> {name: {ms_median, ms_min, ms_q1, ms_q3}}, the variants taking turns"""
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
    res = {}
    for k, t in times.items():
        q = statistics.quantiles(t, n=4)
        res[k] = {"ms_median": round(statistics.median(t), 4), "ms_min": round(min(t), 4), "ms_q1": round(q[0], 4), "ms_q3": round(q[2], 4)}
    return res


def peak_of(run):
    """bytes by which one call raises the allocator's peak, from an emptied cache"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    run()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def kernels_of(run):
    from torch_rgcn import _native
    _native.profile_start()
    run()
    torch.cuda.synchronize()
    return {t: round(sum(v), 4) for t, v in sorted(_native.profile_stop().items())}


def measure(variants, steps, warmup):
    res = alternate(variants, steps, warmup)
    for k, run in variants.items():
        res[k]["peak_bytes"] = peak_of(run)
    return res


def case(N, R0=18, d=200, Q=5000):
    from torch_rgcn import _native
    torch.manual_seed(0)
    nodes = (torch.randn(N, d, device=DEV) * d ** -0.25).requires_grad_(True)      # scores of unit scale: a loss a trained model could have
    rel = (torch.randn(R0, d, device=DEV) * d ** -0.25).requires_grad_(True)
    batch = torch.from_numpy(_native.synthetic_triples_host(N, R0, Q, 5)).to(DEV)
    return nodes, rel, batch


def fused_step(nodes, rel, batch, chunk_bytes=None):
    from torch_rgcn import functional

    def run():
        nodes.grad = rel.grad = None
        loss = functional.distmult_softmax_loss(batch, False, nodes, rel, chunk_bytes=chunk_bytes)
        loss.backward(gradient=functional.unit_gradient(loss.device))
        return loss
    return run


def bf16_leg(nodes, rel, batch, steps, warmup):
    """forward + backward of the bf16 table on both routes of bf16_backward: times, peak memory, the bytes held between the forward and
    the backward, per-kernel times (softmax_grad / softmax_grad_bf16 among them), and how far the two routes' results are apart"""
    from torch_rgcn import functional
    nb = nodes.detach().to(torch.bfloat16).requires_grad_(True)

    def step_of(route):
        def run():
            nb.grad = rel.grad = None
            loss = functional.distmult_softmax_loss(batch, False, nb, rel, bf16_backward=route)
            loss.backward(gradient=functional.unit_gradient(loss.device))
            return loss
        return run

    def held_of(route):
        nb.grad = rel.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        loss = functional.distmult_softmax_loss(batch, False, nb, rel, bf16_backward=route)
        torch.cuda.synchronize()
        held = int(torch.cuda.memory_allocated() - before)
        del loss
        return held
    step = {route: step_of(route) for route in ("upcast", "native")}
    res = measure(step, steps, warmup)
    out = {}
    for route, run in step.items():
        res[route]["held_between_forward_and_backward_bytes"] = held_of(route)
        res[route]["kernels_ms"] = kernels_of(run)
        out[route] = (float(run().detach()), nb.grad.float().clone())
    res["fp32_table_bytes"] = 4 * nodes.numel()
    res["loss"] = {route: out[route][0] for route in out}
    res["dnodes_max_abs_difference_over_max"] = float((out["native"][1] - out["upcast"][1]).abs().max() / out["upcast"][1].abs().max())
    res["native_step_over_upcast"] = round(res["native"]["ms_median"] / res["upcast"]["ms_median"], 3)
    return res


def smooth_leg(N, eps, steps, warmup, repeats=5):
    """smoothed against unsmoothed at one size: {storage: {forward | forward_backward: {plain | smoothed: medians of `repeats`
    alternating measurements, their median and spread, kernels_ms}, smoothed_over_plain}}"""
    from torch_rgcn import functional
    nodes, rel, batch = case(N)
    res = {"shape": {"N": N, "d": nodes.shape[1], "Q": batch.shape[0]}, "label_smoothing": eps, "repeats": repeats}
    for storage in ("fp32", "bf16"):
        nt = nodes if storage == "fp32" else nodes.detach().to(torch.bfloat16).requires_grad_(True)
        nd, rd = nt.detach(), rel.detach()
        kw = {} if storage == "fp32" else {"bf16_backward": "native"}

        def fwd_of(e):
            return lambda: functional.distmult_softmax_loss(batch, False, nd, rd, reduction="none", label_smoothing=e)

        def step_of(e):
            def run():
                nt.grad = rel.grad = None
                loss = functional.distmult_softmax_loss(batch, False, nt, rel, label_smoothing=e, **kw)
                loss.backward(gradient=functional.unit_gradient(loss.device))
                return loss
            return run
        res[storage] = {}
        for what, make in (("forward", fwd_of), ("forward_backward", step_of)):
            variants = {"plain": make(0.0), "smoothed": make(eps)}
            medians = {k: [] for k in variants}
            for r in range(repeats):
                one = alternate(variants, steps, warmup if r == 0 else 1)
                for k in variants:
                    medians[k].append(one[k]["ms_median"])
            leg = {k: {"ms_medians": m, "ms_median": round(statistics.median(m), 4), "ms_spread": [min(m), max(m)],
                       "kernels_ms": kernels_of(variants[k])} for k, m in medians.items()}
            leg["smoothed_over_plain"] = round(leg["smoothed"]["ms_median"] / leg["plain"]["ms_median"], 4)
            res[storage][what] = leg
        res[storage]["loss"] = {"plain": float(step_of(0.0)().detach()), "smoothed": float(step_of(eps)().detach())}
        nt.grad = rel.grad = None
    return res


def aten_step(nodes, rel, batch):
    def run():
        nodes.grad = rel.grad = None
        logits = (nodes[batch[:, 0]] * rel[batch[:, 1]]) @ nodes.t()
        loss = torch.nn.functional.cross_entropy(logits, batch[:, 2])
        loss.backward()
        return loss
    return run


def wn18(steps, warmup, N=40_943):
    from torch_rgcn import _native, functional
    nodes, rel, batch = case(N)
    nd, rd = nodes.detach(), rel.detach()
    res = {"shape": {"N": N, "d": nodes.shape[1], "Q": batch.shape[0]}, "logits_bytes": 4 * batch.shape[0] * N}
    fwd = {"fused": lambda: functional.distmult_softmax_loss(batch, False, nd, rd, reduction="none"),
           "score_all_logsumexp": lambda: torch.logsumexp(_native.distmult_score_all(batch, False, nd, rd), 1)}
    res["forward"] = measure(fwd, steps, warmup)
    res["forward"]["fused"]["kernels_ms"] = kernels_of(fwd["fused"])
    step = {"fused": fused_step(nodes, rel, batch), "fused_chunks_64MiB": fused_step(nodes, rel, batch, 64 << 20),
            "aten_matmul_cross_entropy": aten_step(nodes, rel, batch)}
    res["forward_backward"] = measure(step, steps, warmup)
    for k in ("fused", "fused_chunks_64MiB"):
        res["forward_backward"][k]["kernels_ms"] = kernels_of(step[k])
        res["forward_backward"][k]["chunks"] = len(functional.softmax_chunk_plan(batch.shape[0], N, (64 << 20) if "64" in k else functional.SOFTMAX_CHUNK_BYTES))
    # the two routes compute one loss and one gradient
    a, b = step["fused"](), step["aten_matmul_cross_entropy"]()
    res["loss"] = {"fused": float(a.detach()), "aten": float(b.detach())}
    step["fused"]()
    g_fused = nodes.grad.clone()
    step["aten_matmul_cross_entropy"]()
    res["dnodes_max_abs_difference_over_max"] = float((g_fused - nodes.grad).abs().max() / nodes.grad.abs().max())
    res["fused_forward_over_materialised"] = round(res["forward"]["fused"]["ms_median"] / res["forward"]["score_all_logsumexp"]["ms_median"], 3)
    res["fused_step_over_aten"] = round(res["forward_backward"]["fused"]["ms_median"] / res["forward_backward"]["aten_matmul_cross_entropy"]["ms_median"], 3)
    nodes.grad = rel.grad = None
    res["bf16"] = bf16_leg(nodes, rel, batch, steps, warmup)
    return res


def million(steps, warmup, N=1_000_000):
    from torch_rgcn import functional
    nodes, rel, batch = case(N)
    nd, rd = nodes.detach(), rel.detach()
    Q = batch.shape[0]
    res = {"shape": {"N": N, "d": nodes.shape[1], "Q": Q}, "logits_bytes": 4 * Q * N,
           "chunks": len(functional.softmax_chunk_plan(Q, N, functional.SOFTMAX_CHUNK_BYTES))}
    fwd = {"fused": lambda: functional.distmult_softmax_loss(batch, False, nd, rd, reduction="none")}
    res["forward"] = measure(fwd, steps, warmup)
    step = {"fused": fused_step(nodes, rel, batch)}
    res["forward_backward"] = measure(step, steps, warmup)
    res["forward_backward"]["fused"]["kernels_ms"] = kernels_of(step["fused"])
    res["loss"] = float(step["fused"]().detach())
    nodes.grad = rel.grad = None
    res["bf16"] = bf16_leg(nodes, rel, batch, steps, warmup)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--skip-million", action="store_true")
    ap.add_argument("--smooth", type=float, default=None, metavar="EPS", help="run the label-smoothing leg (smoothed against unsmoothed) instead")
    ap.add_argument("--wn18-n", type=int, default=40_943, help="entities of the WN18-sized case (a multiple of 4 gives the products 16-byte loads of dS)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("softmax_loss_bench: needs the GPU (no CPU fallback)")
    from torch_rgcn import _native
    out = {"tool": "tools/softmax_loss_bench.py", "csrc_sha": _native.csrc_sha(), "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    if args.smooth is not None:
        out["wn18"] = smooth_leg(args.wn18_n, args.smooth, args.steps, args.warmup)
        print(json.dumps({"wn18": out["wn18"]}), flush=True)
        if not args.skip_million:
            steps = max(3, args.steps // 2)
            out["million"] = dict(smooth_leg(1_000_000, args.smooth, steps, max(1, args.warmup // 2)), steps=steps)
            print(json.dumps({"million": out["million"]}), flush=True)
        os.makedirs(args.out, exist_ok=True)
        path = os.path.join(args.out, f"softmax_loss_smooth_bench_{_native.csrc_sha()}.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", path)
        return
    out["wn18"] = wn18(args.steps, args.warmup, args.wn18_n)
    print(json.dumps({"wn18": out["wn18"]}), flush=True)
    if not args.skip_million:
        steps, warmup = max(3, args.steps // 2), max(1, args.warmup // 2)          # 100 ms launches: half the launches
        out["million"] = dict(million(steps, warmup), steps=steps, warmup=warmup)
        print(json.dumps({"million": out["million"]}), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"softmax_loss_bench_{_native.csrc_sha()}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
