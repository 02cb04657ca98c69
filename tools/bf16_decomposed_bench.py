"""bf16 storage of block-diagonal and diagonal layers: fp32 against bf16 on the block / diagonal kernels against bf16 on the
dense-weight route the layers took before (block_path=0 / diag_path=0), in one process.

Workloads (one layer, forward + backward to X and every parameter, upstream gradient given):
  fb_lp_block_d500   FB15k-237-shaped LP layer: N = 14,541, R = 475, ~272 k triples, d = 500, 100 blocks of 5 x 5 (eval mode)
  am_block_d64       AM-shaped NC graph (N = 1,666,764, R = 267, 5,988,321 triples), d = 64, 8 blocks of 8 x 8
  am_block_d32       the same graph, d = 32, 8 blocks of 4 x 4
  am_diag_d32        the same graph, diagonal weights, d = 32
The three variants of a workload ALTERNATE step by step (other work shares the host: a drift hits all three alike); a step is timed with
HIP events; median, minimum and quartiles of --steps steps after --warmup.  Graph and plan builds fall into the warm-up.  On the FB-shaped
layer the peak allocated memory of one step of each bf16 route is recorded too (above what was allocated before the step).

    python tools/bf16_decomposed_bench.py [--steps 20 --warmup 5 --only NAME]   -> profiles/bf16_decomposed_bench_<csrc_sha>.json
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
BF = torch.bfloat16


def nc_workload(tp, N, R, d, decomposition=None, diag=False):
    from torch_rgcn import routes
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.manual_seed(0)
    layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=R, in_features=d, out_features=d, decomposition=decomposition,
                                         diag_weight_matrix=diag).to(DEV)
    X = torch.randn(N, d, device=DEV)
    G = torch.randn(N, d, device=DEV)
    off = {"diag_path": "0"} if diag else {"block_path": "0"}

    def step(x, g, **route):
        def run():
            x.grad = None
            layer.zero_grad(set_to_none=True)
            with routes.override(**route):
                layer(x).backward(g)
        return run
    x32, x16 = X.requires_grad_(True), X.detach().to(BF).requires_grad_(True)
    return {"fp32": step(x32, G), "bf16_new": step(x16, G.to(BF)), "bf16_parent_route": step(x16, G.to(BF), **off)}


def lp_workload(N, R0, E, d, nb):
    from torch_rgcn import _native, routes
    from torch_rgcn.layers import RelationalGraphConvolutionLP
    torch.manual_seed(0)
    ed = {"general": 0.5, "self_loop": 0.2, "self_loop_type": "schlichtkrull-dropout"}
    layer = RelationalGraphConvolutionLP(num_nodes=N, num_relations=2 * R0 + 1, in_features=d, out_features=d, edge_dropout=ed,
                                         decomposition={"type": "block", "num_blocks": nb}, w_init="glorot-normal", b_init="zeros").to(DEV)
    layer.eval()
    graph = torch.from_numpy(_native.synthetic_triples_host(N, R0, E, 0)).to(DEV)
    X = torch.randn(N, d, device=DEV)
    G = torch.randn(N, d, device=DEV)

    def step(x, g, **route):
        def run():
            x.grad = None
            layer.zero_grad(set_to_none=True)
            with routes.override(**route):
                layer(graph, x).backward(g)
        return run
    x32, x16 = X.requires_grad_(True), X.detach().to(BF).requires_grad_(True)
    return {"fp32": step(x32, G), "bf16_new": step(x16, G.to(BF)), "bf16_parent_route": step(x16, G.to(BF), block_path="0")}


def measure(variants, steps, warmup, peak=False):
    from torch_rgcn import _native
    for run in variants.values():
        for _ in range(warmup):
            run()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(steps):
        for k, run in variants.items():          # alternate
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
    for k, run in variants.items():              # which kernels ran (a step of its own: the per-launch timers serialise the stream)
        _native.profile_start()
        run()
        torch.cuda.synchronize()
        res[k]["kernels_ms"] = {t: round(statistics.median(v), 4) for t, v in sorted(_native.profile_stop().items())}
    if peak:
        for k in ("bf16_new", "bf16_parent_route"):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            variants[k]()
            torch.cuda.synchronize()
            res[k]["peak_allocated_MB_above_start"] = round((torch.cuda.max_memory_allocated() - base) / 1e6, 1)
    res["bf16_new_vs_fp32"] = round(res["fp32"]["ms_median"] / res["bf16_new"]["ms_median"], 3)
    res["bf16_new_vs_parent_route"] = round(res["bf16_parent_route"]["ms_median"] / res["bf16_new"]["ms_median"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default=None)
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the graphs (rehearsals; a record is taken at 1.0)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_decomposed_bench: needs the GPU (no CPU fallback)")
    from torch_rgcn import _native
    s = args.scale
    out = {"tool": "tools/bf16_decomposed_bench.py", "csrc_sha": _native.csrc_sha(), "steps": args.steps, "warmup": args.warmup, "scale": s,
           "device": torch.cuda.get_device_name(0), "workloads": {}}
    want = lambda n: args.only in (None, n)
    if want("fb_lp_block_d500"):
        out["workloads"]["fb_lp_block_d500"] = measure(lp_workload(int(14_541 * s), 237, int(272_115 * s), 500, 100), args.steps, args.warmup, peak=True)
        print(json.dumps({"fb_lp_block_d500": out["workloads"]["fb_lp_block_d500"]}), flush=True)
    N, R0, E = int(1_666_764 * s), 133, int(5_988_321 * s)
    tp = None
    for name, d, dec, diag in (("am_block_d64", 64, {"type": "block", "num_blocks": 8}, False),
                               ("am_block_d32", 32, {"type": "block", "num_blocks": 8}, False), ("am_diag_d32", 32, None, True)):
        if not want(name):
            continue
        if tp is None:
            T = _native.synthetic_triples_host(N, R0, E, 0)
            tp = torch.from_numpy(_native.add_inverse_and_self_host(T, N, R0))
        out["workloads"][name] = measure(nc_workload(tp, N, 2 * R0 + 1, d, dec, diag), args.steps, args.warmup)
        print(json.dumps({name: out["workloads"][name]}), flush=True)
        torch.cuda.empty_cache()
    path = os.path.join(ROOT, "profiles", f"bf16_decomposed_bench_{_native.csrc_sha()}.json")
    if s == 1.0 and args.only is None:
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
