"""bf16 storage against fp32 on bench.py's S1 step, in one process.

The step is bench.py's: layer 1 (horizontal) with its ReLU fused, layer 2 (vertical), loss = mean(out^2), backward to X and every
parameter.  bf16: X and the activations bf16, the parameters fp32.  Graph and plan builds are excluded (warm-up steps); a step is timed
with HIP events, the median of --steps.  Per-layer forward / backward times come from the library's per-launch event timers in separate
steps (--steps of them).  Bytes follow SURVEY.md 8(d) with the row width of the storage (64 B fp32 rows, 32 B bf16 rows).

    python tools/bf16_bench.py [--steps 30 --warmup 5]      -> one JSON line
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


def fwd_bytes(M, N, d_in, d_out, eb):
    """SURVEY.md 8(d) with eb bytes per stored element: M*(eb*d_in + 8) + N*eb*d_out"""
    return M * (eb * d_in + 8) + N * eb * d_out


def bwd_bytes(M, N, d_in, d_out, eb, x_needs_grad=True):
    """SURVEY.md 8(d) with eb bytes per stored element: M*(eb*d_out + 8) + N*eb*d_in*(1 + [X needs grad])"""
    return M * (eb * d_out + 8) + N * eb * d_in * (2 if x_needs_grad else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--rels", type=int, default=50)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from torch_rgcn import _native
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    N, R0, E, d = args.nodes, args.rels, args.edges, 16
    dev = torch.device("cuda:0")
    T = _native.synthetic_triples_host(N, R0, E, 0)
    tp = torch.from_numpy(_native.add_inverse_and_self_host(T, N, R0))
    M = int(tp.shape[0])
    kw = dict(triples=tp, num_nodes=N, num_relations=2 * R0 + 1, in_features=d, out_features=d)
    torch.manual_seed(0)
    l1 = RelationalGraphConvolutionNC(vertical_stacking=False, **kw).to(dev)
    l2 = RelationalGraphConvolutionNC(vertical_stacking=True, **kw).to(dev)
    X32 = torch.randn(N, d, device=dev).requires_grad_(True)
    X16 = X32.detach().to(torch.bfloat16).requires_grad_(True)

    def step(X):
        out = l2(l1.forward_activated(X, "relu", private=True))
        loss = out.float().pow(2).mean()
        loss.backward()
        return loss

    res = {}
    for name, X in (("fp32", X32), ("bf16", X16)):
        for _ in range(args.warmup):
            step(X)
        torch.cuda.synchronize()
        times = []
        for _ in range(args.steps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            step(X)
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b))
        _native.profile_start()
        for _ in range(args.steps):
            step(X)
        prof = _native.profile_stop()
        per = {k: statistics.median(v) for k, v in prof.items()}
        # two launches per step of each of the layer kernels (one per layer)
        fwd_tag, bwd_tag = ("spmm_blk_bf16", "bwd_own_bf16") if name == "bf16" else ("spmm_blk", "bwd_fused")
        eb = 2 if name == "bf16" else 4
        f_ms, b_ms = per.get(fwd_tag), per.get(bwd_tag)
        fb, bb = fwd_bytes(M, N, d, d, eb), bwd_bytes(M, N, d, d, eb)
        res[name] = {"step_ms": round(statistics.median(times), 4), "fwd_ms_per_layer": f_ms and round(f_ms, 4),
                     "bwd_ms_per_layer": b_ms and round(b_ms, 4), "fwd_bytes": fb, "bwd_bytes": bb,
                     "fwd_GBs": f_ms and round(fb / f_ms / 1e6, 1), "bwd_GBs": b_ms and round(bb / b_ms / 1e6, 1),
                     "kernels_ms": {k: round(v, 4) for k, v in sorted(per.items())}}
    res["bf16_speedup_step"] = round(res["fp32"]["step_ms"] / res["bf16"]["step_ms"], 3)
    print(json.dumps({"workload": f"S1 N={N} R0={R0} E={E} h={d}", "steps": args.steps, "csrc_sha": _native.csrc_sha(), **res}))


if __name__ == "__main__":
    main()
