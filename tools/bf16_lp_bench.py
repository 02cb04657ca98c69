"""bf16 link prediction: the DistMult decoder and the ranking evaluator in fp32 and on a bf16 entity table, one process.

  evaluator   WN18 size: 5,000 test triples x 40,943 candidates x d = 200 per launch.  fp32 evaluator (v_mfma_f32_16x16x4_f32) on the
              WIDENED table -- what a user with a bf16 encoder had to do -- against the bf16 evaluator (v_mfma_f32_16x16x32_bf16, three-term
              queries) on the bf16 table.  Same fp32 score matrix [Q, N] written by both.
  decoder     forward + backward of 330,000 scored triples (the WN18 training batch), N = 40,943, 18 relations, d = 200, biases on: every
              gradient from the CSR walks; and FB15k-237 shape (N = 14,541, 237 relations, d = 500, 272,115 triples): the relation table is
              beyond the LDS table, so the predicate-sorted kernel + the entity walk.
The variants ALTERNATE launch by launch / step by step (a drift of the shared host hits both alike); HIP events; median, minimum and
quartiles of --steps after --warmup.  No figure is a threshold: the file records the ratio to the fp32 path measured in the same run.

    python tools/bf16_lp_bench.py [--steps 20 --warmup 5 --out DIR]   -> DIR/bf16_lp_bench_<csrc_sha>.json (DIR: profiles/)
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


def kernels_of(run):
    from torch_rgcn import _native
    _native.profile_start()
    run()
    torch.cuda.synchronize()
    return {t: round(sum(v), 4) for t, v in sorted(_native.profile_stop().items())}


def evaluator(steps, warmup, N=40_943, R0=18, d=200, Q=5000):
    from torch_rgcn import _native
    torch.manual_seed(0)
    xb = torch.randn(N, d, device=DEV).to(BF)
    xw = xb.float()                                    # the widened table: the same numbers
    rel = torch.randn(R0, d, device=DEV)
    batch = torch.from_numpy(_native.synthetic_triples_host(N, R0, Q, 5)).to(DEV)
    out = torch.empty(Q, N, device=DEV)
    variants = {"fp32_on_widened": lambda: _native.distmult_score_all(batch, True, xw, rel, out=out),
                "bf16": lambda: _native.distmult_score_all_bf16(batch, True, xb, rel, out=out)}
    res = alternate(variants, steps, warmup)
    a = _native.distmult_score_all(batch, True, xw, rel).double()
    b = _native.distmult_score_all_bf16(batch, True, xb, rel).double()
    flops = 2.0 * Q * N * d
    for k in res:
        res[k]["useful_tflops"] = round(flops / (res[k]["ms_median"] * 1e-3) / 1e12, 2)
    res["score_bytes_written"] = 4 * Q * N
    res["bf16_write_GBps"] = round(4 * Q * N / (res["bf16"]["ms_median"] * 1e-3) / 1e9, 1)
    res["max_abs_difference_over_max_score"] = float((a - b).abs().max() / a.abs().max())
    res["bf16_speedup_over_fp32_on_widened"] = round(res["fp32_on_widened"]["ms_median"] / res["bf16"]["ms_median"], 3)
    res["shape"] = {"N": N, "d": d, "Q": Q}
    return res


def decoder(steps, warmup, N, R0, d, T, route):
    from torch_rgcn import _native, routes
    from torch_rgcn.layers import DistMult
    torch.manual_seed(0)
    dm = DistMult(R0, d, N, R0, b_init="normal").to(DEV)
    tr = torch.from_numpy(_native.synthetic_triples_host(N, R0, T, 12)).to(DEV)
    g = torch.randn(T, device=DEV)
    x32 = torch.randn(N, d, device=DEV).to(BF).float().requires_grad_(True)
    x16 = x32.detach().to(BF).requires_grad_(True)

    def step(x):
        def run():
            x.grad = None
            dm.zero_grad(set_to_none=True)
            with routes.override(distmult_bwd=route):
                dm(tr, x).backward(g)
        return run
    variants = {"fp32": step(x32), "bf16": step(x16)}
    res = alternate(variants, steps, warmup)
    for k, run in variants.items():
        res[k]["kernels_ms"] = kernels_of(run)
    res["bf16_speedup_over_fp32"] = round(res["fp32"]["ms_median"] / res["bf16"]["ms_median"], 3)
    res["shape"] = {"N": N, "relations": R0, "d": d, "triples": T, "route": route}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_lp_bench: needs the GPU (no CPU fallback)")
    from torch_rgcn import _native
    out = {"tool": "tools/bf16_lp_bench.py", "csrc_sha": _native.csrc_sha(), "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0)}
    out["evaluator_wn18"] = evaluator(args.steps, args.warmup)
    print(json.dumps({"evaluator_wn18": out["evaluator_wn18"]}), flush=True)
    out["decoder_wn18_330k"] = decoder(args.steps, args.warmup, 40_943, 18, 200, 330_000, "csr")
    print(json.dumps({"decoder_wn18_330k": out["decoder_wn18_330k"]}), flush=True)
    out["decoder_fb15k237_d500"] = decoder(args.steps, args.warmup, 14_541, 237, 500, 272_115, "csr")
    print(json.dumps({"decoder_fb15k237_d500": out["decoder_fb15k237_d500"]}), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"bf16_lp_bench_{_native.csrc_sha()}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
