#!/usr/bin/env python3
"""Ranking evaluation at WN18 size: N = 40,943 entities, d = 200, 5,000 test triples (10,000 head /
tail queries), filtered against ~150k known triples.  Prints one JSON line: whole evaluate() wall time, the score-all
kernel's MFMA roofline, and the CPU oracle (reference algorithm, numpy) on a bounded sample.
    python tools/eval_bench.py [--test 5000] [--cpu-sample 48] [--no-cpu] [--bf16]
--bf16: the entity table is rounded to bf16 and, in the same process, the fp32 evaluator on the widened table is measured against the bf16
evaluator on the bf16 table (launches alternate): "bf16" in the result."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-rgcn_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from torch_rgcn import _native  # noqa: E402
from torch_rgcn.layers import DistMult  # noqa: E402
from utils import misc  # noqa: E402

MFMA_F32_PEAK_TFLOPS = 157.3     # MI355X dense fp32 matrix peak (MI355X_MICROARCH.md)


class Model(torch.nn.Module):
    def __init__(self, dm, x):
        super().__init__()
        self.scoring_function, self.x = dm, x

    def encode(self, graph):
        return self.x

    def forward(self, graph, triples):
        return self.scoring_function(triples, self.x), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--test", type=int, default=5000)
    ap.add_argument("--cpu-sample", type=int, default=48)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    a = ap.parse_args()
    print(json.dumps(run(a.test, 0 if a.no_cpu else a.cpu_sample, a.bf16)), flush=True)


def bf16_against_fp32(batch, x, rel, out, launches=10):
    """x: the widened bf16 table.  -> per-launch medians of the fp32 evaluator on x and of the bf16 evaluator on x.bfloat16(), taking turns"""
    xb = x.to(torch.bfloat16)
    runs = {"score_all": lambda: _native.distmult_score_all(batch, True, x, rel, out=out),
            "distmult_score_all_bf16": lambda: _native.distmult_score_all_bf16(batch, True, xb, rel, out=out)}
    for r in runs.values():
        for _ in range(3):
            r()
    torch.cuda.synchronize()
    _native.profile_start()
    for _ in range(launches):
        for r in runs.values():
            r()
    torch.cuda.synchronize()
    ks = {k: float(np.median(v)) for k, v in _native.profile_stop().items()}
    a = runs["score_all"]().double()                   # (a copy: both write `out`)
    b = runs["distmult_score_all_bf16"]().double()
    return {"fp32_on_widened_ms": round(ks["score_all"], 4), "bf16_ms": round(ks["distmult_score_all_bf16"], 4),
            "bf16_speedup": round(ks["score_all"] / ks["distmult_score_all_bf16"], 3),
            "max_abs_difference_over_max_score": float((a - b).abs().max() / a.abs().max())}


def run(test=5000, cpu_sample=48, bf16=False):
    """-> the result dict (bench.py's detail file carries it as the evaluator line: tools/config_bench.py line_eval)"""
    import types
    a = types.SimpleNamespace(test=test, cpu_sample=cpu_sample, no_cpu=cpu_sample <= 0)
    N, R0, d, Q = 40_943, 18, 200, a.test
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(N, d, device=dev)
    if bf16:
        x = x.to(torch.bfloat16).float()
    dm = DistMult(R0, d, N, R0).to(dev)
    test = _native.synthetic_triples_host(N, R0, Q, 5)
    known = _native.synthetic_triples_host(N, R0, 146_442, 6)
    t0 = time.perf_counter()
    true_triples = misc.generate_true_dict(np.concatenate([known, test]))
    t_dict = time.perf_counter() - t0
    model = Model(dm, x)
    misc.evaluate(model, None, test[:256], true_triples, N, verbose=False)          # warm-up
    torch.cuda.synchronize()
    _native.profile_start()
    t0 = time.perf_counter()
    mrr, hits, ranks = misc.evaluate(model, None, test, true_triples, N, batch_size=32, verbose=False)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    prof = _native.profile_stop()
    # steady-state kernel time: repeated launches of the full-size score-all
    batch = torch.from_numpy(test).to(dev)
    out = torch.empty(Q, N, device=dev)
    for _ in range(3):
        _native.distmult_score_all(batch, True, x, dm.relations.detach(), out=out)
    torch.cuda.synchronize()
    _native.profile_start()
    for _ in range(10):
        _native.distmult_score_all(batch, True, x, dm.relations.detach(), out=out)
    torch.cuda.synchronize()
    ks = _native.profile_stop()["score_all"]
    k_ms = float(np.mean(ks))
    flops = 2.0 * Q * N * d
    res = {"workload": f"WN18-sized ranking: N={N}, d={d}, {Q} test triples -> {2 * Q} queries x {N} candidates, filtered",
           "evaluate_wall_s": round(wall, 4), "queries_per_s": round(2 * Q / wall), "true_dict_build_s": round(t_dict, 3),
           "mrr": mrr, "kernels_ms_in_evaluate": {k: round(float(np.sum(v)), 3) for k, v in prof.items()},
           "roofline": {"kernel": "score_all_lds_kernel<true> (+ rank_query_kernel)", "bound": "mfma", "achieved": round(flops / (k_ms * 1e-3) / 1e12, 2),
                        "peak": MFMA_F32_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": round(flops / (k_ms * 1e-3) / 1e12 / MFMA_F32_PEAK_TFLOPS, 4),
                        "avg_launch_ms": round(k_ms, 4), "flops_per_launch": flops, "traffic": None}}
    if bf16:
        res["bf16"] = bf16_against_fp32(batch, x, dm.relations.detach(), out)
    if not a.no_cpu:
        from oracle import oracle
        xs, rel = x.cpu().numpy(), dm.relations.detach().cpu().numpy()
        sample = test[: a.cpu_sample]
        t0 = time.perf_counter()
        _, _, cpu_ranks = oracle.evaluate(lambda ts: oracle.distmult_forward(ts, xs, rel), sample, true_triples, N, batch_size=16)
        cpu = time.perf_counter() - t0
        assert cpu_ranks == ranks[: len(sample)] + ranks[Q:Q + len(sample)], "GPU ranks differ from the oracle's"
        res["cpu_baseline"] = {"value": round(2 * len(sample) / cpu, 1), "unit": "queries/s", "cores": 1, "kind": "port",
                               "sample": f"{len(sample)} test triples ({2 * len(sample)} queries) through oracle.evaluate "
                                         f"(reference algorithm incl. the [bn, N, 3] expansion; decoder only -- the reference "
                                         f"also re-runs the encoder per batch of {16}), {cpu:.1f} s; ranks equal the GPU's"}
    return res


if __name__ == "__main__":
    main()
