#!/usr/bin/env python3
"""Ranking evaluation at WN18 size: N = 40,943 entities, d = 200, 5,000 test triples (10,000 head /
tail queries), filtered against ~150k known triples.  Prints one JSON line: whole evaluate() wall time, the score-all
kernel's MFMA roofline, and the CPU oracle (reference algorithm, numpy) on a bounded sample.
    python tools/eval_bench.py [--test 5000] [--cpu-sample 48] [--no-cpu] [--bf16]
--bf16: the entity table is rounded to bf16 and, in the same process, the fp32 evaluator on the widened table is measured against the bf16
evaluator on the bf16 table (launches alternate): "bf16" in the result.
    python tools/eval_bench.py --fused [--test 5000] [--steps 20 --warmup 5 --out DIR]   -> DIR/rank_fused_bench_<csrc_sha>.json (DIR: profiles/)
--fused: nothing of the above; in one process, for fp32 and bf16 tables, the materialised route (score-all, filter, count) against the fused
route, taking turns: whole evaluate() calls by the host clock (they end in a synchronising download of the counts), and
single launches of the full head batch by HIP events.  The counts of the two routes are compared before anything is timed."""
import argparse
import json
import os
import statistics
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
    ap.add_argument("--fused", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    if a.fused:
        res = fused_against_materialised(a.test, a.steps, a.warmup)
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, f"rank_fused_bench_{_native.csrc_sha()}.json"), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        return
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


def _quartiles(t, unit="ms"):
    q = statistics.quantiles(t, n=4)
    return {f"{unit}_median": round(statistics.median(t), 4), f"{unit}_min": round(min(t), 4), f"{unit}_q1": round(q[0], 4),
            f"{unit}_q3": round(q[2], 4)}


def fused_against_materialised(Q=5000, steps=20, warmup=5, evaluations=5):
    """-> the dict of profiles/rank_fused_bench_<csrc_sha>.json"""
    N, R0, d = 40_943, 18, 200
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x32 = torch.randn(N, d, device=dev)
    dm = DistMult(R0, d, N, R0).to(dev)
    rel = dm.relations.detach()
    test = _native.synthetic_triples_host(N, R0, Q, 5)
    known = _native.synthetic_triples_host(N, R0, 146_442, 6)
    true_triples = misc.generate_true_dict(np.concatenate([known, test]))
    batch = torch.from_numpy(test).to(dev)
    rows, cols = misc._filter_index(true_triples, N).lists(test, True)
    fq, fn = torch.from_numpy(rows).to(dev), torch.from_numpy(cols).to(dev)
    scores = torch.empty(Q, N, device=dev)
    res = {"tool": "tools/eval_bench.py --fused", "csrc_sha": _native.csrc_sha(), "steps": steps, "warmup": warmup,
           "evaluations": evaluations, "device": torch.cuda.get_device_name(0),
           "shape": {"N": N, "d": d, "Q": Q, "filter_entries_head": int(len(rows))},
           "score_matrix_bytes": 4 * Q * N}
    for storage, x in (("fp32", x32), ("bf16", x32.to(torch.bfloat16))):
        score_all = _native.distmult_score_all_bf16 if storage == "bf16" else _native.distmult_score_all
        model = Model(dm, x)

        def materialised():
            score_all(batch, True, x, rel, out=scores)
            _native.rank_filter(scores, fq, fn)
            return _native.rank_count(scores, batch, True)

        def fused():
            return _native.distmult_rank_fused(batch, True, x, rel, filt_q=fq, filt_n=fn)[:2]

        a, b = materialised(), fused()
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), "the routes count differently"
        variants = {"materialised": materialised, "fused": fused}
        for run_ in variants.values():
            for _ in range(warmup):
                run_()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(steps):
            for k, run_ in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run_()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1))
        launch = {k: _quartiles(t) for k, t in times.items()}
        launch["fused_speedup"] = round(launch["materialised"]["ms_median"] / launch["fused"]["ms_median"], 3)
        flops = 2.0 * Q * N * d
        launch["fused_useful_tflops"] = round(flops / (launch["fused"]["ms_median"] * 1e-3) / 1e12, 2)
        # whole evaluate() calls: both directions, host filter lists, uploads, the download of the counts
        ranks, walls = {}, {False: [], True: []}
        for f in (False, True):
            ranks[f] = misc.evaluate(model, None, test, true_triples, N, verbose=False, fused=f)[2]        # warm-up
        assert ranks[False] == ranks[True], "the routes rank differently"
        for _ in range(evaluations):
            for f in (False, True):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                misc.evaluate(model, None, test, true_triples, N, verbose=False, fused=f)
                torch.cuda.synchronize()
                walls[f].append(time.perf_counter() - t0)
        ev = {"materialised": _quartiles(walls[False], "s"), "fused": _quartiles(walls[True], "s")}
        ev["fused_speedup"] = round(ev["materialised"]["s_median"] / ev["fused"]["s_median"], 3)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fused()
        peak = torch.cuda.max_memory_allocated() - base
        res[storage] = {"per_launch_head_batch": launch, "evaluate_both_directions": ev,
                        "fused_workspace_bytes": _native.rank_fused_workspace_bytes(Q, N, d, 0, storage == "bf16"),
                        "fused_peak_memory_rise_bytes": int(peak)}
    return res


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
           "roofline": {"kernel": "score_all_kernel<TileF32, true> (+ rank_query_kernel)", "bound": "mfma", "achieved": round(flops / (k_ms * 1e-3) / 1e12, 2),
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
