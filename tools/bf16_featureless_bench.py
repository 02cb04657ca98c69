"""bf16 storage against fp32 for featureless basis layers, in one process, alternating.

Workloads (dataset-shaped synthetic graphs, tools/fbt_bench.py's generator):
  am_l1      AM as shipped, layer 1: N = 1,666,764, R0 = 133, E = 5,988,321, basis 40, hidden 10 -- forward + backward
  am_step    the whole AM NodeClassifier step: layer 1, ReLU, layer 2 to 11 classes, loss = mean(out^2), backward
  bgs_l1     BGS-shaped layer 1: N = 333,845, R0 = 103, E = 916,199, basis 40, hidden 16
  mutag_l1   MUTAG-shaped layer 1: N = 23,644, R0 = 23, E = 74,227, basis 30, hidden 16
bf16: the model .to(torch.bfloat16); fp32: the same model in fp32.  A step is timed with HIP events, the median of --steps after --warmup
(graph and plan builds are in the warm-up); the two dtypes alternate step by step.  Per-kernel times: a separate
`rocprofv3 --kernel-trace --stats` run of this tool.

Algorithmic bytes of layer 1 (eb = bytes per stored element, M messages, N nodes, B bases, d = hidden, ys = padded Y row):
  forward   table B N d eb + messages M (4 rel + 4 val) + Y M ys 4 (write) + gather M (4 perm + ys 4) + out N d eb
  backward  table B N d eb + dbases B N d eb + G rows M d eb + messages M (4 dst + 4 rel + 4 val)

    python tools/bf16_featureless_bench.py [--steps 20 --warmup 5] [--only am_l1,...]    -> one JSON line
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-rgcn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

SHAPES = {"am": (1_666_764, 133, 5_988_321, 40, 10, 11), "bgs": (333_845, 103, 916_199, 40, 16, 2), "mutag": (23_644, 23, 74_227, 30, 16, 2)}


def layer_bytes(M, N, B, d, eb):
    ys = max(4, 1 << (d - 1).bit_length())
    fwd = B * N * d * eb + 8 * M + 4 * M * ys + M * (4 + 4 * ys) + N * d * eb
    bwd = 2 * B * N * d * eb + M * d * eb + 12 * M
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="am_l1,am_step,bgs_l1,mutag_l1")
    args = ap.parse_args()
    from torch_rgcn import _native
    from torch_rgcn.models import NodeClassifier
    from torch_rgcn.utils import add_inverse_and_self
    dev = torch.device("cuda:0")
    res = {}
    for work in args.only.split(","):
        name, what = work.split("_")
        N, R0, E, B, d, C = SHAPES[name]
        T = torch.from_numpy(np.asarray(_native.synthetic_triples_host(N, R0, E, 1)))
        torch.manual_seed(0)
        m32 = NodeClassifier(triples=T, nnodes=N, nrel=R0, nfeat=None, nhid=d, nclass=C, decomposition={"type": "basis", "num_bases": B}).to(dev)
        m16 = copy.deepcopy(m32).to(torch.bfloat16)
        M = int(add_inverse_and_self(T, N, R0).shape[0])
        g = torch.randn(N, d, device=dev)
        g16 = g.to(torch.bfloat16)

        def step(m, gg):
            if what == "step":
                out = m()
                out.float().pow(2).mean().backward()
            else:
                m.rgc1().backward(gg)

        times = {"fp32": [], "bf16": []}
        for k in range(args.warmup + args.steps):
            for key, m, gg in (("fp32", m32, g), ("bf16", m16, g16)):
                m.zero_grad(set_to_none=True)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                step(m, gg)
                b.record()
                b.synchronize()
                if k >= args.warmup:
                    times[key].append(a.elapsed_time(b))
        r = {key: round(statistics.median(v), 4) for key, v in times.items()}
        for key, eb in (("fp32", 4), ("bf16", 2)):
            fb, bb = layer_bytes(M, N, B, d, eb)
            r[f"{key}_layer1_bytes"] = fb + bb
        r["bf16_speedup"] = round(r["fp32"] / r["bf16"], 3)
        res[work] = r
        del m32, m16
        torch.cuda.empty_cache()
    print(json.dumps({"workload": "featureless basis layer 1 / NodeClassifier step, fp32 vs bf16 storage", "steps": args.steps,
                      "csrc_sha": _native.csrc_sha(), **res}))


if __name__ == "__main__":
    main()
