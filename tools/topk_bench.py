"""Top-k link prediction: the fused score-and-select route against what else can answer or nearly answer the question,
one process, filtered, fp32 and bf16 entity tables, k in {1, 10, 32}.

  topk_fused            _native.distmult_topk: the tile product with the selecting epilogue, then the merge; no score matrix
  materialised_topk     distmult_score_all[_bf16] into a [Q, N] fp32 buffer, rank_filter, torch.topk -- what could be done before this
                        route existed (torch.topk does not order equal scores by id: it is timed, not compared)
  rank_fused            _native.distmult_rank_fused: the same product with the cheapest epilogue there is (two compares per cell)

WN18 size (N = 40,943, d = 200, Q = 5,000), and a shape whose score matrix is 20 GB (N = 1,000,000, Q = 5,000), where only the two fused
routes run.  The variants ALTERNATE launch by launch; HIP events; median, minimum and quartiles of --steps after --warmup.  No figure is a
threshold.  The registers and occupancy of the four kernel roles (every storage and load path) are read from the compiler's resource-usage remarks (--remarks FILE: the output of
hipcc -Rpass-analysis=kernel-resource-usage on csrc/rgcn_rank.hip; without it the tool compiles the device code of that file once).

    python tools/topk_bench.py [--steps 20 --warmup 5 --out DIR --remarks FILE --skip-large]   -> DIR/topk_bench_<csrc_sha>.json (DIR: profiles/)
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "torch-rgcn_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

DEV = "cuda:0"
BF = torch.bfloat16
KS = (1, 10, 32)


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


def resource_usage(remarks):
    """{kernel: {vgprs, agprs, occupancy_waves_per_simd, static_lds_bytes, scratch_bytes}} of the four kernel roles of csrc/rgcn_rank.hip
    (score-all, target score, strip count, strip select) in both storages and on both load paths, from the compiler's remarks"""
    if remarks is None:
        csrc = os.path.join(ROOT, "torch-rgcn_amd", "csrc")
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics", "-mllvm",
               "-amdgpu-mfma-vgpr-form", "-I" + os.path.join(ROOT, "include"), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
               "-c", "-o", os.devnull, os.path.join(csrc, "rgcn_rank.hip")]
        text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    else:
        text = open(remarks).read()
    fields = {"VGPRs": "vgprs", "AGPRs": "agprs", "Occupancy [waves/SIMD]": "occupancy_waves_per_simd", "LDS Size [bytes/block]": "static_lds_bytes",
              "ScratchSize [bytes/lane]": "scratch_bytes"}
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            # a mangled instantiation of a role: ...<role>_kernelINS_<Tile>ELb<VEC>EEE...
            name = m.group(1)
            cur = None
            for kern in ("score_all_kernel", "target_score_kernel", "strip_count_kernel", "strip_select_kernel"):
                tile = re.search(kern + r"I\w*?(TileF32|TileBf16)ELb([01])E", name)
                if tile:
                    cur = f"{kern}<{tile.group(1)}, {'VEC' if tile.group(2) == '1' else 'scalar loads'}>"
                    out[cur] = {}
                    break
            continue
        m = re.search(r"remark:\s+(.+?): (\d+)\s", line)
        if cur and m and m.group(1) in fields:
            out[cur][fields[m.group(1)]] = int(m.group(2))
    return out


def shape(steps, warmup, N, Q, d, materialised, R0=18):
    from torch_rgcn import _native
    torch.manual_seed(0)
    res = {"shape": {"N": N, "d": d, "Q": Q, "filter_cells": 3 * Q}, "score_matrix_bytes": 4 * Q * N}
    x32 = torch.randn(N, d, device=DEV).to(BF).float()
    rel = torch.randn(R0, d, device=DEV)
    batch = torch.from_numpy(_native.synthetic_triples_host(N, R0, Q, 5)).to(DEV)
    g = torch.Generator().manual_seed(1)
    fq = torch.randint(0, Q, (3 * Q,), generator=g, dtype=torch.int32).to(DEV)
    fn = torch.randint(0, N, (3 * Q,), generator=g, dtype=torch.int32).to(DEV)
    out = torch.empty(Q, N, device=DEV) if materialised else None
    for storage in ("fp32", "bf16"):
        x = x32 if storage == "fp32" else x32.to(BF)
        score_all = _native.distmult_score_all if storage == "fp32" else _native.distmult_score_all_bf16
        variants = {"rank_fused": lambda: _native.distmult_rank_fused(batch, False, x, rel, filt_q=fq, filt_n=fn)}
        for k in KS:
            variants[f"topk_fused_k{k}"] = lambda k=k: _native.distmult_topk(batch, False, x, rel, k=k, filt_q=fq, filt_n=fn)
            if materialised:
                def run(k=k):
                    score_all(batch, False, x, rel, out=out)
                    _native.rank_filter(out, fq, fn)
                    return torch.topk(out, k, dim=1)
                variants[f"materialised_topk_k{k}"] = run
        r = alternate(variants, steps, warmup)
        for k in KS:
            r[f"topk_fused_k{k}"]["over_rank_fused"] = round(r[f"topk_fused_k{k}"]["ms_median"] / r["rank_fused"]["ms_median"], 3)
            r[f"topk_fused_k{k}"]["useful_tflops"] = round(2.0 * Q * N * d / (r[f"topk_fused_k{k}"]["ms_median"] * 1e-3) / 1e12, 2)
            r[f"topk_fused_k{k}"]["workspace_bytes"] = _native.topk_workspace_bytes(Q, N, d, k, 0, storage == "bf16")
            if materialised:
                r[f"topk_fused_k{k}"]["over_materialised_topk"] = round(r[f"topk_fused_k{k}"]["ms_median"] /
                                                                        r[f"materialised_topk_k{k}"]["ms_median"], 3)
                # the two routes agree on the scores (torch.topk leaves the order of equal scores open, so ids are not compared)
                a = _native.distmult_topk(batch, False, x, rel, k=k, filt_q=fq, filt_n=fn)[1]
                b = variants[f"materialised_topk_k{k}"]()[0]
                r[f"topk_fused_k{k}"]["scores_equal_torch_topk"] = bool(torch.equal(a, b))
        res[storage] = r
        del x
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    ap.add_argument("--remarks", default=None, help="output of hipcc -Rpass-analysis=kernel-resource-usage on csrc/rgcn_rank.hip")
    ap.add_argument("--skip-large", action="store_true", help="leave out the N = 1,000,000 shape")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: needs the GPU (no CPU fallback)")
    from torch_rgcn import _native
    out = {"tool": "tools/topk_bench.py", "csrc_sha": _native.csrc_sha(), "steps": args.steps, "warmup": args.warmup,
           "device": torch.cuda.get_device_name(0), "kernel_resources": resource_usage(args.remarks)}
    print(json.dumps({"kernel_resources": out["kernel_resources"]}), flush=True)
    out["wn18"] = shape(args.steps, args.warmup, 40_943, 5_000, 200, True)
    print(json.dumps({"wn18": out["wn18"]}), flush=True)
    if not args.skip_large:
        out["million_entities"] = shape(args.steps, args.warmup, 1_000_000, 5_000, 200, False)
        print(json.dumps({"million_entities": out["million_entities"]}), flush=True)
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"topk_bench_{_native.csrc_sha()}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
