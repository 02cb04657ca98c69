"""World size 2 on ONE GPU: two processes share cuda:0 and talk over gloo (RCCL refuses two ranks on one device), so
the real HIP kernels, the slab-overlapped asynchronous all-reduce and the relation partition run with a genuine peer.
The 8-GPU RCCL run itself belongs to the driver; this pins everything but the transport."""
import os
import socket

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, outdir, backend="gloo"):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "torch-rgcn_amd")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    from oracle import oracle
    from torch_rgcn.dist import shard_layer
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    index = rank if backend == "nccl" else 0            # RCCL: one GPU per rank; gloo: both ranks share cuda:0
    torch.cuda.set_device(index)
    dev = torch.device("cuda", index)
    extra = {"device_id": dev} if backend == "nccl" else {}
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, **extra)
    try:
        N, R0, E = 5000, 6, 90_000
        T = oracle.synthetic_triples(N, R0, E, seed=17)
        T[: E // 4, 0] = 5                                   # a hub: its tile is cut into several work units
        tp = torch.from_numpy(oracle.add_inverse_and_self(T, N, R0))
        res = {}
        for d_in, d_out in ((16, 16), (16, 4)):              # hidden-16 kernels and the padded output layer
            for sharded in (False, True):
                torch.manual_seed(0)
                layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=2 * R0 + 1,
                                                     in_features=d_in, out_features=d_out).to(dev)
                with torch.no_grad():
                    layer.bias.normal_()
                if sharded:
                    shard_layer(layer, dist.group.WORLD, keep="lpt")
                X = torch.randn(N, d_in, device=dev, requires_grad=True)
                out = layer(X)
                out.backward(torch.cos(out.detach()))
                wg = layer.weights.grad.clone()
                bg = layer.bias.grad.clone()
                if sharded:                                   # weight gradients stay with the owner: sum them for the check
                    dist.all_reduce(wg)
                res[(d_in, d_out, sharded)] = [t.detach().cpu().numpy() for t in (out, X.grad, wg, bg)]
                if sharded:
                    owned = layer._graph.owned_relations
                    assert 0 < len(owned) < 2 * R0 + 1
        if rank == 0:
            np.savez(os.path.join(outdir, "res.npz"), **{f"{k[0]}_{k[1]}_{int(k[2])}_{i}": a for k, v in res.items()
                                                        for i, a in enumerate(v)})
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_sharded_layer_matches_unsharded(tmp_path):
    import torch.multiprocessing as mp
    port = _free_port()
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "res.npz"))
    for d_in, d_out in ((16, 16), (16, 4)):
        for i, name in enumerate(("out", "dX", "dW", "db")):
            a, b = z[f"{d_in}_{d_out}_1_{i}"], z[f"{d_in}_{d_out}_0_{i}"]
            assert np.abs(a - b).max() <= 3e-5 * np.abs(b).max(), (d_in, d_out, name)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (the single-GPU boxes run the gloo variant above)")
def test_two_ranks_two_gpus_rccl_sharded_layer_matches_unsharded(tmp_path):
    """the same check over RCCL / xGMI when the box has two GPUs"""
    import torch.multiprocessing as mp
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), "nccl"), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "res.npz"))
    for d_in, d_out in ((16, 16), (16, 4)):
        for i, name in enumerate(("out", "dX", "dW", "db")):
            a, b = z[f"{d_in}_{d_out}_1_{i}"], z[f"{d_in}_{d_out}_0_{i}"]
            assert np.abs(a - b).max() <= 3e-5 * np.abs(b).max(), (d_in, d_out, name)


def _bench_path_worker(rank, world, port, outdir, backend="gloo"):
    """bench.py's own strong-scaling path (build_layers(keep="lpt") + the step) at 1/10 of S1, every collective variant,
    plus the unsharded run of the same graph on the same device."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "torch-rgcn_amd")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    import bench
    from torch_rgcn.dist import gather_owned_parameters
    index = rank if backend == "nccl" else 0
    torch.cuda.set_device(index)
    dev = torch.device("cuda", index)
    extra = {"device_id": dev} if backend == "nccl" else {}
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, **extra)
    try:
        N, R0, E, d = 100_000, 50, 1_000_000, 16
        res = {}

        def run(tag, group, comm=None, slabs=None):
            l1, l2, _ = bench.build_layers(N, R0, E, d, seed=0, device=dev, group=group, keep="lpt")
            if comm is not None:
                from torch_rgcn.dist import set_transport
                set_transport(l1, comm, int(slabs)), set_transport(l2, comm, int(slabs))
            with torch.no_grad():
                l1.bias.normal_()
                l2.bias.normal_()
            torch.manual_seed(99)
            X = torch.randn(N, d, device=dev, requires_grad=True)
            out = l2(l1.forward_activated(X, "relu", private=True))
            loss = out.pow(2).mean()
            loss.backward()
            grads = [l1.weights.grad.clone(), l2.weights.grad.clone()]
            if group is not None:     # relation rows live on their owners: sum the (disjoint) rows for the comparison
                for gte in grads:
                    dist.all_reduce(gte)
                full = gather_owned_parameters(l1)["weights"]
                assert torch.equal(full, l1.weights.detach())   # same seed on every rank and no optimiser step yet
                assert 0 < len(l1._graph.owned_relations) < 2 * R0 + 1
            res[tag] = [t.detach().cpu().numpy() for t in (out, X.grad, grads[0], grads[1], l1.bias.grad, l2.bias.grad)]

        run("ref", None)
        for comm, slabs in (("allreduce", "0"), ("rs_ag", "0"), ("a2a", "0"), ("allreduce", "2")):
            run(f"{comm}{slabs}", dist.group.WORLD, comm, slabs)
        if rank == 0:
            np.savez(os.path.join(outdir, "bench_path.npz"), **{f"{k}_{i}": a for k, v in res.items() for i, a in enumerate(v)})
    finally:
        dist.destroy_process_group()


def _check_bench_path(tmp_path):
    z = np.load(os.path.join(str(tmp_path), "bench_path.npz"))
    for tag in ("allreduce0", "rs_ag0", "a2a0", "allreduce2"):
        for i, name in enumerate(("out", "dX", "dW1", "dW2", "db1", "db2")):
            a, b = z[f"{tag}_{i}"], z[f"ref_{i}"]
            assert np.abs(a - b).max() <= 3e-5 * np.abs(b).max(), (tag, name)


def test_bench_strong_scaling_path_matches_unsharded_two_ranks_one_gpu(tmp_path):
    """the sharded == unsharded check on bench.py's OWN strong-scaling path (1/10 of S1, LPT shards),
    for every collective variant bench.py may pick; gloo, both ranks on cuda:0."""
    import torch.multiprocessing as mp
    mp.spawn(_bench_path_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    _check_bench_path(tmp_path)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (the single-GPU boxes run the gloo variant above)")
def test_bench_strong_scaling_path_matches_unsharded_rccl(tmp_path):
    import torch.multiprocessing as mp
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    mp.spawn(_bench_path_worker, args=(2, _free_port(), str(tmp_path), "nccl"), nprocs=2, join=True)
    _check_bench_path(tmp_path)


def _basis_worker(rank, world, port, outdir):
    """relation-sharded layers with basis decomposition -- `bases` gets gradient from every relation, so the
    shard hook must all-reduce it; `comps` rows live on the owners."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "torch-rgcn_amd")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    from oracle import oracle
    from torch_rgcn.dist import gather_owned_parameters, shard_layer
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        N, R0, E, d = 4000, 5, 60_000, 16
        tp = torch.from_numpy(oracle.add_inverse_and_self(oracle.synthetic_triples(N, R0, E, seed=5), N, R0))
        res = {}
        for sharded in (False, True):
            torch.manual_seed(0)
            layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=2 * R0 + 1, in_features=d,
                                                 out_features=d, decomposition={"type": "basis", "num_bases": 3}).to(dev)
            if sharded:
                shard_layer(layer, dist.group.WORLD, keep="lpt")
            opt = torch.optim.SGD(layer.parameters(), lr=0.5)
            X = torch.randn(N, d, device=dev)
            for _ in range(3):                      # replicas of `bases` must stay in step over optimiser steps
                opt.zero_grad()
                layer(X).pow(2).mean().backward()
                opt.step()
            comps = gather_owned_parameters(layer)["comps"] if sharded else layer.comps.detach()
            res[sharded] = [layer.bases.detach().cpu().numpy(), comps.cpu().numpy(), layer.bias.detach().cpu().numpy()]
            if sharded:
                b = layer.bases.detach().clone()
                dist.all_reduce(b)
                assert torch.allclose(b / world, layer.bases.detach(), rtol=0, atol=0), "bases replicas diverged"
        if rank == 0:
            np.savez(os.path.join(outdir, "basis.npz"), **{f"{int(k)}_{i}": a for k, v in res.items() for i, a in enumerate(v)})
    finally:
        dist.destroy_process_group()


def test_sharded_basis_layer_trains_like_unsharded(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_basis_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "basis.npz"))
    for i, name in enumerate(("bases", "comps", "bias")):
        a, b = z[f"1_{i}"], z[f"0_{i}"]
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), name


def _run_bench(extra_args, env_extra=None, world=2):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, RGCN_BENCH_ONE_DEVICE="1", RGCN_DIST_BACKEND="gloo", **(env_extra or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "3", "--warmup", "1",
           "--nodes", "200000", "--edges", "1000000", "--rels", "20", "--full"] + extra_args
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        env["RGCN_BENCH_DETAIL"] = os.path.join(tmp, "detail.json")
        out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, out.stdout[-2000:]
        with open(env["RGCN_BENCH_DETAIL"]) as f:
            detail = json.load(f)
    return _line_and_detail(lines[0], detail)


def _line_and_detail(text, detail):
    """the ONE stdout line is the compact record (< 8 KB, the contract's keys, comm summary); the assertions below read the detail file,
    after checking that the line says the same thing"""
    import json
    assert len(text) < 8192, len(text)
    line = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert line[k] == detail[k], k
    assert line["config"] == {k: detail["config"][k] for k in ("workload", "sharding")}
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "algorithmic_bytes_per_launch"):
        assert k in line["roofline"], k
    assert line["roofline"]["frac"] == detail["roofline"]["frac"]
    if "comm" in detail:
        for k in ("collective", "world_size_seen_by_backend", "backend", "exposed_ms_per_step", "compute_alone_ms_per_step"):
            assert line["comm"][k] == detail["comm"][k], k
    assert "cpu_baseline" not in line or set(line["cpu_baseline"]) >= {"value", "unit", "cores", "kind", "sample"}
    return detail


def test_bench_contract_with_two_ranks_on_one_gpu():
    """`torch.distributed.run --nproc-per-node 2 bench.py --gpus 2` exactly as the driver launches it, both ranks on
    cuda:0 over gloo, reduced workload: ONE JSON line, on rank 0; default = STRONG scaling of one graph (BASELINE
    configs[4]): value = E / t, LPT shards, collective timings reported."""
    res = _run_bench([])
    assert res["n_gpus"] == 2 and res["steps"] == 3 and res["warmup"] == 1 and res["scaling"] == "strong"
    assert res["unit"] == "edges/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert abs(res["value"] - 1_000_000 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]
    assert "cpu_baseline" not in res and res["roofline"]["bound"] == "hbm" and "relation-sharded x2" in res["config"]["sharding"]
    comm = res["comm"]
    assert sum(comm["messages_per_rank"]) == 2 * 1_000_000 + 200_000 and min(comm["messages_per_rank"]) > 0
    assert comm["collectives_per_step"] == 4 and comm["compute_alone_ms_per_step"] > 0 and comm["collectives_alone_ms_per_step"] > 0
    assert comm["collective"] in comm["candidates_ms_per_step"] and res["graph_build_ms"] > 0
    # the strong-scaling line carries the LOCAL kernels' rooflines (forward and backward on rank 0's shard) and the
    # exposed communication time
    roof = res["roofline"]
    assert roof["local_messages"] == comm["messages_per_rank"][0]
    assert roof["forward"]["kernel"].startswith("spmm_d16_kernel") and 0 < roof["forward"]["frac"] < 1
    assert "backward" in roof and 0 < roof["backward"]["frac"] < 1 and roof["backward"]["launches_per_step"] == 2
    assert roof["backward"]["algorithmic_bytes_per_launch"] == roof["local_messages"] * (4 * 16 + 8) + 2 * 200_000 * 64
    assert "exposed_ms_per_step" in comm and comm["exposed_ms_per_step"] == pytest.approx(res["ms_per_step"] - comm["compute_alone_ms_per_step"], abs=1e-3)


def test_bench_contract_with_eight_ranks_on_one_gpu():
    """VERDICT r4 #8b: the command the driver's SCALE run ends with -- `torch.distributed.run --nproc-per-node 8 bench.py --gpus 8` -- with
    all eight ranks on cuda:0 over gloo: the JSON contract at world 8, the LPT packing of 41 relations onto 8 ranks (balance <= 1.07 of the
    mean at S1's shape is asserted on the CPU in test_dist_gloo; here every rank must hold messages), what the backend saw, and
    sharded == unsharded for the step the line times (`--check-unsharded`: rank 0 runs the same step on the whole graph)."""
    res = _run_bench(["--check-unsharded"], world=8)
    assert res["n_gpus"] == 8 and res["scaling"] == "strong" and "relation-sharded x8" in res["config"]["sharding"]
    assert abs(res["value"] - 1_000_000 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]
    comm = res["comm"]
    assert len(comm["messages_per_rank"]) == 8 and sum(comm["messages_per_rank"]) == 2 * 1_000_000 + 200_000 and min(comm["messages_per_rank"]) > 0
    assert max(comm["messages_per_rank"]) <= 1.25 * (sum(comm["messages_per_rank"]) / 8)           # 41 relations of ~50 k messages on 8 ranks
    assert comm["world_size_seen_by_backend"] == 8 and comm["backend"] == "gloo" and "backend_version" in comm
    assert comm["collectives_per_step"] == 4 and comm["overlap"] in ("side-stream", "none")
    chk = res["sharded_vs_unsharded"]
    assert chk["max_rel_err"] < 1e-4, chk


def test_bench_weak_mode_still_available():
    res = _run_bench(["--weak"])
    assert res["scaling"] == "weak" and abs(res["value"] - 2 * 1_000_000 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]


def test_plain_bench_command_launches_its_own_ranks():
    """`python bench.py --gpus 2` -- the shape of the command the driver uses at N = 1, no launcher around
    it -- re-runs itself under torch.distributed.run (one rank per GPU) instead of dying on WORLD_SIZE != --gpus, and the
    launcher process prints rank 0's ONE JSON line as the last line of stdout.  Both ranks on cuda:0 over gloo here."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(RGCN_BENCH_ONE_DEVICE="1", RGCN_DIST_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--nodes", "100000",
           "--edges", "500000", "--rels", "10", "--full"]
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        env["RGCN_BENCH_DETAIL"] = os.path.join(tmp, "detail.json")
        out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1 and lines[-1].startswith("{"), out.stdout[-2000:]
        with open(env["RGCN_BENCH_DETAIL"]) as f:
            res = _line_and_detail(lines[-1], json.load(f))
    assert res["n_gpus"] == 2 and res["steps"] == 2 and res["scaling"] == "strong" and "relation-sharded x2" in res["config"]["sharding"]
    assert abs(res["value"] - 500_000 / (res["ms_per_step"] * 1e-3)) < 1e-6 * res["value"]


def _hub_owner_worker(rank, world, port, outdir):
    """a hub whose relation ONE rank owns.  That rank's tall-tile backward plan has hub pieces (the fused slab-by-slab
    backward does not take them), the other rank's has none: left to themselves the ranks would pick different routes and post all-reduces
    over different row ranges.  The route is agreed over the group (functional._all_ranks_agree); sharded == unsharded."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "torch-rgcn_amd")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    from oracle import oracle
    from torch_rgcn import _native
    from torch_rgcn.dist import shard_layer
    from torch_rgcn.layers import RelationalGraphConvolutionNC
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        N, R0, E = 60_000, 4, 600_000
        T = oracle.synthetic_triples(N, R0, E, seed=23)
        T[: E // 3, 1] = 0                                   # a third of the triples: relation 0 ...
        T[: E // 3, 2] = 7                                   # ... into ONE object: a hub row of the transposed plan, in relation 0 only
        tp = torch.from_numpy(oracle.add_inverse_and_self(T, N, R0))
        res = {}
        for sharded in (False, True):
            torch.manual_seed(0)
            layer = RelationalGraphConvolutionNC(triples=tp, num_nodes=N, num_relations=2 * R0 + 1, in_features=16, out_features=16).to(dev)
            with torch.no_grad():
                layer.bias.normal_()
            if sharded:
                shard_layer(layer, dist.group.WORLD, keep="lpt", comm="allreduce", slabs=3)
            X = torch.randn(N, 16, device=dev, requires_grad=True)
            out = layer(X)
            out.backward(torch.cos(out.detach()))
            wg = layer.weights.grad.clone()
            if sharded:
                dist.all_reduce(wg)
                bp = layer._graph.bwd_blk_plan()
                assert bp is not None, "the test wants the block-tile backward's plan (graph too small?)"
                pieces = torch.tensor([_native._blk_units(bp)[2]], device=dev, dtype=torch.int64)
                both = [torch.zeros_like(pieces) for _ in range(world)]
                dist.all_gather(both, pieces)
                both = [int(t.item()) for t in both]
                assert (both[0] > 0) != (both[1] > 0), f"hub pieces per rank {both}: the scenario needs them on exactly one rank"
                agreed = layer._graph._group_routes
                assert agreed == {("bwd_fused_slabs", 3): False}, agreed
            res[sharded] = [t.detach().cpu().numpy() for t in (out, X.grad, wg, layer.bias.grad)]
        if rank == 0:
            np.savez(os.path.join(outdir, "hub.npz"), **{f"{int(k)}_{i}": a for k, v in res.items() for i, a in enumerate(v)})
    finally:
        dist.destroy_process_group()


def test_two_ranks_hub_relation_owned_by_one_rank_routes_agree(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_hub_owner_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    z = np.load(os.path.join(str(tmp_path), "hub.npz"))
    for i, name in enumerate(("out", "dX", "dW", "db")):
        a, b = z[f"1_{i}"], z[f"0_{i}"]
        assert np.abs(a - b).max() <= 3e-5 * np.abs(b).max(), name
