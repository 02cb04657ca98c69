"""bench.py's ONE stdout line stays small enough for the driver to parse (round 5's was 27 KB and was recorded as `parsed: null`).

The canned result (tests/data/bench_result_canned.json) is a full one-GPU result object of round 5 -- eight config lines with per-kernel
counter blocks -- i.e. the input that broke the contract."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _canned():
    with open(os.path.join(ROOT, "tests", "data", "bench_result_canned.json")) as f:
        return json.load(f)


def _strict(text):
    def no_const(name):
        raise ValueError(f"non-strict JSON constant {name}")
    return json.loads(text, parse_constant=no_const)


def test_compact_line_is_small_strict_json_with_the_contract_keys():
    import bench
    res = _canned()
    assert len(json.dumps(res)) > 20000            # the canned input really is the oversized one
    text = bench.compact_line(res, "bench_detail.json")
    assert len(text) < bench.LINE_TARGET_BYTES < bench.LINE_LIMIT_BYTES == 8192
    assert "\n" not in text
    line = _strict(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in line, k
    assert line["metric"] == res["metric"] and line["value"] == res["value"] and line["ms_per_step"] == res["ms_per_step"]
    assert set(line["config"]) == {"workload", "sharding"}
    roof = line["roofline"]
    for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "algorithmic_bytes_per_launch", "traffic", "step_frac"):
        assert k in roof, k
    assert roof["frac"] == pytest.approx(roof["achieved"] / roof["peak"], rel=1e-3)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in line["cpu_baseline"], k
    assert "configs" not in line and "kernels_traffic" not in text


def test_compact_line_multi_gpu_shape_and_nan_handling():
    import bench
    res = _canned()
    res.pop("configs"), res.pop("cpu_baseline")
    res["n_gpus"] = 8
    res["comm"] = {"collective": "allreduce/slabs=0", "candidates_ms_per_step": {"allreduce/slabs=0": 1.0, "a2a/slabs=0": None},
                   "collectives_per_step": 4, "bytes_per_collective": 64000000, "compute_alone_ms_per_step": 0.4,
                   "exposed_ms_per_step": float("nan"), "world_size_seen_by_backend": 8, "backend": "nccl", "model": "x" * 5000}
    clean = bench._no_nan(res)
    assert clean["comm"]["exposed_ms_per_step"] is None
    text = bench.compact_line(clean)
    assert len(text) < bench.LINE_TARGET_BYTES
    line = _strict(text)
    assert line["comm"]["world_size_seen_by_backend"] == 8 and "model" not in line["comm"]
    assert "cpu_baseline" not in line


def test_oversized_line_is_refused():
    import bench
    res = _canned()
    res["config"]["workload"] = "w" * 9000
    with pytest.raises(AssertionError):
        bench.compact_line(res)


def test_emit_prints_the_line_last_and_writes_the_detail_file(tmp_path):
    detail = tmp_path / "detail.json"
    code = ("import json, sys; sys.path.insert(0, %r); import bench; "
            "bench.emit(json.load(open(%r)))" % (ROOT, os.path.join(ROOT, "tests", "data", "bench_result_canned.json")))
    env = dict(os.environ, RGCN_BENCH_DETAIL=str(detail))
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    out = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(out) == 1 and len(out[0]) < 8192
    line = _strict(out[0])
    full = _strict(detail.read_text())
    assert full["value"] == line["value"] and len(full["configs"]) == 8
    assert "bench.py detail: " in p.stderr


@pytest.mark.gpu
def test_real_one_gpu_bench_line_parses(tmp_path):
    """the real thing, small sizes: the last stdout line of `python bench.py` is strict JSON < 8 KB with roofline and cpu_baseline"""
    env = dict(os.environ, RGCN_BENCH_DETAIL=str(tmp_path / "d.json"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "1", "--no-cpu-s1", "--no-configs",
                        "--sustained-steps", "0"], capture_output=True, text=True, env=env, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    last = [ln for ln in p.stdout.splitlines() if ln.strip()][-1]
    assert len(last) < 8192
    line = _strict(last)
    assert line["n_gpus"] == 1 and line["roofline"]["frac"] > 0 and line["cpu_baseline"]["kind"] == "port"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(10_000_000 / (line["ms_per_step"] * 1e-3), rel=1e-6)


def test_options_for_the_plain_and_the_full_run():
    """--full and --dump-outputs exist; --steps really is the number of timed steps, so 0 is refused (before any GPU work)"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "--full" in p.stdout and "--dump-outputs" in p.stdout
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_dump_outputs_writes_a_fixed_sample_as_float32(tmp_path):
    """dump_outputs on CPU tensors of S1's shape: the loss, a seeded sample of the N x d rows (the same rows every time), every parameter
    gradient whole, float32 (row indices float64), under the 64 MB limit"""
    import types

    import numpy as np
    import torch

    import bench
    N, d, R = 1_000_000, 16, 101
    g = torch.Generator().manual_seed(0)
    out = torch.randn(N, d, generator=g)
    X = torch.zeros(N, d, requires_grad=True)
    X.grad = torch.randn(N, d, generator=g)
    layers = [types.SimpleNamespace(weights=types.SimpleNamespace(grad=torch.randn(R, d, d, generator=g)),
                                    bias=types.SimpleNamespace(grad=torch.randn(d, generator=g))) for _ in range(2)]
    for k in range(2):
        bench.dump_outputs(str(tmp_path / f"o{k}"), torch.tensor(0.5), out, X, *layers)
    names = {"loss", "out", "x_grad", "rows", "l1_weights_grad", "l1_bias_grad", "l2_weights_grad", "l2_bias_grad"}
    assert {f[:-4] for f in os.listdir(tmp_path / "o0")} == names
    a = {n: np.load(str(tmp_path / "o0" / (n + ".npy"))) for n in names}
    b = {n: np.load(str(tmp_path / "o1" / (n + ".npy"))) for n in names}
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert all(v.dtype == (np.float64 if n == "rows" else np.float32) for n, v in a.items())
    rows = a["rows"].astype(np.int64)
    assert len(rows) == bench.DUMP_ROWS and np.all(np.diff(rows) > 0) and rows[-1] < N
    assert np.array_equal(a["out"], out.numpy()[rows]) and np.array_equal(a["x_grad"], X.grad.numpy()[rows])
    assert np.array_equal(a["l2_weights_grad"], layers[1].weights.grad.numpy()) and a["loss"].tolist() == [0.5]
    assert all(np.array_equal(a[n], b[n]) for n in names)


@pytest.mark.gpu
def test_plain_bench_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    """a plain run (no --full): ONE strict JSON line with the contract's keys and nothing that needs runs of its own (no rooflines, CPU
    baseline, config lines, sustained leg or detail file); --dump-outputs writes the last timed step's outputs, and a second run with the
    same arguments gives the same numbers"""
    import numpy as np
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--nodes", "100000", "--edges", "1000000", "--rels", "10"]
    dumps = []
    for k in range(2):
        env = dict(os.environ, RGCN_BENCH_DETAIL=str(tmp_path / f"d{k}.json"))
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--dump-outputs", str(tmp_path / f"o{k}")],
                           capture_output=True, text=True, env=env, timeout=600)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, p.stdout[-2000:]
        line = _strict(lines[0])
        assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["ms_per_step"] > 0
        assert line["unit"] == "edges/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["value"] == pytest.approx(1_000_000 / (line["ms_per_step"] * 1e-3), rel=1e-6)
        assert line["roofline"] is None and not {"cpu_baseline", "configs_ms", "sustained_ms_per_step", "detail"} & set(line)
        assert not (tmp_path / f"d{k}.json").exists()
        dumps.append({f[:-4]: np.load(str(tmp_path / f"o{k}" / f)) for f in os.listdir(tmp_path / f"o{k}")})
    a, b = dumps
    assert set(a) == {"loss", "out", "x_grad", "rows", "l1_weights_grad", "l1_bias_grad", "l2_weights_grad", "l2_bias_grad"}
    assert a["out"].shape == (65536, 16) and a["x_grad"].shape == (65536, 16) and a["l1_weights_grad"].shape == (21, 16, 16)
    assert np.isfinite(a["out"]).all() and np.abs(a["x_grad"]).max() > 0
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and a[n].shape == b[n].shape, n
        assert np.abs(a[n].astype(np.float64) - b[n]).max() <= 1e-5 * max(np.abs(b[n]).max(), 1e-30), n
