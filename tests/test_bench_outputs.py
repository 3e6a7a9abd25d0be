"""bench.py's plain / --full split and --dump-outputs on CPU: a plain run asks for none of the
extra measurements, --full keeps them with their --no-* switches, and dump_outputs writes float32
or float64 .npy files, whole within the byte budget and as a fixed seeded sample beyond it.
The dump of a real run is tests/test_gpu_configs.py::test_bench_plain_run_dumps_last_step."""
import json
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_measures_only_the_steps():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert a.no_kernel_timing and a.no_cpu_baseline


def test_full_keeps_every_measurement_and_its_switches():
    a = bench.parse_args(["--full"])
    assert a.full and not a.no_kernel_timing and not a.no_cpu_baseline and a.stream_probe and a.hbm_only
    b = bench.parse_args(["--full", "--no-cpu-baseline", "--no-stream-probe"])
    assert b.no_cpu_baseline and not b.no_kernel_timing and not b.stream_probe
    assert bench.parse_args(["--full", "--in-flight-timing"]).in_flight_timing
    with pytest.raises(SystemExit):
        bench.parse_args(["--in-flight-timing"])


def test_dump_whole_within_budget(tmp_path):
    d16 = (torch.arange(6 * 5, dtype=torch.int32).reshape(1, 6, 5) - 16).to(torch.int16)
    xyz = torch.linspace(-3, 3, 90, dtype=torch.float32).reshape(1, 6, 5, 3)
    cnt = np.array([3.0, 5.0])
    bench.dump_outputs(str(tmp_path / "o"), {"disparity": d16, "xyz": xyz, "counts": cnt})
    got = {f: np.load(tmp_path / "o" / f) for f in sorted(os.listdir(tmp_path / "o")) if f.endswith(".npy")}
    assert sorted(got) == ["counts.npy", "disparity.npy", "xyz.npy"]
    assert got["disparity.npy"].dtype == np.float32 and np.array_equal(got["disparity.npy"], d16.numpy())
    assert got["xyz.npy"].dtype == np.float32 and np.array_equal(got["xyz.npy"], xyz.numpy())
    assert got["counts.npy"].dtype == np.float64 and np.array_equal(got["counts.npy"], cnt)
    man = json.load(open(tmp_path / "o" / "outputs.json"))
    assert man["xyz"] == {"shape": [1, 6, 5, 3], "dtype": "float32", "sampled": False}


def test_dump_samples_beyond_budget_the_same_every_time(tmp_path):
    big = torch.arange(3 << 20, dtype=torch.float32)        # 12 MiB
    other = torch.arange(1 << 20, dtype=torch.float32) * 2  # 4 MiB
    small = torch.ones(10, dtype=torch.float32)
    budget = 4 << 20
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "other": other, "small": small}, budget=budget)
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("big", "other", "small")}
    b = {n: np.load(tmp_path / "b" / f"{n}.npy") for n in ("big", "other", "small")}
    assert sum(v.nbytes for v in a.values()) <= budget
    assert a["small"].shape == (10,)                         # small arrays stay whole
    assert 0.2 * big.numel() < a["big"].size < big.numel() // 3 + 1   # each in proportion (1/4 here)
    assert abs(a["big"].size / big.numel() - a["other"].size / other.numel()) < 1e-3
    for n in a:
        assert a[n].dtype == np.float32 and np.array_equal(a[n], b[n])
    # a sample holds elements of the array at sorted positions (values = positions here)
    assert np.all(np.diff(a["big"]) >= 0) and a["big"].max() < big.numel()
    man = json.load(open(tmp_path / "a" / "outputs.json"))
    assert man["big"]["sampled"] and man["big"]["shape"] == [3 << 20] and not man["small"]["sampled"]


def test_dump_names_other_ranks(tmp_path):
    bench.dump_outputs(str(tmp_path), {"disparity": torch.zeros(4, dtype=torch.int16)}, rank=2)
    assert sorted(os.listdir(tmp_path)) == ["disparity_rank2.npy", "outputs_rank2.json"]
