"""bench.py: a plain run measures the headline alone; --full adds the per-kernel profile, the roofline, the side
workloads and the CPU baselines beside the same headline fields."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")
FULL_ONLY = ("kernels", "roofline", "cpu_baseline", "other_workloads")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(args), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone(td):
    line = _bench("--n", "2048", "--steps", "2", "--warmup", "1")
    for key in HEADLINE:
        assert key in line, key
    assert line["steps"] == 2 and line["warmup"] == 1 and line["value"] > 0 and line["total_cost"] == 10 * 2048
    for key in FULL_ONLY:
        assert key not in line, key


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements(td):
    line = _bench("--n", "2048", "--steps", "2", "--warmup", "1", "--full", "--no-extras", "--cpu-seconds", "0.5")
    for key in HEADLINE:
        assert key in line, key
    assert line["total_cost"] == 10 * 2048
    assert line["kernels"] and line["roofline"] is not None
    assert line["cpu_baseline"]["last_total"] == 10 * 2048
    assert "other_workloads" not in line


@pytest.mark.gpu
def test_plain_pool_run_has_no_cpu_port(td):
    line = _bench("--workload", "pool", "--steps", "1")
    assert "cpu_baseline" not in line and line["value"] > 0
    for case in line["pool"].values():
        assert case["gpu_ms"] > 0 and "cpu_port_ms" not in case and "reference_binary_ms_build_container" not in case
