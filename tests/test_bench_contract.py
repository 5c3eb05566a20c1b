"""bench.py prints ONE JSON line with the fields the driver reads (GPU box only: there is no CPU path to benchmark)."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


#: what a --full line carries beside the headline (N = 1)
FULL_KEYS = {"pipelined", "configs", "eager", "fused_rollout", "fused_rollout_c4", "roofline_large", "gen_obs_large", "one_hot_large",
             "aux_kernels", "device_generation", "persistent", "byte_grid_overhead", "closed_loop", "cpu_baseline",
             "cpu_baseline_1core", "cpu_baseline_python_1core"}


def _bench_line(*extra):
    """Run `bench.py --gpus 1 --steps 40 --warmup 5 [extra]`; returns (its one JSON line, the run's wall seconds)."""
    t0 = time.perf_counter()
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5", *extra],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0]), wall


def _check_headline(d):
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 40 and d["warmup"] == 5
    assert d["higher_is_better"] is True and d["scaling"] == "strong" and d["vs_baseline"] is None    # (N = 1: no other point)
    assert "weak" not in d and "strong" not in d
    assert d["dtype"] == "u8" and d["data"] == "synthetic" and "workload" in d["config"]
    assert "valid" not in d                                     # the product library, no debug knobs
    # the headline is the north-star configuration: Empty-16x16, 4 agents, 65536 envs, all on this GPU
    assert d["config"]["global_batch"] == 65536 and d["config"]["batch_per_gpu"] == 65536 and "16x16" in d["config"]["workload"]
    # --steps is the number of timed steps, and ms_per_step is the timed region over them
    assert d["timed_steps"] == 40 and abs(d["timed_region_ms"] - 40 * d["ms_per_step"]) < 1e-2
    assert d["value"] > 1e8 and abs(d["value"] - 65536 * 4 / (d["ms_per_step"] / 1e3)) / d["value"] < 0.01
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    # the headline is the lock-step path -- ONE launch of the whole batch per step -- so `roofline.frac` is the literal
    # per-launch number a kernel trace reproduces; --full carries the sub-sharded (pipelined) variant beside it with its own
    # per-launch fraction and the aggregate over the step
    assert d["config"]["sub_shards"] == 1 and r["algorithmic_bytes"] == 65536 * 4 * 339
    assert abs(r["ms_per_launch"] - d["ms_per_step"]) / d["ms_per_step"] < 0.1


def test_bench_prints_the_contract_line():
    """The plain run times the headline and nothing else: what --full adds is absent, and the run spends well under 30 s
    outside its warm-up and timed steps."""
    d, wall = _bench_line()
    _check_headline(d)
    assert not FULL_KEYS & set(d), FULL_KEYS & set(d)
    assert wall - (40 + 5) * d["ms_per_step"] / 1e3 < 30, wall


def test_bench_full_carries_every_other_point():
    """--full: the same headline, and beside it the pipelined variant, the other configurations, the HBM-resident kernels and
    the CPU baselines."""
    d, _ = _bench_line("--full")
    _check_headline(d)
    assert FULL_KEYS <= set(d), FULL_KEYS - set(d)
    assert {"c1", "c2", "c3", "c5"} <= set(d["configs"]) and d["roofline"]["hbm_resident"]["batch"] == 1 << 20
    p = d["pipelined"]
    assert p["sub_shards"] == 2 and p["launch"]["batch"] * 2 == 65536          # (mgx_sub_shards' answer: two chains, round 5)
    assert p["value"] > d["value"] * 0.9 and p["launch"]["frac"] < p["step_frac"]
    assert abs(p["step_frac"] - p["launch"]["frac"] * p["mean_launches_in_flight"]) < 0.02


def test_bench_dump_outputs_are_the_last_step_and_repeat_run_to_run(tmp_path):
    """--dump-outputs DIR: what the timed path's last step returned, as float32 / float64 .npy files within 64 MB; the inputs are
    seeded, so two runs with the same arguments write the same arrays."""
    import numpy as np
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5",
                              "--no-extras", "--no-pipelined", "--dump-outputs", str(d)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        assert sum(f.stat().st_size for f in d.iterdir()) <= 64e6
        runs.append({f.stem: np.load(f) for f in d.iterdir()})
    a, b = runs
    assert set(a) == {"obs", "obs_env_index", "dir", "reward", "terminated", "truncated"}
    assert all(v.dtype == (np.float64 if k in ("reward", "obs_env_index") else np.float32) for k, v in a.items())
    B, A, v = 65536, 4, 7
    assert a["dir"].shape == a["reward"].shape == a["terminated"].shape == (B, A) and a["truncated"].shape == (B,)
    idx = a["obs_env_index"]
    assert a["obs"].shape == (len(idx), A, v, v, 3) and len(idx) > 1000
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < B
    assert a["obs"].any() and set(np.unique(a["dir"])) <= {0.0, 1.0, 2.0, 3.0}
    for k in a:
        assert np.array_equal(a[k], b[k]), k
