"""bench.py as the driver runs it: `python bench.py --gpus N ...` with no launcher around it.  N = 1 prints the contract's JSON
line; N = 2 starts its own ranks (a child `torch.distributed.run`, never a re-exec) -- rehearsed here with the gloo backend so
that both ranks can share the one GPU of the box -- and relays rank 0's line.  The records beside the headline need --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--scale", "1", "--steps", "3", "--warmup", "1", "--full", "--no-strong-x1000", "--no-cpu-baseline"]
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config")


def _run(args, env=None):
    e = dict(os.environ)
    e.pop("WORLD_SIZE", None)
    e.pop("RANK", None)
    e.update(env or {})
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), *args], capture_output=True, text=True, env=e,
                       timeout=900, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]          # stdout carries exactly ONE line
    return json.loads(lines[0])


def test_bench_prints_the_contract_line_on_one_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = _run(SMALL + ["--no-extras"])
    for k in KEYS:
        assert k in out, k
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["value"] > 0 and out["scaling"] == "weak"
    assert "workload" in out["config"] and out["config"]["ranks"] == 1
    assert 0.0 < out["roofline"]["frac"] <= 1.0 and out["roofline"]["bound"] in ("hbm", "mfma")
    assert "supervised pairs" in out["metric"]


def test_bench_gpus_2_starts_its_own_ranks():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    out = _run(["--gpus", "2", "--strong-scale", "2", "--scale", "1", "--steps", "3", "--warmup", "1", "--full",
                "--no-cpu-baseline", "--no-kernels"], env={"MMG_DIST_BACKEND": "gloo"})
    assert out["n_gpus"] == 2 and out["config"]["ranks"] == 2 and out["config"]["collective_backend"] == "gloo"
    assert out["value"] > 0 and "segments" in out["config"]["launch"]           # gloo cannot be recorded: the segment chain
    # north_star's curve -- ONE graph sharded over the ranks -- sits inside `config`, where a parser of the contract keeps it
    for k in ("strong_x2_ms_per_step", "strong_x2_edges_per_s", "strong_x2_d128_ms_per_step", "strong_x2_d128_edges_per_s"):
        assert out["config"][k] > 0, k
    assert out["strong_x1000"]["n_gpus"] == 2 and out["strong_x1000"]["scaling"] == "strong"


FULL_ONLY = ("fixed_supervision_mask", "trainer_epoch", "chain_overhead_ms", "chain", "roofline", "kernels", "strong_x1000",
             "strong_x1000_d128", "cpu_baseline")


def test_bench_plain_run_times_the_headline_and_dumps_its_last_step(tmp_path):
    """Without --full the line carries the headline alone; --dump-outputs writes the last timed step's loss, predictions and
    updated parameters, and two runs with the same arguments write the same arrays (seeded inputs)."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    runs = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        out = _run(["--scale", "1", "--steps", "4", "--warmup", "1", "--dump-outputs", str(d)])
        for k in KEYS:
            assert k in out, k
        assert out["steps"] == 4 and out["ms_per_step"] > 0 and out["value"] > 0
        assert not [k for k in FULL_ONLY if k in out]
        arrays = {f.name[:-4]: np.load(f) for f in d.glob("*.npy")}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert arrays["loss"].shape == () and float(arrays["loss"]) == out["loss"]
        assert arrays["pred"].shape == (out["config"]["train_pairs_rank0"],) and np.isfinite(arrays["pred"]).all()
        assert any(k.startswith("param.") for k in arrays)
        runs.append(arrays)
    assert sorted(runs[0]) == sorted(runs[1])
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
