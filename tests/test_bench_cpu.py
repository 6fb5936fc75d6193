"""bench.py harness validation on CPU: the exact torchrun invocation the
driver uses, world_size=2 over gloo-delegated cgx, JSON contract checks."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dist_utils import free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(extra, world=2, timeout=420):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(free_port()), "bench.py",
           "--device", "cpu", "--steps", "2", "--warmup", "1",
           "--batch", "2"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0, f"stdout:\n{r.stdout}\nstderr:\n{r.stderr}"
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert lines, r.stdout
    return json.loads(lines[-1])


def test_bench_resnet_cpu_ws2():
    d = _run_bench(["--gpus", "2"])
    assert d["n_gpus"] == 2
    assert d["value"] > 0
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["bits"] == 4
    assert d["config"]["compression_active"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"


def test_bench_show_registry_ws2():
    d = _run_bench(["--gpus", "2", "--show-registry"])
    split = d["config"]["layerwise_filter"]
    # ResNet-50: conv kernels compressed; BN weights/biases (dim<=1) and
    # small layers registered at bits=32 by the layerwise filter
    assert split["compressed_layers"] > 0
    assert split["bits32_layers"] > 0


def _run_single(extra):
    cmd = [sys.executable, "bench.py", "--device", "cpu", "--steps", "1",
           "--warmup", "0", "--batch", "2"] + extra
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads([ln for ln in r.stdout.splitlines()
                       if ln.startswith("{")][-1])


def test_bench_dump_outputs_and_full(tmp_path):
    """--dump-outputs writes the last timed step's results as float32 .npy
    files within the 64 MB budget; with the same arguments two runs start
    from identical inputs, so their outputs agree; --full still prints the
    headline line and adds the secondary reports to it."""
    a, b = tmp_path / "a", tmp_path / "b"
    d = _run_single(["--dump-outputs", str(a), "--full"])
    assert d["steps"] == 1 and d["ms_per_step"] > 0
    assert "layerwise_filter" in d["config"]
    d2 = _run_single(["--dump-outputs", str(b)])
    assert "layerwise_filter" not in d2["config"]
    assert sorted(p.name for p in a.iterdir()) == ["loss.npy", "params.npy"]
    total = 0
    for f in sorted(a.iterdir()):
        x, y = np.load(f), np.load(b / f.name)
        total += x.nbytes
        assert x.dtype == np.float32 and x.size > 0
        assert np.isfinite(x).all()
        # same seed, same inputs: only fp reassociation may differ
        np.testing.assert_allclose(x, y, rtol=1e-4, atol=1e-5)
    assert total <= 64 * 1000 * 1000
    assert np.load(a / "loss.npy").shape == (1,)
    assert np.load(a / "params.npy").size == 4 * 1024 * 1024


def test_seed_miopen_find_db_merges_without_overwriting(tmp_path, monkeypatch):
    """bench.py adds the recorded find results for shapes the user's MIOpen
    find-db lacks and leaves the user's own entries alone."""
    import bench
    src = os.path.join(ROOT, "benchmarks", "miopen_find_db")
    names = [n for n in os.listdir(src) if n.endswith(".ufdb.txt")]
    assert names
    with open(os.path.join(src, names[0])) as f:
        shipped = f.read().splitlines()
    assert all("=" in ln for ln in shipped)
    monkeypatch.setenv("MIOPEN_USER_DB_PATH", str(tmp_path))
    own_key = shipped[0].split("=", 1)[0]
    (tmp_path / names[0]).write_text(f"{own_key}=Mine:1,0,algo\nother=X:2,0,a")
    bench.seed_miopen_find_db()
    got = (tmp_path / names[0]).read_text().splitlines()
    assert got[:2] == [f"{own_key}=Mine:1,0,algo", "other=X:2,0,a"]
    assert got[2:] == shipped[1:]
    keys = [ln.split("=", 1)[0] for ln in got]
    assert len(keys) == len(set(keys))
    bench.seed_miopen_find_db()
    assert (tmp_path / names[0]).read_text().splitlines() == got
    assert sorted(p.name for p in tmp_path.iterdir()) == [names[0]]


def test_bench_json_contract_single():
    d = _run_single([])
    for key in ["metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"]:
        assert key in d, key
    assert d["n_gpus"] == 1
    # an N=1 run must be honestly labeled: the backend+hook run, but no
    # gradient compression/communication happens
    assert d["config"]["compression_active"] is False
