"""bench.py's command line on the CPU path: --dump-outputs writes what the last timed step computed,
identically from run to run; a plain run carries the headline fields only and --full adds the
replica check."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--cpu", "--model", "llama-micro",
                        "--seq-len", "64", "--batch-per-gpu", "2", "--steps", "3", "--warmup", "1"] + list(extra),
                       capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_are_float32_and_repeat(tmp_path):
    outs = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for js in outs:
        assert all(k in js for k in HEADLINE) and js["steps"] == 3 and js["ms_per_step"] > 0
        assert js["full"] is False and "params_identical_across_ranks" not in js
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["exp_avg.npy", "exp_avg_sq.npy", "loss.npy", "params.npy"]
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and np.isfinite(a).all() and np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 * 2**20
    assert abs(float(np.load(tmp_path / "a" / "loss.npy")[0]) - outs[0]["final_loss"]) < 1e-3
    assert np.abs(np.load(tmp_path / "a" / "exp_avg.npy")).max() > 0  # three optimizer steps happened


def test_dump_samples_large_buffers_at_fixed_positions(tmp_path, monkeypatch):
    import types

    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    data = torch.arange(1000, dtype=torch.float32).to(torch.bfloat16)
    flat = types.SimpleNamespace(data=data)
    opt = types.SimpleNamespace(exp_avg=torch.ones(50), exp_avg_sq=torch.arange(1000.0), master=None)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(2.5), flat, opt)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("loss", "params", "exp_avg", "exp_avg_sq")}
    assert a["loss"].tolist() == [2.5] and a["exp_avg"].shape == (50,)  # small buffers are written whole
    assert a["params"].shape == a["exp_avg_sq"].shape == (100,)
    idx = a["exp_avg_sq"].astype(np.int64)  # exp_avg_sq[i] == i: the sample shows its own positions
    assert (np.diff(idx) >= 0).all() and len(set(idx.tolist())) > 50
    assert np.array_equal(a["params"], data.float().numpy()[idx])  # same length, same positions
    assert all(np.array_equal(v, np.load(tmp_path / "b" / (n + ".npy"))) for n, v in a.items())


def test_full_adds_the_replica_check():
    js = _bench("--full")
    assert all(k in js for k in HEADLINE) and js["full"] is True
    assert js["params_identical_across_ranks"] is True and js["optimizer_identical_across_ranks"] is True
