"""bench.py: --dump-outputs writes a fixed, bounded set of arrays; a plain run and a --full run time the same sweep and return the
same outputs, and only --full takes the figures beyond the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_the_same_rows_within_the_limit(tmp_path):
    N, M = 1 << 14, 41
    g = torch.Generator().manual_seed(5)
    arrays = {"log_weights": torch.randn(N, dtype=torch.float64, generator=g), "T1": torch.randn(N, M, M, dtype=torch.float64, generator=g),
              "ancestors": torch.arange(N, dtype=torch.int32), "S": torch.randn(M, M, dtype=torch.float64, generator=g)}
    assert 8 * sum(t.numel() for t in arrays.values()) > bench.DUMP_MAX_BYTES
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), arrays, rows=N)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["S.npy", "T1.npy", "ancestors.npy", "log_weights.npy", "sampled_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in names) <= bench.DUMP_MAX_BYTES
    rows = np.load(tmp_path / "a" / "sampled_rows.npy").astype(np.int64)
    assert rows.shape == (bench.DUMP_SAMPLE_ROWS,) and np.all(np.diff(rows) > 0)
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float64 and np.array_equal(a, b), n
    assert np.array_equal(np.load(tmp_path / "a" / "ancestors.npy"), rows)
    assert np.array_equal(np.load(tmp_path / "a" / "T1.npy"), arrays["T1"].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "S.npy"), arrays["S"].numpy())


def test_dump_outputs_small_arrays_whole_and_too_large_refused(tmp_path):
    traj = torch.randn(2000, 2, dtype=torch.float64)
    bench.dump_outputs(torch, str(tmp_path / "small"), {"trajectory": traj})
    assert sorted(os.listdir(tmp_path / "small")) == ["trajectory.npy"]
    assert np.array_equal(np.load(tmp_path / "small" / "trajectory.npy"), traj.numpy())
    with pytest.raises(SystemExit):
        bench.dump_outputs(torch, str(tmp_path / "big"), {"x": torch.zeros(bench.DUMP_MAX_BYTES // 8 + 1, dtype=torch.float64)})
    assert not (tmp_path / "big").exists()


def _run_bench(args, timeout):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_plain_and_full_time_the_same_sweep(tmp_path):
    T = 64
    common = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--particles", "65536", "--T", str(T)]
    plain = _run_bench(common + ["--dump-outputs", str(tmp_path / "plain")], timeout=300)
    full = _run_bench(common + ["--full", "--cpu-steps", "2", "--dump-outputs", str(tmp_path / "full")], timeout=600)
    for r in (plain, full):
        assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["unit"] == "particle-steps/s"
        assert r["higher_is_better"] is True and r["dtype"] == "f64"
        assert r["value"] == pytest.approx(65536 * (T - 1) / (r["ms_per_step"] * 1e-3), rel=1e-9)
    assert "cpu_baseline" not in plain and "roofline" not in plain and plain["config"]["verified"].startswith("not checked")
    assert "cpu_baseline" in full and full["config"]["verified"].startswith("last timed sweep checked")
    assert os.listdir(tmp_path / "plain") == ["trajectory.npy"] and os.listdir(tmp_path / "full") == ["trajectory.npy"]
    a, b = np.load(tmp_path / "plain" / "trajectory.npy"), np.load(tmp_path / "full" / "trajectory.npy")
    assert a.shape == (T, 2) and a.dtype == np.float64 and np.isfinite(a).all()
    assert np.array_equal(a, b)
