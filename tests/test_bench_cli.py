"""bench.py's command line: --dump-outputs (what the timed path returned, as .npy files) and the plain run's line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_seeded_row_sample(tmp_path):
    import bench
    b = bench.DUMP_ROWS + 1000
    lp = torch.arange(b, dtype=torch.float32)                # row index as value: the sample can be read back
    z = lp[:, None].repeat(1, bench.D)
    lq = -lp
    stats = torch.tensor([float(lp.sum()), float(b)], dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), lp, stats, z, lq)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["log_prob.npy", "log_prob_sum_count.npy", "sample_log_q.npy", "sample_z.npy"]
    total = 0
    for n in names:
        a, a2 = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64)
        assert np.array_equal(a, a2), n                      # the same rows every run
        total += os.path.getsize(tmp_path / "a" / n)
    assert total <= 64 << 20
    rows = np.load(tmp_path / "a" / "log_prob.npy")
    assert rows.shape == (bench.DUMP_ROWS,) and len(np.unique(rows)) == bench.DUMP_ROWS
    assert np.all(np.diff(rows) > 0) and rows[-1] < b
    assert np.array_equal(np.load(tmp_path / "a" / "sample_z.npy"), np.repeat(rows[:, None], bench.D, 1))
    assert np.array_equal(np.load(tmp_path / "a" / "sample_log_q.npy"), -rows)
    assert np.load(tmp_path / "a" / "log_prob_sum_count.npy").tolist() == stats.tolist()


def test_dump_outputs_small_batch_whole(tmp_path):
    import bench
    lp, lq = torch.randn(300), torch.randn(300)
    z = torch.randn(300, bench.D)
    bench.dump_outputs(str(tmp_path), lp, torch.zeros(2, dtype=torch.float64), z, lq)
    assert np.array_equal(np.load(tmp_path / "log_prob.npy"), lp.numpy())
    assert np.array_equal(np.load(tmp_path / "sample_z.npy"), z.numpy())


@pytest.mark.gpu
def test_plain_run_line_and_dump(hip, tmp_path):
    """A plain run prints the headline line (no --full legs) and writes the last timed step's outputs."""
    batch, out = 8192, tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--batch", str(batch), "--dump-outputs", str(out)]
    run = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-4000:]
    line = json.loads(run.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["value"] > 0 and line["unit"] == "transforms/s" and line["higher_is_better"] is True
    for k in ("other_matrix_path", "extra_configs", "cpu_baseline", "log_prob_rate", "roofline_hbm_spline_kernel"):
        assert k not in line, k
    lp, z, lq = (np.load(out / (n + ".npy")) for n in ("log_prob", "sample_z", "sample_log_q"))
    stats = np.load(out / "log_prob_sum_count.npy")
    assert lp.shape == (batch,) and z.shape == (batch, 64) and lq.shape == (batch,)
    assert lp.dtype == np.float32 and stats.dtype == np.float64
    assert np.isfinite(lp).all() and np.isfinite(z).all() and np.isfinite(lq).all()
    assert stats[1] == batch and abs(stats[0] - lp.astype(np.float64).sum()) <= 1e-6 * abs(stats[0]) + 1e-3
