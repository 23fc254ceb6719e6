"""bench.py --dump-outputs: the writer (bench.dump_outputs) stores each array as float32
.npy, cuts an array above its byte budget to a fixed seeded sample, and bench.py takes
the options a plain and a full run are started with.  CPU only."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_float32_npy(tmp_path):
    arrays = {"loss": torch.tensor(1.5, dtype=torch.float64),
              "est_source": torch.arange(24, dtype=torch.bfloat16).reshape(2, 3, 4)}
    out = tmp_path / "sub" / "dir"            # created on demand
    bench.dump_outputs(str(out), arrays)
    assert sorted(os.listdir(out)) == ["est_source.npy", "loss.npy"]
    loss = np.load(out / "loss.npy")
    est = np.load(out / "est_source.npy")
    assert loss.dtype == est.dtype == np.float32
    assert loss.shape == () and float(loss) == 1.5
    assert est.shape == (2, 3, 4)
    assert np.array_equal(est, np.arange(24, dtype=np.float32).reshape(2, 3, 4))


def test_dump_outputs_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_ARRAY_BYTES", 4 * 100)      # 100 float32 elements
    big = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    small = torch.arange(100, dtype=torch.float32)               # exactly at the budget: whole
    bench.dump_outputs(str(tmp_path / "a"), {"big": big, "small": small})
    bench.dump_outputs(str(tmp_path / "b"), {"big": big + 0.5, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == b.shape == (100,) and a.dtype == np.float32
    # the values are their own flat indices: 100 distinct ones, ascending, the same in both runs
    assert len(set(a.tolist())) == 100 and (np.diff(a) > 0).all()
    assert np.array_equal(b, a + 0.5)
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())


def test_default_budget_keeps_four_arrays_under_64_mb():
    assert 4 * (bench.DUMP_ARRAY_BYTES + 128) <= 64 * 10 ** 6    # 128: the .npy header


def test_bench_options():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs", "--full"):
        assert opt in p.stdout
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps" in p.stderr
