"""bench.py's run modes: a plain run times --steps clips and prints the headline line only; --full adds the legs after the timed region;
--dump-outputs writes what the timed path returned in its last step (float32 .npy, at most 64 MB, seeded sample beyond that)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def test_dump_outputs_writes_float32_and_samples_within_the_limit(tmp_path):
    import bench
    small = torch.arange(12, dtype=torch.bfloat16).reshape(3, 4)
    big = torch.randn(4096, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    limit = 8192                                   # 4096 bytes per array: `small` fits, `big` (16 KB as float32) is sampled
    bench.dump_outputs(str(tmp_path / "a"), {"small": small, "big": big}, limit=limit)
    bench.dump_outputs(str(tmp_path / "b"), {"small": small, "big": big}, limit=limit)
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.float().numpy())
    assert b.dtype == np.float32 and b.size == 1024 and s.nbytes + b.nbytes <= limit
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))          # the same positions on every run
    assert np.isin(b, big.float().numpy()).all()


def test_full_and_dump_outputs_are_off_by_default(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--ddim-steps", "4", *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_full_adds_the_legs(tmp_path):
    d = _bench("--dump-outputs", str(tmp_path / "plain"))
    assert all(k in d for k in HEADLINE_KEYS) and d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert not {"roofline", "cpu_baseline", "end_to_end"} & set(d) and d["config"]["output_finite"]
    plain = np.load(tmp_path / "plain" / "videos.npy")
    assert plain.dtype == np.float32 and plain.shape == (1, 4, 16, 32, 32) and np.isfinite(plain).all()

    f = _bench("--full", "--no-cpu-baseline", "--no-psnr", "--no-end-to-end", "--dump-outputs", str(tmp_path / "full"))
    assert f["steps"] == 2 and f["roofline"]["frac"] > 0 and f["config"]["achieved_tflops"] > 0
    full = np.load(tmp_path / "full" / "videos.npy")
    # same arguments, same seeded inputs and weights, same timed path: --full only adds work after it
    rng = float(plain.max() - plain.min())
    assert np.abs(full - plain).max() <= 1e-3 * rng
