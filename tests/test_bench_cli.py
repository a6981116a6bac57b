"""bench.py's command line: a plain run prints the headline only, --full adds the records that take
runs of their own, --dump-outputs writes the last timed step's logits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._util import CONV_TOL, normwise_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config")
FULL_ONLY = ("roofline", "layer_roofline", "cpu_baseline")
SMALL = ["--gpus", "1", "--image", "32", "--batch", "8", "--classes", "10", "--model", "resnet20"]


def run_bench(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_outputs_float32_and_fixed_sample(tmp_path, monkeypatch):
    import bench

    t = torch.arange(4096, dtype=torch.float64).reshape(64, 64)
    bench.dump_outputs(str(tmp_path / "a"), {"logits": t.to(torch.bfloat16), "wide": t})
    a, w = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "a" / "wide.npy")
    assert a.dtype == np.float32 and a.shape == (64, 64) and w.dtype == np.float64
    assert np.array_equal(w, t.numpy()) and np.array_equal(a, t.to(torch.bfloat16).float().numpy())
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)  # the file with its header: 96 float64 of the 4096
    bench.dump_outputs(str(tmp_path / "b"), {"wide": t})
    bench.dump_outputs(str(tmp_path / "c"), {"wide": t})
    s = np.load(tmp_path / "b" / "wide.npy")
    assert s.shape == (96,) and os.path.getsize(tmp_path / "b" / "wide.npy") <= 1024
    assert np.array_equal(s, np.load(tmp_path / "c" / "wide.npy"))
    assert np.all(np.diff(s) > 0) and np.isin(s, t.numpy()).all()  # distinct elements of t, in order


def test_steps_and_warmup_are_validated():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--selftest", "--steps", "0"], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_and_full_runs(tmp_path):
    """The same small chain twice, plain (eager steps) and --full (steps replayed from a HIP graph, so the
    dominant kernel is timed from launches of its own): the plain line is the headline alone, the --full
    line carries the roofline records too, both time exactly --steps steps and dump the same logits (same
    seeded inputs; the autotuner may pick another plan, so equal within the conv parity bar)."""
    plain = run_bench(SMALL + ["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / "p")])
    full = run_bench(SMALL + ["--steps", "2", "--warmup", "1", "--graph", "--full", "--no-cpu-baseline",
                              "--dump-outputs", str(tmp_path / "f")])
    for out, steps in ((plain, 3), (full, 2)):
        assert all(k in out for k in HEADLINE), out
        assert out["steps"] == steps and out["unit"] == "images/s" and out["higher_is_better"] is True
        # value = images per step / time per step; ms_per_step is printed with 3 decimals
        assert out["ms_per_step"] > 0 and abs(8 * 1e3 / out["value"] - out["ms_per_step"]) <= 0.0006
    assert plain["full"] is False and not any(k in plain for k in FULL_ONLY), plain
    assert full["full"] is True and all(k in full for k in FULL_ONLY), full
    assert full["roofline"]["avg_launch_ms"] > 0
    p, f = np.load(tmp_path / "p" / "logits.npy"), np.load(tmp_path / "f" / "logits.npy")
    assert p.dtype == np.float32 and p.shape == (8, 10) and np.isfinite(p).all() and np.abs(p).max() > 0
    assert normwise_err(f, p) <= CONV_TOL
