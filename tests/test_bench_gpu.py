"""bench.py without --full: the headline figure and nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_run_measures_the_headline_only(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` sets up, warms up, times the K steps, writes the last step's
    outputs and prints the line.  Every other leg (roofline, sustained, batch sweep, product modes, parity, CPU baselines, e2e, train,
    render, fit) runs under --full only, and so does the write of bench_detail.json."""
    detail = os.path.join(ROOT, "bench_detail.json")
    before = os.stat(detail).st_mtime_ns if os.path.exists(detail) else None
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == "denoise-steps/sec" and line["unit"] == "denoise-steps/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["n_gpus"] == 1 and line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] > 0 and abs(line["value"] * line["ms_per_step"] - 4 * 1000) < 4.0     # value = B * K / s, ms_per_step = 1000 s / K
    for k in ("roofline", "cpu_baseline", "parity", "e2e", "render", "fit", "train", "rccl", "detail"):
        assert line[k] is None, k
    assert line["summary"]["denoise_steps_per_s_b4"] == line["value"] and line["summary"]["render_mrays_per_s"] is None
    after = os.stat(detail).st_mtime_ns if os.path.exists(detail) else None
    assert after == before
    for name in ("sample", "pred_xstart"):
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == (4, 27, 256, 256) and np.isfinite(a).all()
