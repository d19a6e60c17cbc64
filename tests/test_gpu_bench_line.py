"""A plain `bench.py --gpus 1 --steps K --warmup W` run: the result line carries the headline figure and nothing that
takes runs of its own (those are behind --full: tests/test_gpu_dist.py reads one), K sets the timed steps, and
--dump-outputs writes the last timed step's arrays within its size budget."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_prints_the_headline_line_and_dumps_the_last_step(tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "img/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["ms_per_step"] > 0 and "Mask R-CNN R50-FPN detection hot path" in d["metric"]
    assert abs(d["value"] - 2 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]  # 2 images per step
    for moved in ("roofline", "ops", "ms_per_step_windows", "roi_tiles", "cpu_baseline", "extra_workloads"):
        assert moved not in d, moved
    files = sorted(os.listdir(tmp_path))
    for name in ("loss", "box_features", "mask_features", "anchor_labels", "sample_boxes", "mask_logits_grad",
                 "feature_grad_p2", "feature_grad_p3", "feature_grad_p4", "feature_grad_p5"):
        assert name + ".npy" in files, (name, files)
    assert sum(os.path.getsize(tmp_path / f) for f in files) <= 64 * 10 ** 6
    for f in files:
        a = np.load(tmp_path / f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0 and np.isfinite(a).all(), f
    assert np.load(tmp_path / "loss.npy").shape == () and np.abs(np.load(tmp_path / "feature_grad_p2.npy")).max() > 0
