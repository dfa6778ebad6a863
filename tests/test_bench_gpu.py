"""GPU: a plain `bench.py` run as the driver starts it — the headline line only (the --full legs null), and --dump-outputs
writing what the last timed step returned, the same arrays bit for bit when the same command runs twice."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENVS = 256


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--envs", str(ENVS),
           "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    first = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in first, k
    assert first["steps"] == 20 and first["value"] > 0 and first["ms_per_step"] > 0 and first["full"] is False
    assert first["value"] == pytest.approx(ENVS * 1e3 / first["ms_per_step"], rel=1e-9)
    for k in ("sustained", "solver_sibling", "tolerance_sibling", "train", "train_kernel_shares", "learner_rooflines"):
        assert first[k] is None, k
    assert "cpu_baseline" not in first
    shapes = {"reward": (ENVS,), "done": (ENVS,), "failed": (ENVS,), "info": (ENVS, 7), "obs": (ENVS, 5, 144),
              "voltage": (ENVS, 33)}
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in shapes)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in shapes}
    for k, shape in shapes.items():
        assert got[k].shape == shape and got[k].dtype in (np.float32, np.float64), (k, got[k].shape, got[k].dtype)
        assert np.isfinite(got[k]).all(), k
    assert set(np.unique(got["done"])) <= {0.0, 1.0} and not got["failed"].any()
    assert (got["voltage"] > 0.5).all() and (got["voltage"] < 1.5).all()

    _bench(tmp_path / "b")
    for k in shapes:
        assert np.array_equal(np.load(tmp_path / "b" / (k + ".npy")), got[k]), k
