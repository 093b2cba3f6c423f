"""bench.py's plain run: the timed loop and the line only (everything else is --full), --steps timed steps, and --dump-outputs
writing what the last timed step computed, identically for identical arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "16", "--epoch-len", "2"]


def _run(tmp_path, name):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    out = tmp_path / name
    detail = tmp_path / f"{name}_detail.json"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, "--dump-outputs", str(out), "--detail", str(detail)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    assert not detail.exists()                                   # the detail file is --full's
    return json.loads(lines[0]), out


def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    r, out = _run(tmp_path, "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in r, k
    assert r["steps"] == 3 and r["warmup"] == 1 and r["unit"] == "images/sec" and r["higher_is_better"] is True
    assert abs(r["value"] - 3 * 16 / (r["ms_per_step"] * 3 / 1e3)) <= 1e-3 * r["value"]
    for k in ("train_only_images_per_sec", "cpu_baseline", "kernel_rooflines", "roofline_step", "comm"):
        assert k not in r, k
    files = sorted(os.listdir(out))
    for k in ("loss.npy", "params_sample.npy", "tail_features_sample.npy", "tail_labels_sample.npy", "fds_running_mean.npy", "fds_running_var.npy"):
        assert k in files, (k, files)
    arrays = {f: np.load(os.path.join(out, f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert float(arrays["loss.npy"][0]) == pytest.approx(r["config"]["final_loss"], rel=1e-4)
    assert arrays["tail_features_sample.npy"].shape == (16, 2048)          # 3 steps, epoch length 2: the last tail saw one batch
    assert all(np.isfinite(a).all() for a in arrays.values())
    # identical arguments -> identical inputs: a second run computes the same outputs
    _, out2 = _run(tmp_path, "b")
    assert sorted(os.listdir(out2)) == files
    for f in files:
        np.testing.assert_allclose(np.load(os.path.join(out2, f)), arrays[f], rtol=1e-5, atol=1e-6, err_msg=f)
