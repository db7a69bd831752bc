"""bench.py's plain run on the GPU at a toy size: the result line carries the headline fields and
none of the `--full` objects, `--steps` sets the number of timed steps, and `--dump-outputs`
writes the last timed step's loss, state and gradients as float arrays."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_outputs(dev, tmp_path):
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--height", "256", "--width", "256", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(line) == 1, r.stdout
    out = json.loads(line[0])
    assert out["steps"] == 2 and out["unit"] == "frames/s" and out["dtype"] == "fp32" and out["higher_is_better"]
    # 2 samples x 2 views per step
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] * 1e-3 - 4) < 1e-2
    for k in ("f32_exact", "perf_bf16", "dmap", "bl", "cpu_baseline"):
        assert k not in out, k
    assert sorted(os.listdir(out_dir)) == ["grads.npy", "loss.npy", "state.npy"]
    loss, state, grads = (np.load(out_dir / f"{n}.npy") for n in ("loss", "state", "grads"))
    assert loss.dtype == np.float64 and loss.shape == (1,) and loss[0] == out["config"]["last_loss"]
    assert state.dtype == np.float32 and grads.dtype == np.float32 and 0 < grads.size < state.size
    assert np.isfinite(state).all() and np.isfinite(grads).all() and np.abs(grads).max() > 0
    assert sum(a.nbytes for a in (loss, state, grads)) <= 64 << 20
    assert os.listdir(tmp_path) == ["dump"]  # nothing else left behind
