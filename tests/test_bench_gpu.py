"""bench.py end to end on one GPU: a plain run prints the headline line with exactly the timed steps asked for, and --dump-outputs writes what the last
timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.timeout(600)
def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--workload", "autopet96", "--batch", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=500, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-1000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True
    assert d["unit"] == "patches/s" and d["dtype"] == "f32" and isinstance(d["metric"], str)
    for extra in ("dispersion", "kernel_pass", "roofline", "eager_rocm_baseline", "cpu_baseline"):
        assert extra not in d, extra                          # --full only
    files = d["dump_outputs"]["files"]
    assert sorted(files) == ["grads", "loss", "params", "reconstruction", "seg_logits"]
    total = 0
    for name in files:
        a = np.load(out / f"{name}.npy")
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    assert abs(float(np.load(out / "loss.npy")[0]) - d["config"]["final_loss"]) <= 1e-5 * max(1.0, abs(d["config"]["final_loss"]))
    assert np.abs(np.load(out / "grads.npy")).sum() > 0
