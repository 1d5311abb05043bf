"""bench.py's host side (no GPU): the options that shape a run and the writer behind --dump-outputs."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _bench():
    import bench
    bench.torch = torch
    return bench


def test_dump_outputs_writes_small_tensors_whole_and_large_ones_as_a_fixed_sample(tmp_path):
    B = _bench()
    g = torch.Generator().manual_seed(3)
    arrays = {"loss": torch.tensor([2.5]), "params": torch.randn(1000, generator=g), "seg_logits": torch.randn(2, 2, 100, 100, 500, generator=g).to(torch.bfloat16),
              "dice": torch.tensor([0.25, 0.5], dtype=torch.float64)}
    a = B._dump_outputs(str(tmp_path / "a"), arrays)
    b = B._dump_outputs(str(tmp_path / "b"), arrays)
    assert a["files"] == b["files"] and a["bytes"] <= B.DUMP_LIMIT
    assert a["files"]["params"] == [1000] and a["files"]["seg_logits"] == f"sample {B.DUMP_SAMPLE} of {2 * 2 * 100 * 100 * 500}"
    for name in arrays:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == (np.float64 if name == "dice" else np.float32)
        assert np.array_equal(x, y), name                       # the same run writes the same values: the sample indices are fixed
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "params.npy"), arrays["params"].numpy())
    s = np.load(tmp_path / "a" / "seg_logits.npy")
    assert s.shape == (B.DUMP_SAMPLE,) and np.isin(s, arrays["seg_logits"].float().reshape(-1).numpy()).all()


def test_train_outputs_are_what_a_caller_of_the_step_holds():
    import types
    B = _bench()
    outs = [[torch.randn(2, 2, 4, 4, 4), torch.zeros(1)], [torch.randn(2, 1, 4, 4, 4), torch.zeros(1)], [torch.randn(2, 1, 4, 4, 4), torch.zeros(1)]]
    eng = types.SimpleNamespace(flush=lambda: None, loss=torch.tensor(1.5), flat=types.SimpleNamespace(param=torch.randn(10), grad=torch.randn(10)),
                                graphs={}, _outs=outs, last_outputs=None, model=types.SimpleNamespace(num_branches=3))
    sync = torch.cuda.synchronize
    torch.cuda.synchronize = lambda *a: None
    try:
        r = B._train_outputs(eng)
    finally:
        torch.cuda.synchronize = sync
    assert sorted(r) == ["grads", "loss", "params", "reconstruction", "seg_logits"]
    assert r["seg_logits"] is outs[0][0] and torch.equal(r["reconstruction"], torch.cat([outs[1][0], outs[2][0]], dim=1)) and r["loss"].shape == (1,)


def test_options_of_a_run():
    run = lambda *a: subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *a], capture_output=True, text=True, timeout=120, cwd=ROOT)
    h = run("--help")
    assert h.returncode == 0 and "--full" in h.stdout and "--dump-outputs" in h.stdout
    r = run("--steps", "0")
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr
