"""CPU side of the ensemble inference (utils/ensemble.py, csrc/ensemble.hip): the restatement the GPU tests lean on against torch.softmax in fp64, the weight rule,
every argument error of the Python surface -- raised before any GPU work, so also on a machine without a GPU --, the error codes of the two C-ABI entries, which
check their arguments before they launch, and the command lines of run_test.py (unchanged) and run_ensemble.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ensemble_ref as ER

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INF, NAN = float("inf"), float("nan")


def _randn(shape, seed, scale=1.0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale


@pytest.mark.parametrize("scale", [1.0, 10.0, 80.0])
@pytest.mark.parametrize("K", [1, 2, 4, 9])
def test_restated_softmax_equals_torch_fp64_on_random_columns(K, scale):
    """the same formula in the same precision: the maximum is exact, and exp, the sum over at most 9 terms and the quotient differ by a few fp64 roundings at most"""
    x = _randn((2, K, 3, 5, 7), 11 + K, scale)
    got, want = ER.softmax64(x), torch.softmax(x, dim=1, dtype=torch.float64)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 16 * 2.0 ** -53
    assert float((got.sum(1) - 1).abs().max()) <= 16 * 2.0 ** -53


def test_restated_softmax_equals_torch_fp64_on_special_columns():
    cols = torch.tensor([[0.0, -INF, -INF, 0.0],            # two of four: 0.5, 0, 0, 0.5 exactly
                         [-INF, -INF, -INF, -INF],          # all -inf: all-NaN
                         [0.0, INF, 1.0, -INF],             # a +inf: all-NaN
                         [0.0, NAN, 1.0, 2.0],              # a NaN: all-NaN
                         [INF, INF, 0.0, 0.0],
                         [3.0, -INF, -200.0, 3.0]]).t().reshape(1, 4, 6, 1, 1)
    got, want = ER.softmax64(cols), torch.softmax(cols, dim=1, dtype=torch.float64)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.equal(torch.isnan(got)[0, :, :, 0, 0].all(0), torch.tensor([False, True, True, True, True, False]))
    assert torch.equal(torch.isnan(got)[0, :, :, 0, 0].any(0), torch.tensor([False, True, True, True, True, False]))
    ok = ~torch.isnan(got)
    assert torch.equal(got[ok], want[ok])
    assert got[0, :, 0, 0, 0].tolist() == [0.5, 0.0, 0.0, 0.5] and got[0, 1, 5, 0, 0] == 0.0
    h = ER.entropy64(got)[0, 0, :, 0, 0]
    assert abs(float(h[0]) - np.log(2.0)) <= 2.0 ** -52 and bool(torch.isnan(h[1:5]).all())


def test_restated_argmax_rule_is_first_nan_else_first_maximum():
    x = torch.tensor([[1.0, 3.0, 3.0], [NAN, 5.0, NAN], [2.0, NAN, 9.0], [-0.0, 0.0, -1.0], [-INF, -INF, -INF], [0.25, 0.25, 0.5]]).t().reshape(1, 3, 6)
    assert ER.argmax_rule(x)[0, 0].tolist() == [1, 0, 1, 0, 0, 2]
    y = _randn((2, 5, 40), 3)
    assert torch.equal(ER.argmax_rule(y).long(), y.argmax(1, keepdim=True))


def test_exact_columns_are_what_they_say():
    for K in (1, 2, 3, 4, 5, 9):
        x, p = ER.exact_columns(K, (3, 5, 7), K)
        want = ER.softmax64(x[None], 1)[0]
        assert ER.same_bits(p, want.float()) and torch.equal(torch.isnan(want), torch.isnan(want.float()))
        assert bool(torch.isnan(p[:, 0, 0, :3]).all()) and not bool(torch.isnan(p.flatten(1)[:, 3:]).any())
        vals = set(p.flatten()[~torch.isnan(p.flatten())].tolist())
        assert vals <= {0.0, 0.25, 0.5, 1.0, float(np.float32(1) / np.float32(3)), float(np.float32(0.2))} and (K < 2 or 0.5 in vals) and (K < 3 or len(vals) >= 4)


def test_weight_normalisation():
    from veloxseg_amd.utils.ensemble import normalise_weights
    for n in (1, 2, 3, 4, 5, 7):
        w = normalise_weights(None, n)
        assert w == [float(np.float32(1.0 / n))] * n and w == ER.normalise_weights(None, n)
    assert normalise_weights(None, 3)[0] != 1.0 / 3                             # the fp32 value, not the fp64 one
    assert normalise_weights([0.5, 0.25, 0.25], 3) == [0.5, 0.25, 0.25]
    assert normalise_weights([2, 1, 1], 3) == [0.5, 0.25, 0.25]
    assert normalise_weights([1, 2, 3], 3) == [float(np.float32(1 / 6)), float(np.float32(2 / 6)), float(np.float32(3 / 6))] == ER.normalise_weights([1, 2, 3], 3)
    assert normalise_weights((np.float32(3.0),), 1) == [1.0]
    assert normalise_weights(torch.tensor([1.0, 3.0]), 2) == [0.25, 0.75]
    for w in normalise_weights([0.3, 0.3, 0.4], 3):
        assert w == float(np.float32(w))


BAD_WEIGHTS = [[], [1.0], [1.0, 1.0, 1.0], [1.0, 0.0], [1.0, -1.0], [1.0, INF], [1.0, NAN], [1.0, "1"], [1.0, None], [True, 1.0], 0.5, "ab", [1e-300, 1e300]]


class _Declares(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.n_classes = k

    def forward(self, x):
        raise AssertionError("a model ran although the arguments are bad")


def test_argument_errors_are_raised_before_any_gpu_work():
    """everything below runs on CPU tensors on a machine without a GPU: a ValueError must come before the "MI355X only" RuntimeError, which comes before any launch"""
    from veloxseg_amd.utils import ensemble as E
    from veloxseg_amd.utils.inference_runtime import Net
    vol = torch.zeros((1, 1, 8, 8, 8))
    two = [_Declares(2).train(), _Declares(2).eval()]
    for bad in BAD_WEIGHTS:
        with pytest.raises(ValueError, match="weights"):
            E.normalise_weights(bad, 2)
        with pytest.raises(ValueError, match="weights"):
            E.infer_ensemble(two, vol, (4, 4, 4), 1, 0.5, weights=bad)
        with pytest.raises(ValueError, match="weights"):
            E.softmax_mean([torch.zeros((1, 2, 2, 2, 2))] * 2, weights=bad)
    for empty in ([], ()):
        with pytest.raises(ValueError, match="at least one"):
            E.infer_ensemble(empty, vol, (4, 4, 4), 1, 0.5)
        with pytest.raises(ValueError, match="at least one"):
            E.softmax_mean(empty)
    with pytest.raises(ValueError, match="classes"):
        E.infer_ensemble([_Declares(2), Net(_Declares(3))], vol, (4, 4, 4), 1, 0.5)
    with pytest.raises(ValueError, match="classes"):
        E.softmax_mean([torch.zeros((1, 2, 2, 2, 2)), torch.zeros((1, 3, 2, 2, 2))])
    with pytest.raises(ValueError, match="shapes"):
        E.softmax_mean([torch.zeros((1, 2, 2, 2, 2)), torch.zeros((1, 2, 2, 2, 4))])
    with pytest.raises(ValueError, match="float32"):
        E.softmax_mean([torch.zeros((1, 2, 2, 2, 2), dtype=torch.float64)])
    with pytest.raises(ValueError, match="native"):
        E.infer_ensemble(two, vol, (4, 4, 4), 1, 0.5, native={"native_shape": (8, 8, 8)})
    with pytest.raises(RuntimeError, match="MI355X only"):
        E.infer_ensemble(two, vol, (4, 4, 4), 1, 0.5)
    with pytest.raises(RuntimeError, match="MI355X only"):
        E.infer_ensemble(two, vol, (4, 4, 4), 1, 0.5, weights=[1, 2], entropy=True)
    with pytest.raises(RuntimeError, match="MI355X only"):
        E.softmax_mean([torch.zeros((1, 2, 2, 2, 2))] * 2)
    assert two[0].training and not two[1].training
    with pytest.raises(RuntimeError, match="MI355X only"):
        E.ProbabilityAccumulator(2, (4, 4, 4), "cpu")
    for K in (0, 257):
        with pytest.raises(ValueError, match="classes"):
            E.ProbabilityAccumulator(K, (4, 4, 4), "cuda")
    for kw in (dict(spatial=(4, 4)), dict(spatial=(4, 0, 4)), dict(spatial=(4, 4, 4), batch=0)):
        with pytest.raises(ValueError, match="extent"):
            E.ProbabilityAccumulator(2, device="cuda", **kw)


def test_new_entry_points_return_error_codes_without_gpu():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    # (logits, psum, B, K, V, weight, first, stream): pointers that are never dereferenced -- every call fails its checks first
    for ptrs in ((None, 32), (16, None), (None, None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            _hip.call("vx_softmax_accumulate", *ptrs, 1, 2, 64, 0.5, 1, None)
    with pytest.raises(RuntimeError, match="alias"):
        _hip.call("vx_softmax_accumulate", 16, 16, 1, 2, 64, 0.5, 1, None)
    for K in (0, -1, 257):
        with pytest.raises(RuntimeError, match=f"{K} classes outside 1..256"):
            _hip.call("vx_softmax_accumulate", 16, 32, 1, K, 64, 0.5, 1, None)
        with pytest.raises(RuntimeError, match=f"{K} classes outside 1..256"):
            _hip.call("vx_prob_finalize", 16, 32, 48, 1, K, 64, None)
    for B, V in ((0, 64), (-1, 64), (1, 0), (1, -4)):
        with pytest.raises(RuntimeError, match="non-positive extent"):
            _hip.call("vx_softmax_accumulate", 16, 32, B, 2, V, 0.5, 0, None)
        with pytest.raises(RuntimeError, match="non-positive extent"):
            _hip.call("vx_prob_finalize", 16, 32, None, B, 2, V, None)
    # (psum, labels, entropy, B, K, V, stream): either output may be null, not both
    for ptrs in ((None, 32, 48), (16, None, None), (None, None, None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            _hip.call("vx_prob_finalize", *ptrs, 1, 2, 64, None)
    assert {"vx_softmax_accumulate", "vx_prob_finalize"} <= set(_hip.LIB.protos)


def _run(script, *extra):
    base = ["--dataset_name", "AutoPETII", "--model_name", "VeloxSeg", "--model_config", "m.json", "--train_config", "t.json", "--test_config", "e.json"]
    return subprocess.run([sys.executable, os.path.join(ROOT, script), *base, *extra], capture_output=True, text=True, timeout=120)


def test_run_test_parses_as_before_and_run_ensemble_takes_its_command_line():
    """both command lines end at their first check after parsing (--use_hd95 is refused before any file is read or torch is imported), so this needs no GPU.
    run_test.py is the file it was: its arguments parse and the refusal of --use_hd95 stays.  run_ensemble.py takes EVERY option of run_test.py (read from the two
    --help texts, so the two cannot drift apart unnoticed), with a list of names in --checkpoint_index, which it requires, and refuses --use_hd95 too"""
    import re
    opts = {}
    for script in ("run_test.py", "run_ensemble.py"):
        h = subprocess.run([sys.executable, os.path.join(ROOT, script), "--help"], capture_output=True, text=True, timeout=120)
        assert h.returncode == 0
        opts[script] = set(re.findall(r"--[a-z_0-9]+", h.stdout))
    assert len(opts["run_test.py"]) >= 18 and opts["run_test.py"] <= opts["run_ensemble.py"], sorted(opts["run_test.py"] - opts["run_ensemble.py"])
    every = ["--train_date", "d", "--model_index", "0", "--checkpoint_dir", "c", "--gpu_id", "0", "--num_workers", "2", "--specific_sample", "1", "--select_modal", "0",
             "--synthetic", "1", "--volume_shape", "8", "8", "8", "--data_module", "m", "--out_csv", "o.csv"]
    for script, names in (("run_test.py", "a"), ("run_ensemble.py", "a,b")):
        r = _run(script, *every, "--checkpoint_index", names)                # the same invocation parses in both; the first config file does not exist
        assert r.returncode == 1 and "m.json" in r.stderr, (script, r.stderr[-500:])
    r = _run("run_test.py", "--use_hd95", "1")
    assert r.returncode == 1 and "HD95" in r.stderr and "usage" not in r.stderr, r.stderr[-500:]
    r = _run("run_test.py")                                                  # parsed; the first config file does not exist
    assert r.returncode == 1 and "m.json" in r.stderr
    r = _run("run_ensemble.py", "--use_hd95", "1", "--checkpoint_index", "a,b,c")
    assert r.returncode == 1 and "HD95" in r.stderr and "usage" not in r.stderr, r.stderr[-500:]
    r = _run("run_ensemble.py", "--checkpoint_index", "a,b")                 # parsed; the first config file does not exist
    assert r.returncode == 1 and "m.json" in r.stderr
    r = _run("run_ensemble.py")
    assert r.returncode == 2 and "--checkpoint_index" in r.stderr
    r = _run("run_ensemble.py", "--checkpoint_index", ",")
    assert r.returncode == 1 and "at least one name" in r.stderr
