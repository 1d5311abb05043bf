"""GPU: mirror test-time augmentation of the sliding-window inference -- the window movers of csrc/infer.hip against torch.flip restatements, and the
driver (sequential, pipelined, taped) against the sliding-window oracle run on a mirror-averaging predictor (tests/tta_ref.py).  Everything is held to ==."""
import ctypes
import json
import os
import subprocess
import sys

import pytest
import torch

import tta_ref as TR
from oracle import sliding_window_oracle as SO  # (checker only)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAD = 64            # sentinel floats behind every output buffer: a kernel that runs past its extent is caught, not only suffered


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev())


def _extract(vol, rows, roi, mask):
    """vx_sw_extract_mirror on a (B, C, D, H, W) volume; rows = [(b, z0, y0, x0), ...] -> (nwin, C, rd, rh, rw)"""
    from veloxseg_amd import _hip as H
    B, C, D, Hh, W = vol.shape
    rd, rh, rw = roi
    n = len(rows) * C * rd * rh * rw
    buf = torch.full((n + PAD,), -7.0, device=vol.device)
    tab = (ctypes.c_int * (4 * len(rows)))(*[v for r in rows for v in r])
    H.call("vx_sw_extract_mirror", H.P(vol), H.P(buf), ctypes.addressof(tab), len(rows), mask, B, C, D, Hh, W, rd, rh, rw, H.stream_ptr())
    torch.cuda.synchronize()
    assert bool((buf[n:] == -7.0).all()), "the kernel wrote behind its windows"
    return buf[:n].view(len(rows), C, rd, rh, rw)


def _want_windows(vol, rows, roi, mask):
    rd, rh, rw = roi
    return torch.stack([TR.flip_mask(vol[b, :, z:z + rd, y:y + rh, x:x + rw], mask, 1) for b, z, y, x in rows])


EXTRACT_CASES = [
    ((1, 3, 9, 10, 16), (4, 6, 8), [(0, 0, 0, 0), (0, 5, 4, 8)]),        # four-voxel path: x0 = 0 and 8
    ((1, 3, 9, 10, 16), (4, 6, 8), [(0, 2, 1, 3)]),                      # misaligned origin: scalar path
    ((1, 2, 5, 6, 7), (5, 6, 7), [(0, 0, 0, 0)]),                        # window = volume, odd row
    ((1, 1, 4, 4, 9), (1, 1, 1), [(0, 3, 2, 8)]),                        # one voxel
    ((1, 2, 8, 8, 12), (8, 8, 4), [(0, 0, 0, 8)]),                       # the clamped far corner
]


@pytest.mark.parametrize("shape,roi,rows", EXTRACT_CASES)
def test_mirrored_extract_equals_flip_of_the_slice(shape, roi, rows):
    vol = _rand(shape, 1)
    for mask in range(8):
        got = _extract(vol, rows, roi, mask)
        assert torch.equal(got, _want_windows(vol, rows, roi, mask)), mask


def test_mirrored_extract_at_the_full_capacity_of_the_table():
    from veloxseg_amd.utils.inference_runtime import SW_MAX_WINDOWS
    vol = _rand((2, 3, 9, 10, 16), 2)
    roi = (4, 6, 8)
    rows = [(k % 2, (k * 3) % 6, (k * 5) % 5, 8 * ((k // 2) % 2)) for k in range(SW_MAX_WINDOWS)]
    assert {r[0] for r in rows} == {0, 1} and len(rows) == 16
    for mask in range(8):
        assert torch.equal(_extract(vol, rows, roi, mask), _want_windows(vol, rows, roi, mask)), mask
    rows[5] = (1, 1, 2, 5)                                                 # one misaligned window: the whole launch takes the scalar path
    for mask in (0, 4, 7):
        assert torch.equal(_extract(vol, rows, roi, mask), _want_windows(vol, rows, roi, mask)), mask


@pytest.mark.parametrize("rows", [1, 6])
@pytest.mark.parametrize("roi", [(3, 4, 8), (3, 4, 7), (2, 3, 1)])
def test_mirror_back_and_sum_equals_the_torch_restatement(rows, roi):
    from veloxseg_amd import _hip as H
    rd, rh, rw = roi
    n = rows * rd * rh * rw
    pred = _rand((rows, rd, rh, rw), 3)
    start = _rand((rows, rd, rh, rw), 4)
    for mask in range(8):
        back = TR.flip_mask(pred, mask, 1)
        for first, want in ((1, back), (0, start + back)):
            buf = torch.full((n + PAD,), -7.0, device=pred.device)
            buf[:n] = start.reshape(-1)
            H.call("vx_sw_mirror_sum", H.P(pred), H.P(buf), rows, rd, rh, rw, mask, first, H.stream_ptr())
            torch.cuda.synchronize()
            assert bool((buf[n:] == -7.0).all())
            assert torch.equal(buf[:n].view(rows, rd, rh, rw), want), (mask, first)


@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("vol,roi,origin", [((5, 6, 16), (3, 4, 8), (2, 1, 8)), ((5, 6, 16), (3, 4, 8), (1, 2, 3)), ((4, 5, 9), (3, 4, 7), (1, 1, 2)),
                                            ((3, 3, 5), (2, 3, 1), (1, 0, 4)), ((3, 4, 8), (3, 4, 8), (0, 0, 0))])
def test_fused_last_mirror_accumulate_equals_sum_then_accumulate(K, vol, roi, origin):
    """acc += weight * (wsum + flip(pred)) into a NON-ZERO accumulator: the three roundings of the unfused sequence, in its order"""
    from veloxseg_amd import _hip as H
    D, Hh, W = vol
    rd, rh, rw = roi
    z0, y0, x0 = origin
    pred, wsum = _rand((K, rd, rh, rw), 5), _rand((K, rd, rh, rw), 6)
    acc0 = _rand((K, D, Hh, W), 7)
    for mask in range(8):
        for weight in (0.5, 0.125):
            want = acc0.clone()
            want[:, z0:z0 + rd, y0:y0 + rh, x0:x0 + rw] += weight * (wsum + TR.flip_mask(pred, mask, 1))
            n = acc0.numel()
            buf = torch.full((n + PAD,), -7.0, device=pred.device)
            buf[:n] = acc0.reshape(-1)
            H.call("vx_sw_mirror_accumulate", H.P(pred), H.P(wsum), H.P(buf), K, D, Hh, W, rd, rh, rw, z0, y0, x0, mask, weight, H.stream_ptr())
            torch.cuda.synchronize()
            assert bool((buf[n:] == -7.0).all())
            assert torch.equal(buf[:n].view(K, D, Hh, W), want), (mask, weight)


DRIVER_CASES = [((2, 3, 20, 17, 9), (8, 8, 8), 3, 0.5), ((1, 2, 5, 6, 7), (8, 4, 16), 2, 0.25), ((1, 4, 40, 33, 21), (16, 16, 16), 2, 0.5), ((3, 1, 12, 12, 12), (12, 12, 12), 4, 0.5)]
_ORACLE = {}


def _driver_input(case):
    return _rand(case[0], 3)


@pytest.mark.parametrize("axes", [(2,), (0,), (1, 2), (0, 1, 2), (2, 0)])
@pytest.mark.parametrize("case", DRIVER_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_driver_matches_the_oracle_on_a_mirror_averaging_predictor(case, axes):
    from veloxseg_amd.utils import inference_runtime as IR
    shape, roi, swb, overlap = case
    x = _driver_input(case)
    key = (case, tuple(sorted(axes)))
    if key not in _ORACLE:                                              # ((2, 0) shares the reference of (0, 2): the order of the axes is irrelevant)
        _ORACLE[key] = SO.sliding_window_inference(x, roi, swb, TR.mirror_average(TR.ramp_predictor, sorted(axes)), overlap)
    want = _ORACLE[key]
    got, labels = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, mirror_axes=axes, return_labels=True)
    assert got.shape == want.shape
    assert torch.equal(got, want), float((got - want).abs().max())
    assert labels.dtype == torch.uint8 and torch.equal(labels.long(), want.argmax(1, keepdim=True))
    plain = SO.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap)
    assert not torch.equal(plain, want), "the test predictor does not tell the augmented result from the plain one"


@pytest.mark.parametrize("case", DRIVER_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_no_mirror_axes_is_the_call_without_the_keyword(case):
    from veloxseg_amd.utils import inference_runtime as IR
    shape, roi, swb, overlap = case
    x = _driver_input(case)
    a, la = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, return_labels=True)
    b, lb = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, mirror_axes=(), return_labels=True)
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert torch.equal(a, SO.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap))


@pytest.mark.parametrize("axes", [(2,), (0,), (0, 1), (1, 2), (0, 2)])
def test_position_independent_predictor_is_unchanged_by_the_augmentation(axes):
    """n equal fp32 values v summed one after the other and multiplied by 1 / n give v back exactly for n = 2 and n = 4: 2v and 4v are representable, and
    the one rounded partial sum, 3v, is off by at most half a unit of 4v's last place with the tie going to 4v (its mantissa is even).  That is every schedule of
    one or two axes.  At n = 8 the partial sums 5v, 6v and 7v round independently and v + ... + v is NOT 8v for about four values in ten (v = 0x1.7245fap-2 comes
    back as 0x1.7245fcp-2): three axes are held to the oracle on the mirror-averaging predictor instead, which rounds the same way."""
    from veloxseg_amd.utils import inference_runtime as IR
    for case in DRIVER_CASES[:2]:
        shape, roi, swb, overlap = case
        x = _driver_input(case)
        plain, lp = IR.sliding_window_inference(x, roi, swb, TR.flat_predictor, overlap, return_labels=True)
        got, lg = IR.sliding_window_inference(x, roi, swb, TR.flat_predictor, overlap, mirror_axes=axes, return_labels=True)
        assert torch.equal(got, plain) and torch.equal(lg, lp)


def test_position_independent_predictor_under_three_axes_equals_the_oracle():
    from veloxseg_amd.utils import inference_runtime as IR
    for case in DRIVER_CASES[:2]:
        shape, roi, swb, overlap = case
        x = _driver_input(case)
        want = SO.sliding_window_inference(x, roi, swb, TR.mirror_average(TR.flat_predictor, (0, 1, 2)), overlap)
        assert torch.equal(IR.sliding_window_inference(x, roi, swb, TR.flat_predictor, overlap, mirror_axes=(0, 1, 2)), want)


@pytest.fixture(scope="module")
def hip_model(golden_dir):
    sys.path.insert(0, golden_dir)
    from recipe import CASES, fill_state_dict
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    cfg, _ = CASES["g2_32_m2"]
    model = VeloxSeg(**cfg)
    sd = model.state_dict()
    fill_state_dict(sd)
    model.load_state_dict(sd)
    return model.to(dev()).eval()


def test_mirror_augmentation_with_the_hip_model_taped_eager_pipelined(hip_model):
    from veloxseg_amd.utils import inference_runtime as IR
    model = hip_model
    x = _rand((1, 2, 48, 40, 36), 5)
    roi, axes = (32, 32, 32), (0, 1, 2)
    assert len(SO.dense_patch_starts((48, 40, 36), roi, SO.get_scan_interval((48, 40, 36), roi, 0.5))) == 8
    with torch.inference_mode():
        IR.infer_volume(model, x, roi, 2, 0.5)                              # the non-augmented run of this shape: captures the tape and its replicas
        tp = model.__dict__["_vx_taped_predictor"]
        tapes = dict(tp._tapes)
        replicas = dict(tp.__dict__.get("_replicas", {}))
        assert any(k != "sig" and e is not None for k, e in replicas.items()), "no replica of the tape was replayed"
        slots = []
        real_slot = tp.forward_slot
        tp.forward_slot = lambda w, slot: (slots.append((slot, real_slot(w, slot)))) or slots[-1][1]
        try:
            got, labels = IR.infer_volume(model, x, roi, 2, 0.5, mirror_axes=axes)
        finally:
            del tp.forward_slot
        # the augmented run took the taped two-in-flight path: 4 window batches x 8 mirrors = 32 forwards, the very first the plain way on the caller's stream, the
        # other 31 replayed from the replicas of the two slots (16 on slot 1's, 15 on slot 0's), none of them falling back to eager launches
        assert len(slots) == 31 and all(out is not None for _, out in slots)
        assert sorted(s_ for s_, _ in slots) == [1] * 15 + [2] * 16
        # no capture beyond those of the non-augmented run: the mirrored windows have its shape
        assert set(tp._tapes) == set(tapes) and all(tp._tapes[k] is tapes[k] for k in tapes)
        assert set(tp._replicas) == set(replicas) and all(tp._replicas[k] is replicas[k] for k in replicas)
        eager, labels_eager = IR.infer_volume(model, x, roi, 2, 0.5, taped=False, mirror_axes=axes)
        want = SO.sliding_window_inference(x, roi, 2, TR.mirror_average(IR.Net(model), axes), 0.5)
        assert IR.SW_PIPELINE
        IR.SW_PIPELINE = False
        try:
            seq, labels_seq = IR.infer_volume(model, x, roi, 2, 0.5, mirror_axes=axes)
        finally:
            IR.SW_PIPELINE = True
        plain, _ = IR.infer_volume(model, x, roi, 2, 0.5)
    assert torch.equal(got, eager) and torch.equal(labels, labels_eager)
    assert torch.equal(got, want) and torch.equal(labels.long(), want.argmax(1, keepdim=True))
    assert torch.equal(got, seq) and torch.equal(labels, labels_seq)
    assert not torch.equal(got, plain), "the augmentation left the network's result untouched"


def test_result_device_and_window_device_keywords():
    from veloxseg_amd.utils import inference_runtime as IR
    shape, roi, swb, overlap = DRIVER_CASES[0]
    x = _driver_input(DRIVER_CASES[0])
    P = TR.ramp_predictor
    on_gpu, lab_gpu = IR.sliding_window_inference(x, roi, swb, P, overlap, mirror_axes=(2,), return_labels=True)
    got, lab = IR.sliding_window_inference(x, roi, swb, P, overlap, mirror_axes=(2,), return_labels=True, sw_device=x.device, device="cpu")
    assert got.device.type == "cpu" and lab.device.type == "cpu"
    assert torch.equal(got, on_gpu.cpu()) and torch.equal(lab, lab_gpu.cpu())
    same = IR.sliding_window_inference(x, roi, swb, P, overlap, sw_device="cuda", device=x.device)
    assert same.device == x.device and torch.equal(same, IR.sliding_window_inference(x, roi, swb, P, overlap))
    with pytest.raises(ValueError):
        IR.sliding_window_inference(x, roi, swb, P, overlap, sw_device="cpu")
    with pytest.raises(NotImplementedError):
        IR.sliding_window_inference(x, roi, swb, P, overlap, sw_device=x.device, device="cpu", progress=True)
    cfg = {"sliding_window": {"overlap": overlap}}
    ref_call = IR.sliding_window_predict(x, P, roi, swb, cfg, sw_device=x.device, device="cpu")          # the reference's huge-volume call
    assert ref_call.device.type == "cpu" and torch.equal(ref_call, IR.sliding_window_inference(x, roi, swb, P, overlap).cpu())
    cfg_tta = {"sliding_window": {"overlap": overlap, "mirror_axes": [2]}}
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, cfg_tta), on_gpu)
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, cfg_tta, mirror_axes=()), IR.sliding_window_inference(x, roi, swb, P, overlap))   # the keyword wins


def test_run_test_takes_mirror_axes_from_the_test_config_end_to_end(tmp_path):
    """run_test.py hands its test config to sliding_window_predict, which reads test_config["sliding_window"]["mirror_axes"]: a fresh child process on seeded
    weights runs the augmented inference and writes its CSV; an axis outside (0, 1, 2) in the config is refused, so the key is read and not ignored."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    cfg, _ = CASES["g2_32_m2"]
    mc, tc = tmp_path / "models.json", tmp_path / "train.json"
    mc.write_text(json.dumps({"VeloxSeg": cfg}))
    tc.write_text(json.dumps(dict(TRAIN_CFG, patch_size={"AutoPETII": [32, 32, 32]})))

    def run(axes, name):
        te = tmp_path / f"{name}.json"
        te.write_text(json.dumps({"sliding_window": {"overlap": 0.25, "mirror_axes": axes}}))
        return subprocess.run([sys.executable, os.path.join(ROOT, "run_test.py"), "--dataset_name", "AutoPETII", "--model_name", "VeloxSeg", "--train_config", str(tc),
                               "--model_config", str(mc), "--test_config", str(te), "--synthetic", "1", "--volume_shape", "48", "40", "36",
                               "--out_csv", str(tmp_path / f"{name}.csv")], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    r = run([2], "tta")
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(tmp_path / "tta.csv") and "synthetic_0" in r.stdout
    bad = run([3], "bad")
    assert bad.returncode != 0 and "mirror_axes" in bad.stderr and not os.path.exists(tmp_path / "bad.csv")
