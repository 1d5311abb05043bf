"""GPU: Gaussian importance blending of the sliding-window inference -- the weighted accumulate (plain and mirrored) and the finalize with its normaliser formed on
the fly (csrc/infer.hip) against torch restatements, and the driver (sequential, pipelined, mirrored, taped) against tests/blend_ref.py.  Everything is held to ==
except the constant-valued predictor, which is held to the summation bound."""
import json
import os
import subprocess
import sys

import pytest
import torch

import blend_ref as BR
import tta_ref as TR
from oracle import sliding_window_oracle as SO  # (checker only)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAD = 64            # sentinel floats behind every output buffer: a kernel that runs past its extent is caught, not only suffered
SIGMAS = [0.125, (0.25, 0.125, 0.5)]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rand(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev())


def _tables(roi, sigma):
    """the three axis tables behind one device pointer, and the floor -- from the restatement, not from the driver"""
    return torch.cat([BR.axis_table(r, s) for r, s in zip(roi, BR.sigmas(sigma))]).to(dev()), BR.floor_of(roi, sigma)


@pytest.mark.parametrize("sigma", SIGMAS, ids=["s0.125", "s3"])
@pytest.mark.parametrize("K", [1, 6])
@pytest.mark.parametrize("vol,roi,origin", [((5, 6, 16), (3, 4, 8), (2, 1, 8)), ((5, 6, 16), (3, 4, 8), (1, 2, 3)), ((4, 5, 9), (3, 4, 7), (1, 1, 2)),
                                            ((3, 3, 5), (2, 3, 1), (1, 0, 4)), ((3, 4, 8), (3, 4, 8), (0, 0, 0))])
def test_weighted_accumulate_and_its_mirrored_form_equal_the_torch_restatement(K, vol, roi, origin, sigma):
    """acc += w * flip(pred) and acc += w * (weight * (wsum + flip(pred))) into a NON-ZERO accumulator, every rounding of the unfused torch sequence in its order"""
    from veloxseg_amd import _hip as H
    D, Hh, W = vol
    rd, rh, rw = roi
    z0, y0, x0 = origin
    pred, wsum = _rand((K, rd, rh, rw), 5), _rand((K, rd, rh, rw), 6)
    acc0 = _rand((K, D, Hh, W), 7)
    g, floor = _tables(roi, sigma)
    w = BR.importance_map(roi, sigma).to(dev())
    assert float(w.min()) == floor
    n = acc0.numel()
    for mask in range(8):
        back = TR.flip_mask(pred, mask, 1)
        for weight in (None, 0.5, 0.125):                                   # None: the plain form (wsum = NULL)
            want = acc0.clone()
            want[:, z0:z0 + rd, y0:y0 + rh, x0:x0 + rw] += w * (back if weight is None else weight * (wsum + back))
            buf = torch.full((n + PAD,), -7.0, device=pred.device)
            buf[:n] = acc0.reshape(-1)
            H.call("vx_sw_blend_accumulate", H.P(pred), None if weight is None else H.P(wsum), H.P(buf), H.P(g), floor, K, D, Hh, W, rd, rh, rw, z0, y0, x0,
                   mask, 1.0 if weight is None else weight, H.stream_ptr())
            torch.cuda.synchronize()
            assert bool((buf[n:] == -7.0).all()), "the kernel wrote behind the accumulator"
            assert torch.equal(buf[:n].view(K, D, Hh, W), want), (mask, weight)
    assert not torch.equal(want, acc0)


def _geometry_tables(image_size, patch, starts, sigma):
    """the tables vx_sw_blend_finalize takes, by brute force: per axis the number of windows over every coordinate, and the axis-table values of those windows in
    ascending start, rows padded to the largest count with a value the kernel must not read"""
    axes = [sorted({s[a] for s in starts}) for a in range(3)]
    counts, values, strides = [], [], []
    for a, r, m, s_ in zip(axes, patch, image_size, BR.sigmas(sigma)):
        g = BR.axis_table(r, s_).tolist()
        rows = [[g[c - s] for s in a if s <= c < s + r] for c in range(m)]
        strides.append(max(len(row) for row in rows))
        counts += [len(row) for row in rows]
        values += [v for row in rows for v in row + [float("nan")] * (strides[-1] - len(row))]
    return torch.tensor(counts, dtype=torch.int32).to(dev()), torch.tensor(values, dtype=torch.float32).to(dev()), strides, axes


FINALIZE_CASES = [((20, 17, 9), (8, 8, 8), 0.5),          # H: starts 0, 4, 8, 9 -- the clamped last window, unequal spacing; W: 0, 1
                  ((12, 10, 12), (8, 8, 8), 0.75),        # up to 18 windows over one voxel
                  ((12, 12, 12), (12, 12, 12), 0.5),      # one window
                  ((9, 33, 21), (4, 16, 16), 0.5),
                  ((24, 20, 16), (8, 8, 8), 0.5),
                  ((13, 10, 12), (8, 8, 8), 0.75)]        # D: starts 0, 2, 4, 5 -- four windows over z = 5


@pytest.mark.parametrize("sigma", SIGMAS, ids=["s0.125", "s3"])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("image_size,roi,overlap", FINALIZE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_finalize_divides_by_the_window_order_sum_of_the_weights(image_size, roi, overlap, K, sigma):
    from veloxseg_amd import _hip as H
    starts = SO.dense_patch_starts(image_size, roi, SO.get_scan_interval(image_size, roi, overlap))
    tab, gc, strides, axes = _geometry_tables(image_size, roi, starts, sigma)
    if image_size == (20, 17, 9):
        assert axes[1] == [0, 4, 8, 9] and strides == [2, 3, 2]
    if image_size == (13, 10, 12):
        assert strides == [4, 2, 3]
    floor = BR.floor_of(roi, sigma)
    cnt = BR.count_map(image_size, roi, starts, BR.importance_map(roi, sigma).to(dev()))
    D, Hh, W = image_size
    V = D * Hh * W
    acc = _rand((K,) + image_size, 11)
    nan_at = torch.zeros(image_size, dtype=torch.bool, device=dev())
    nan_at.view(-1)[::7] = True
    acc[K // 2][nan_at] = float("nan")                                       # one NaN channel: its index is the label wherever it is NaN
    want = acc / cnt
    want_labels = torch.where(nan_at, torch.full_like(nan_at, K // 2, dtype=torch.int64), torch.nan_to_num(want, nan=-float("inf")).argmax(0))
    for in_place in (True, False):
        src = torch.full((K * V + PAD,), -7.0, device=dev())
        src[:K * V] = acc.reshape(-1)
        dst = src if in_place else torch.full((K * V + PAD,), -7.0, device=dev())
        lab = torch.full((V + PAD,), 99, dtype=torch.uint8, device=dev())
        H.call("vx_sw_blend_finalize", H.P(src), H.P(dst), H.P(lab, torch.uint8), H.P(gc), floor, H.P(tab, torch.int32), *strides, K, D, Hh, W, H.stream_ptr())
        torch.cuda.synchronize()
        assert bool((dst[K * V:] == -7.0).all()) and bool((src[K * V:] == -7.0).all()) and bool((lab[V:] == 99).all())
        got = dst[:K * V].view((K,) + image_size)
        assert torch.equal(got.isnan(), want.isnan()) and bool(got.isnan().any())
        assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))
        assert torch.equal(lab[:V].view(image_size).long(), want_labels)
        if not in_place:
            assert torch.equal(torch.nan_to_num(src[:K * V], nan=0.0), torch.nan_to_num(acc.reshape(-1), nan=0.0))
    # labels alone / quotient alone
    lab = torch.full((V + PAD,), 99, dtype=torch.uint8, device=dev())
    H.call("vx_sw_blend_finalize", H.P(acc), None, H.P(lab, torch.uint8), H.P(gc), floor, H.P(tab, torch.int32), *strides, K, D, Hh, W, H.stream_ptr())
    out = torch.full((K * V + PAD,), -7.0, device=dev())
    H.call("vx_sw_blend_finalize", H.P(acc), H.P(out), None, H.P(gc), floor, H.P(tab, torch.int32), *strides, K, D, Hh, W, H.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(lab[:V].view(image_size).long(), want_labels) and bool((lab[V:] == 99).all())
    assert torch.equal(torch.nan_to_num(out[:K * V].view_as(want), nan=0.0), torch.nan_to_num(want, nan=0.0)) and bool((out[K * V:] == -7.0).all())


DRIVER_CASES = [((2, 3, 20, 17, 9), (8, 8, 8), 3, 0.5), ((1, 2, 5, 6, 7), (8, 4, 16), 2, 0.25), ((1, 4, 40, 33, 21), (16, 16, 16), 2, 0.5), ((3, 1, 12, 12, 12), (12, 12, 12), 4, 0.5),
                ((1, 2, 24, 20, 16), (8, 8, 8), 2, 0.5),           # 60 windows, every origin a multiple of 4: the 16-byte path end to end
                ((1, 1, 12, 10, 12), (8, 8, 8), 2, 0.75),          # up to 18 windows over one voxel
                ((1, 1, 13, 10, 12), (8, 8, 8), 2, 0.75)]          # four windows over one z (the clamped last window)
_CASE_IDS = lambda c: "x".join(map(str, c[0]))
_REF = {}


def _driver_input(case):
    return _rand(case[0], 3)


def _num_windows(case):
    image_size, patch, pad, starts = BR.geometry(case[0], case[1], case[3])
    return len(starts)


def _reference(case, sigma, axes):
    key = (case, sigma, tuple(axes))
    if key not in _REF:
        shape, roi, swb, overlap = case
        P = TR.mirror_average(TR.ramp_predictor, axes) if axes else TR.ramp_predictor
        _REF[key] = BR.sliding_window_inference(_driver_input(case), roi, swb, P, overlap, sigma)
    return _REF[key]


def test_the_cases_are_the_geometries_they_are_meant_to_be():
    assert _num_windows(DRIVER_CASES[3]) == 1
    image_size, patch, pad, starts = BR.geometry(*[DRIVER_CASES[4][i] for i in (0, 1, 3)])
    assert len(starts) == 60 and all(s[2] % 4 == 0 for s in starts) and image_size[2] % 4 == 0 and patch[2] % 4 == 0
    image_size, patch, pad, starts = BR.geometry(*[DRIVER_CASES[5][i] for i in (0, 1, 3)])
    assert BR.max_cover(image_size, patch, starts) == 18


@pytest.mark.parametrize("axes", [(), (2,), (0, 1, 2)], ids=["plain", "mirror2", "mirror012"])
@pytest.mark.parametrize("sigma", SIGMAS, ids=["s0.125", "s3"])
@pytest.mark.parametrize("case", DRIVER_CASES, ids=_CASE_IDS)
def test_driver_equals_the_restatement(case, sigma, axes):
    from veloxseg_amd.utils import inference_runtime as IR
    shape, roi, swb, overlap = case
    x = _driver_input(case)
    want = _reference(case, sigma, axes)
    got, labels = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, mirror_axes=axes, return_labels=True, blend="gaussian", sigma_scale=sigma)
    assert got.shape == want.shape
    assert torch.equal(got, want), float((got - want).abs().max())
    assert labels.dtype == torch.uint8 and torch.equal(labels.long(), want.argmax(1, keepdim=True))
    if _num_windows(case) > 1:
        const = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, mirror_axes=axes)
        diff = float((got - const).abs().max())
        print(f"max |gaussian - constant| = {diff:.4f}")
        assert not torch.equal(got, const), "the Gaussian weights left the result where constant blending puts it"
        if len(axes) < 3:            # (averaged over all eight mirrors the ramps of the test predictor cancel: what is left to tell the two blendings apart is rounding)
            assert diff > 0.1


@pytest.mark.parametrize("case", DRIVER_CASES, ids=_CASE_IDS)
def test_constant_blend_is_the_call_without_the_keyword_and_the_oracle(case):
    from veloxseg_amd.utils import inference_runtime as IR
    shape, roi, swb, overlap = case
    x = _driver_input(case)
    a, la = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, return_labels=True)
    b, lb = IR.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap, return_labels=True, blend="constant", sigma_scale=(0.25, 0.125, 0.5))
    assert torch.equal(a, b) and torch.equal(la, lb)
    assert torch.equal(a, SO.sliding_window_inference(x, roi, swb, TR.ramp_predictor, overlap))


def test_mode_gaussian_still_raises_not_implemented():
    from veloxseg_amd.utils import inference_runtime as IR
    x = _driver_input(DRIVER_CASES[1])
    for kw in ({}, {"blend": "gaussian"}):
        with pytest.raises(NotImplementedError):
            IR.sliding_window_inference(x, (8, 4, 16), 2, TR.ramp_predictor, 0.25, mode="gaussian", **kw)
    with pytest.raises(ValueError, match="blend"):
        IR.sliding_window_inference(x, (8, 4, 16), 2, TR.ramp_predictor, 0.25, blend="hann")
    with pytest.raises(ValueError, match="sigma_scale"):
        IR.sliding_window_inference(x, (8, 4, 16), 2, TR.ramp_predictor, 0.25, blend="gaussian", sigma_scale=(0.125, 0.0, 0.125))


CONSTANTS = (0.7314, -3.25, 1e-3, 117.0)


def _constant_predictor(w):
    return torch.cat([torch.full_like(w[:, :1], c) for c in CONSTANTS], 1)


@pytest.mark.parametrize("case", DRIVER_CASES, ids=_CASE_IDS)
def test_constant_valued_predictor_comes_back_within_the_summation_bound(case):
    """sum of w_i * c over n windows divided by the sum of w_i: every product and every partial sum of either sum carries one rounding, the quotient one more --
    at most (2 n + 2) * 2^-24 relative to first order, n = the largest number of windows over a voxel"""
    from veloxseg_amd.utils import inference_runtime as IR
    shape, roi, swb, overlap = case
    image_size, patch, pad, starts = BR.geometry(shape, roi, overlap)
    n_cover = BR.max_cover(image_size, patch, starts)
    x = _driver_input(case)
    got = IR.sliding_window_inference(x, roi, swb, _constant_predictor, overlap, blend="gaussian", sigma_scale=0.125)
    for k, c in enumerate(torch.tensor(CONSTANTS, dtype=torch.float32).tolist()):
        err = float((got[:, k].double() - c).abs().max())
        print(f"c = {c}: n_cover {n_cover}, worst error {err / abs(c) * 2 ** 24:.2f} * 2^-24 |c|")
        assert err <= (2 * n_cover + 2) * 2.0 ** -24 * abs(c), (c, err)


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


@pytest.mark.parametrize("axes", [(), (0, 1, 2)], ids=["plain", "mirror012"])
def test_gaussian_blend_with_the_hip_model_taped_eager_pipelined(hip_model, axes):
    from veloxseg_amd.utils import inference_runtime as IR
    model = hip_model
    x = _rand((1, 2, 48, 40, 36), 5)
    roi = (32, 32, 32)
    kw = dict(mirror_axes=axes, blend="gaussian")
    with torch.inference_mode():
        plain, _ = IR.infer_volume(model, x, roi, 2, 0.5, mirror_axes=axes)    # the constant run of this shape: captures the tape and its replicas
        tp = model.__dict__["_vx_taped_predictor"]
        tapes = dict(tp._tapes)
        replicas = dict(tp.__dict__.get("_replicas", {}))
        slots = []
        real_slot = tp.forward_slot
        tp.forward_slot = lambda w, slot: (slots.append((slot, real_slot(w, slot)))) or slots[-1][1]
        try:
            got, labels = IR.infer_volume(model, x, roi, 2, 0.5, **kw)
        finally:
            del tp.forward_slot
        # the two-in-flight path on the replicas: 4 window batches x n forwards, all but the very first replayed from a slot, none falling back to eager launches
        assert len(slots) == 4 * 2 ** len(axes) - 1 and all(out is not None for _, out in slots)
        # no capture beyond those of the constant run
        assert set(tp._tapes) == set(tapes) and all(tp._tapes[k] is tapes[k] for k in tapes)
        assert set(tp._replicas) == set(replicas) and all(tp._replicas[k] is replicas[k] for k in replicas)
        eager, labels_eager = IR.infer_volume(model, x, roi, 2, 0.5, taped=False, **kw)
        net = IR.Net(model)
        want = BR.sliding_window_inference(x, roi, 2, TR.mirror_average(net, axes) if axes else net, 0.5, 0.125)
        assert IR.SW_PIPELINE
        IR.SW_PIPELINE = False
        try:
            seq, labels_seq = IR.infer_volume(model, x, roi, 2, 0.5, **kw)
        finally:
            IR.SW_PIPELINE = True
    assert torch.equal(got, eager) and torch.equal(labels, labels_eager)
    assert torch.equal(got, want) and torch.equal(labels.long(), want.argmax(1, keepdim=True))
    assert torch.equal(got, seq) and torch.equal(labels, labels_seq)
    assert not torch.equal(got, plain), "the Gaussian weights left the network's result untouched"


def test_sliding_window_predict_reads_blend_and_sigma_scale_from_the_config():
    from veloxseg_amd.utils import inference_runtime as IR
    case = DRIVER_CASES[0]
    shape, roi, swb, overlap = case
    x = _driver_input(case)
    P = TR.ramp_predictor
    const = IR.sliding_window_inference(x, roi, swb, P, overlap)
    cfg = {"sliding_window": {"overlap": overlap, "blend": "gaussian"}}
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, cfg), _reference(case, SIGMAS[0], ()))
    cfg3 = {"sliding_window": {"overlap": overlap, "blend": "gaussian", "sigma_scale": list(SIGMAS[1]), "mirror_axes": [2]}}
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, cfg3), _reference(case, SIGMAS[1], (2,)))
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, cfg3, sigma_scale=0.125), _reference(case, SIGMAS[0], (2,)))      # the keywords win
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, cfg3, blend="constant", mirror_axes=()), const)
    assert torch.equal(IR.sliding_window_predict(x, P, roi, swb, {"sliding_window": {"overlap": overlap}}), const)
    with pytest.raises(ValueError, match="blend"):
        IR.sliding_window_predict(x, P, roi, swb, {"sliding_window": {"overlap": overlap, "blend": "hann"}})


def test_run_test_takes_blend_from_the_test_config_end_to_end(tmp_path):
    """run_test.py hands its test config to sliding_window_predict, which reads test_config["sliding_window"]["blend"]: a fresh child process on seeded weights runs
    the Gaussian-blended inference and writes its CSV; an unknown blend in the config is refused, so the key is read and not ignored."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    cfg, _ = CASES["g2_32_m2"]
    mc, tc = tmp_path / "models.json", tmp_path / "train.json"
    mc.write_text(json.dumps({"VeloxSeg": cfg}))
    tc.write_text(json.dumps(dict(TRAIN_CFG, patch_size={"AutoPETII": [32, 32, 32]})))

    def run(sw, name):
        te = tmp_path / f"{name}.json"
        te.write_text(json.dumps({"sliding_window": sw}))
        return subprocess.run([sys.executable, os.path.join(ROOT, "run_test.py"), "--dataset_name", "AutoPETII", "--model_name", "VeloxSeg", "--train_config", str(tc),
                               "--model_config", str(mc), "--test_config", str(te), "--synthetic", "1", "--volume_shape", "48", "40", "36",
                               "--out_csv", str(tmp_path / f"{name}.csv")], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    r = run({"overlap": 0.25, "blend": "gaussian"}, "gauss")
    assert r.returncode == 0, r.stderr[-2000:]
    assert os.path.exists(tmp_path / "gauss.csv") and "synthetic_0" in r.stdout
    bad = run({"overlap": 0.25, "blend": "hann"}, "bad")
    assert bad.returncode != 0 and "blend" in bad.stderr and not os.path.exists(tmp_path / "bad.csv")
