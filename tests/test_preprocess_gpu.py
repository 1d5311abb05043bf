"""Volume preprocessing on the GPU (csrc/preprocess.hip, utils/preprocess.py) against the fp64 restatements of tests/preprocess_ref.py.

Bounds (none is taken from what the kernels return):
* moments: the worst-case error of adding n numbers in any order is n 2^-53 times the sum of their magnitudes, so |mean - want| <= n 2^-53 mean|x| and
  |std - want| <= n 2^-53 rms(x - mean); the count is exact.
* normalisation: |got - want| <= 4 2^-24 (|x| + |mean|) / s -- the fp32 rounding of the mean, the subtraction, the rounding of s and the division.
* order statistics: exact by value; percentiles within 4 fp64 ulp of np.percentile (same linear rule on the same two order statistics).
* trilinear: integer-valued data with dyadic weights is exact; otherwise seven lerps of at most two roundings each, 16 2^-24 max|x| (14 plus margin)."""
import csv
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import preprocess_ref as R
from veloxseg_amd import _hip as H
from veloxseg_amd.utils import preprocess as P

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS53, EPS24 = 2.0 ** -53, 2.0 ** -24


def _rs(seed):
    return np.random.RandomState(seed)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ====================================================================================================================== moments
def _moment_cases():
    g = _rs(7)
    cases = {}
    for n in (1, 63, 257, 70001):
        cases[f"n{n}"] = (g.randn(n) * 3.0 + 1.5).astype(np.float32)
    cases["vol_5x7x9"] = (g.randn(5, 7, 9) * 20.0 - 4.0).astype(np.float32)
    rep = (np.abs(g.randn(70001)) * 5.0 + 0.25).astype(np.float32)
    rep[g.rand(70001) < 0.6] = -2.0
    cases["min_repeats"] = rep                                            # the minimum many times
    one = np.full(4099, -7.5, dtype=np.float32)
    one[1234] = 3.25
    cases["all_but_one_at_min"] = one                                     # one selected voxel
    cases["constant"] = np.full((6, 5, 7), 2.75, dtype=np.float32)        # empty foreground
    cases["ill_conditioned"] = (1e4 + g.randn(30011)).astype(np.float32)  # mean 1e4, std ~ 1
    return cases


_MOMENTS = _moment_cases()


def _check_moments(got, sel):
    """got = (count, mean, std) from the device; sel = the selected values, fp64"""
    n = sel.size
    assert got[0] == n
    if n == 0:
        assert got[1] == 0.0 and got[2] == 0.0
        return
    mean, std = np.mean(sel), np.std(sel)
    print(f"n={n} mean err {abs(got[1] - mean):.3e} bound {n * EPS53 * np.mean(np.abs(sel)):.3e}; std err {abs(got[2] - std):.3e} bound "
          f"{n * EPS53 * np.sqrt(np.mean((sel - mean) ** 2)):.3e}")
    assert abs(got[1] - mean) <= n * EPS53 * np.mean(np.abs(sel))
    assert abs(got[2] - std) <= n * EPS53 * np.sqrt(np.mean((sel - mean) ** 2))


@pytest.mark.parametrize("foreground", [False, True])
@pytest.mark.parametrize("name", list(_MOMENTS))
def test_moments(name, foreground):
    x = _MOMENTS[name]
    t = _dev(x)
    a = P.moments(t, foreground)
    b = P.moments(t, foreground)
    torch.cuda.synchronize()
    a, b = a.cpu().numpy(), b.cpu().numpy()
    assert a.tobytes() == b.tobytes()                                     # bit-identical on repetition
    x64 = x.astype(np.float64).reshape(-1)
    _check_moments(a, x64[x64 > x64.min()] if foreground else x64)


def test_moments_on_an_unaligned_view_match_the_aligned_copy():
    x = _MOMENTS["n70001"]
    t = _dev(np.concatenate([np.zeros(1, np.float32), x]))[1:]            # 4-byte aligned only: the scalar-load path
    assert t.data_ptr() % 16 != 0
    a = P.moments(t).cpu().numpy()
    _check_moments(a, x.astype(np.float64))


# ====================================================================================================================== normalisation
def _norm_volumes():
    g = _rs(11)
    bg = np.full((2, 9, 10, 11), -1.5, dtype=np.float32)
    bg[0, 2:7, 1:8, 3:9] = (np.abs(g.randn(5, 7, 6)) * 30.0 + 2.0).astype(np.float32)
    bg[1, 1:8, 2:9, 0:7] = (g.randn(7, 7, 7) * 0.01 + 100.0).astype(np.float32)
    ints = g.randint(-1024, 3072, size=(1, 7, 9, 5)).astype(np.float32)
    const = np.stack([np.full((5, 6, 7), 4.5, dtype=np.float32), g.randn(5, 6, 7).astype(np.float32)])          # channel 0 constant
    flat_fg = np.full((1, 4, 5, 6), -3.0, dtype=np.float32)
    flat_fg[0, 1:3, 1:4, 2:5] = 8.0                                                                            # foreground of one value: std == 0, non-empty mask
    return {"background": bg, "integer": ints, "constant_channel": const, "flat_foreground": flat_fg}


_NORM = _norm_volumes()


def _assert_normalised(got, want, xc, mean, s, touched=None):
    bound = 4.0 * EPS24 * (np.abs(xc) + abs(mean)) / s
    err = np.abs(got.astype(np.float64) - want)
    if touched is not None:
        err, bound = err[touched], bound[touched]
    if err.size:
        print(f"max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("name", list(_NORM))
def test_zscore_foreground(name):
    x = _NORM[name]
    got = P.zscore_foreground(_dev(x)).cpu().numpy()
    inplace = _dev(x)
    assert P.zscore_foreground(inplace, out=inplace) is inplace
    assert inplace.cpu().numpy().tobytes() == got.tobytes()
    for c in range(x.shape[0]):
        x64 = x[c].astype(np.float64)
        want = R.zscore_foreground(x64)
        at_min = x64 == x64.min()
        assert got[c][at_min].tobytes() == x[c][at_min].tobytes()                                # untouched voxels: bit-equal to the input
        n, mean, std = R.foreground_moments(x64)
        if n == 0:
            assert got[c].tobytes() == x[c].tobytes()                                            # constant channel: unchanged
            continue
        _assert_normalised(got[c], want, x64, mean, max(std, 1e-8), ~at_min)
        if std == 0.0:
            assert np.all(got[c][~at_min] == 0.0)                                                # (x - x) / 1e-8
    got3 = P.zscore_foreground(_dev(x[0])).cpu().numpy()                                         # (D, H, W)
    assert got3.tobytes() == got[0].tobytes()


@pytest.mark.parametrize("name", list(_NORM))
def test_zscore_volume_is_the_reference_call(name):
    x = _NORM[name]
    got = P.zscore_volume(_dev(x)).cpu().numpy()
    for c in range(x.shape[0]):
        x64 = x[c].astype(np.float64)
        want = R.zscore_reference_call(x64)
        _assert_normalised(got[c], want, x64, x64.mean(), max(x64.std(), 1e-8))


@pytest.mark.parametrize("std", [77.5, 0.0])
def test_ct_normalize(std):
    props = {"mean": 101.25, "std": std, "percentile_00_5": -900.0, "percentile_99_5": 1800.5}
    x = _NORM["integer"]
    got = P.ct_normalize(_dev(x), props).cpu().numpy()
    x64 = x.astype(np.float64)
    want = R.ct_norm(x64, props)
    clipped = np.clip(x64, props["percentile_00_5"], props["percentile_99_5"])
    assert (clipped != x64).sum() > 5
    _assert_normalised(got, want, clipped, props["mean"], max(std, 1e-8))
    inplace = _dev(x)
    P.ct_normalize(inplace, props, out=inplace)
    assert inplace.cpu().numpy().tobytes() == got.tobytes()
    got3 = P.ct_normalize(_dev(x)[0, :, :, 1:], props).cpu().numpy()                             # non-contiguous (D, H, W) view
    assert got3.tobytes() == np.ascontiguousarray(got[0, :, :, 1:]).tobytes()


@pytest.mark.parametrize("channel_wise", [True, False])
@pytest.mark.parametrize("name", ["background", "constant_channel"])
def test_normalize_intensityd(name, channel_wise):
    x = _NORM[name]
    data = {"image": _dev(x), "other": 3}
    out = P.NormalizeIntensityd(["image"], channel_wise=channel_wise)(data)
    assert out["other"] == 3 and data["image"].cpu().numpy().tobytes() == x.tobytes()            # the input is left alone
    got = out["image"].cpu().numpy()
    x64 = x.astype(np.float64)
    want = R.normalize_intensity(x64, channel_wise)
    for c in range(x.shape[0]):
        ref = x64[c] if channel_wise else x64
        std = ref.std()
        _assert_normalised(got[c], want[c], x64[c], ref.mean(), std if std != 0.0 else 1.0)
        if std == 0.0:
            assert np.all(got[c] == 0.0)                                                         # std == 0 divides by 1
    if channel_wise:
        assert name != "constant_channel" or np.all(got[0] == 0.0)


# ====================================================================================================================== dataset statistics
_SHAPES = [(7, 9, 11), (4, 5, 6), (16, 16, 16)]
_TOTAL = sum(int(np.prod(s)) for s in _SHAPES)          # 4909


def _masks(n_selected, seed, dtypes):
    """masks over the three volumes selecting exactly n_selected voxels; values 0 / positive, a negative entry where the dtype has one (not selected)"""
    g = _rs(seed)
    flat = np.zeros(_TOTAL, dtype=np.int64)
    flat[g.permutation(_TOTAL)[:n_selected]] = g.randint(1, 4, size=n_selected)
    out, at = [], 0
    for s, dt in zip(_SHAPES, dtypes):
        k = int(np.prod(s))
        m = flat[at:at + k].reshape(s).astype(dt)
        at += k
        out.append(m)
    if np.issubdtype(np.dtype(dtypes[2]), np.signedinteger) or np.dtype(dtypes[2]) == np.float32:
        zero = np.argwhere(out[2] == 0)[0]
        out[2][tuple(zero)] = -1
    return out


def _datasets():
    g = _rs(21)
    d = {}
    hu = [g.choice(np.array([-1024, -1000, -998, -100, 0, 1, 40, 41, 42, 300, 3071]), size=s, p=[.3, .1, .05, .05, .1, .1, .1, .05, .05, .05, .05]).astype(np.float32)
          for s in _SHAPES]
    d["integer_hu"] = (hu, _masks(2001, 1, (np.uint8, np.int32, np.int64)))                     # (n - 1) q / 100 an integer for every q
    special = np.array([-0.0, 0.0, 1e-45, -1e-45, 3e-40, -3e-40, 1.17549435e-38, -1.5, 2.5], dtype=np.float32)
    fl = []
    for s in _SHAPES:
        v = (g.randn(*s) * 50.0).astype(np.float32)
        idx = g.rand(*s) < 0.3
        v[idx] = g.choice(special, size=int(idx.sum()))
        fl.append(v)
    d["floats"] = (fl, _masks(1998, 2, (np.float32, np.uint8, np.float32)))                     # never an integer
    d["all_equal"] = ([np.full(s, -17.25, dtype=np.float32) for s in _SHAPES], _masks(777, 3, (np.int64, np.uint8, np.int32)))
    d["one_voxel"] = ([(g.randn(*s) * 9.0).astype(np.float32) for s in _SHAPES], _masks(1, 4, (np.uint8, np.int64, np.float32)))
    return d


_DATA = _datasets()


def _run_statistics(vols, masks, stats=None, per_round=None):
    s = stats or P.IntensityStatistics()
    tv, tm = [_dev(v) for v in vols], [_dev(m) for m in masks]
    rounds = 0
    while not s.done:
        for i, (v, m) in enumerate(zip(tv, tm)):
            if per_round is None or per_round(rounds, i):
                s.update(v, m)
        s.end_round()
        rounds += 1
    assert rounds == P.IntensityStatistics.rounds <= 4
    return s


@pytest.mark.parametrize("name", list(_DATA))
def test_intensity_statistics(name):
    vols, masks = _DATA[name]
    sel = np.concatenate([v[m > 0].reshape(-1) for v, m in zip(vols, masks)]).astype(np.float64)
    n = sel.size
    s = _run_statistics(vols, masks)
    res = s.result()
    assert list(res) == ["mean", "median", "std", "min", "max", "percentile_99_5", "percentile_00_5"]
    assert all(type(v) is float for v in res.values())
    want = R.intensity_statistics(sel)
    srt = np.sort(sel)
    assert s.n == n and res["min"] == srt[0] and res["max"] == srt[-1] and res["min"] == want["min"] and res["max"] == want["max"]
    integral = []
    for q, key in ((0.5, "percentile_00_5"), (50.0, "median"), (99.5, "percentile_99_5")):
        v = (n - 1) * (q / 100.0)
        lo = int(np.floor(v))
        integral.append(float(v).is_integer())
        for r in (lo, min(lo + 1, n - 1)):
            assert s.order_statistic(r) == srt[r], (q, r)                                        # exact, by value
        print(key, res[key], want[key])
        assert abs(res[key] - want[key]) <= 4 * np.spacing(abs(want[key]))
        assert abs(s.percentile(q) - np.percentile(sel, q)) <= 4 * np.spacing(abs(np.percentile(sel, q)))
    if name == "integer_hu":
        assert n == 2001 and all(integral)
    if name == "floats":
        assert n == 1998 and not any(integral)
    mean = np.mean(sel)
    assert abs(res["mean"] - mean) <= n * EPS53 * np.mean(np.abs(sel))
    assert abs(res["std"] - np.std(sel)) <= n * EPS53 * np.sqrt(np.mean((sel - mean) ** 2))


def test_intensity_statistics_refuses_bad_input():
    vols, masks = _DATA["integer_hu"]
    s = P.IntensityStatistics()
    for v, m in zip(vols, masks):
        s.update(_dev(v), _dev(np.zeros_like(m)))
    with pytest.raises(ValueError, match="no selected voxels"):
        s.end_round()
    bad = [v.copy() for v in vols]
    bad[1][tuple(np.argwhere(masks[1] > 0)[0])] = np.nan
    s = P.IntensityStatistics()
    for v, m in zip(bad, masks):
        s.update(_dev(v), _dev(m))
    with pytest.raises(ValueError, match="NaN"):
        s.end_round()
    unselected = [v.copy() for v in vols]
    unselected[1][masks[1] <= 0] = np.nan                  # NaNs outside the mask do not matter
    assert _run_statistics(unselected, masks).result() == _run_statistics(vols, masks).result()
    with pytest.raises(ValueError, match="same volumes"):
        _run_statistics(vols, masks, per_round=lambda rnd, i: not (rnd == 1 and i == 2))         # round 2 misses a volume
    with pytest.raises(ValueError, match="same volumes"):
        _run_statistics(vols, masks, per_round=lambda rnd, i: not (rnd == 2 and i == 0))         # round 3 misses a volume
    with pytest.raises(ValueError, match="same volumes"):
        _run_statistics(vols, masks, per_round=lambda rnd, i: rnd != 1)                          # round 2 sees no volume at all
    with pytest.raises(ValueError):
        P.IntensityStatistics().update(_dev(vols[0]), _dev(masks[1]))                            # shapes differ
    with pytest.raises(RuntimeError):
        P.IntensityStatistics().result()                                                         # rounds remain


def test_key_histogram_prefix_and_bins_against_the_host_key_map():
    vols, masks = _DATA["floats"]
    x, m = vols[2].reshape(-1), masks[2].reshape(-1)
    keys = P.float_key(x[m > 0])
    tx, tm = _dev(x), _dev(m)
    for prefix_bits, bin_bits in ((0, 11), (11, 11), (22, 10), (3, 5), (31, 1)):
        prefix = int(keys[len(keys) // 3]) >> (32 - prefix_bits) if prefix_bits else 0
        hist = torch.zeros(1 << bin_bits, dtype=torch.int64, device="cuda")
        for _ in range(2):                                                                       # the entry ADDS: two calls, twice the counts
            H.call("vx_key_histogram", tx.data_ptr(), tm.data_ptr(), -4, x.size, prefix, prefix_bits, bin_bits, hist.data_ptr(), None, None, H.stream_ptr())
        k = keys if not prefix_bits else keys[(keys >> np.uint32(32 - prefix_bits)) == prefix]
        want = np.bincount(((k >> np.uint32(32 - prefix_bits - bin_bits)) & np.uint32((1 << bin_bits) - 1)).astype(np.int64), minlength=1 << bin_bits)
        assert k.size > 0 and np.array_equal(hist.cpu().numpy(), 2 * want)


# ====================================================================================================================== resampling
def _tables(shape, src, dst, mode="bilinear"):
    so = P.output_shape(shape, src, dst)
    return so, [P.axis_table(n, no, s, d, mode) for n, no, s, d in zip(shape, so, src, dst)]


def test_resample_identity_is_bit_equal():
    x = _rs(3).randn(2, 5, 6, 7).astype(np.float32)
    for mode in ("bilinear", "nearest"):
        got = P.resample_to_spacing(_dev(x), (1.5, 0.8, 2.0), (1.5, 0.8, 2.0), mode)
        assert got.cpu().numpy().tobytes() == x.tobytes()


@pytest.mark.parametrize("ratio", [2.0, 0.5, 0.25])
def test_resample_dyadic_ratios_are_exact(ratio):
    x = _rs(5).randint(-3, 4, size=(2, 9, 6, 13)).astype(np.float32)
    src, dst = (ratio, ratio, ratio), (1.0, 1.0, 1.0)
    so, tabs = _tables(x.shape[1:], src, dst)
    assert so == tuple(R.out_size(n, ratio, 1.0) for n in x.shape[1:])
    got = P.resample_to_spacing(_dev(x), src, dst, "bilinear").cpu().numpy()
    want = R.resample_linear(x, tabs)
    assert got.shape == (2,) + so and want.astype(np.float32).astype(np.float64).tobytes() == want.tobytes()          # the premise: exactly representable
    assert got.tobytes() == want.astype(np.float32).tobytes()
    if ratio < 1:
        assert len({float(v) for t in tabs for v in t[2]}) > 1                                                        # fractional weights took part


@pytest.mark.parametrize("shape, src, dst", [((2, 7, 12, 10), (3.0, 1.0, 0.8), (1.5, 1.5, 1.5)), ((2, 9, 8, 11), (0.7, 0.7, 0.7), (1.0, 1.0, 1.0)),
                                             ((2, 1, 9, 14), (2.0, 1.0, 0.7), (1.0, 0.7, 1.0)), ((3, 6, 1, 1), (1.0, 5.0, 5.0), (0.3, 1.0, 1.0))])
def test_resample_trilinear(shape, src, dst):
    x = (_rs(8).randn(*shape) * 40.0).astype(np.float32)
    so, tabs = _tables(shape[1:], src, dst)
    got = P.resample_to_spacing(_dev(x), src, dst, "bilinear").cpu().numpy()
    assert got.shape == (shape[0],) + so
    want = R.resample_linear(x, tabs)                                                            # fp64, the same fp32 weights
    err = np.max(np.abs(got.astype(np.float64) - want))
    print(f"max err {err:.3e} bound {16 * EPS24 * np.max(np.abs(x)):.3e}")
    assert err <= 16 * EPS24 * np.max(np.abs(x))
    one = P.resample_to_spacing(_dev(x[1]), src, dst).cpu().numpy()                              # (D, H, W)
    assert one.tobytes() == got[1].tobytes()


@pytest.mark.parametrize("dtype", [np.uint8, np.int32, np.int64, np.float32])
def test_resample_nearest_labels_are_exact(dtype):
    g = _rs(13)
    lab = g.randint(0, 5, size=(2, 6, 7, 9)).astype(dtype)
    if dtype == np.int64:
        lab[0, 0, 0, 0], lab[1, 5, 6, 8] = (1 << 40) + 3, -(1 << 35)                             # all 64 bits travel
    if dtype == np.float32:
        lab[0, 1, 2, 3] = np.float32(-0.0)
    for src, dst in (((1.0, 1.0, 1.0), (2.0, 2.0, 2.0)), ((1.0, 3.0, 0.8), (2.0, 1.5, 1.5)), ((1.0, 1.0, 1.0), (0.5, 0.4, 1.0))):
        so = P.output_shape(lab.shape[1:], src, dst)
        idx = [R.nearest_index(n, no, s, d) for n, no, s, d in zip(lab.shape[1:], so, src, dst)]
        got = P.resample_to_spacing(_dev(lab), src, dst, "nearest").cpu().numpy()
        assert got.dtype == lab.dtype and got.shape == (2,) + so
        assert got.tobytes() == np.ascontiguousarray(R.resample_nearest(lab, idx)).tobytes()
    c = R.coords(6, 3, 1.0, 2.0)                                                                 # the first case: coordinates j / 2, ties at 1/2 and 1 1/2
    assert list(c) == [0.0, 0.5, 1.0] and list(R.nearest_index(7, 4, 1.0, 2.0)) == [0, 0, 1, 2]


def test_resample_nearest_half_ties_go_to_even():
    lab = np.arange(6, dtype=np.uint8).reshape(1, 1, 1, 6) + 10
    src, dst = (1.0, 1.0, 2.0), (1.0, 1.0, 1.0)                                                  # coordinates 0, 2, 4, then clamped to 5; size round(11) = 11
    got = P.resample_to_spacing(_dev(lab), src, dst, "nearest").cpu().numpy()
    assert got.reshape(-1).tolist() == [10, 12, 14] + [15] * 8
    src, dst = (1.0, 1.0, 1.0), (1.0, 1.0, 2.0)                                                  # size round(3.5) = 4; coordinates 0, .5, 1, 1.5 -> 0, 0, 1, 2
    assert P.resample_to_spacing(_dev(lab), src, dst, "nearest").cpu().numpy().reshape(-1).tolist() == [10, 10, 11, 12]
    lab5 = np.arange(5, dtype=np.int64).reshape(1, 1, 1, 5)
    src, dst = (1.0, 1.0, 0.5), (1.0, 1.0, 1.0)                                                  # coordinates 0, .5, 1 (size round(3.0) = 3): 0.5 -> 0
    assert P.resample_to_spacing(_dev(lab5), src, dst, "nearest").cpu().numpy().reshape(-1).tolist() == [0, 0, 1]
    lab9 = np.arange(9, dtype=np.float32).reshape(1, 1, 1, 9)
    src, dst = (1.0, 1.0, 1.5), (1.0, 1.0, 1.0)                                                  # 0, 1.5, 3, 4.5, 6, 7.5, ... size 13: 1.5 -> 2, 4.5 -> 4, 7.5 -> 8
    assert P.resample_to_spacing(_dev(lab9), src, dst, "nearest").cpu().numpy().reshape(-1).tolist() == [0, 2, 3, 4, 6, 8, 8, 8, 8, 8, 8, 8, 8]


def test_spacingd():
    g = _rs(17)
    img = (g.randn(2, 6, 8, 5) * 10).astype(np.float32)
    lab = g.randint(0, 3, size=(1, 6, 8, 5)).astype(np.uint8)
    data = {"image": _dev(img), "label": _dev(lab), "pixdim": (2.0, 1.0, 3.0), "label_pixdim": (2.0, 1.0, 3.0)}
    out = P.Spacingd(["image", "label"], (1.0, 1.5, 1.5), mode=("bilinear", "nearest"))(data)
    assert out["pixdim"] == (1.0, 1.5, 1.5) and out["label_pixdim"] == (1.0, 1.5, 1.5) and data["pixdim"] == (2.0, 1.0, 3.0)
    so = P.output_shape(img.shape[1:], (2.0, 1.0, 3.0), (1.0, 1.5, 1.5))
    assert tuple(out["image"].shape) == (2,) + so and tuple(out["label"].shape) == (1,) + so and out["label"].dtype == torch.uint8
    assert out["image"].cpu().numpy().tobytes() == P.resample_to_spacing(data["image"], (2.0, 1.0, 3.0), (1.0, 1.5, 1.5)).cpu().numpy().tobytes()
    with pytest.raises(KeyError):
        P.Spacingd(["image"], (1, 1, 1))({"image": data["image"]})
    with pytest.raises(ValueError):
        P.resample_to_spacing(data["image"], (1.0, 0.0, 1.0), (1.0, 1.0, 1.0))


# ====================================================================================================================== run_test.py
def test_run_test_with_the_preprocessing_data_module(tmp_path):
    """run_test.py (unchanged) as a fresh child process with --data_module veloxseg_amd.utils.preprocess: normalise per channel and resample from (2, 2, 3) to
    (1, 1, 1.5) on the GPU in front of the sliding window"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    cfg, _ = CASES["g2_32_m2"]
    mc, tc, te = tmp_path / "models.json", tmp_path / "train.json", tmp_path / "test.json"
    mc.write_text(json.dumps({"VeloxSeg": cfg}))
    tc.write_text(json.dumps(dict(TRAIN_CFG, patch_size={"AutoPETII": [32, 32, 32]})))
    te.write_text(json.dumps({"sliding_window": {"overlap": 0.25},
                              "preprocess": {"normalize": "channel", "resample_from": [2, 2, 3], "resample_to": [1, 1, 1.5]}}))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_test.py"), "--dataset_name", "AutoPETII", "--model_name", "VeloxSeg", "--train_config", str(tc),
                        "--model_config", str(mc), "--test_config", str(te), "--synthetic", "2", "--volume_shape", "24", "20", "22", "--out_csv", str(tmp_path / "res.csv"),
                        "--data_module", "veloxseg_amd.utils.preprocess"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = list(csv.reader(open(tmp_path / "res.csv")))
    assert len(rows) == 1 + 2 and [row[0] for row in rows[1:]] == ["synthetic_0", "synthetic_1"]
    assert all(np.isfinite(float(v)) for v in rows[1][1:])
    so = P.output_shape((24, 20, 22), (2, 2, 3), (1, 1, 1.5))
    assert so == (47, 39, 43) and float(rows[1][5]) <= np.prod(so) and 0 < float(rows[1][6]) <= np.prod(so)          # label count of the RESAMPLED volume
    assert float(rows[1][6]) > 24 * 20 * 22                                                                              # more labelled voxels than the source holds


def test_preprocessing_data_module_settings():
    import types
    args = types.SimpleNamespace(dataset_name="AutoPETII")
    for bad in ({"normalise": "channel"}, {"normalize": "minmax"}):
        with pytest.raises(ValueError):
            next(P.iter_volumes(args, {}, {"preprocess": bad}))
    inner = types.ModuleType("vx_test_inner_volumes")
    x = _rs(4).randn(1, 2, 6, 5, 7).astype(np.float32)
    y = _rs(5).randint(0, 2, size=(1, 1, 6, 5, 7))
    inner.iter_volumes = lambda a, tr, te: iter([("a", torch.from_numpy(x), torch.from_numpy(y), (2.0, 1.0, 1.0)), ("b", torch.from_numpy(x), torch.from_numpy(y))])
    sys.modules[inner.__name__] = inner
    try:
        got = list(P.iter_volumes(args, {"spacing": {"AutoPETII": [1.0, 1.0, 1.0]}}, {"preprocess": {"data_module": inner.__name__, "normalize": "zscore_foreground"}}))
        with pytest.raises(ValueError, match="target spacing"):
            list(P.iter_volumes(args, {}, {"preprocess": {"data_module": inner.__name__}}))
    finally:
        del sys.modules[inner.__name__]
    (na, xa, ya), (nb, xb, yb) = got
    assert (na, nb) == ("a", "b") and xa.is_cuda and ya.is_cuda
    assert tuple(xa.shape) == (1, 2, 11, 5, 7) and tuple(ya.shape) == (1, 1, 11, 5, 7) and ya.dtype == torch.int64          # the 4-tuple's spacing: resampled
    assert tuple(xb.shape) == (1, 2, 6, 5, 7) and tuple(yb.shape) == (1, 1, 6, 5, 7)                                          # no spacing, no resample_from: as it came
    assert xb[0].cpu().numpy().tobytes() == P.zscore_foreground(torch.from_numpy(x[0]).cuda()).cpu().numpy().tobytes()
