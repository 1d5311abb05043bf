"""Volume preprocessing, host side (no GPU): the fp64 restatements against the golden recorded from the reference, the resampling tables, the key map, and the
argument checks of every new C entry."""
import os

import numpy as np
import pytest
import torch

import preprocess_ref as R
from veloxseg_amd.utils import preprocess as P


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = torch.load(os.path.join(golden_dir, "preprocess.pt"), weights_only=True)
    assert all(isinstance(v, torch.Tensor) for v in g.values())
    return {k: v.numpy() for k, v in g.items()}


def _props(v):
    return {"mean": float(v[0]), "std": float(v[1]), "percentile_00_5": float(v[2]), "percentile_99_5": float(v[3])}


@pytest.mark.parametrize("name", ["integer", "float", "min_repeats", "constant"])
def test_zscore_restatement_equals_the_reference_bit_for_bit(golden, name):
    x = golden["in_" + name]
    assert x.dtype == np.float64
    got = R.zscore_reference_call(x)
    assert got.tobytes() == golden["zscore_" + name].tobytes()
    assert R.zscore(x, x > x.min()).tobytes() == golden["zscore_" + name].tobytes()


def test_the_reference_call_normalises_every_voxel(golden):
    """`mask = seg >= 0` of a boolean seg is true everywhere: the recorded output rewrote the voxels at the minimum too and used whole-volume statistics, which is
    what zscore_volume computes; zscore_foreground (statistics over x > x.min(), minimum voxels untouched) is a different function on such a volume"""
    x, z = golden["in_min_repeats"], golden["zscore_min_repeats"]
    at_min = x == x.min()
    assert at_min.sum() > 1000 and not np.any(z[at_min] == x[at_min])
    flat = x.reshape(-1)
    want = (x - flat.mean()) / max(flat.std(), 1e-8)
    assert z.tobytes() == want.tobytes()
    fg = R.zscore_foreground(x)
    assert np.array_equal(fg[at_min], x[at_min]) and not np.allclose(fg[~at_min], z[~at_min])
    n, mean, std = R.foreground_moments(x)
    assert n == (~at_min).sum() and abs(fg[~at_min].mean()) < 1e-12 and abs(fg[~at_min].std() - 1.0) < 1e-12
    assert np.array_equal(R.zscore_foreground(golden["in_constant"]), golden["in_constant"])            # empty mask: unchanged
    assert np.all(golden["zscore_constant"] == 0.0)                                                      # the reference: (x - x) / 1e-8


def test_ctnorm_restatement_equals_the_reference_bit_for_bit(golden):
    assert R.ct_norm(golden["in_integer"], _props(golden["ct_props"])).tobytes() == golden["ct_integer"].tobytes()
    flat = _props(golden["ct_flat_props"])
    assert flat["std"] == 0.0
    assert R.ct_norm(golden["in_float"], flat).tobytes() == golden["ct_flat_float"].tobytes()


def test_normalize_intensity_restatement():
    x = np.random.RandomState(0).randn(2, 3, 4, 5) * 3 + 2
    x[1] = 4.0
    got = R.normalize_intensity(x, True)
    assert abs(got[0].mean()) < 1e-12 and abs(got[0].std() - 1) < 1e-12 and np.all(got[1] == 0.0)
    whole = R.normalize_intensity(x, False)
    assert abs(whole.mean()) < 1e-12 and abs(whole.std() - 1) < 1e-12


# ====================================================================================================================== resampling tables
@pytest.mark.parametrize("n, src, dst, want", [(4, 1.0, 2.0, 2), (6, 1.0, 2.0, 4), (1, 1.0, 2.0, 1), (1, 3.0, 0.5, 1), (5, 1.0, 1.0, 5), (5, 2.0, 1.0, 9),
                                               (9, 1.0, 4.0, 3), (7, 3.0, 1.5, 13), (10, 1.0, 0.7, 14), (8, 1.0, 2.0, 4), (2, 1.0, 2.0, 2), (3, 1.0, 4.0, 2)])
def test_output_shape_rounds_half_to_even(n, src, dst, want):
    assert R.out_size(n, src, dst) == want
    assert P.output_shape((n, n, n), (src,) * 3, (dst,) * 3) == (want,) * 3
    assert P.output_shape((n, 1, 5), (src, 1.0, 1.0), (dst, 9.0, 1.0)) == (want, 1, 5)


def test_half_even_cases_are_what_they_claim():
    assert (4 - 1) * 1.0 / 2.0 + 1 == 2.5 and (6 - 1) * 1.0 / 2.0 + 1 == 3.5 and (2 - 1) / 2.0 + 1 == 1.5 and (3 - 1) / 4.0 + 1 == 1.5


@pytest.mark.parametrize("n, src, dst", [(7, 3.0, 1.5), (10, 1.0, 0.7), (6, 1.0, 2.0), (9, 0.8, 1.5), (1, 2.0, 1.0), (5, 1.0, 1.0), (4, 1.0, 0.25)])
def test_axis_table_against_direct_arithmetic(n, src, dst):
    no = R.out_size(n, src, dst)
    i0, i1, w = P.axis_table(n, no, src, dst)
    assert i0.dtype == np.int32 and i1.dtype == np.int32 and w.dtype == np.float32 and len(i0) == len(i1) == len(w) == no
    for j in range(no):
        c = min(max(j * src / dst, 0.0), float(n - 1))
        f = int(np.floor(c))
        assert (int(i0[j]), int(i1[j])) == (f, min(f + 1, n - 1)) and w[j] == np.float32(c - f)
        assert 0 <= i0[j] <= i1[j] <= n - 1 and 0.0 <= w[j] < 1.0
    r0, r1, rw = R.table(n, no, src, dst)
    assert np.array_equal(r0, i0) and np.array_equal(r1, i1) and np.array_equal(rw.astype(np.float32), w)


def test_axis_table_clamps_at_the_far_edge():
    # more outputs than the rule gives: the coordinate is clamped to n - 1, where i1 = i0 = n - 1 and w = 0
    i0, i1, w = P.axis_table(5, 12, 2.0, 1.0)
    assert list(i0[:3]) == [0, 2, 4] and list(i1[:3]) == [1, 3, 4] and np.all(i0[2:] == 4) and np.all(i1[2:] == 4) and np.all(w == 0.0)
    i0, i1, w = P.axis_table(4, 4, 1.5, 1.0)                   # 0, 1.5, 3, 4.5 -> clamp 3
    assert list(i0) == [0, 1, 3, 3] and list(i1) == [1, 2, 3, 3] and list(w) == [0.0, 0.5, 0.0, 0.0]


def test_nearest_table_ties_go_to_even():
    i0, i1, w = P.axis_table(6, 11, 1.0, 2.0, "nearest")      # coordinates 0, .5, 1, 1.5, 2, 2.5 ... clamped at 5
    assert list(i0) == [0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 5] and np.array_equal(i0, i1) and np.all(w == 0)
    assert np.array_equal(R.nearest_index(6, 11, 1.0, 2.0), i0)


@pytest.mark.parametrize("bad", [(0.0, 1.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 1.0), (1.0, 1.0, float("inf"))])
def test_spacings_must_be_positive(bad):
    with pytest.raises(ValueError):
        P.output_shape((4, 4, 4), bad, (1.0, 1.0, 1.0))
    with pytest.raises(ValueError):
        P.output_shape((4, 4, 4), (1.0, 1.0, 1.0), bad)
    with pytest.raises(ValueError):
        P.Spacingd(["image"], bad)


# ====================================================================================================================== key map
def test_key_map_is_strictly_order_preserving():
    tiny = np.float32(1e-45)
    vals = np.array([-np.inf, -3.4e38, -1024.0, -1.5, -1.0, -1.17549435e-38, -3e-45, -tiny, -0.0, 0.0, tiny, 3e-45, 1.17549435e-38, 0.5, 1.0, 3071.0, 3.4e38, np.inf],
                    dtype=np.float32)
    assert np.array_equal(np.sort(vals, kind="stable"), vals) and vals[6] < vals[7] < 0 < vals[10] < vals[11]          # denormals survive
    keys = P.float_key(vals)
    assert keys.dtype == np.uint32 and np.all(keys[1:] > keys[:-1])
    back = P.key_float(keys)
    assert back.view(np.uint32).tolist() == vals.view(np.uint32).tolist()
    rnd = np.random.RandomState(1).randn(4096).astype(np.float32) * 1e3
    order = np.argsort(P.float_key(rnd), kind="stable")
    assert np.array_equal(rnd[order], np.sort(rnd))


# ====================================================================================================================== C entries without a GPU
_BAD_CALLS = [
    ("vx_moments_partials", (None, 8, None, None, 0, None, 1, None)),
    ("vx_moments_partials", (1, 8, None, None, 0, None, None, None)),
    ("vx_moments_partials", (1, 0, None, None, 0, None, 1, None)),
    ("vx_moments_partials", (1, 8, None, 1, 2, None, 1, None)),
    ("vx_moments_reduce", (None, 1, 0, None, -1, None)),
    ("vx_moments_reduce", (1, None, 0, None, -1, None)),
    ("vx_moments_reduce", (1, 1, 0, None, 0, None)),
    ("vx_moments_reduce", (1, 1, 0, 1, 2, None)),
    ("vx_moments_stats", (None, 8, None, 1, 1, None)),
    ("vx_moments_stats", (1, 8, None, None, 1, None)),
    ("vx_moments_stats", (1, 8, None, 1, None, None)),
    ("vx_moments_stats", (1, -1, None, 1, 1, None)),
    ("vx_normalize_apply", (None, 1, 8, None, None, 0.0, 1.0, 0, 0.0, 0.0, 0, 1e-8, None)),
    ("vx_normalize_apply", (1, None, 8, None, None, 0.0, 1.0, 0, 0.0, 0.0, 0, 1e-8, None)),
    ("vx_normalize_apply", (1, 1, 0, None, None, 0.0, 1.0, 0, 0.0, 0.0, 0, 1e-8, None)),
    ("vx_normalize_apply", (1, 1, 8, None, None, 0.0, 1.0, 0, 0.0, 0.0, 2, 1e-8, None)),
    ("vx_normalize_apply", (1, 1, 8, None, None, 0.0, 1.0, 1, 2.0, 1.0, 0, 1e-8, None)),
    ("vx_normalize_apply", (4096, 4096 + 16, 8, None, None, 0.0, 1.0, 0, 0.0, 0.0, 0, 1e-8, None)),
    ("vx_key_histogram", (None, None, 0, 8, 0, 0, 11, 1, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 8, 0, 0, 11, None, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 0, 0, 0, 11, 1, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 8, 0, 0, 12, 1, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 8, 0, 0, 0, 1, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 8, 0, 22, 11, 1, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 8, 2048, 11, 11, 1, None, None, None)),
    ("vx_key_histogram", (1, None, 0, 8, 1, 0, 11, 1, None, None, None)),
    ("vx_key_histogram", (1, 1, 2, 8, 0, 0, 11, 1, None, None, None)),
    ("vx_resample_axes", (None, 1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1, 0, None)),
    ("vx_resample_axes", (1, 1, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1, 0, None)),
    ("vx_resample_axes", (1, 2, 1, 2, 2, 2, 2, 2, 2, None, 1, 1, 0, None)),
    ("vx_resample_axes", (1, 2, 1, 2, 2, 2, 2, 2, 2, 1, None, 1, 0, None)),
    ("vx_resample_axes", (1, 2, 1, 2, 2, 2, 2, 2, 2, 1, 1, None, 0, None)),
    ("vx_resample_axes", (1, 2, 1, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, None)),
    ("vx_resample_axes", (1, 2, 1, 2, 0, 2, 2, 2, 2, 1, 1, 1, 0, None)),
    ("vx_resample_axes", (1, 2, 1, 2, 2, 2, 2, 2, 0, 1, 1, 1, 0, None)),
    ("vx_resample_axes_label", (None, 2, 1, 1, 2, 2, 2, 2, 2, 2, 1, None)),
    ("vx_resample_axes_label", (1, 2, 1, 1, 2, 2, 2, 2, 2, 2, None, None)),
    ("vx_resample_axes_label", (1, 2, 2, 1, 2, 2, 2, 2, 2, 2, 1, None)),
    ("vx_resample_axes_label", (1, 2, 1, 0, 2, 2, 2, 2, 2, 2, 1, None)),
]


@pytest.mark.parametrize("case", range(len(_BAD_CALLS)))
def test_bad_arguments_return_error_codes_without_gpu(case):
    from veloxseg_amd import _hip
    name, args = _BAD_CALLS[case]
    with pytest.raises(RuntimeError, match=name + r" failed \(rc=-[13]\): " + name):
        _hip.call(name, *args)


def test_every_new_entry_is_covered_and_constant_queries_answer():
    from veloxseg_amd import _hip
    new = {n for n in _hip.parse_header() if n.startswith(("vx_moments_", "vx_normalize_", "vx_key_", "vx_resample_"))}
    assert new == {"vx_moments_blocks", "vx_moments_ws_doubles", "vx_moments_partials", "vx_moments_reduce", "vx_moments_stats", "vx_normalize_apply",
                   "vx_key_histogram", "vx_resample_axes", "vx_resample_axes_label"}
    assert new - {n for n, _ in _BAD_CALLS} == {"vx_moments_blocks", "vx_moments_ws_doubles"}
    assert _hip.query("vx_moments_ws_doubles") == 3 * _hip.query("vx_moments_blocks") > 0


def test_cpu_tensors_raise():
    x = torch.zeros(1, 4, 4, 4)
    for fn in (P.zscore_foreground, P.zscore_volume, P.moments, lambda t: P.ct_normalize(t, {"mean": 0, "std": 1, "percentile_00_5": 0, "percentile_99_5": 1}),
               lambda t: P.resample_to_spacing(t, (1, 1, 1), (2, 2, 2)), lambda t: P.NormalizeIntensityd(["image"])({"image": t}),
               lambda t: P.Spacingd(["image"], (2, 2, 2))({"image": t, "pixdim": (1, 1, 1)}),
               lambda t: P.IntensityStatistics().update(t, t)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)


def test_surface_refuses_what_it_does_not_implement():
    for kw in ({"nonzero": True}, {"subtrahend": 1.0}, {"divisor": 2.0}):
        with pytest.raises(NotImplementedError):
            P.NormalizeIntensityd(["image"], **kw)
    with pytest.raises(ValueError):
        P.Spacingd(["image", "label"], (1, 1, 1), mode=("bilinear",))
    with pytest.raises(ValueError):
        P.Spacingd(["image"], (1, 1, 1), mode="cubic")
    with pytest.raises(ValueError):
        P.IntensityStatistics(percentiles=(101.0,))
    assert P.IntensityStatistics.rounds == 3 <= 4
