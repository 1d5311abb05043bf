"""Segmentations on the image's own grid, host side (no GPU): the inverse tables against tests/native_ref.py, the arg-max rule of the restatement, the header entry,
the argument checks of vx_native_argmax, the refusals of the new Python functions and the geometry check."""
import numpy as np
import pytest
import torch

import native_ref as N
import preprocess_ref as R
from veloxseg_amd.utils import preprocess as P


# ====================================================================================================================== tables
@pytest.mark.parametrize("net, native, s_net, s_nat", [((7, 12, 10), (14, 9, 67), (3.0, 1.0, 0.8), (1.5, 1.3, 0.11)), ((9, 8, 11), (6, 6, 8), (0.7,) * 3, (1.0,) * 3),
                                                       ((1, 9, 14), (1, 13, 10), (2.0, 1.0, 0.7), (1.0, 0.7, 1.0)), ((4, 7, 17), (13, 7, 67), (4.0, 1.0, 1.0), (1.0, 1.0, 0.25))])
def test_inverse_tables_against_the_restatement(net, native, s_net, s_nat):
    got = P.inverse_tables(net, native, s_net, s_nat)
    want = N.tables(net, native, s_net, s_nat)
    assert len(got) == 3
    for n, no, (i0, i1, w), (r0, r1, rw) in zip(net, native, got, want):
        assert i0.dtype == np.int32 and i1.dtype == np.int32 and w.dtype == np.float32 and len(i0) == len(i1) == len(w) == no          # the GIVEN extent
        assert np.array_equal(i0, r0) and np.array_equal(i1, r1) and w.tobytes() == rw.tobytes()
        assert 0 <= i0.min() and i1.max() <= n - 1 and np.all(i0 <= i1) and np.all((0.0 <= w) & (w < 1.0))
    near = P.inverse_tables(net, native, s_net, s_nat, "nearest")
    for no, s, d, n, (i0, i1, w) in zip(native, s_net, s_nat, net, near):
        assert np.array_equal(i0, R.nearest_index(n, no, s, d)) and np.array_equal(i0, i1) and np.all(w == 0)


def test_inverse_tables_where_round_does_not_invert():
    """13 voxels at spacing 1 go to the network's spacing 3 as round(12 / 3 + 1) = 5 voxels; back, the rule gives round(4 * 3 + 1) = 13 only by luck -- 14 voxels go
    to round(13 / 3 + 1) = round(5.33) = 5 as well, and 5 voxels come back as 13, not 14.  The native extent is therefore GIVEN, and the tail is clamped."""
    assert P.output_shape((14, 14, 13), (1.0,) * 3, (3.0,) * 3) == (5, 5, 5)
    assert P.output_shape((5, 5, 5), (3.0,) * 3, (1.0,) * 3) == (13, 13, 13)                     # not (14, 14, 13)
    tz, ty, tx = P.inverse_tables((5, 5, 5), (14, 14, 13), (3.0,) * 3, (1.0,) * 3)
    assert len(tz[0]) == 14 and len(tx[0]) == 13
    assert list(tz[0]) == [0, 3] + [4] * 12 and list(tz[1]) == [1, 4] + [4] * 12 and np.all(tz[2] == 0.0)          # past the last network voxel: i0 = i1 = n - 1, w = 0
    frac = P.inverse_tables((5, 5, 5), (14, 14, 13), (1.0,) * 3, (3.0,) * 3)[0]
    assert list(frac[0][:4]) == [0, 0, 0, 1] and frac[2][1] == np.float32(1.0 / 3.0)
    for bad in (dict(net_shape=(5, 5)), dict(native_shape=(14, 0, 13)), dict(native_shape=(14.5, 14, 13)), dict(net_spacing=(3.0, 0.0, 3.0)),
                dict(native_spacing=(1.0, float("nan"), 1.0)), dict(mode="cubic")):
        kw = dict(net_shape=(5, 5, 5), native_shape=(14, 14, 13), net_spacing=(3.0,) * 3, native_spacing=(1.0,) * 3)
        kw.update(bad)
        with pytest.raises(ValueError):
            P.inverse_tables(**kw)


def test_the_restated_argmax_rule():
    nan, inf = np.nan, np.inf
    v = np.array([[1.0, 2.0, -0.0, nan, -inf, 3.0, inf, 5.0],
                  [1.0, 3.0, 0.0, 7.0, -inf, nan, inf, nan],
                  [0.5, 3.0, 0.0, nan, -inf, nan, -inf, nan]])
    assert N.first_nan_else_first_max(v).tolist() == [0, 1, 0, 0, 0, 1, 0, 1]
    assert N.first_nan_else_first_max(v).dtype == np.uint8
    assert N.top_two_margin(np.array([[1.0, 4.0], [3.0, 4.0], [2.5, -1.0]])).tolist() == [0.5, 0.0]
    x = np.random.RandomState(2).randn(3, 4, 5, 6)
    assert np.array_equal(N.first_nan_else_first_max(x), np.argmax(x, axis=0))
    ident = N.labels_on_native_grid(x, (4, 5, 6), (2.0, 1.0, 0.5), (2.0, 1.0, 0.5))
    assert np.array_equal(ident, np.argmax(x, axis=0))


# ====================================================================================================================== C entry without a GPU
def test_header_declares_the_entry():
    from veloxseg_amd import _hip
    protos = _hip.parse_header()
    ret, args = protos["vx_native_argmax"]
    assert ret == "int"
    assert [a for _, a in args] == ["logits", "labels", "C", "D", "H", "W", "Do", "Ho", "Wo", "i0", "i1", "w", "stream"]
    assert [t for t, _ in args] == ["const float*", "unsigned char*"] + ["int"] * 7 + ["const int*", "const int*", "const float*", "void*"]
    assert not "vx_native_argmax".startswith(("vx_resample_", "vx_moments_", "vx_normalize_", "vx_key_"))
    assert _hip.ABI_VERSION == 1


_BAD_CALLS = [
    ("null logits", (None, 1, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, None)),
    ("null labels", (1, None, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, None)),
    ("null i0", (1, 1, 2, 2, 2, 2, 2, 2, 2, None, 1, 1, None)),
    ("null i1", (1, 1, 2, 2, 2, 2, 2, 2, 2, 1, None, 1, None)),
    ("null w", (1, 1, 2, 2, 2, 2, 2, 2, 2, 1, 1, None, None)),
    ("C = 0", (1, 1, 0, 2, 2, 2, 2, 2, 2, 1, 1, 1, None)),
    ("C = 257", (1, 1, 257, 2, 2, 2, 2, 2, 2, 1, 1, 1, None)),
    ("C < 0", (1, 1, -1, 2, 2, 2, 2, 2, 2, 1, 1, 1, None)),
    ("D = 0", (1, 1, 2, 0, 2, 2, 2, 2, 2, 1, 1, 1, None)),
    ("W = 0", (1, 1, 2, 2, 2, 0, 2, 2, 2, 1, 1, 1, None)),
    ("Ho = 0", (1, 1, 2, 2, 2, 2, 2, 0, 2, 1, 1, 1, None)),
    ("Wo < 0", (1, 1, 2, 2, 2, 2, 2, 2, -3, 1, 1, 1, None)),
]


@pytest.mark.parametrize("case", range(len(_BAD_CALLS)), ids=[c[0] for c in _BAD_CALLS])
def test_bad_arguments_return_error_codes_without_gpu(case):
    from veloxseg_amd import _hip
    with pytest.raises(RuntimeError, match=r"vx_native_argmax failed \(rc=-1\): vx_native_argmax"):
        _hip.call("vx_native_argmax", *_BAD_CALLS[case][1])


# ====================================================================================================================== Python surface
def test_cpu_tensors_raise():
    x = torch.zeros(2, 4, 4, 4)
    for fn in (lambda t: P.labels_on_native_grid(t, (8, 8, 8), (2, 2, 2), (1, 1, 1)), lambda t: P.labels_on_native_grid(t[None], (8, 8, 8), (2, 2, 2), (1, 1, 1)),
               lambda t: P.resample_to_shape(t, (8, 8, 8), (2, 2, 2), (1, 1, 1)), lambda t: P.resample_to_shape(t.to(torch.uint8), (8, 8, 8), (2, 2, 2), (1, 1, 1), "nearest")):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)


def test_infer_volume_refuses_a_bad_native_dict_before_any_gpu_work():
    from veloxseg_amd.utils import inference_runtime as IR
    model = torch.nn.Identity()
    good = {"native_shape": (8, 8, 8), "native_spacing": (1.0, 1.0, 1.0), "net_spacing": (2.0, 2.0, 2.0)}
    for bad in ({"native_shape": (8, 8, 8)}, dict(good, native_shape=(8, 8)), dict(good, native_shape=(8, 0, 8)), dict(good, net_spacing=(2.0, 2.0)),
                dict(good, native_spacing=(1.0, -1.0, 1.0)), dict(good, more=1), [8, 8, 8]):
        with pytest.raises(ValueError):
            IR.infer_volume(model, torch.zeros(1, 1, 4, 4, 4), (4, 4, 4), 1, 0.5, native=bad)
    with pytest.raises(RuntimeError, match="MI355X"):                                            # a good dict gets as far as the sliding window, which has no CPU path
        IR.infer_volume(model, torch.zeros(1, 1, 4, 4, 4), (4, 4, 4), 1, 0.5, native=good)


def test_check_native_geometry():
    good = {"native_shape": [8, 9, 10], "native_spacing": [1, 1.5, 2], "net_spacing": np.array([2.0, 2.0, 2.0])}
    got = P.check_native_geometry(good)
    assert got == {"native_shape": (8, 9, 10), "native_spacing": (1.0, 1.5, 2.0), "net_spacing": (2.0, 2.0, 2.0)}
    assert all(type(v) is int for v in got["native_shape"]) and all(type(v) is float for v in got["native_spacing"] + got["net_spacing"])
    assert P.check_native_geometry(got) == got
    for bad in ({"native_shape": (8, 8, 8)}, dict(good, native_shape=(8, 8)), dict(good, native_shape=(8, 0, 8)), dict(good, native_shape=(8, 8.5, 8)),
                dict(good, native_shape=(8, True, 8)), dict(good, net_spacing=(2.0, 2.0)), dict(good, native_spacing=(1.0, float("inf"), 1.0)), dict(good, more=1), None, (8, 8, 8)):
        with pytest.raises(ValueError):
            P.check_native_geometry(bad)
