"""Segmentations on the image's own grid (csrc/preprocess.hip vx_native_argmax, utils/preprocess.py labels_on_native_grid / resample_to_shape,
infer_volume(native=)) against the composition of the existing kernels and the numpy restatement of tests/native_ref.py.

What is held to `==`: the fused labels against vx_argmax_channels of the resampled logits on every input (NaN, inf, -0.0 planted); against the fp64 restatement where
every interpolated value is exactly representable (integer data, dyadic ratios), ties included.  Off exact data the restatement decides a voxel only where its fp64
top-two margin is at least 2 * 16 * 2^-24 * max|x|: twice the per-value bound tests/test_preprocess_gpu.py::test_resample_trilinear holds the interpolation to (two values
move towards each other by at most that much); at most 0.1 % of the voxels may fall under it."""

import numpy as np
import pytest
import torch

import native_ref as N
from veloxseg_amd import _hip as H
from veloxseg_amd.utils import preprocess as P

pytestmark = pytest.mark.gpu
EPS24 = 2.0 ** -24

# (K, network shape, native shape, network spacing, native spacing).  Together they reach every row form of the kernel: rows whose two z (y) source indices differ
# and rows where they are the same index (z: the tail of the first and last geometry and all of the third; y: the tail of the third, the last row of the fourth).
_GEOMETRIES = {
    "up_odd_w67": (2, (7, 12, 10), (14, 9, 67), (3.0, 1.0, 0.8), (1.5, 1.3, 0.11)),          # Wo neither a multiple of 4 nor of 64, 14 * 9 rows no multiple of 4
    "down_w8": (4, (9, 8, 11), (6, 6, 8), (0.7, 0.7, 0.7), (1.0, 1.0, 1.0)),                  # downsampling, Wo % 4 == 0, fractional weights on every axis
    "d1": (3, (1, 9, 14), (1, 13, 10), (2.0, 1.0, 0.7), (1.0, 0.7, 1.0)),                     # D = 1: i1 is clamped to i0
    "w130": (9, (6, 5, 7), (11, 5, 130), (1.0, 1.0, 1.0), (0.5, 1.0, 0.05)),                  # Wo > 128: a lane walks more than two voxels
}


def _rs(seed):
    return np.random.RandomState(seed)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _argmax_channels(t):
    """vx_argmax_channels of a (K, D, H, W) device tensor -> uint8 (D, H, W)"""
    K, V = int(t.shape[0]), int(t[0].numel())
    out = torch.empty(tuple(t.shape[1:]), dtype=torch.uint8, device=t.device)
    H.call("vx_argmax_channels", H.P(t.contiguous()), H.P(out, torch.uint8), 1, K, V, H.stream_ptr())
    return out


def _composition(t, so, s_net, s_nat):
    return _argmax_channels(P.resample_to_shape(t, so, s_net, s_nat, "bilinear"))


def _plant(x, tabs):
    """special values over a random volume, in place: NaN, +-inf and -0.0 voxels, whole columns of +-0.0, and one NaN that the native grid reaches only through a
    zero weight -> the (class, z, y, x) of that NaN, or None when the geometry has no such voxel"""
    g = _rs(21)
    K = x.shape[0]
    n = x[0].size
    flat = x.reshape(K, n)
    for val in (np.nan, np.inf, -np.inf, -0.0):
        idx = g.randint(0, n, size=max(n // 40, 2))
        flat[g.randint(0, K, size=idx.size), idx] = val
    cols = g.randint(0, n, size=max(n // 40, 2))
    flat[:, cols] = 0.0
    flat[g.randint(0, K, size=cols.size), cols] = -0.0                 # a column of zeros of both signs: the first one wins
    for axis, (i0, i1, w) in enumerate(tabs):
        only_zero = [int(v) for v, wt in zip(i1, w) if wt == 0.0 and int(v) not in set(int(u) for u in i0)]
        if only_zero:
            at = [0, 0, 0]
            at[axis] = only_zero[0]
            x[:, :2, :2, :2] = g.randn(*x[:, :2, :2, :2].shape).astype(np.float32)          # nothing else special around the first native voxel
            x[(K - 1,) + tuple(at)] = np.nan
            return (K - 1,) + tuple(at)
    return None


@pytest.mark.parametrize("name", list(_GEOMETRIES))
def test_fused_labels_equal_the_composition_byte_for_byte(name):
    K, sp, so, s_net, s_nat = _GEOMETRIES[name]
    x = (_rs(8).randn(K, *sp) * 40.0).astype(np.float32)
    tabs = N.tables(sp, so, s_net, s_nat)
    corner = _plant(x, tabs)
    t = _dev(x)
    got = P.labels_on_native_grid(t, so, s_net, s_nat)
    want = _composition(t, so, s_net, s_nat)
    assert got.dtype == torch.uint8 and tuple(got.shape) == so and got.is_contiguous()
    assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    assert P.labels_on_native_grid(t[None], so, s_net, s_nat).cpu().numpy().tobytes() == got.cpu().numpy().tobytes()          # (1, K, d, h, w)
    labels = got.cpu().numpy()
    vals = N.values_on_native_grid(x, so, s_net, s_nat)
    # a + w (b - a) with a = +-inf is NaN for every w; an inf comes out only where b = +-inf meets a finite a under a fractional weight
    assert np.isinf(x).sum() > 2 and np.isnan(vals).any(0).sum() > 0 and (name != "down_w8" or np.isinf(vals).sum() > 0)
    nan_cols = np.isnan(vals).any(0)
    assert np.array_equal(labels[nan_cols], N.first_nan_else_first_max(vals)[nan_cols])          # NaN in or out is exact in any precision
    if name == "up_odd_w67":
        # the premise: network plane z = 1 is reached only as i1 of native z = 0, with weight 0 -- and the NaN still decides that voxel (0 * NaN is NaN)
        assert corner == (K - 1, 1, 0, 0) and tabs[0][1][0] == 1 and tabs[0][2][0] == 0.0 and 1 not in tabs[0][0]
        assert np.isnan(x[:, :2, :2, :2]).sum() == 1 and np.isnan(vals[K - 1, 0, 0, 0]) and labels[0, 0, 0] == K - 1
    # the label base needs no alignment
    buf = torch.zeros(int(np.prod(so)) + 1, dtype=torch.uint8, device="cuda")
    i0, i1, w = (_dev(np.concatenate([tb[k] for tb in P.inverse_tables(sp, so, s_net, s_nat)])) for k in range(3))
    H.call("vx_native_argmax", t.data_ptr(), buf.data_ptr() + 1, K, *sp, *so, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), H.stream_ptr())
    assert int(buf[0]) == 0 and buf[1:].cpu().numpy().tobytes() == labels.tobytes()


def test_identity_geometry_is_the_plain_argmax():
    """equal spacings and the shape itself: every weight is 0 and the value is a + 0 (b - a) = a for finite data, so the labels are vx_argmax_channels' of the logits
    (ties and zeros of both signs planted).  With NaN / inf planted a neighbour reaches a voxel through the zero weight (0 * NaN), and the fused labels are the
    composition's, not the plain arg-max's."""
    so, sp3 = (6, 7, 12), (1.5, 0.75, 2.0)
    # the premise: every weight is 0 (a spacing of 0.8 would not do: 3 * 0.8 / 0.8 is 3 + 4.4e-16 in fp64, and that weight moves a zero)
    assert all(np.all(w == 0.0) and np.array_equal(i0, np.arange(n)) for n, (i0, _, w) in zip(so, P.inverse_tables(so, so, sp3, sp3)))
    x = (_rs(8).randn(5, *so) * 40.0).astype(np.float32)
    g = _rs(22)
    cols = g.randint(0, x[0].size, size=40)
    x.reshape(5, -1)[:, cols[:20]] = 0.0
    x.reshape(5, -1)[g.randint(0, 5, size=20), cols[:20]] = -0.0                             # columns of zeros of both signs
    x.reshape(5, -1)[g.randint(1, 5, size=20), cols[20:]] = x.reshape(5, -1)[0, cols[20:]] + 1000.0
    x.reshape(5, -1)[0, cols[20:]] += 1000.0                                                  # an exact tie of class 0 and a later class at the top
    t = _dev(x)
    got = P.labels_on_native_grid(t, so, sp3, sp3).cpu().numpy()
    assert got.tobytes() == _argmax_channels(t).cpu().numpy().tobytes()
    assert got.tobytes() == _composition(t, so, sp3, sp3).cpu().numpy().tobytes()
    assert got.tobytes() == N.first_nan_else_first_max(x).tobytes() and np.all(got.reshape(-1)[cols] == 0)
    assert np.array_equal(P.resample_to_shape(t, so, sp3, sp3).cpu().numpy(), x)          # by value: -0.0 + 0 * (b - a) is +0.0
    _plant(x, [])
    t = _dev(x)
    got = P.labels_on_native_grid(t, so, sp3, sp3).cpu().numpy()
    assert got.tobytes() == _composition(t, so, sp3, sp3).cpu().numpy().tobytes()
    assert got.tobytes() != _argmax_channels(t).cpu().numpy().tobytes()                      # the zero weights let NaN through


@pytest.mark.parametrize("K, sp, so, s_net, s_nat", [(4, (5, 6, 9), (9, 11, 17), (2.0,) * 3, (1.0,) * 3), (2, (9, 6, 13), (5, 3, 7), (1.0,) * 3, (2.0,) * 3),
                                                     (3, (4, 7, 17), (13, 7, 67), (4.0, 1.0, 1.0), (1.0, 1.0, 0.25))])
def test_exact_oracle_with_ties(K, sp, so, s_net, s_nat):
    """integer data and dyadic ratios: every interpolated value is exactly representable, so the kernel's values are the restatement's and the labels are held to ==,
    at the many exact ties too (first maximum): 45.8 %, 9.5 % and 26.9 % of the voxels under the coordinate rule of axis_table (native index j samples the network
    coordinate j * net / native).  The third geometry asks for 67 voxels where the spacings give 65: the clamped tail."""
    x = _rs(5).randint(-3, 4, size=(K,) + sp).astype(np.float32)
    want_v = N.values_on_native_grid(x, so, s_net, s_nat)
    assert want_v.astype(np.float32).astype(np.float64).tobytes() == want_v.tobytes()          # the premise: exactly representable
    ties = float(np.mean(N.top_two_margin(want_v) == 0.0))
    print(f"exact top-two ties: {100 * ties:.1f} % of {want_v[0].size} voxels")
    assert ties >= 0.05
    if so[2] == 67:
        assert P.output_shape(sp, s_net, s_nat)[2] == 65 and tuple(P.inverse_tables(sp, so, s_net, s_nat)[2][0][-3:]) == (16, 16, 16)
    got = P.labels_on_native_grid(_dev(x), so, s_net, s_nat).cpu().numpy()
    assert got.shape == so and got.tobytes() == N.first_nan_else_first_max(want_v).tobytes()
    res = P.resample_to_shape(_dev(x), so, s_net, s_nat).cpu().numpy()
    assert res.tobytes() == want_v.astype(np.float32).tobytes()


@pytest.mark.parametrize("name", list(_GEOMETRIES))
def test_independent_oracle_off_exact_data(name):
    K, sp, so, s_net, s_nat = _GEOMETRIES[name]
    x = (_rs(8).randn(K, *sp) * 40.0).astype(np.float32)
    want_v = N.values_on_native_grid(x, so, s_net, s_nat)
    want = N.first_nan_else_first_max(want_v)
    decided = N.top_two_margin(want_v) >= 2 * 16 * EPS24 * np.max(np.abs(x))
    print(f"{name}: {int((~decided).sum())} of {decided.size} voxels under the margin")
    assert (~decided).mean() <= 1e-3
    got = P.labels_on_native_grid(_dev(x), so, s_net, s_nat).cpu().numpy()
    assert np.array_equal(got[decided], want[decided])


def test_class_range():
    one = P.labels_on_native_grid(_dev((_rs(3).randn(1, 4, 5, 6) * 9).astype(np.float32)), (7, 3, 9), (1.0, 2.0, 1.0), (0.5, 3.0, 0.7))
    assert tuple(one.shape) == (7, 3, 9) and int(one.max()) == 0
    x = _rs(4).randn(256, 2, 2, 3).astype(np.float32)
    x[255] = 50.0
    got = P.labels_on_native_grid(_dev(x), (3, 3, 5), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5))
    assert tuple(got.shape) == (3, 3, 5) and bool((got == 255).all())
    big = torch.zeros((257, 2, 2, 3), device="cuda")
    with pytest.raises(ValueError, match="256"):
        P.labels_on_native_grid(big, (3, 3, 5), (1.0, 1.0, 1.0), (0.5, 0.5, 0.5))
    out = torch.full((3, 3, 5), 77, dtype=torch.uint8, device="cuda")
    i0, i1, w = (_dev(np.concatenate([tb[k] for tb in P.inverse_tables((2, 2, 3), (3, 3, 5), (1.0,) * 3, (0.5,) * 3)])) for k in range(3))
    for C in (257, 0):
        with pytest.raises(RuntimeError, match=r"vx_native_argmax failed \(rc=-1\)"):
            H.call("vx_native_argmax", big.data_ptr(), out.data_ptr(), C, 2, 2, 3, 3, 3, 5, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), H.stream_ptr())
    torch.cuda.synchronize()
    assert bool((out == 77).all())                                                       # a refused call writes nothing
    with pytest.raises(TypeError):
        P.labels_on_native_grid(big.double(), (3, 3, 5), (1.0,) * 3, (0.5,) * 3)
    for bad in (dict(native_shape=(3, 3)), dict(native_shape=(3, 0, 5)), dict(net_spacing=(1.0, 0.0, 1.0)), dict(native_spacing=(1.0, 1.0))):
        kw = dict(native_shape=(3, 3, 5), net_spacing=(1.0,) * 3, native_spacing=(0.5,) * 3)
        kw.update(bad)
        with pytest.raises(ValueError):
            P.labels_on_native_grid(big[:2], **kw)
    with pytest.raises(ValueError):
        P.labels_on_native_grid(big[0], (3, 3, 5), (1.0,) * 3, (0.5,) * 3)              # (d, h, w): no class axis


# ====================================================================================================================== infer_volume(native=)
def test_infer_volume_native():
    from recipe import CASES, fill_state_dict
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils import inference_runtime as IR
    from veloxseg_amd.utils.components import Postprocess
    cfg, _ = CASES["g2_32_m2"]
    model = VeloxSeg(**cfg)
    sd = model.state_dict()
    fill_state_dict(sd)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    x = torch.randn((1, 2, 24, 20, 22), generator=torch.Generator().manual_seed(5)).cuda()
    native = {"native_shape": (13, 17, 30), "native_spacing": (2.0, 1.2, 0.75), "net_spacing": (1.0, 1.0, 1.0)}
    with torch.inference_mode():
        logits0, labels0 = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5)
        logits, labels = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5, native=native)
        assert torch.equal(logits, logits0) and tuple(logits.shape[2:]) == (24, 20, 22)          # the logits stay on the network grid
        assert labels.dtype == torch.uint8 and tuple(labels.shape) == (1, 1, 13, 17, 30)
        want = P.labels_on_native_grid(logits[0], native["native_shape"], native["net_spacing"], native["native_spacing"])
        print(f"foreground on the native grid: {int((want > 0).sum())} of {want.numel()} voxels")
        assert torch.equal(labels[0, 0], want)
        pp = Postprocess(min_voxels=4, connectivity=6)
        for given in (pp, {"min_voxels": 4, "connectivity": 6}):
            _, cleaned = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5, postprocess=given, native=native)
            assert cleaned.shape == labels.shape and torch.equal(cleaned, pp(labels))
        l2, lab2 = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5, native=None)
        assert torch.equal(l2, logits0) and torch.equal(lab2, labels0) and tuple(lab2.shape) == (1, 1, 24, 20, 22)
        for bad in ({"native_shape": (13, 17, 30)}, dict(native, native_shape=(13, 17)), dict(native, net_spacing=(1.0, -1.0, 1.0)), dict(native, extra=1)):
            with pytest.raises(ValueError):
                IR.infer_volume(model, x, (32, 32, 32), 2, 0.5, native=bad)


# ====================================================================================================================== the closed loop in native voxels
def test_closed_loop_is_scored_on_the_native_grid():
    """preprocess -> predict -> labels on the native grid -> clean up -> score, with the volumes and the settings of
    tests/test_preprocess_gpu.py::test_run_test_with_the_preprocessing_data_module ((24, 20, 22) at (2, 2, 3) resampled to (1, 1, 1.5), channel-wise normalisation):
    the inputs are resampled, the label is not, and Dice is taken against the label on its own grid.  (run_test.py has no native path: it stays as it is.)"""
    from recipe import CASES, fill_state_dict
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils import inference_runtime as IR
    from veloxseg_amd.utils.metric.metrics import metrics_tensor
    cfg, _ = CASES["g2_32_m2"]
    model = VeloxSeg(**cfg)
    sd = model.state_dict()
    fill_state_dict(sd)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    native = {"native_shape": (24, 20, 22), "native_spacing": (2.0, 2.0, 3.0), "net_spacing": (1.0, 1.0, 1.5)}
    g = torch.Generator().manual_seed(12345)
    for _ in range(2):
        x = torch.randn((1, sum(cfg["in_ch"]), 24, 20, 22), generator=g).cuda()
        y = torch.randint(0, cfg["n_classes"], (1, 1, 24, 20, 22), generator=g).cuda()
        xr = P.resample_to_spacing(x[0], native["native_spacing"], native["net_spacing"], "bilinear")
        xr = P.NormalizeIntensityd(["image"], channel_wise=True)({"image": xr})["image"][None]
        assert tuple(xr.shape[2:]) == (47, 39, 43)
        logits, labels = IR.infer_volume(model, xr, (32, 32, 32), 2, 0.25, native=native, postprocess={"min_voxels": 2, "connectivity": 6})
        assert tuple(logits.shape[2:]) == (47, 39, 43) and labels.shape == y.shape and labels.dtype == torch.uint8
        fp, fn, _, _, _, iou, dice = metrics_tensor(y, labels)
        prediction, label = float((labels > 0).sum()), float((y > 0).sum())
        print(f"Dice {dice:.4f} IoU {iou:.4f} FP {fp:.4f} FN {fn:.4f} prediction {prediction:.0f} label {label:.0f}")
        assert 0 < label <= 24 * 20 * 22 and 0 <= prediction <= 24 * 20 * 22          # counts in NATIVE voxels: the resampled volume holds 47 * 39 * 43
        assert all(np.isfinite(v) for v in (fp, fn, iou, dice))
