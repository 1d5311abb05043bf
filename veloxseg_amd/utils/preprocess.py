"""Volume preprocessing on the GPU: the inference-side and dataset-side counterparts of utils/augment.py.

Reference: preprocess/normalization_MRI.py:7-12,52 and preprocess/normalization_CT_PET.py:6-11,67 (`zscore(data, data > data.min())`), :23-31 (`CTnorm`),
:65-81 (CT foreground intensity statistics over the dataset), utils/inference_extern_mri.py:73-75,95 (MONAI Spacingd(bilinear, bilinear, nearest) and
NormalizeIntensityd(channel_wise=True)).  The reductions, the radix-select histograms and the resampling are HIP kernels (csrc/preprocess.hip) on tensors
resident in HBM; statistics stay on the device between the kernels of one function.  There is no CPU fallback.

Two things a user has to know:

* The reference's `zscore(image, seg)` forms `mask = seg >= 0` from a BOOLEAN seg, which is true everywhere: as called, it normalises EVERY voxel with
  the whole-volume mean and std.  `zscore_volume` computes exactly that (it is what the reference's preprocessed datasets hold).  `zscore_foreground` is the
  statistic the call spells out -- mean / std over {x > x.min()}, written to those voxels only, the minimum voxels keeping their raw value.
* `resample_to_spacing` / `Spacingd` restate MONAI's `Spacing` for axis-aligned affines (output size round((n - 1) src / dst + 1), output index j samples
  input coordinate j src / dst, border clamp).  MONAI is not available here, so this is UNPINNED against MONAI itself, like oracle/augment_oracle.py.

* The way back: `inverse_tables` / `resample_to_shape` / `labels_on_native_grid` take a prediction from the network grid to the image's own grid with the SAME coordinate
  rule, the native extent given instead of computed; the label map comes from one kernel that interpolates the logits and keeps only their arg-max.

`IntensityStatistics` takes THREE rounds over the dataset (11 + 11 + 10 key bits; the mean rides on round 1, the std on round 2, min / max on round 1)."""
import math

import numpy as np
import torch

from .. import _hip as H
from .augment import label_code

_FLOOR = 1e-8
_ROUND_BITS = (11, 11, 10)


def _need_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")


def _channels(image, what):
    _need_cuda(image, what)
    if image.dim() not in (3, 4):
        raise ValueError(f"{what}: expected (D, H, W) or (C, D, H, W), got {tuple(image.shape)}")
    if image.dtype != torch.float32:
        raise TypeError(f"{what}: expected float32, got {image.dtype}")
    if image.numel() == 0:
        raise ValueError(f"{what}: empty volume")


def _workspace(device):
    return torch.empty(H.query("vx_moments_ws_doubles"), dtype=torch.float64, device=device)


# ====================================================================================================================== moments / z-score
def moments(x: torch.Tensor, foreground: bool = False) -> torch.Tensor:
    """-> device tensor (count, mean, population std) in fp64 over all voxels of x, or over {x > x.min()}; two passes, bit-reproducible, no host sync"""
    _need_cuda(x, "moments")
    if x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError("moments: expected a non-empty float32 tensor")
    x = x.contiguous()
    st = H.stream_ptr()
    stats = torch.empty(3, dtype=torch.float64, device=x.device)
    thr = None
    if foreground:
        thr = torch.full((1,), float("inf"), device=x.device)
        H.call("vx_min_value", x.data_ptr(), x.numel(), thr.data_ptr(), st)
    H.call("vx_moments_stats", x.data_ptr(), x.numel(), None if thr is None else thr.data_ptr(), _workspace(x.device).data_ptr(), stats.data_ptr(), st)
    return stats


def _zscore(image, out, foreground, policy, what, whole=False):
    _channels(image, what)
    src = image.contiguous()
    if out is None:
        out = torch.empty_like(src)
    elif out is image:
        if not image.is_contiguous():
            raise ValueError(f"{what}: in-place use needs a contiguous tensor")
    elif out.shape != src.shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"{what}: out must be a contiguous float32 CUDA tensor of the input's shape")
    st = H.stream_ptr()
    ws = _workspace(src.device)
    planes = [(src, out)] if (src.dim() == 3 or whole) else [(src[c], out[c]) for c in range(src.shape[0])]
    stats = torch.empty((len(planes), 3), dtype=torch.float64, device=src.device)          # one row per plane; the apply kernel reads it from the device
    thr = torch.full((len(planes),), float("inf"), device=src.device) if foreground else None
    for k, (xin, xout) in enumerate(planes):
        n = xin.numel()
        tp = None
        if foreground:
            tp = thr[k].data_ptr()
            H.call("vx_min_value", xin.data_ptr(), n, tp, st)
        H.call("vx_moments_stats", xin.data_ptr(), n, tp, ws.data_ptr(), stats[k].data_ptr(), st)
        H.call("vx_normalize_apply", xin.data_ptr(), xout.data_ptr(), n, tp, stats[k].data_ptr(), 0.0, 1.0, 0, 0.0, 0.0, policy, _FLOOR, st)
    return out


def zscore_foreground(image: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """each channel on its own: (x - mean) / max(std, 1e-8) with mean / std over {x > x.min()}, written to those voxels only (voxels at the minimum keep their raw
    value; a constant channel comes back unchanged).  min -> moments -> apply run stream-ordered without a host synchronisation; out may be image (in place)."""
    return _zscore(image, out, True, 0, "zscore_foreground")


def zscore_volume(image: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """each channel on its own: (x - mean) / max(std, 1e-8) over ALL voxels -- what the reference's `zscore(data, data > data.min())` computes, because its
    `mask = seg >= 0` is true everywhere for a boolean seg (preprocess/normalization_MRI.py:8)"""
    return _zscore(image, out, False, 0, "zscore_volume")


def ct_normalize(image: torch.Tensor, properties, out: torch.Tensor = None) -> torch.Tensor:
    """the reference's CTnorm: clip to [percentile_00_5, percentile_99_5], subtract mean, divide by max(std, 1e-8); the whole tensor at once"""
    _channels(image, "ct_normalize")
    mean, std = float(properties["mean"]), float(properties["std"])
    lo, hi = float(properties["percentile_00_5"]), float(properties["percentile_99_5"])
    if not lo <= hi:
        raise ValueError("ct_normalize: percentile_00_5 must not exceed percentile_99_5")
    src = image.contiguous()
    if out is None:
        out = torch.empty_like(src)
    elif out is image and not image.is_contiguous():
        raise ValueError("ct_normalize: in-place use needs a contiguous tensor")
    elif out.shape != src.shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError("ct_normalize: out must be a contiguous float32 CUDA tensor of the input's shape")
    H.call("vx_normalize_apply", src.data_ptr(), out.data_ptr(), src.numel(), None, None, mean, std, 1, lo, hi, 0, _FLOOR, H.stream_ptr())
    return out


class NormalizeIntensityd:
    """MONAI NormalizeIntensityd on dicts of (C, D, H, W) CUDA tensors: (x - mean) / std over all voxels (of each channel with channel_wise=True, else of the whole
    tensor); std == 0 divides by 1"""

    def __init__(self, keys, subtrahend=None, divisor=None, nonzero=False, channel_wise=False):
        if nonzero or subtrahend is not None or divisor is not None:
            raise NotImplementedError("NormalizeIntensityd: nonzero=True, subtrahend and divisor are not implemented on the HIP path (the reference uses none of them)")
        self.keys, self.channel_wise = list(keys), bool(channel_wise)

    def __call__(self, data):
        out = dict(data)
        for k in self.keys:
            x = data[k]
            _need_cuda(x, "NormalizeIntensityd")
            if x.dim() != 4:
                raise ValueError(f"NormalizeIntensityd: expected (C, D, H, W), got {tuple(x.shape)}")
            out[k] = _zscore(x, None, False, 1, "NormalizeIntensityd", whole=not self.channel_wise)
        return out


# ====================================================================================================================== exact dataset statistics
def float_key(x) -> np.ndarray:
    """host mirror of the kernel's key map: uint32 keys whose unsigned order is the order of the float32 values (-0 below +0)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_float(key) -> np.ndarray:
    """inverse of float_key"""
    k = np.asarray(key, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def linear_ranks(n: int, q: float):
    """numpy's linear percentile rule: -> (virtual index (n - 1) * (q / 100), the two ranks that bracket it)"""
    v = (n - 1) * (q / 100.0)
    lo = int(math.floor(v))
    return v, lo, min(lo + 1, n - 1)


def linear_lerp(a, b, v: float, lo: int) -> float:
    """numpy's _lerp between the order statistics a (rank lo) and b (rank lo + 1) at the virtual index v, in fp64"""
    a, b, t = np.float64(a), np.float64(b), np.float64(v - lo)
    diff = b - a
    return float(b - diff * (1 - t)) if t >= 0.5 else float(a + diff * t)


class IntensityStatistics:
    """The reference's CT foreground statistics (preprocess/normalization_CT_PET.py:65-81) without gathering the voxels: exact min / max / order statistics by radix
    select over the order-preserving 32-bit keys, mean / std in two fp64 passes over the union of the selected voxels (mask > 0).

        s = IntensityStatistics()
        while not s.done:
            for ct, mask in volumes: s.update(ct, mask)
            s.end_round()
        props = s.result()

    THREE rounds, each over the same volumes: round 1 histograms key bits 31..21 and sums x (mean), finds min / max and counts NaNs; round 2 refines every wanted rank
    inside its 11-bit prefix (bits 20..10) and sums (x - mean)^2; round 3 resolves the last 10 bits.  Interpolation between the two order statistics that bracket a
    percentile happens on the host in fp64 with numpy's linear rule."""

    rounds = len(_ROUND_BITS)

    def __init__(self, percentiles=(0.5, 50.0, 99.5)):
        self.percentiles = tuple(float(q) for q in percentiles)
        if any(not 0.0 <= q <= 100.0 for q in self.percentiles):
            raise ValueError("percentiles must lie in [0, 100]")
        self.round, self.done = 0, False
        self.n = None
        self._prefix = {0: [0]}             # round -> sorted distinct key prefixes to refine
        self._dev = None
        self._values = None

    # ---- device buffers of the current round
    def _begin(self, device):
        bits = _ROUND_BITS[self.round]
        self._dev = {"hist": torch.zeros((len(self._prefix[self.round]), 1 << bits), dtype=torch.int64, device=device),
                     "acc": torch.zeros(3, dtype=torch.float64, device=device), "ws": _workspace(device),
                     "nan": torch.zeros(1, dtype=torch.int64, device=device),
                     "minmax": torch.tensor([-1, 0], dtype=torch.int32, device=device),          # bit patterns 0xffffffff, 0
                     "center": None if self.round != 1 else torch.tensor([self.mean], dtype=torch.float64, device=device)}

    def update(self, ct: torch.Tensor, mask: torch.Tensor):
        if self.done:
            raise RuntimeError("IntensityStatistics: all rounds are finished")
        _need_cuda(ct, "IntensityStatistics.update")
        _need_cuda(mask, "IntensityStatistics.update")
        if ct.dtype != torch.float32:
            raise TypeError(f"IntensityStatistics.update: expected a float32 volume, got {ct.dtype}")
        if ct.shape != mask.shape:
            raise ValueError(f"IntensityStatistics.update: volume {tuple(ct.shape)} and mask {tuple(mask.shape)} differ in shape")
        if ct.numel() == 0:
            return
        ct, mask = ct.contiguous(), mask.contiguous()
        code = label_code(mask)
        if self._dev is None:
            self._begin(ct.device)
        d, st, n = self._dev, H.stream_ptr(), ct.numel()
        done_bits = sum(_ROUND_BITS[:self.round])
        for row, prefix in enumerate(self._prefix[self.round]):
            first = self.round == 0
            H.call("vx_key_histogram", ct.data_ptr(), mask.data_ptr(), code, n, int(prefix), done_bits, _ROUND_BITS[self.round], d["hist"][row].data_ptr(),
                   d["minmax"].data_ptr() if first else None, d["nan"].data_ptr() if first else None, st)
        if self.round < 2:
            H.call("vx_moments_partials", ct.data_ptr(), n, None, mask.data_ptr(), code, None if d["center"] is None else d["center"].data_ptr(), d["ws"].data_ptr(), st)
            H.call("vx_moments_reduce", d["ws"].data_ptr(), d["acc"].data_ptr(), 1, None, -1, st)

    def end_round(self):
        if self.done:
            raise RuntimeError("IntensityStatistics: all rounds are finished")
        if self._dev is None:
            if self.round == 0:
                raise ValueError("IntensityStatistics: no selected voxels (the round saw no volume)")
            raise ValueError(f"IntensityStatistics: round {self.round + 1} saw no volume: every round must see the same volumes")
        d = self._dev
        hist = d["hist"].cpu().numpy()
        acc = d["acc"].cpu().numpy()
        if self.round == 0:
            n = int(hist.sum())
            if int(d["nan"].item()):
                raise ValueError(f"IntensityStatistics: {int(d['nan'].item())} NaN among the selected voxels")
            if n == 0:
                raise ValueError("IntensityStatistics: no selected voxels")
            assert int(acc[0]) == n
            self.n, self.mean = n, float(acc[1]) / n
            mm = d["minmax"].cpu().numpy().view(np.uint32)
            self.min, self.max = (float(v) for v in key_float(mm))
            # numpy's linear rule: virtual index (n - 1) * (q / 100), the order statistics at its floor and floor + 1
            self._virtual = {q: linear_ranks(n, q)[0] for q in self.percentiles}
            ranks = set()
            for q in self.percentiles:
                ranks.update(linear_ranks(n, q)[1:])
            self._rank = {r: (0, r) for r in sorted(ranks)}          # rank -> (key prefix so far, rank inside that prefix)
            counts = {0: n}
        else:
            counts = self._expected
            if self.round == 1:
                if int(acc[0]) != self.n:
                    raise ValueError(f"IntensityStatistics: round 2 selected {int(acc[0])} voxels, round 1 selected {self.n}: every round must see the same volumes")
                self.std = math.sqrt(float(acc[2]) / self.n)
        bits = _ROUND_BITS[self.round]
        row_of = {p: i for i, p in enumerate(self._prefix[self.round])}
        for p, i in row_of.items():
            if int(hist[i].sum()) != counts[p]:
                raise ValueError(f"IntensityStatistics: round {self.round + 1} counted {int(hist[i].sum())} voxels where the round before counted {counts[p]}: "
                                 "every round must see the same volumes")
        expected = {}
        for r, (p, k) in self._rank.items():
            h = hist[row_of[p]]
            cum = np.cumsum(h)
            b = int(np.searchsorted(cum, k, side="right"))
            np_ = (p << bits) | b
            self._rank[r] = (np_, k - (int(cum[b - 1]) if b else 0))
            expected[np_] = int(h[b])
        self._expected = expected
        self.round += 1
        self._dev = None
        if self.round == self.rounds:
            self.done = True
            self._values = {r: float(key_float(np.uint32(p))) for r, (p, _) in self._rank.items()}
        else:
            self._prefix[self.round] = sorted(expected)

    def order_statistic(self, rank: int) -> float:
        """exact value of the rank-th smallest selected voxel (only the ranks that bracket a requested percentile are resolved)"""
        if not self.done:
            raise RuntimeError("IntensityStatistics: rounds remain (loop `while not s.done`)")
        return self._values[rank]

    def percentile(self, q: float) -> float:
        if float(q) not in self._virtual:
            raise KeyError(float(q))
        v, lo, hi = linear_ranks(self.n, float(q))
        return linear_lerp(self.order_statistic(lo), self.order_statistic(hi), v, lo)

    def result(self):
        if not self.done:
            raise RuntimeError("IntensityStatistics: rounds remain (loop `while not s.done`)")
        for q in (0.5, 50.0, 99.5):
            if q not in self._virtual:
                raise ValueError(f"IntensityStatistics.result: the reference's dict needs percentile {q}")
        return {"mean": self.mean, "median": self.percentile(50.0), "std": self.std, "min": self.min, "max": self.max,
                "percentile_99_5": self.percentile(99.5), "percentile_00_5": self.percentile(0.5)}


# ====================================================================================================================== resampling
def _spacing3(v, what):
    v = [float(s) for s in (v.tolist() if hasattr(v, "tolist") else v)]
    if len(v) != 3 or any(not (s > 0.0 and math.isfinite(s)) for s in v):
        raise ValueError(f"{what}: three positive finite spacings expected, got {v}")
    return v


def output_shape(shape, src_spacing, dst_spacing):
    """per axis int(np.round((n - 1) * src / dst + 1)) (round half to even)"""
    src, dst = _spacing3(src_spacing, "src_spacing"), _spacing3(dst_spacing, "dst_spacing")
    return tuple(max(int(np.round((int(n) - 1) * s / d + 1)), 1) for n, s, d in zip(shape, src, dst))


def axis_table(n, n_out, src, dst, mode="bilinear"):
    """-> (i0 int32, i1 int32, w float32) of n_out entries: output index j samples the input coordinate c = clamp(j * src / dst, 0, n - 1), formed in fp64.
    bilinear: i0 = floor(c), i1 = min(i0 + 1, n - 1), w = fp32(c - i0); nearest: i0 = i1 = rint(c) (ties to even), w = 0."""
    if not (src > 0 and dst > 0):
        raise ValueError("spacings must be positive")
    c = np.clip(np.arange(int(n_out), dtype=np.float64) * float(src) / float(dst), 0.0, float(n - 1))
    if mode == "nearest":
        i0 = np.rint(c).astype(np.int32)
        return i0, i0.copy(), np.zeros(int(n_out), dtype=np.float32)
    if mode != "bilinear":
        raise ValueError(f"mode {mode!r} not supported (bilinear, nearest)")
    i0 = np.floor(c).astype(np.int32)
    return i0, np.minimum(i0 + 1, n - 1).astype(np.int32), (c - i0).astype(np.float32)


def _shape3(v, what):
    v = list(v.tolist() if hasattr(v, "tolist") else v)
    if len(v) != 3 or any(isinstance(n, bool) or int(n) != n or int(n) < 1 for n in v):
        raise ValueError(f"{what}: three positive integer extents expected, got {v}")
    return tuple(int(n) for n in v)


def inverse_tables(net_shape, native_shape, net_spacing, native_spacing, mode="bilinear"):
    """the tables that take a volume on the network grid back to the image's own grid: per axis axis_table(n_net, n_native, src=net_spacing, dst=native_spacing,
    mode).  The output extent is GIVEN (the native shape), not recomputed: where round() in output_shape did not invert, the native coordinates past the last network
    voxel are clamped to n_net - 1 by axis_table (i0 = i1 = n_net - 1, w = 0)."""
    net, nat = _shape3(net_shape, "net_shape"), _shape3(native_shape, "native_shape")
    src, dst = _spacing3(net_spacing, "net_spacing"), _spacing3(native_spacing, "native_spacing")
    return [axis_table(n, no, s, d, mode) for n, no, s, d in zip(net, nat, src, dst)]


def check_native_geometry(native):
    """the geometry of a volume that was resampled to the network's spacing, as infer_volume(native=) takes it: a dict with exactly the keys native_shape (three
    positive integers), native_spacing and net_spacing (three positive finite numbers each) -> the same dict with tuples of int / float; anything else: ValueError"""
    if not isinstance(native, dict) or set(native) != {"native_shape", "native_spacing", "net_spacing"}:
        raise ValueError("native: a dict with exactly the keys native_shape, native_spacing, net_spacing expected")
    return {"native_shape": _shape3(native["native_shape"], "native_shape"), "native_spacing": tuple(_spacing3(native["native_spacing"], "native_spacing")),
            "net_spacing": tuple(_spacing3(native["net_spacing"], "net_spacing"))}


def _device_tables(tabs, device, k):
    return torch.from_numpy(np.concatenate([t[k] for t in tabs])).to(device)


def resample_to_spacing(x: torch.Tensor, src_spacing, dst_spacing, mode: str = "bilinear") -> torch.Tensor:
    """(D, H, W) or (C, D, H, W) resampled from src_spacing to dst_spacing (one value per spatial axis, in the tensor's axis order).  "bilinear": float32, three
    nested lerps; "nearest": float32 or a label dtype (uint8, int32, int64), copied bit for bit."""
    return _resample(x, None, src_spacing, dst_spacing, mode, "resample_to_spacing")


def resample_to_shape(x: torch.Tensor, out_shape, src_spacing, dst_spacing, mode: str = "bilinear") -> torch.Tensor:
    """resample_to_spacing with the output extent GIVEN (three integers) instead of computed from the spacings: the way back from the network grid to an image's own
    grid (inverse_tables), for logits or any float map, and for labels with "nearest".  Output coordinates past the last input voxel are clamped to it."""
    return _resample(x, out_shape, src_spacing, dst_spacing, mode, "resample_to_shape")


def _resample(x, out_shape, src_spacing, dst_spacing, mode, what):
    _need_cuda(x, what)
    if mode not in ("bilinear", "nearest"):
        raise ValueError(f"mode {mode!r} not supported (bilinear, nearest)")
    if x.dim() not in (3, 4) or x.numel() == 0:
        raise ValueError(f"{what}: expected a non-empty (D, H, W) or (C, D, H, W), got {tuple(x.shape)}")
    src, dst = _spacing3(src_spacing, "src_spacing"), _spacing3(dst_spacing, "dst_spacing")
    if mode == "bilinear" and x.dtype != torch.float32:
        raise TypeError(f"{what}: bilinear needs float32, got {x.dtype}")
    code = label_code(x)
    xin = x.contiguous()
    C = 1 if x.dim() == 3 else x.shape[0]
    sp = tuple(x.shape[-3:])
    so = output_shape(sp, src, dst) if out_shape is None else _shape3(out_shape, "out_shape")
    tabs = [axis_table(n, no, s, d, mode) for n, no, s, d in zip(sp, so, src, dst)]
    i0 = torch.from_numpy(np.concatenate([t[0] for t in tabs])).to(x.device)
    out = torch.empty(tuple(x.shape[:-3]) + so, dtype=x.dtype, device=x.device)
    st = H.stream_ptr()
    if x.dtype == torch.float32:
        i1 = torch.from_numpy(np.concatenate([t[1] for t in tabs])).to(x.device)
        w = torch.from_numpy(np.concatenate([t[2] for t in tabs])).to(x.device)
        H.call("vx_resample_axes", xin.data_ptr(), out.data_ptr(), C, *sp, *so, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), 0 if mode == "bilinear" else 1, st)
    else:
        H.call("vx_resample_axes_label", xin.data_ptr(), out.data_ptr(), code, C, *sp, *so, i0.data_ptr(), st)
    return out


def labels_on_native_grid(logits: torch.Tensor, native_shape, net_spacing, native_spacing) -> torch.Tensor:
    """the inverse of Spacingd for a prediction: (K, d, h, w) or (1, K, d, h, w) float32 logits on the network grid (spacing net_spacing) -> uint8 label map
    (D, H, W) = native_shape on the image's own grid (spacing native_spacing), in ONE kernel (vx_native_argmax): per native voxel the K trilinear values are formed
    in registers and only their arg-max is stored.  Byte for byte vx_argmax_channels(resample_to_shape(logits, native_shape, net_spacing, native_spacing)) -- first
    NaN, else first maximum -- without the (K, D, H, W) float volume.  The LOGITS are interpolated, not soft-max probabilities (MONAI's Invertd followed by
    AsDiscrete(argmax=True)).  K <= 256."""
    _need_cuda(logits, "labels_on_native_grid")
    if logits.dtype != torch.float32:
        raise TypeError(f"labels_on_native_grid: expected float32 logits, got {logits.dtype}")
    if logits.dim() == 5 and logits.shape[0] == 1:
        logits = logits[0]
    if logits.dim() != 4 or logits.numel() == 0:
        raise ValueError(f"labels_on_native_grid: expected non-empty (K, d, h, w) or (1, K, d, h, w) logits, got {tuple(logits.shape)}")
    K, sp = int(logits.shape[0]), tuple(logits.shape[1:])
    if K > 256:
        raise ValueError(f"labels_on_native_grid: {K} classes do not fit a uint8 label map (at most 256)")
    so = check_native_geometry({"native_shape": native_shape, "net_spacing": net_spacing, "native_spacing": native_spacing})["native_shape"]
    tabs = inverse_tables(sp, so, net_spacing, native_spacing)
    xin = logits.contiguous()
    i0, i1, w = (_device_tables(tabs, xin.device, k) for k in range(3))
    out = torch.empty(so, dtype=torch.uint8, device=xin.device)
    H.call("vx_native_argmax", xin.data_ptr(), out.data_ptr(), K, *sp, *so, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), H.stream_ptr())
    return out


class Spacingd:
    """MONAI Spacingd on dicts of (C, D, H, W) CUDA tensors with axis-aligned geometry: the source spacing of key k is data[k + "_pixdim"], else data["pixdim"];
    the new spacing is written back under the key it was read from"""

    def __init__(self, keys, pixdim, mode="bilinear"):
        self.keys, self.pixdim = list(keys), _spacing3(pixdim, "pixdim")
        self.mode = [mode] * len(self.keys) if isinstance(mode, str) else list(mode)
        if len(self.mode) != len(self.keys):
            raise ValueError("mode must have one entry per key")
        for m in self.mode:
            if m not in ("bilinear", "nearest"):
                raise ValueError(f"mode {m!r} not supported (bilinear, nearest)")

    def __call__(self, data):
        out = dict(data)
        for k, m in zip(self.keys, self.mode):
            name = k + "_pixdim" if k + "_pixdim" in data else "pixdim"
            if name not in data:
                raise KeyError(f"Spacingd: neither {k + '_pixdim'!r} nor 'pixdim' gives the source spacing of {k!r}")
            x = data[k]
            _need_cuda(x, "Spacingd")
            if x.dim() != 4:
                raise ValueError(f"Spacingd: expected (C, D, H, W), got {tuple(x.shape)}")
            out[k] = resample_to_spacing(x, data[name], self.pixdim, m)
            out[name] = tuple(self.pixdim)
        return out


# ====================================================================================================================== run_test.py data module
def iter_volumes(args, train_config, test_config):
    """`run_test.py --data_module veloxseg_amd.utils.preprocess`: the GPU preprocessing in front of sliding_window_predict, run_test.py itself unchanged.
    Settings come from test_config["preprocess"]:
      "data_module":   module whose iter_volumes(args, train_config, test_config) yields (name, inputs (1, C, D, H, W), label (1, 1, D, H, W)) or a 4-tuple whose
                       last item is the source spacing; absent: the synthetic volumes of run_test.py (--synthetic, --volume_shape)
      "normalize":     "none" (default) | "zscore_foreground" | "channel" (NormalizeIntensity, channel_wise), per input channel
      "resample_from": source spacing [SX, SY, SZ] of volumes that bring none; inputs are resampled bilinear, labels nearest, to
                       train_config["spacing"][dataset] when present, else to "resample_to"
    Yields (name, inputs, label) on the GPU."""
    import importlib
    import json
    cfg = dict(test_config.get("preprocess") or {})
    unknown = set(cfg) - {"data_module", "normalize", "resample_from", "resample_to"}
    if unknown:
        raise ValueError(f"test_config['preprocess']: unknown keys {sorted(unknown)}")
    normalize = cfg.get("normalize", "none")
    if normalize not in ("none", "zscore_foreground", "channel"):
        raise ValueError(f"test_config['preprocess']['normalize']: {normalize!r} is none of none, zscore_foreground, channel")
    spacing_cfg = train_config.get("spacing")
    target = spacing_cfg.get(args.dataset_name) if isinstance(spacing_cfg, dict) else None
    target = target if target is not None else cfg.get("resample_to")
    if cfg.get("data_module"):
        source_volumes = importlib.import_module(cfg["data_module"]).iter_volumes(args, train_config, test_config)
    else:
        with open(args.model_config, "r", encoding="utf-8") as f:
            mcfg = json.load(f)[args.model_name]

        def synthetic():
            g = torch.Generator().manual_seed(12345)
            for i in range(args.synthetic):
                yield (f"synthetic_{i}", torch.randn((1, sum(mcfg["in_ch"]), *args.volume_shape), generator=g),
                       torch.randint(0, mcfg["n_classes"], (1, 1, *args.volume_shape), generator=g))
        source_volumes = synthetic()
    for item in source_volumes:
        name, x, y = item[:3]
        source = item[3] if len(item) > 3 else cfg.get("resample_from")
        x, y = x.cuda().float(), y.cuda()
        if source is not None:
            if target is None:
                raise ValueError("resampling needs a target spacing: train_config['spacing'][dataset] or test_config['preprocess']['resample_to']")
            x = resample_to_spacing(x[0], source, target, "bilinear")[None]
            y = resample_to_spacing(y[0], source, target, "nearest")[None]
        if normalize == "zscore_foreground":
            x = zscore_foreground(x[0])[None]
        elif normalize == "channel":
            x = NormalizeIntensityd(["image"], channel_wise=True)({"image": x[0]})["image"][None]
        yield name, x, y
