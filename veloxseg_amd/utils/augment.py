"""GPU stand-in for the three MONAI dictionary transforms of the reference's training pipeline (utils/train_autopet.py:132-152, utils/train_brats.py):
CropForegroundd(select_fn = x > x.min()), RandCropByPosNegLabeld and RandRotated(range_z) -- same class names, keys and argument meaning, operating on
(C, D, H, W) tensors that are already resident in HBM.  The reductions, the label rank-select and the resampling are HIP kernels (csrc/augment.hip);
random draws are taken on the host from numpy's RandomState in MONAI's order.  There is no CPU fallback.
Beyond the reference's three: RandFlipd, RandScaleIntensityd, RandShiftIntensityd, RandGaussianNoised and BatchAssembler, which applies them while ONE kernel call
(csrc/augment_batch.hip) writes the (B, M, D, H, W) batch and its int64 labels; from_config reads train_config["augment"]."""
import math

import numpy as np
import torch

from .. import _hip as H

_CHUNK = 1 << 16
_INT_MAX = 0x7FFFFFFF


def rotation_range_from_degrees(degrees):
    """reference: utils/runtime.py:115"""
    return math.radians(float(degrees))


def image_label_modes(image_key_count):
    """reference: utils/runtime.py:119"""
    if image_key_count <= 0:
        raise ValueError("image_key_count must be greater than 0")
    return tuple(["bilinear"] * image_key_count + ["nearest"])


def _need_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    if t.dim() != 4:
        raise ValueError(f"{what}: expected (C, D, H, W), got {tuple(t.shape)}")


def label_code(lab):
    """bytes code of a label / mask tensor for the C entries: uint8 1, int32 4, int64 8, float32 -4"""
    code = {torch.uint8: 1, torch.int32: 4, torch.int64: 8, torch.float32: -4}.get(lab.dtype)
    if code is None:
        raise TypeError(f"label dtype {lab.dtype} not supported (uint8, int32, int64, float32)")
    return code


def foreground_box(source: torch.Tensor):
    """bounding box (start[3], end[3]) of {source > source.min()} over all channels; zeros when empty"""
    _need_cuda(source, "foreground_box")
    x = source.contiguous().float()
    C, D, Hh, W = x.shape
    st = H.stream_ptr()
    mn = torch.full((1,), float("inf"), device=x.device)
    H.call("vx_min_value", x.data_ptr(), x.numel(), mn.data_ptr(), st)
    box = torch.tensor([_INT_MAX] * 3 + [-1] * 3, dtype=torch.int32, device=x.device)
    H.call("vx_bbox_gt", x.data_ptr(), float(mn.item()), C, D, Hh, W, box.data_ptr(), st)
    b = box.tolist()
    if b[3] < 0:
        return [0, 0, 0], [0, 0, 0]
    return b[:3], [v + 1 for v in b[3:]]


class _LabelIndex:
    """rank-select over the flat label volume: number of foreground / background voxels and the flat index of the k-th one"""

    def __init__(self, label: torch.Tensor):
        _need_cuda(label, "label")
        if label.shape[0] != 1:
            raise ValueError("label must have one channel")
        self.lab = label.contiguous()
        self.code = label_code(self.lab)
        self.n = self.lab.numel()
        nb = (self.n + _CHUNK - 1) // _CHUNK
        cnt = torch.empty(nb, dtype=torch.int32, device=label.device)
        H.call("vx_label_chunk_count", self.lab.data_ptr(), self.code, self.n, _CHUNK, 1, cnt.data_ptr(), H.stream_ptr())
        fg = cnt.cpu().numpy().astype(np.int64)
        sizes = np.minimum(_CHUNK, self.n - np.arange(nb, dtype=np.int64) * _CHUNK)
        self.cum = {1: np.cumsum(fg), 0: np.cumsum(sizes - fg)}
        self.out = torch.empty(1, dtype=torch.int64, device=label.device)

    def count(self, fg: int) -> int:
        return int(self.cum[fg][-1])

    def kth(self, fg: int, k: int) -> int:
        cum = self.cum[fg]
        ch = int(np.searchsorted(cum, k, side="right"))
        before = int(cum[ch - 1]) if ch else 0
        H.call("vx_label_kth_in_chunk", self.lab.data_ptr(), self.code, self.n, ch * _CHUNK, _CHUNK, fg, k - before, self.out.data_ptr(), H.stream_ptr())
        return int(self.out.item())


def _correct_center(center, spatial_size, shape, allow_smaller):
    spatial_size = list(spatial_size)
    if any(s - p < 0 for s, p in zip(shape, spatial_size)):
        if not allow_smaller:
            raise ValueError("The size of the proposed random crop ROI is larger than the image size")
        spatial_size = [min(s, p) for s, p in zip(shape, spatial_size)]
    out = []
    for c, p, s in zip(center, spatial_size, shape):
        lo = p // 2
        hi = int(s + 1 - p / 2.0)
        if hi == lo:
            hi += 1
        out.append(int(min(max(c, lo), hi - 1)))
    return out


class _Randomizable:
    def set_random_state(self, seed=None, state=None):
        self.R = state if state is not None else np.random.RandomState(seed)
        return self


class CropForegroundd:
    def __init__(self, keys, source_key, select_fn=None):
        self.keys, self.source_key = list(keys), source_key
        if select_fn is not None:      # only the reference's selector (x > x.min()) runs on the GPU: check that this is what was passed
            for probe in (torch.tensor([[-3.0, -3.0, 5.0, -1.0]]), torch.tensor([[10.0, 11.0, 10.5, 10.0]])):
                if torch.equal(torch.as_tensor(select_fn(probe)), probe > probe.min()):
                    continue
                raise NotImplementedError("CropForegroundd: only select_fn = (x > x.min()) is implemented on the HIP path")

    def __call__(self, data):
        start, end = foreground_box(data[self.source_key])
        out = dict(data)
        for k in self.keys:
            out[k] = data[k][:, start[0]:end[0], start[1]:end[1], start[2]:end[2]]
        out["foreground_start_coord"], out["foreground_end_coord"] = start, end
        return out


class RandCropByPosNegLabeld(_Randomizable):
    def __init__(self, keys, label_key, spatial_size, pos=1.0, neg=1.0, num_samples=1, allow_smaller=False):
        if pos < 0 or neg < 0 or pos + neg == 0:
            raise ValueError("pos and neg must be nonnegative and not both zero")
        self.keys, self.label_key, self.spatial_size = list(keys), label_key, list(spatial_size)
        self.pos_ratio, self.num_samples, self.allow_smaller = pos / (pos + neg), int(num_samples), allow_smaller
        self.set_random_state()

    def centers(self, label):
        index = _LabelIndex(label)
        shape = tuple(label.shape[1:])
        nfg, nbg = index.count(1), index.count(0)
        ratio = self.pos_ratio
        if nfg == 0 and nbg == 0:
            raise ValueError("No sampling location available.")
        if nfg == 0 or nbg == 0:
            ratio = 0 if nfg == 0 else 1
        out = []
        for _ in range(self.num_samples):
            fg = 1 if self.R.rand() < ratio else 0
            flat = index.kth(fg, int(self.R.randint(nfg if fg else nbg)))
            out.append(_correct_center(list(np.unravel_index(flat, shape)), self.spatial_size, shape, self.allow_smaller))
        return out

    def __call__(self, data):
        shape = tuple(data[self.label_key].shape[1:])
        res = []
        for c in self.centers(data[self.label_key]):
            sl = tuple(slice(max(ci - p // 2, 0), min(max(ci - p // 2, 0) + p, s)) for ci, p, s in zip(c, self.spatial_size, shape))
            d = dict(data)
            for k in self.keys:
                d[k] = data[k][(slice(None),) + sl].contiguous()
            d["crop_center"] = c
            res.append(d)
        return res


def rotate_z(x: torch.Tensor, angle: float, mode: str = "bilinear") -> torch.Tensor:
    _need_cuda(x, "rotate_z")
    if mode not in ("bilinear", "nearest"):
        raise ValueError(f"mode {mode!r} not supported")
    xin = x.contiguous().float()
    out = torch.empty_like(xin)
    C, D, Hh, W = xin.shape
    H.call("vx_rotate_z", xin.data_ptr(), out.data_ptr(), C, D, Hh, W, math.cos(angle), math.sin(angle), 0 if mode == "bilinear" else 1, H.stream_ptr())
    return out.to(x.dtype) if x.dtype != torch.float32 else out


class RandRotated(_Randomizable):
    def __init__(self, keys, range_x=0.0, range_y=0.0, range_z=0.0, prob=0.1, mode="bilinear", padding_mode="border"):
        if range_x or range_y:
            raise NotImplementedError("RandRotated: only rotation about z (range_z) is implemented on the HIP path (the reference uses no other)")
        if padding_mode != "border":
            raise NotImplementedError("RandRotated: only padding_mode='border' (MONAI's default) is implemented")
        self.keys, self.range_z, self.prob = list(keys), float(range_z), float(prob)
        self.mode = [mode] * len(self.keys) if isinstance(mode, str) else list(mode)
        if len(self.mode) != len(self.keys):
            raise ValueError("mode must have one entry per key")
        self.set_random_state()

    def draw(self):
        do = self.R.rand() < self.prob
        self.R.uniform(low=-0.0, high=0.0)
        self.R.uniform(low=-0.0, high=0.0)
        return do, float(self.R.uniform(low=-self.range_z, high=self.range_z))

    def __call__(self, data):
        if isinstance(data, list):
            return [self(d) for d in data]
        do, angle = self.draw()
        out = dict(data)
        if do:
            for k, m in zip(self.keys, self.mode):
                out[k] = rotate_z(data[k], angle, m)
        return out


# ---- batch assembly: mirror, intensity steps and noise in one table-driven pass (csrc/augment_batch.hip) ----------------------------------
# MONAI is not installed here: the draw orders below model MONAI 1.x (RandomizableTransform.randomize draws R.rand() < prob first, the parameters only when that
# fires) and are UNPINNED against MONAI itself, like oracle/augment_oracle.py; tests/intensity_ref.py restates them.
AUG_RECORD_BYTES, AUG_MAX_STEPS, AUG_LABEL = 192, 8, -1
AUG_NOISE_STREAM = 0x564158475541          # VX_AUG_NOISE_STREAM of include/veloxseg_hip.h: dropout site ids count up from 1 and never get there
_OP_MUL, _OP_ADD, _OP_NOISE = 1, 2, 3
_REC = np.dtype([("src", "<u8"), ("stride", "<i8", (3,)), ("dtype", "<i4"), ("b", "<i4"), ("c", "<i4"), ("flip", "<i4"), ("n_steps", "<i4"), ("pad", "<i4", (3,)),
                 ("step", [("op", "<u4"), ("a", "<f4"), ("b", "<f4"), ("key", "<u4")], (AUG_MAX_STEPS,))])
assert _REC.itemsize == AUG_RECORD_BYTES


def _flip_mask(spatial_axis):
    """None -> all three axes; an int or a sequence of ints -> those (0 = D, 1 = H, 2 = W; negative axes count from the end); bit a = axis a"""
    if spatial_axis is None:
        return 7
    axes = list(spatial_axis) if isinstance(spatial_axis, (list, tuple)) else [spatial_axis]
    mask = 0
    for a in axes:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not -3 <= a < 3:
            raise ValueError(f"spatial_axis {spatial_axis!r}: every axis must be an int in -3..2 (0 = D, 1 = H, 2 = W)")
        mask |= 1 << (int(a) % 3)
    return mask


def _range(v, what):
    """MONAI's reading of `factors` / `offsets`: a number r means (-|r|, |r|), a pair means (min, max)"""
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
        lo, hi = min(-float(v), float(v)), max(-float(v), float(v))
    else:
        try:
            pair = [float(t) for t in v]
        except (TypeError, ValueError):
            raise ValueError(f"{what} {v!r}: a number or a pair of numbers") from None
        if len(pair) != 2:
            raise ValueError(f"{what} should be a number or pair of numbers, got {v!r}")
        lo, hi = min(pair), max(pair)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{what} {v!r} is not finite")
    return lo, hi


def _prob(p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"prob {p} outside [0, 1]")
    return p


class _Program:
    """what the transforms drawn so far do to one key of one sample: a flip mask and the pointwise steps [op, a, b, key, mask of the flips that follow, noise channel]"""

    def __init__(self):
        self.flip, self.steps = 0, []

    def add_flip(self, mask):
        self.flip ^= mask
        for s in self.steps:
            s[4] ^= mask

    def add_step(self, op, a=0.0, b=0.0, key=0, chan=0):
        if len(self.steps) == AUG_MAX_STEPS:
            raise ValueError(f"more than {AUG_MAX_STEPS} pointwise steps fired on one key: the record holds no more")
        self.steps.append([op, a, b, key, 0, chan])


def _check_source(t, what, image):
    """raises before any GPU work: RuntimeError (not on the device), TypeError (dtype), ValueError (shape) -> the element code of the record"""
    _need_cuda(t, what)
    if image:
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: image dtype {t.dtype} not supported (float32)")
        return 0
    return label_code(t)


def _pack(entries):
    """entries: [(tensor (D, H, W) view, element code, b, c, _Program)] -> the record table as a host uint8 tensor"""
    tab = np.zeros(len(entries), dtype=_REC)
    for r, (t, code, b, c, prog) in zip(tab, entries):
        r["src"], r["stride"], r["dtype"], r["b"], r["c"], r["flip"], r["n_steps"] = t.data_ptr(), t.stride(), code, b, c, prog.flip, len(prog.steps)
        for k, (op, a, sb, key, post, chan) in enumerate(prog.steps):
            r["step"][k] = (op | (post << 4) | (chan << 8), a, sb, key)
    return torch.from_numpy(tab.view(np.uint8).reshape(-1))


def _launch(entries, x_out, y_out, B, M, spatial):
    """entries as in _pack, images first -> ONE table, ONE upload, ONE call of vx_augment_batch"""
    n_image = sum(1 for e in entries if e[3] != AUG_LABEL)
    dev = (x_out if x_out is not None else y_out).device
    table = _pack(entries).to(dev)
    H.call("vx_augment_batch", table.data_ptr(), n_image, len(entries) - n_image, None if x_out is None else x_out.data_ptr(), None if y_out is None else y_out.data_ptr(),
           8, B, M, *spatial, H.stream_ptr())


class _BatchTransform(_Randomizable):
    """common part of the four dictionary transforms below.  Draw order (modelled on MONAI 1.x, unpinned against MONAI itself, which is not installed): one RandomState
    per transform; every call draws R.rand() < prob FIRST and its parameters ONLY IF that fires; the one draw set of a call is shared by all keys of that call."""
    intensity = True

    def draw(self):
        """-> None (the call does not fire) or the parameters of this call"""
        raise NotImplementedError

    def fold(self, params, key_index, chan0, prog):
        """add what this call does to channel `chan0 + (channel within the key)` of key number `key_index` to `prog`"""
        raise NotImplementedError

    def __call__(self, data):
        if isinstance(data, list):
            return [self(d) for d in data]
        params = self.draw()
        out = dict(data)
        if params is None:
            return out
        images, labels, chan0 = [], [], 0
        for ki, k in enumerate(self.keys):
            t = data[k]
            code = _check_source(t, f"{type(self).__name__}[{k!r}]", self.intensity or t.dtype == torch.float32)
            (images if code == 0 else labels).append((k, ki, chan0, t, code))
            chan0 += t.shape[0]
        spatial = {tuple(t.shape[1:]) for _, _, _, t, _ in images + labels}
        if len(spatial) != 1:
            raise ValueError(f"{type(self).__name__}: keys of different spatial shapes {sorted(spatial)} in one call")
        spatial = spatial.pop()
        if 0 in spatial:
            raise ValueError(f"{type(self).__name__}: empty spatial shape {spatial}")
        entries = []
        M = max([t.shape[0] for _, _, _, t, _ in images] or [1])           # every float32 key is one "sample" of the image output: the channels of a key stay together
        if M > 64:
            raise ValueError(f"{type(self).__name__}: {M} channels in one key (at most 64)")
        x_out = torch.empty((len(images), M) + spatial, dtype=torch.float32, device=images[0][3].device) if images else None
        nlab = sum(t.shape[0] for _, _, _, t, _ in labels)
        y_out = torch.empty((nlab, 1) + spatial, dtype=torch.int64, device=labels[0][3].device) if labels else None
        for b, (k, ki, chan0, t, code) in enumerate(images):
            for ch in range(t.shape[0]):
                prog = _Program()
                self.fold(params, ki, chan0 + ch, prog)
                entries.append((t[ch], 0, b, ch, prog))
            out[k] = x_out[b, :t.shape[0]]
        b = 0
        for k, ki, chan0, t, code in labels:
            for ch in range(t.shape[0]):
                prog = _Program()
                self.fold(params, ki, chan0 + ch, prog)
                entries.append((t[ch], code, b + ch, AUG_LABEL, prog))
            out[k] = y_out[b:b + t.shape[0], 0]
            b += t.shape[0]
        _launch(entries, x_out, y_out, max(len(images), nlab, 1), M, spatial)
        return out


class RandFlipd(_BatchTransform):
    """MONAI RandFlipd(keys, prob, spatial_axis): mirror the listed spatial axes (0 = D, 1 = H, 2 = W; None = all three) of every key with probability prob.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, nothing else.  float32 keys come back as float32, bit for bit (NaN and inf included); integer keys
    (uint8, int32, int64) come back as int64 -- the value .long() gives, the label dtype of the batch."""
    intensity = False

    def __init__(self, keys, prob=0.1, spatial_axis=None):
        self.keys, self.prob, self.mask = list(keys), _prob(prob), _flip_mask(spatial_axis)
        self.set_random_state()

    def draw(self):
        return () if self.R.rand() < self.prob else None

    def fold(self, params, key_index, chan, prog):
        prog.add_flip(self.mask)


class RandScaleIntensityd(_BatchTransform):
    """MONAI RandScaleIntensityd(keys, factors, prob): v * fp32(1 + f), one fp32 multiplication.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, f = R.uniform(-factors, factors) (a pair gives low, high); one f for all keys."""

    def __init__(self, keys, factors, prob=0.1, channel_wise=False):
        if channel_wise:
            raise NotImplementedError("RandScaleIntensityd: channel_wise=True is not implemented on the HIP path")
        self.keys, self.prob, self.factors = list(keys), _prob(prob), _range(factors, "factors")
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return float(np.float32(1.0 + self.R.uniform(low=self.factors[0], high=self.factors[1])))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_MUL, params)


class RandShiftIntensityd(_BatchTransform):
    """MONAI RandShiftIntensityd(keys, offsets, prob): v + fp32(o), one fp32 addition.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, o = R.uniform(-offsets, offsets) (a pair gives low, high); one o for all keys."""

    def __init__(self, keys, offsets, prob=0.1, channel_wise=False):
        if channel_wise:
            raise NotImplementedError("RandShiftIntensityd: channel_wise=True is not implemented on the HIP path")
        self.keys, self.prob, self.offsets = list(keys), _prob(prob), _range(offsets, "offsets")
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return float(np.float32(self.R.uniform(low=self.offsets[0], high=self.offsets[1])))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_ADD, params)


class RandGaussianNoised(_BatchTransform):
    """MONAI RandGaussianNoised(keys, prob, mean, std, sample_std): v + (mean + s * n), n standard normal, independent per key and channel.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, s = R.uniform(0, std) if sample_std else std, then key = int(R.randint(2**31 - 1)).
    The normals come from the DEVICE generator (Philox4x32-7 of (key, e) under the stream AUG_NOISE_STREAM, Box-Muller; e = c * D*H*W + flat voxel index, c running
    over the channels of the keys in their listed order), not from R.normal: MONAI draws one host array per key there, so every draw AFTER this transform's
    differs from MONAI's."""

    def __init__(self, keys, prob=0.1, mean=0.0, std=0.1, sample_std=True):
        self.keys, self.prob, self.mean, self.std, self.sample_std = list(keys), _prob(prob), float(mean), float(std), bool(sample_std)
        if not (math.isfinite(self.mean) and math.isfinite(self.std)) or self.std < 0:
            raise ValueError(f"RandGaussianNoised: mean {mean!r} / std {std!r} must be finite, std >= 0")
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        s = self.R.uniform(0, self.std) if self.sample_std else self.std
        return float(np.float32(s)), int(self.R.randint(2 ** 31 - 1))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_NOISE, float(np.float32(self.mean)), params[0], params[1], chan)


class BatchAssembler:
    """the four transforms above, in any order, applied while the batch is assembled: samples (a list of dicts of (C, D, H, W) CUDA tensors, the output of the crop /
    rotation chain) -> (x (B, M, D, H, W) float32, y (B, 1, D, H, W) int64) with the bytes of running `transforms` as a Compose on each sample in turn and then
    torch.cat over image_keys, .long() of the label and torch.stack -- in ONE call of vx_augment_batch (one table, one upload, at most two launches).
    Draws: sample by sample, transform by transform, exactly what that Compose would draw.  Sources may be views (no .contiguous())."""

    def __init__(self, image_keys, label_key, transforms):
        self.image_keys, self.label_key, self.transforms = list(image_keys), label_key, list(transforms)
        if not self.image_keys:
            raise ValueError("BatchAssembler: no image keys")
        known = set(self.image_keys) | {label_key}
        for t in self.transforms:
            if not isinstance(t, _BatchTransform):
                raise TypeError(f"BatchAssembler: {type(t).__name__} is not one of RandFlipd, RandScaleIntensityd, RandShiftIntensityd, RandGaussianNoised")
            if set(t.keys) - known:
                raise ValueError(f"BatchAssembler: {type(t).__name__} names keys {sorted(set(t.keys) - known)} that the batch does not hold")
            if t.intensity and label_key in t.keys:
                raise ValueError(f"BatchAssembler: {type(t).__name__} on the label key {label_key!r}")

    def set_random_state(self, seed=None):
        rs = np.random.RandomState(seed)
        for t in self.transforms:
            t.set_random_state(seed=int(rs.randint(2 ** 31 - 1)))
        return self

    def __call__(self, samples):
        samples = list(samples)
        if not samples:
            raise ValueError("BatchAssembler: no samples")
        keys = self.image_keys + [self.label_key]
        spatial, device, chans = None, None, None
        for i, d in enumerate(samples):                      # every check before any GPU work
            for k in keys:
                _check_source(d[k], f"BatchAssembler: sample {i} key {k!r}", k != self.label_key)
                spatial = tuple(d[k].shape[1:]) if spatial is None else spatial
                device = d[k].device if device is None else device
                if tuple(d[k].shape[1:]) != spatial:
                    raise ValueError(f"BatchAssembler: sample {i} key {k!r} has the patch shape {tuple(d[k].shape[1:])}, the batch {spatial}")
                if d[k].device != device:
                    raise ValueError(f"BatchAssembler: sample {i} key {k!r} lives on {d[k].device}, the batch on {device}")
            if d[self.label_key].shape[0] != 1:
                raise ValueError("BatchAssembler: the label must have one channel")
            c = [d[k].shape[0] for k in self.image_keys]
            chans = c if chans is None else chans
            if c != chans:
                raise ValueError(f"BatchAssembler: sample {i} has {c} channels per image key, the batch {chans}")
        M = sum(chans)
        if 0 in spatial or not 1 <= M <= 64:
            raise ValueError(f"BatchAssembler: patch shape {spatial}, {M} channels (1..64)")
        images, labels = [], []
        for b, d in enumerate(samples):
            progs = {k: [_Program() for _ in range(d[k].shape[0])] for k in keys}
            for t in self.transforms:
                params = t.draw()
                if params is None:
                    continue
                chan0 = 0
                for ki, k in enumerate(t.keys):
                    for ch, prog in enumerate(progs[k]):
                        t.fold(params, ki, chan0 + ch, prog)
                    chan0 += len(progs[k])
            c = 0
            for k in self.image_keys:
                for ch, prog in enumerate(progs[k]):
                    images.append((d[k][ch], 0, b, c, prog))
                    c += 1
            labels.append((d[self.label_key][0], label_code(d[self.label_key]), b, AUG_LABEL, progs[self.label_key][0]))
        B = len(samples)
        x = torch.empty((B, M) + spatial, dtype=torch.float32, device=device)
        y = torch.empty((B, 1) + spatial, dtype=torch.int64, device=device)
        _launch(images + labels, x, y, B, M, spatial)
        return x, y


_CONFIG_KEYS = ("flip_axes", "flip_prob", "scale", "scale_prob", "shift", "shift_prob", "noise_std", "noise_prob")


def from_config(cfg, image_keys, label_key):
    """train_config["augment"] -> BatchAssembler.  Keys (all optional; an unknown key raises ValueError): flip_axes (list of 0 = D, 1 = H, 2 = W: one RandFlipd per
    axis, each with flip_prob, default 0.5, on images and label), scale / scale_prob (RandScaleIntensityd factors, default prob 0.1), shift / shift_prob
    (RandShiftIntensityd offsets, 0.1), noise_std / noise_prob (RandGaussianNoised std with sample_std=True, 0.1); the order is flips, scale, shift, noise."""
    if not isinstance(cfg, dict):
        raise ValueError(f"augment config must be a dict, got {type(cfg).__name__}")
    unknown = sorted(set(cfg) - set(_CONFIG_KEYS))
    if unknown:
        raise ValueError(f"augment config: unknown keys {unknown} (known: {', '.join(_CONFIG_KEYS)})")
    image_keys = list(image_keys)
    ts = []
    axes = cfg.get("flip_axes")
    if axes is not None:
        for a in ([axes] if isinstance(axes, int) else list(axes)):
            ts.append(RandFlipd(image_keys + [label_key], prob=cfg.get("flip_prob", 0.5), spatial_axis=a))
    if cfg.get("scale") is not None:
        ts.append(RandScaleIntensityd(image_keys, factors=cfg["scale"], prob=cfg.get("scale_prob", 0.1)))
    if cfg.get("shift") is not None:
        ts.append(RandShiftIntensityd(image_keys, offsets=cfg["shift"], prob=cfg.get("shift_prob", 0.1)))
    if cfg.get("noise_std") is not None:
        ts.append(RandGaussianNoised(image_keys, prob=cfg.get("noise_prob", 0.1), mean=0.0, std=cfg["noise_std"]))
    return BatchAssembler(image_keys, label_key, ts)


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def set_random_state(self, seed=None):
        rs = np.random.RandomState(seed)
        for t in self.transforms:
            if isinstance(t, _Randomizable):
                t.set_random_state(seed=int(rs.randint(2 ** 31 - 1)))
        return self

    def __call__(self, data):
        for t in self.transforms:
            data = [t(d) for d in data] if isinstance(data, list) and not isinstance(t, RandRotated) else t(data)
        return data
