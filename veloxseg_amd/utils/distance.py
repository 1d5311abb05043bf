"""Exact Euclidean distance transform on the GPU (csrc/distance.hip).  The reference reaches it through medpy's hd95, i.e. through
scipy.ndimage.distance_transform_edt on the host; here the volume stays on the device.  Device tensors only; there is no CPU fallback.

The result is the fp64 map  sqrt(min over the sites of fl(fl(t_z + t_y) + t_x)),  t_a = fl(fl(d_a * s_a)^2): scipy's own order of accumulation, so the squared map
and its square root equal scipy.ndimage.distance_transform_edt(sampling=) bit for bit (tests/test_distance_cpu.py holds the oracle to scipy, tests/test_distance_gpu.py
the kernels to the oracle).  A volume without any site gives +inf everywhere (scipy's result for it is unspecified)."""
import math

import torch

from .. import _hip as H
from .morphology import PackedMask, pack


def _sampling(sampling, what):
    """None -> (1, 1, 1); a number -> that number on every axis (as scipy); else three finite numbers > 0 in (z, y, x) order"""
    if sampling is None:
        return (1.0, 1.0, 1.0)
    if isinstance(sampling, (int, float)):
        sampling = (sampling,) * 3
    s = tuple(float(v) for v in (sampling.tolist() if hasattr(sampling, "tolist") else sampling))
    if len(s) != 3 or any(not (math.isfinite(v) and v > 0.0) for v in s):
        raise ValueError(f"{what}: three finite spacings > 0 expected, got {s}")
    return s


def _packed(x, label, what):
    """a PackedMask of x != 0 (or x == label); floating masks such as (labels == 3).float() are compared on the device first"""
    if isinstance(x, PackedMask):
        if label is not None:
            raise ValueError(f"{what}: a packed mask has no labels to select from")
        return x
    if isinstance(x, torch.Tensor) and x.is_floating_point():
        if not x.is_cuda:
            raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
        x, label = ((x != 0) if label is None else (x == label)), None
    return pack(x, label)


def edt_sq(p: PackedMask, invert: bool, sampling) -> torch.Tensor:
    """(B, D, H, W) fp64: the squared distance to the nearest set (invert False) or clear (invert True) voxel of every sample of a packed mask"""
    D, Hh, W = p.shape
    cap = H.query("vx_edt_max_extent")
    if max(D, Hh, W) > cap:
        raise ValueError(f"distance transform: extents {p.shape} exceed the longest line a pass holds in LDS ({cap})")
    sz, sy, sx = sampling
    out = torch.empty((p.bits.shape[0], D, Hh, W), dtype=torch.float64, device=p.bits.device)
    st = H.stream_ptr()
    for b in range(out.shape[0]):
        H.call("vx_edt_sq", p.bits[b].data_ptr(), int(bool(invert)), out[b].data_ptr(), D, Hh, W, sz, sy, sx, st)
    return out


def sqrt_(x: torch.Tensor) -> torch.Tensor:
    """the correctly rounded square root of a contiguous fp64 device tensor, in place"""
    flat, st = x.view(-1), H.stream_ptr()
    step = 2 ** 31 - 1
    for i in range(0, flat.numel(), step):
        part = flat[i:i + step]
        H.call("vx_edt_sqrt", part.data_ptr(), part.numel(), st)
    return x


def _transform(x, invert, sampling, squared, label, what):
    s = _sampling(sampling, what)
    p = _packed(x, label, what)
    out = edt_sq(p, invert, s)
    if not squared:
        sqrt_(out)
    return out.reshape(p.like_shape)


def distance_transform_edt(x, sampling=None, squared: bool = False, label=None) -> torch.Tensor:
    """scipy.ndimage.distance_transform_edt: for every voxel where x != 0 (or x == label) the distance to the nearest voxel where that is false, 0 on those voxels.
    x: a (D, H, W) or (B, 1, D, H, W) device tensor (bool, uint8, int32, int64 or floating) or a PackedMask; sampling: the voxel spacing (z, y, x), default 1.
    -> fp64 of the input's shape; squared=True returns the squared distances (no square root is taken)."""
    return _transform(x, True, sampling, squared, label, "distance_transform_edt")


def distance_to(mask_or_packed, sampling=None, squared: bool = False) -> torch.Tensor:
    """the distance of every voxel to the nearest SET voxel of the mask (x != 0), 0 on the mask itself: the form the surface metrics use"""
    return _transform(mask_or_packed, False, sampling, squared, None, "distance_to")
