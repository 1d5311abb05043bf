"""Test helper (not an oracle), CPU only: the batch-assembly transforms of veloxseg_amd.utils.augment restated independently of the package.

  * flips as torch.flip, scale and shift as fp32 torch operations, ONE operation per step (so nothing can be contracted);
  * the draw orders of RandFlipd / RandScaleIntensityd / RandShiftIntensityd / RandGaussianNoised written out again on their own numpy RandomState
    (modelled on MONAI 1.x, unpinned against MONAI itself, which is not installed): R.rand() < prob first, the parameters only when that fires;
  * the standard normals of the noise step restated in fp64 from oracle.philox.philox4x32(ctr, stream, key):
        element e = c * D*H*W + (flat index of the voxel in the patch) uses the words r[0..3] of counter e >> 2 under the stream NOISE_STREAM and the 64-bit key `key`;
        elements 4k and 4k + 1 share the pair (r[0], r[1]), elements 4k + 2 and 4k + 3 the pair (r[2], r[3]);
        u1 = ((ra >> 8) + 1) / 2^24 in (0, 1], u2 = (rb >> 8) / 2^24 in [0, 1), rad = sqrt(-2 ln u1);
        the even element gets rad * cos(2 pi u2), the odd one rad * sin(2 pi u2).
"""
import math

import numpy as np
import torch

from oracle.philox import philox4x32

NOISE_STREAM = 0x564158475541          # "AUGXAV"; dropout site ids count up from 1
MAX_ABS_NORMAL = math.sqrt(2.0 * 24.0 * math.log(2.0))          # u1 >= 2^-24


def flip(t, mask):
    """mirror the spatial axes named by `mask` (bit 0 = D, 1 = H, 2 = W) of a (..., D, H, W) tensor"""
    dims = [t.dim() - 3 + a for a in range(3) if mask >> a & 1]
    return torch.flip(t, dims) if dims else t.clone()


def mask_of(spatial_axis):
    if spatial_axis is None:
        return 7
    axes = [spatial_axis] if isinstance(spatial_axis, int) else list(spatial_axis)
    m = 0
    for a in axes:
        m |= 1 << (a % 3)
    return m


def scale(t, f32):
    return t * torch.tensor(f32, dtype=torch.float32)


def shift(t, o32):
    return t + torch.tensor(o32, dtype=torch.float32)


def normals(key, n, e0=0):
    """fp64 (n,): the standard normals of elements e0 .. e0 + n - 1"""
    lo, hi = e0 >> 2, (e0 + n - 1) >> 2
    w = philox4x32(np.arange(lo, hi + 1, dtype=np.uint64), NOISE_STREAM, key).astype(np.uint64)
    out = np.empty((hi - lo + 1, 4), dtype=np.float64)
    for p in (0, 1):
        u1 = ((w[:, 2 * p] >> np.uint64(8)).astype(np.float64) + 1.0) / 16777216.0
        u2 = (w[:, 2 * p + 1] >> np.uint64(8)).astype(np.float64) / 16777216.0
        rad = np.sqrt(-2.0 * np.log(u1))
        out[:, 2 * p] = rad * np.cos(2.0 * np.pi * u2)
        out[:, 2 * p + 1] = rad * np.sin(2.0 * np.pi * u2)
    return out.reshape(-1)[e0 - 4 * lo: e0 - 4 * lo + n]


def patch_normals(key, c, spatial):
    """fp64 (D, H, W): the normals of channel c of a patch"""
    V = int(np.prod(spatial))
    return normals(key, V, c * V).reshape(spatial)


# ---- draw orders: every function consumes from R exactly what one call of the transform consumes, and returns None when the call does not fire ----------------
def _pair(v):
    if isinstance(v, (int, float)):
        return min(-v, v), max(-v, v)
    return min(v), max(v)


def draw_flip(R, prob):
    return () if R.rand() < prob else None


def draw_scale(R, prob, factors):
    if not R.rand() < prob:
        return None
    lo, hi = _pair(factors)
    return float(np.float32(1.0 + R.uniform(low=lo, high=hi)))


def draw_shift(R, prob, offsets):
    if not R.rand() < prob:
        return None
    lo, hi = _pair(offsets)
    return float(np.float32(R.uniform(low=lo, high=hi)))


def draw_noise(R, prob, std, sample_std=True):
    if not R.rand() < prob:
        return None
    s = R.uniform(0, std) if sample_std else std
    return float(np.float32(s)), int(R.randint(2 ** 31 - 1))


def compose_seeds(seed, n):
    """the seeds Compose.set_random_state / BatchAssembler.set_random_state hand to their n randomizable transforms"""
    rs = np.random.RandomState(seed)
    return [int(rs.randint(2 ** 31 - 1)) for _ in range(n)]
