"""Test helper (not an oracle): mirror test-time augmentation restated with torch.flip, independently of veloxseg_amd.

schedule(axes): the identity, then every itertools.combinations(sorted axes, i) for i = 1 .. len(axes) -- nnU-Net's order.
mirror_average(P, axes): the predictor w -> (P(w) + sum over the schedule of flip(P(flip(w, dims)), dims)) / n, summed by sequential `+` in schedule order.
The sliding-window oracle run on this predictor is what sliding_window_inference(..., mirror_axes=axes) has to equal bit for bit.
"""
import itertools

import torch


def schedule(axes):
    """-> list of tuples of spatial axes, the identity () first"""
    axes = sorted(int(a) for a in axes)
    return [()] + [c for i in range(1, len(axes) + 1) for c in itertools.combinations(axes, i)]


def masks(axes):
    """the schedule as masks: bit a set = spatial axis a mirrored"""
    return [sum(1 << a for a in c) for c in schedule(axes)]


def dims_of_mask(mask, first_spatial_dim):
    return [first_spatial_dim + a for a in range(3) if mask >> a & 1]


def flip_mask(t, mask, first_spatial_dim):
    d = dims_of_mask(mask, first_spatial_dim)
    return torch.flip(t, d) if d else t


def mirror_average(predictor, axes):
    combos = schedule(axes)

    def averaged(w):
        total = predictor(w)
        total = total[0] if isinstance(total, (list, tuple)) else total
        for c in combos[1:]:
            dims = [2 + a for a in c]
            p = predictor(torch.flip(w, dims))
            p = p[0] if isinstance(p, (list, tuple)) else p
            total = total + torch.flip(p, dims)
        return total / len(combos)
    return averaged


def ramp_predictor(w):
    """position-DEPENDENT inside the window: ramps of different slopes along D, H and W plus channel mixing -- a missing or wrong mirror-back on any axis
    changes the values.  (B, C, d, h, w) -> (B, 3, d, h, w)"""
    d, h, x = w.shape[2:]
    rz = torch.arange(d, device=w.device, dtype=torch.float32).view(1, 1, d, 1, 1) * 0.37
    ry = torch.arange(h, device=w.device, dtype=torch.float32).view(1, 1, 1, h, 1) * -0.11
    rx = torch.arange(x, device=w.device, dtype=torch.float32).view(1, 1, 1, 1, x) * 0.053
    return torch.cat([w[:, :1] * 2.0 + rz + rx, w[:, -1:] * (1.0 + ry) - rz, w.mean(1, keepdim=True) * rx + ry], 1)


def flat_predictor(w):
    """position-INDEPENDENT: mirror augmentation must not change the result at all"""
    return torch.cat([w[:, :1] * 2 - 1, w[:, -1:]], 1)
