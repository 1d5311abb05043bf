"""Test helper (not an oracle): Gaussian importance blending of the sliding-window inference restated with torch, independently of veloxseg_amd.

Restates MONAI 1.5 `compute_importance_map(mode="gaussian")` and the blending loop of `sliding_window_inference` for the argument subset the driver takes.  MONAI is
not installed here, so this is UNPINNED against MONAI itself (like oracle/sliding_window_oracle.py); MONAI forms its map on sw_device, this file on the host CPU.

  axis table     g_a = exp(x^2 / (-2 (r_a s_a)^2)),  x = arange(-(r_a - 1) / 2, (r_a - 1) / 2 + 1) in fp32, on the CPU
  window weight  w = clamp((g_0 (x) g_1) (x) g_2, min=floor),  floor = max(min of the unclamped product, 1e-3)
  blending       out[window] += w * prediction,  count[window] += w,  window after window in the order of dense_patch_starts;  result = out / count

sliding_window_inference(..., sigma_scale) is what the driver's blend="gaussian" has to equal bit for bit; with mirror_axes, run it on tta_ref.mirror_average(...).
"""
import torch
import torch.nn.functional as F

from oracle.sliding_window_oracle import dense_patch_starts, get_scan_interval, get_valid_patch_size


def sigmas(sigma_scale):
    return tuple(float(s) for s in sigma_scale) if isinstance(sigma_scale, (tuple, list)) else (float(sigma_scale),) * 3


def axis_table(r, s):
    x = torch.arange(-(r - 1) / 2.0, (r - 1) / 2.0 + 1, dtype=torch.float32)
    return torch.exp(x ** 2 / (-2 * (r * s) ** 2))


def unclamped_map(patch, sigma_scale):
    g = [axis_table(r, s) for r, s in zip(patch, sigmas(sigma_scale))]
    return (g[0].view(-1, 1, 1) * g[1].view(1, -1, 1)) * g[2].view(1, 1, -1)


def floor_of(patch, sigma_scale):
    """the clamp's lower bound as the fp32 value the clamp compares with"""
    return float(torch.tensor(max(float(unclamped_map(patch, sigma_scale).min()), 1e-3), dtype=torch.float32))


def importance_map(patch, sigma_scale):
    """(rd, rh, rw) fp32 on the CPU"""
    m = unclamped_map(patch, sigma_scale)
    return torch.clamp(m, min=max(float(m.min()), 1e-3))


def geometry(shape, roi_size, overlap):
    """-> (padded image size, roi, pad list as F.pad takes it, window starts) of a (B, C, D, H, W) input"""
    image_size_ = list(shape[2:])
    roi = tuple(int(r) if r else int(m) for r, m in zip(roi_size, image_size_))
    image_size = tuple(max(m, r) for m, r in zip(image_size_, roi))
    pad = []
    for k in range(4, 1, -1):
        diff = max(roi[k - 2] - shape[k], 0)
        pad.extend([diff // 2, diff - diff // 2])
    starts = dense_patch_starts(image_size, roi, get_scan_interval(image_size, roi, overlap))
    return image_size, get_valid_patch_size(image_size, roi), pad, starts


def count_map(image_size, patch, starts, w):
    """the normaliser: w added window after window, in window order, into zeros"""
    count = torch.zeros(tuple(image_size), dtype=torch.float32, device=w.device)
    for st in starts:
        count[tuple(slice(s, s + p) for s, p in zip(st, patch))] += w
    return count


def max_cover(image_size, patch, starts):
    """the largest number of windows over one voxel"""
    n = torch.zeros(tuple(image_size), dtype=torch.int64)
    for st in starts:
        n[tuple(slice(s, s + p) for s, p in zip(st, patch))] += 1
    return int(n.max())


def sliding_window_inference(inputs, roi_size, sw_batch_size, predictor, overlap=0.25, sigma_scale=0.125, cval=0.0):
    """Gaussian blending: out = (sum over windows of w * predictor(window)) / (sum over the covering windows of w)"""
    batch_size = inputs.shape[0]
    image_size_ = list(inputs.shape[2:])
    image_size, patch, pad, starts = geometry(inputs.shape, roi_size, overlap)
    if any(pad):
        inputs = F.pad(inputs, pad=pad, mode="constant", value=cval)
    w = importance_map(patch, sigma_scale).to(inputs.device)
    num_win = len(starts)
    total = num_win * batch_size
    out = None
    for g in range(0, total, sw_batch_size):
        idxs = list(range(g, min(g + sw_batch_size, total)))
        sl = [(slice(i // num_win, i // num_win + 1), slice(None)) + tuple(slice(s, s + p) for s, p in zip(starts[i % num_win], patch)) for i in idxs]
        prob = predictor(torch.cat([inputs[s] for s in sl]))
        if isinstance(prob, (list, tuple)):
            prob = prob[0]
        if out is None:
            out = torch.zeros((batch_size, prob.shape[1]) + tuple(image_size), dtype=torch.float32, device=prob.device)
        for k, s in enumerate(sl):
            out[s] += w * prob[k:k + 1]
    out = out / count_map(image_size, patch, starts, w)
    if any(pad):
        lo = [pad[4], pad[2], pad[0]]
        out = out[(slice(None), slice(None)) + tuple(slice(l, l + m) for l, m in zip(lo, image_size_))]
    return out
