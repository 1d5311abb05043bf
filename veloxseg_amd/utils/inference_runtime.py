"""Sliding-window inference on MI355X -- drop-in for the reference's utils/inference_runtime.py.

`sliding_window_predict(inputs, predictor, roi_size, sw_batch_size, test_config, **kwargs)` keeps the reference signature
(utils/inference_runtime.py:4-19); the MONAI call underneath it (monai.inferers.sliding_window_inference, constant blending,
constant padding) is re-implemented natively: window origins on the host, window extraction / blending / normalisation / argmax in
HIP kernels (csrc/infer.hip), the predictor being the HIP VeloxSeg forward.  Semantics restated in oracle/sliding_window_oracle.py.
Beyond the reference's call: mirror test-time augmentation (mirror_axes) and Gaussian importance blending (blend="gaussian", MONAI's
mode="gaussian"; restated in tests/blend_ref.py).
"""
from __future__ import annotations

import ctypes
import itertools
import math
import numbers
import os
from typing import Callable, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

from .. import _hip as H


def _valid_patch(image_size, patch_size):
    return tuple(min(m, p) if p else m for m, p in zip(image_size, patch_size))


def scan_interval(image_size, roi_size, overlap: float) -> Tuple[int, ...]:
    """int(roi * (1 - overlap)) >= 1 per axis; the whole roi where it spans the axis (monai `_get_scan_interval`)"""
    out = []
    for m, r in zip(image_size, roi_size):
        if r == m:
            out.append(int(r))
        else:
            iv = int(r * (1 - overlap))
            out.append(iv if iv > 0 else 1)
    return tuple(out)


def window_starts(image_size, roi_size, interval) -> List[Tuple[int, int, int]]:
    """window origins, first axis slowest, last window of every axis clamped to the edge (monai `dense_patch_slices`)"""
    per_axis = []
    for m, r, iv in zip(image_size, roi_size, interval):
        if iv == 0:
            n = 1
        else:
            num = int(math.ceil(float(m) / iv))
            first = next((d for d in range(num) if d * iv + r >= m), None)
            n = first + 1 if first is not None else 1
        per_axis.append([k * iv - max(k * iv + r - m, 0) for k in range(n)])
    return [(a, b, c) for a in per_axis[0] for b in per_axis[1] for c in per_axis[2]]


def _axis_counts(starts_axis: Sequence[int], r: int, m: int, device) -> torch.Tensor:
    c = torch.zeros(m, dtype=torch.float32)
    for s in starts_axis:
        c[s:s + r] += 1.0
    return c.to(device)


BLEND_MODES = ("constant", "gaussian")


def _check_blend(blend, sigma_scale) -> Tuple[str, Tuple[float, float, float]]:
    """-> (blend, one sigma_scale per spatial axis); ValueError on an unknown blend or a sigma_scale that is not one or three positive finite numbers"""
    if not isinstance(blend, str) or blend not in BLEND_MODES:
        raise ValueError(f"blend: one of {BLEND_MODES} expected, got {blend!r}")
    s = list(sigma_scale) if isinstance(sigma_scale, (list, tuple)) else [sigma_scale] * 3
    if len(s) != 3 or any(isinstance(v, bool) or not isinstance(v, numbers.Real) or not (0.0 < float(v) < math.inf) for v in s):
        raise ValueError(f"sigma_scale: one or three positive finite numbers expected, got {sigma_scale!r}")
    return blend, tuple(float(v) for v in s)


def gaussian_axis_table(r: int, sigma_scale: float) -> torch.Tensor:
    """the Gaussian of one window axis, r fp32 values on the host (monai `compute_importance_map`, mode "gaussian", per axis): sigma = r * sigma_scale"""
    x = torch.arange(-(r - 1) / 2.0, (r - 1) / 2.0 + 1, dtype=torch.float32)
    return torch.exp(x ** 2 / (-2 * (r * sigma_scale) ** 2))


def gaussian_tables(roi: Sequence[int], sigma_scale: Sequence[float]) -> Tuple[List[torch.Tensor], float]:
    """-> (the three axis tables, floor).  The weight of a window voxel is max((g0[z] * g1[y]) * g2[x], floor), floor = max(smallest unclamped weight, 1e-3) in fp32;
    the tables are positive and symmetric and rounded multiplication is monotone, so the smallest weight is the corner's."""
    g = [gaussian_axis_table(int(r), float(s)) for r, s in zip(roi, sigma_scale)]
    corner = (g[0][0] * g[1][0]) * g[2][0]
    return g, float(torch.tensor(max(float(corner), 1e-3), dtype=torch.float32))


def _cover_tables(starts_axis: Sequence[int], g: torch.Tensor, m: int) -> Tuple[List[int], torch.Tensor]:
    """one axis of the normaliser's geometry: for every coordinate c < m the number of windows [s, s + len(g)) that cover it, and a (m, largest count) table whose row c
    holds g[c - s] of those windows in ascending start (the rest of a row is 0 and never read)"""
    r = int(g.numel())
    cover = [[c - s for s in starts_axis if s <= c < s + r] for c in range(m)]
    stride = max(len(row) for row in cover)
    idx = torch.tensor([row + [0] * (stride - len(row)) for row in cover], dtype=torch.long)
    keep = torch.tensor([[1.0] * len(row) + [0.0] * (stride - len(row)) for row in cover], dtype=torch.float32)
    return [len(row) for row in cover], g[idx] * keep


class _Blend:
    """what the Gaussian blending of one volume geometry hands to the kernels: the axis tables (g) for the accumulation, the per-coordinate covering counts (tab) and
    covering table values (gc) for the normaliser, all on the device, and the floor"""

    def __init__(self, starts, roi, image_size, sigma_scale, device):
        g, self.floor = gaussian_tables(roi, sigma_scale)
        self.g = torch.cat(g).to(device)
        per_axis = [_cover_tables(sorted({s[a] for s in starts}), g[a], image_size[a]) for a in range(3)]
        self.strides = tuple(int(t.shape[1]) for _, t in per_axis)
        self.tab = torch.tensor([n for counts, _ in per_axis for n in counts], dtype=torch.int32).to(device)
        self.gc = torch.cat([t.reshape(-1) for _, t in per_axis]).to(device)


_BLENDS = {}          # the last few geometries' tables: a few KB each, read-only once uploaded (a volume series shares one geometry)


def _blend_tables(starts, roi, image_size, sigma_scale, device) -> _Blend:
    key = (tuple(roi), tuple(image_size), tuple(sigma_scale), tuple(starts[0]), tuple(starts[-1]), len(starts), str(device))
    hit = _BLENDS.get(key)
    if hit is None or hit[0] != starts:
        if len(_BLENDS) >= 8:
            _BLENDS.pop(next(iter(_BLENDS)))
        hit = _BLENDS[key] = (list(starts), _Blend(starts, roi, image_size, sigma_scale, device))
    return hit[1]


def _accumulate(prob_k, acc_b, K, dhw, roi, origin, blend, stream):
    """one window into the blending: acc[window] += prob (constant) or += w * prob (Gaussian)"""
    if blend is None:
        H.call("vx_sw_accumulate", H.P(prob_k), H.P(acc_b), K, *dhw, *roi, *origin, 1.0, stream)
    else:
        H.call("vx_sw_blend_accumulate", H.P(prob_k), None, H.P(acc_b), H.P(blend.g), blend.floor, K, *dhw, *roi, *origin, 0, 1.0, stream)


SW_MAX_WINDOWS = 16  # VX_SW_MAX_WINDOWS of include/veloxseg_hip.h: windows per vx_sw_extract_mirror launch (a larger sw_batch_size takes several)


def mirror_schedule(axes: Sequence[int]) -> List[int]:
    """the mirrors of a test-time augmentation over the spatial axes `axes` (0 = D, 1 = H, 2 = W; any order), as masks (bit a = axis a mirrored) in nnU-Net's order:
    the identity, then every itertools.combinations(sorted axes, i) for i = 1 .. len(axes).  (0, 1, 2) -> [0, 1, 2, 4, 3, 5, 6, 7]."""
    axes = list(axes)
    if any(isinstance(a, (bool, float, str)) or a not in (0, 1, 2) for a in axes):
        raise ValueError(f"mirror_axes: spatial axes out of (0, 1, 2) expected, got {axes}")
    axes = [int(a) for a in axes]
    if len(set(axes)) != len(axes):
        raise ValueError(f"mirror_axes: duplicate axis in {axes}")
    axes = sorted(axes)
    return [0] + [sum(1 << a for a in c) for i in range(1, len(axes) + 1) for c in itertools.combinations(axes, i)]


def _extract_mirrored(inputs, win, idxs, starts, num_win, geom, mask, stream):
    """win[k] = window idxs[k] of the (B, C, D, H, W) input, mirrored by `mask` inside its own extent: one launch per SW_MAX_WINDOWS windows"""
    B, C, D, Hh, W, rd, rh, rw = geom
    for g in range(0, len(idxs), SW_MAX_WINDOWS):
        part = idxs[g:g + SW_MAX_WINDOWS]
        tab = (ctypes.c_int * (4 * len(part)))(*[v for i in part for v in (i // num_win,) + tuple(starts[i % num_win])])
        H.call("vx_sw_extract_mirror", H.P(inputs), H.P(win[g:g + len(part)]), ctypes.addressof(tab), len(part), mask, B, C, D, Hh, W, rd, rh, rw, stream)


def _mirrored_forwards(inputs, win, idxs, starts, num_win, geom, masks, run, wsum, stream, span=None):
    """the len(masks) forwards of ONE window batch, in schedule order, all on `stream`: -> (wsum, prediction of the last mask).  wsum holds
    P(w) + sum of flip_f(P(flip_f(w))) over every mask but the last, added in schedule order; the last one is added by vx_sw_mirror_accumulate on its way into the
    blending.  A taped predictor hands out its static output, which its next replay overwrites: every prediction is folded into wsum on the same stream before
    the next forward is started.  wsum: a (sw_batch_size, K, rd, rh, rw) buffer from an earlier batch, or None (allocated here, on the current stream).
    span = (j0, j1): only the schedule positions j0 .. j1 - 1 (-> (wsum, None) when the last mask is not among them)."""
    rd, rh, rw = geom[5:]
    prob = None
    for j in range(*(span or (0, len(masks)))):
        f = masks[j]
        _extract_mirrored(inputs, win, idxs, starts, num_win, geom, f, stream)
        prob = run(win)
        if isinstance(prob, (list, tuple)):
            prob = prob[0]
        prob = prob.contiguous().float()
        if tuple(prob.shape[2:]) != (rd, rh, rw) or prob.shape[0] != len(idxs):
            raise NotImplementedError("predictor output must have the window's spatial size")
        if wsum is None:
            wsum = torch.empty_like(prob)
        if tuple(wsum.shape[1:]) != tuple(prob.shape[1:]) or wsum.shape[0] < len(idxs):
            raise NotImplementedError("predictor output changed its shape between the forwards of a volume")
        if j == len(masks) - 1:
            return wsum, prob
        H.call("vx_sw_mirror_sum", H.P(prob), H.P(wsum[:len(idxs)]), len(idxs) * int(prob.shape[1]), rd, rh, rw, f, 1 if j == 0 else 0, stream)
    return wsum, None


def _accumulate_mirrored(prob, wsum, acc, idxs, starts, num_win, geom, mask, weight, stream, blend=None):
    """acc[window] += weight * (wsum + flip_mask(prob)), one launch per window in window order; blend (Gaussian): += w * (weight * (wsum + flip_mask(prob)))"""
    D, Hh, W, rd, rh, rw = geom[2:]
    K = int(prob.shape[1])
    for k, i in enumerate(idxs):
        z0, y0, x0 = starts[i % num_win]
        if blend is None:
            H.call("vx_sw_mirror_accumulate", H.P(prob[k]), H.P(wsum[k]), H.P(acc[i // num_win]), K, D, Hh, W, rd, rh, rw, z0, y0, x0, mask, weight, stream)
        else:
            H.call("vx_sw_blend_accumulate", H.P(prob[k]), H.P(wsum[k]), H.P(acc[i // num_win]), H.P(blend.g), blend.floor, K, D, Hh, W, rd, rh, rw, z0, y0, x0,
                   mask, weight, stream)


# two window batches in flight (round 6): each forward of a window batch is a ~250-launch tape that leaves most of the chip idle at the reference's sw_batch_size of 2; the next
# batch's forward is replayed from a second caller stream on a replica of the tape (engine.TapedPredictor.forward_slot) while the first one runs.  The blending stays in the
# reference's window order -- the accumulation of batch i + 1 waits for the one of batch i -- so the result is bit for bit the sequential one.  SW_PIPELINE = False: sequential (tests).
SW_PIPELINE = True
SW_INFLIGHT = 2      # window batches in flight


def _pipelined(inputs, predictor, starts, num_win, total, swb, cdhw, roi, blend=None):
    C, D, Hh, W = cdhw
    rd, rh, rw = roi
    dev = inputs.device
    cur = torch.cuda.current_stream(dev)
    streams = _SW_STREAMS.setdefault(str(dev), [torch.cuda.Stream(device=dev) for _ in range(SW_INFLIGHT)])
    wins = [torch.empty((swb, C, rd, rh, rw), device=dev, dtype=torch.float32) for _ in range(SW_INFLIGHT)]
    # the first batch the plain way (captures / validates the tape of this shape; tells us K)
    g0 = 0
    for k in range(swb):
        z0, y0, x0 = starts[k % num_win]
        H.call("vx_sw_extract", H.P(inputs[k // num_win]), H.P(wins[0][k]), C, D, Hh, W, rd, rh, rw, z0, y0, x0, H.stream_ptr())
    prob = predictor(wins[0])
    if isinstance(prob, (list, tuple)):
        prob = prob[0]
    if prob.dtype != torch.float32 or not prob.is_contiguous() or tuple(prob.shape[2:]) != (rd, rh, rw):
        return None
    K = int(prob.shape[1])
    B = inputs.shape[0]
    acc = torch.zeros((B, K, D, Hh, W), device=dev, dtype=torch.float32)
    for k in range(swb):
        _accumulate(prob[k], acc[k // num_win], K, (D, Hh, W), roi, starts[k % num_win], blend, H.stream_ptr())
    # the rest alternately on the two slot streams
    for s_ in streams:
        s_.wait_stream(cur)
    last_acc = None                                          # event after the accumulation of the previous batch
    nb = total // swb
    for bi in range(1, nb):
        # replicas 1 and 2 of the tape, each always replayed from ITS stream (replica 0 -- the plain call above -- stays on the caller's stream: a tape whose caller stream
        # changes between replays synchronises the host once)
        slot = bi % SW_INFLIGHT
        st_ = streams[slot]
        with torch.cuda.stream(st_):
            for k in range(swb):
                i = bi * swb + k
                z0, y0, x0 = starts[i % num_win]
                H.call("vx_sw_extract", H.P(inputs[i // num_win]), H.P(wins[slot][k]), C, D, Hh, W, rd, rh, rw, z0, y0, x0, st_.cuda_stream)
            out = predictor.forward_slot(wins[slot], 1 + slot)
            if out is None:                                  # no replica (capture refused): this batch on the eager launches, on this stream
                out = predictor.model(wins[slot]) if hasattr(predictor, "model") else predictor(wins[slot])
            if isinstance(out, (list, tuple)):
                out = out[0]
            out = out.contiguous().float()
            if last_acc is not None:
                st_.wait_event(last_acc)                     # blending in window order: bit for bit the sequential sums
            for k in range(swb):
                i = bi * swb + k
                _accumulate(out[k], acc[i // num_win], K, (D, Hh, W), roi, starts[i % num_win], blend, st_.cuda_stream)
            last_acc = torch.cuda.Event()
            last_acc.record(st_)
    for s_ in streams:
        cur.wait_stream(s_)
    return acc, K


def _pipelined_mirrored(inputs, predictor, starts, num_win, total, swb, geom, masks, blend=None):
    """_pipelined with mirror test-time augmentation: the len(masks) forwards of a window batch run one after the other on that batch's slot (its tape replica, its
    stream); two batches stay in flight, their forwards issued in turn, and the blending of batch i + 1 waits for the one of batch i, so the sums are those of the
    sequential loop bit for bit."""
    B, C, D, Hh, W, rd, rh, rw = geom
    dev = inputs.device
    cur = torch.cuda.current_stream(dev)
    streams = _SW_STREAMS.setdefault(str(dev), [torch.cuda.Stream(device=dev) for _ in range(SW_INFLIGHT)])
    wins = [torch.empty((swb, C, rd, rh, rw), device=dev, dtype=torch.float32) for _ in range(SW_INFLIGHT)]
    weight = 1.0 / len(masks)
    # the FIRST forward of the first batch the plain way, on the caller's stream (captures / validates the tape of this shape; tells us K).  Its other forwards are
    # slot 0's: a first batch held on the caller's stream to its end would run its len(masks) forwards with nothing beside them
    wsum0, _ = _mirrored_forwards(inputs, wins[0], list(range(swb)), starts, num_win, geom, masks, predictor, None, H.stream_ptr(), span=(0, 1))
    K = int(wsum0.shape[1])
    acc = torch.zeros((B, K, D, Hh, W), device=dev, dtype=torch.float32)
    wsums = [torch.empty_like(wsum0) if s_ else wsum0 for s_ in range(SW_INFLIGHT)]
    for s_ in streams:
        s_.wait_stream(cur)
    last_acc = None

    def run(w, slot):
        out = predictor.forward_slot(w, 1 + slot)
        if out is None:                                      # no replica (capture refused): the eager launches, on this stream
            out = predictor.model(w) if hasattr(predictor, "model") else predictor(w)
        return out
    nb = total // swb
    idxs_of = lambda bi: list(range(bi * swb, (bi + 1) * swb))
    for b0 in range(0, nb, SW_INFLIGHT):
        # the batches in flight are enqueued forward by forward in turn (batch b0 mask 0, batch b0 + 1 mask 0, batch b0 mask 1, ...); enqueued batch by batch -- all
        # len(masks) tapes of one, then those of the other -- the two hardly overlap
        group = range(b0, min(b0 + SW_INFLIGHT, nb))
        last = {}
        for j in range(len(masks)):
            for bi in group:
                if bi == 0 and j == 0:
                    continue                                 # (done above, on the caller's stream)
                slot = bi % SW_INFLIGHT
                with torch.cuda.stream(streams[slot]):
                    _, prob = _mirrored_forwards(inputs, wins[slot], idxs_of(bi), starts, num_win, geom, masks, lambda w, s_=slot: run(w, s_), wsums[slot],
                                                 streams[slot].cuda_stream, span=(j, j + 1))
                last[bi] = prob
        for bi in group:
            st_ = streams[bi % SW_INFLIGHT]
            with torch.cuda.stream(st_):
                if last_acc is not None:
                    st_.wait_event(last_acc)                 # blending in window order
                _accumulate_mirrored(last[bi], wsums[bi % SW_INFLIGHT], acc, idxs_of(bi), starts, num_win, geom, masks[-1], weight, st_.cuda_stream, blend)
                last_acc = torch.cuda.Event()
                last_acc.record(st_)
    for s_ in streams:
        cur.wait_stream(s_)
    return acc, K


def _run_mirrored(inputs, predictor, starts, num_win, total, swb, geom, masks, blend=None):
    """mirror test-time augmentation: len(masks) forwards per window batch, summed window by window -> (acc, K).  Pipelined under the plain driver's conditions
    (a predictor with tape replicas, at least two full window batches, no ragged one), else one batch after the other on the caller's stream."""
    if SW_PIPELINE and hasattr(predictor, "forward_slot") and total >= 2 * swb and total % swb == 0:
        return _pipelined_mirrored(inputs, predictor, starts, num_win, total, swb, geom, masks, blend)
    B, C, D, Hh, W, rd, rh, rw = geom
    acc = win = wsum = None
    for g in range(0, total, swb):
        idxs = list(range(g, min(g + swb, total)))
        if win is None:
            win = torch.empty((len(idxs), C, rd, rh, rw), device=inputs.device, dtype=torch.float32)
        wsum, prob = _mirrored_forwards(inputs, win[:len(idxs)], idxs, starts, num_win, geom, masks, predictor, wsum, H.stream_ptr())
        if acc is None:
            acc = torch.zeros((B, int(prob.shape[1]), D, Hh, W), device=inputs.device, dtype=torch.float32)
        _accumulate_mirrored(prob, wsum, acc, idxs, starts, num_win, geom, masks[-1], 1.0 / len(masks), H.stream_ptr(), blend)
    return acc, int(acc.shape[1])


_SW_STREAMS = {}


def sliding_window_inference(inputs: torch.Tensor, roi_size: Sequence[int], sw_batch_size: int, predictor: Callable, overlap: float = 0.25,
                             mode: str = "constant", padding_mode: str = "constant", cval: float = 0.0, return_labels: bool = False,
                             mirror_axes: Sequence[int] = (), sw_device=None, device=None, blend: str = "constant", sigma_scale=0.125, **unsupported):
    """-> blended predictions (B, K, D, H, W) fp32, or (predictions, uint8 argmax labels (B, 1, D, H, W)) with return_labels.
    Only the arguments the reference drivers use are supported (constant blending / padding); anything else raises.
    mirror_axes: mirror test-time augmentation over these spatial axes (0 = D, 1 = H, 2 = W): every window is also predicted under each mirror of
    mirror_schedule(mirror_axes), the predictions are mirrored back and summed window by window in schedule order, and the window enters the blending with weight
    1 / n -- bit for bit the result of the plain call on the predictor that averages its mirrored predictions.  () = off.
    blend: "constant" (every window counts the same; the default, and with it every launch is the one of the call without the keyword) or "gaussian": every window is
    weighted by a Gaussian importance map, w = max((g_0[z] * g_1[y]) * g_2[x], floor) with g_a = exp(-x^2 / (2 (r_a * sigma_scale_a)^2)) over the window axis a and
    floor = max(smallest such product, 1e-3), and the sum is divided by the sum of the weights of the covering windows, added in window order.
    blend="gaussian" is MONAI's mode="gaussian" (restated from MONAI 1.5, not pinned against MONAI itself: it forms its map on sw_device, here the axis tables are formed
    on the host); `mode` keeps its contract -- "constant" only, anything else raises NotImplementedError -- and aliasing it is left to a later change.
    sigma_scale: one positive number or one per spatial axis (used by blend="gaussian").  An unknown blend or a bad sigma_scale raises ValueError before any GPU work.
    With mirror_axes the window enters as w * ((1 / n) * sum of its mirrored-back predictions): the plain Gaussian call on the mirror-averaging predictor.
    sw_device: where the windows are predicted -- None or the inputs' device (there is no other path).  device: where the RESULT lives (the reference's huge-volume
    call passes "cpu"); the blending itself stays on the GPU and the result is moved once at the end."""
    if str(mode).lower() not in ("constant", "blendmode.constant") or str(padding_mode).lower() not in ("constant", "pytorchpadmode.constant"):
        raise NotImplementedError("veloxseg_amd sliding window: constant blending / constant padding only (what utils/inference_*.py use)")
    if unsupported:
        raise NotImplementedError(f"veloxseg_amd sliding window: unsupported arguments {sorted(unsupported)}")
    blend, sigma_scale = _check_blend(blend, sigma_scale)
    if inputs.dim() != 5:
        raise ValueError("sliding window expects (B, C, D, H, W)")
    if not inputs.is_cuda:
        raise RuntimeError("veloxseg_amd sliding window runs on MI355X only (no CPU path); move the volume to a cuda device")
    if sw_device is not None:
        swd = torch.device(sw_device)
        if swd.type == "cuda" and swd.index is None:
            swd = torch.device("cuda", torch.cuda.current_device())
        if swd != inputs.device:
            raise ValueError(f"veloxseg_amd sliding window: windows are predicted where the inputs are ({inputs.device}), not on sw_device={sw_device}")
    masks = mirror_schedule(mirror_axes if mirror_axes is not None else ())
    inputs = inputs.contiguous().float()
    B, C = inputs.shape[:2]
    image_size_ = list(inputs.shape[2:])
    roi = tuple(int(r) if r else int(m) for r, m in zip(roi_size, image_size_))
    image_size = tuple(max(m, r) for m, r in zip(image_size_, roi))
    pad = []
    for k in range(4, 1, -1):
        diff = max(roi[k - 2] - inputs.shape[k], 0)
        pad.extend([diff // 2, diff - diff // 2])
    if any(pad):
        inputs = F.pad(inputs, pad=pad, mode="constant", value=cval).contiguous()
    iv = scan_interval(image_size, roi, overlap)
    starts = window_starts(image_size, roi, iv)
    patch = _valid_patch(image_size, roi)
    D, Hh, W = image_size
    rd, rh, rw = patch
    dev = inputs.device
    st = H.stream_ptr
    gauss = _blend_tables(starts, patch, image_size, sigma_scale, dev) if blend == "gaussian" else None
    if gauss is None:
        cz = _axis_counts(sorted({s[0] for s in starts}), rd, D, dev)
        cy = _axis_counts(sorted({s[1] for s in starts}), rh, Hh, dev)
        cx = _axis_counts(sorted({s[2] for s in starts}), rw, W, dev)
    num_win = len(starts)
    total = num_win * B
    acc = None
    K = None
    if len(masks) > 1:
        acc, K = _run_mirrored(inputs, predictor, starts, num_win, total, sw_batch_size, (B, C, D, Hh, W, rd, rh, rw), masks, gauss)
        total = 0                                           # (the plain path below has nothing left)
    if (SW_PIPELINE and hasattr(predictor, "forward_slot") and total >= 2 * sw_batch_size and total % sw_batch_size == 0):
        done = _pipelined(inputs, predictor, starts, num_win, total, sw_batch_size, (C, D, Hh, W), (rd, rh, rw), gauss)
        if done is not None:
            acc, K = done
            total = 0                                       # (every window batch is in; the loop below has nothing left)
    for g in range(0, total, sw_batch_size):
        idxs = range(g, min(g + sw_batch_size, total))
        win = torch.empty((len(idxs), C, rd, rh, rw), device=dev, dtype=torch.float32)
        for k, i in enumerate(idxs):
            z0, y0, x0 = starts[i % num_win]
            H.call("vx_sw_extract", H.P(inputs[i // num_win]), H.P(win[k]), C, D, Hh, W, rd, rh, rw, z0, y0, x0, st())
        prob = predictor(win)
        if isinstance(prob, (list, tuple)):
            prob = prob[0]
        prob = prob.contiguous().float()
        if acc is None:
            K = prob.shape[1]
            if tuple(prob.shape[2:]) != (rd, rh, rw):
                raise NotImplementedError("predictor output must have the window's spatial size")
            acc = torch.zeros((B, K, D, Hh, W), device=dev, dtype=torch.float32)
        for k, i in enumerate(idxs):
            _accumulate(prob[k], acc[i // num_win], K, (D, Hh, W), patch, starts[i % num_win], gauss, st())
    labels = torch.empty((B, 1, D, Hh, W), device=dev, dtype=torch.uint8) if return_labels else None
    for b in range(B):
        if gauss is None:
            H.call("vx_sw_finalize", H.P(acc[b]), H.P(acc[b]), H.P(labels[b], torch.uint8) if return_labels else None, H.P(cz), H.P(cy), H.P(cx),
                   K, D, Hh, W, st())
        else:
            H.call("vx_sw_blend_finalize", H.P(acc[b]), H.P(acc[b]), H.P(labels[b], torch.uint8) if return_labels else None, H.P(gauss.gc), gauss.floor,
                   H.P(gauss.tab, torch.int32), *gauss.strides, K, D, Hh, W, st())
    if any(pad):
        lo = [pad[4], pad[2], pad[0]]
        crop = (slice(None), slice(None)) + tuple(slice(l, l + m) for l, m in zip(lo, image_size_))
        acc = acc[crop]
        labels = labels[crop].contiguous() if return_labels else None
    if device is not None:
        acc = acc.to(device)
        labels = labels.to(device) if return_labels else None
    return (acc, labels) if return_labels else acc


def sliding_window_predict(inputs, predictor, roi_size, sw_batch_size, test_config, **kwargs):
    """reference signature (utils/inference_runtime.py:4-19): overlap comes from test_config["sliding_window"]["overlap"], and so does mirror_axes
    (test_config["sliding_window"]["mirror_axes"], optional) unless the keyword is given; likewise blend and sigma_scale (test_config["sliding_window"]["blend"],
    ["sigma_scale"], both optional)"""
    for key in ("blend", "sigma_scale"):
        if key not in kwargs and test_config["sliding_window"].get(key) is not None:
            kwargs[key] = test_config["sliding_window"][key]
    if "mirror_axes" not in kwargs and test_config["sliding_window"].get("mirror_axes") is not None:
        kwargs["mirror_axes"] = tuple(test_config["sliding_window"]["mirror_axes"])
    return sliding_window_inference(inputs, roi_size, sw_batch_size, predictor=predictor, overlap=test_config["sliding_window"]["overlap"], **kwargs)


class Net(torch.nn.Module):
    """forward = first output of the wrapped model (utils/inference_brats.py:41-53 without the Lightning / MONAI data plumbing)"""

    def __init__(self, model: torch.nn.Module):
        super().__init__()
        self._model = model

    def forward(self, x):
        out = self._model(x)
        return out[0] if isinstance(out, (list, tuple)) else out


@torch.inference_mode()
def infer_volume(model: torch.nn.Module, volume: torch.Tensor, roi_size: Sequence[int], sw_batch_size: int, overlap: float, taped: bool = True, postprocess=None,
                 mirror_axes: Sequence[int] = (), blend: str = "constant", sigma_scale=0.125, native=None):
    """eval-mode sliding-window segmentation of one (B, C, D, H, W) volume -> (blended logits, uint8 label map).
    postprocess (a utils.components.Postprocess, or the dict its from_config takes): the returned label map is the cleaned-up one (components below a voxel
    count dropped / the k largest kept, on the GPU); the returned logits are untouched.
    taped (default): the forward of a full window batch is captured once per model and replayed as a launch tape (engine.TapedPredictor); the result
    is the eager forward's (checked at capture).  The accumulator of the blending reads the predictor's static output before the next replay
    overwrites it (same stream).  The predictor hangs on the model object (no process-wide cache, nothing outlives the model) and re-captures
    when the parameters / buffers were re-homed since the capture (TrainEngine's flat buffer, .to(), a parameter swap): a tape bakes in raw
    device pointers.
    mirror_axes: mirror test-time augmentation (sliding_window_inference); mirrored windows have the window's shape and replay the same tape and replicas.
    blend, sigma_scale: constant or Gaussian importance blending (sliding_window_inference); the forwards, their tapes and replicas are the same for both.
    native: None (every launch is the one of the call without the keyword), or {"native_shape": (D, H, W), "native_spacing", "net_spacing"} for a volume that was
    resampled to the network's spacing (utils.preprocess.Spacingd): the returned label map is then on the image's OWN grid, (B, 1, *native_shape), formed from the
    blended logits by utils.preprocess.labels_on_native_grid (one kernel per batch item, no float volume on the native grid).  postprocess runs on those labels:
    its voxel-count thresholds are in NATIVE voxels.  The returned logits stay on the network grid, untouched.  A bad dict raises before any GPU work."""
    if native is not None:
        from .preprocess import check_native_geometry
        native = check_native_geometry(native)
    was_training = model.training
    model.eval()
    try:
        net = Net(model) if not isinstance(model, Net) else model
        net.eval()
        pred = net
        if taped and volume.is_cuda and os.environ.get("VELOXSEG_INFER_TAPE", "1") != "0":
            from ..engine import TapedPredictor
            pred = model.__dict__.get("_vx_taped_predictor")
            if pred is None:
                pred = TapedPredictor(net)
                model.__dict__["_vx_taped_predictor"] = pred       # plain attribute (not a sub-module): dies with the model
        out = sliding_window_inference(volume, roi_size, sw_batch_size, pred, overlap=overlap, return_labels=native is None, mirror_axes=mirror_axes, blend=blend,
                                       sigma_scale=sigma_scale)
        logits, labels = out if native is None else (out, None)
        if native is not None:
            from .preprocess import labels_on_native_grid
            labels = torch.stack([labels_on_native_grid(logits[b], native["native_shape"], native["net_spacing"], native["native_spacing"])
                                  for b in range(logits.shape[0])])[:, None]
        if postprocess is not None:
            from .components import Postprocess
            labels = (postprocess if isinstance(postprocess, Postprocess) else Postprocess.from_config(postprocess))(labels)
        return logits, labels
    finally:
        model.train(was_training)
