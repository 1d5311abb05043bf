#!/usr/bin/env python3
"""Gaussian importance blending of the sliding-window inference, timed on the bench's sliding volume: (1, 4, 240, 240, 155), overlap 0.5, sw_batch_size 2, roi 128^3
(18 windows, the brats128 network) and roi 96^3 (48 windows, brats96), seeded random weights, utils.inference_runtime.infer_volume (taped, two window batches in flight).

1. The kernels alone (csrc/infer.hip), REPS back-to-back launches between device events, three runs each, every new kernel next to the constant-blending one it stands
   in for, on the same window / volume, timed in turn in the same run: vx_sw_blend_accumulate (plain and mirrored, mask 0 and 7) beside vx_sw_accumulate and
   vx_sw_mirror_accumulate on the clamped last window of the volume (W = 155: the scalar path) and on a 16-byte-aligned volume (W = 160, x0 = 32: the four-voxel path);
   vx_sw_blend_finalize beside vx_sw_finalize on the whole volume with the window geometry of each roi.
2. Time per volume of infer_volume for blend = "constant" / "gaussian", without and with mirror_axes = (0, 1, 2), per roi: every mode warmed up first (tape capture,
   replicas, allocator), then the modes timed alternately, ROUNDS times, each window ending in a device synchronise; all rounds are printed, the ratios use the medians,
   and the spread of the constant mode's rounds stands beside them.
Prints one JSON object; `--json FILE` also writes it.  Needs the GPU: there is nothing to time without one."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from bench import WORKLOADS
from veloxseg_amd import _hip as H
from veloxseg_amd.model.VeloxSeg import VeloxSeg
from veloxseg_amd.utils import inference_runtime as IR

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--seconds", type=float, default=0.7, help="length of one timed window of a mode (the volume count is derived from the warm-up's time per volume)")
ap.add_argument("--rois", type=int, nargs="+", default=[128, 96])
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("blend_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
OVERLAP, SWB, REPS, SIGMA = 0.5, 2, 20, 0.125
VOLUME = (240, 240, 155)


def timed(fn):
    for _ in range(5):
        fn()
    runs = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(round(e0.elapsed_time(e1) * 1000 / REPS, 2))
    return runs


def pair(out, name, new, old, nbytes):
    """`old` (the constant-blending kernel) and `new` timed in turn: old, new, old"""
    a, n, b = timed(old), timed(new), timed(old)
    base = statistics.median(a + b)
    out[name] = {"bytes_read_and_written": nbytes, "constant_us": a + b, "gaussian_us": n, "ratio": round(statistics.median(n) / base, 3),
                 "constant_spread": round((max(a + b) - min(a + b)) / base, 3)}


def kernels(roi):
    K = 4
    r = (roi,) * 3
    per = roi ** 3
    out = {}
    st = H.stream_ptr()
    pred, wsum = torch.randn(K, *r, device=dev), torch.randn(K, *r, device=dev)
    for (D, Hh, W), origin, tag in ((VOLUME, (240 - roi, 240 - roi, 155 - roi), "W = 155, scalar path"), ((240, 240, 160), (240 - roi, 240 - roi, 32), "W = 160, four-voxel path")):
        acc = torch.zeros(K, D, Hh, W, device=dev)
        starts = IR.window_starts((D, Hh, W), r, IR.scan_interval((D, Hh, W), r, OVERLAP))
        b = IR._Blend(starts, r, (D, Hh, W), (SIGMA,) * 3, dev)
        g, gc, tab = H.P(b.g), H.P(b.gc), H.P(b.tab, torch.int32)
        pair(out, f"accumulate, one window ({tag})",
             lambda: H.call("vx_sw_blend_accumulate", H.P(pred), None, H.P(acc), g, b.floor, K, D, Hh, W, *r, *origin, 0, 1.0, st),
             lambda: H.call("vx_sw_accumulate", H.P(pred), H.P(acc), K, D, Hh, W, *r, *origin, 1.0, st), 3 * K * per * 4)
        for mask in (0, 7):
            pair(out, f"mirrored accumulate mask {mask}, one window ({tag})",
                 lambda: H.call("vx_sw_blend_accumulate", H.P(pred), H.P(wsum), H.P(acc), g, b.floor, K, D, Hh, W, *r, *origin, mask, 0.125, st),
                 lambda: H.call("vx_sw_mirror_accumulate", H.P(pred), H.P(wsum), H.P(acc), K, D, Hh, W, *r, *origin, mask, 0.125, st), 4 * K * per * 4)
        cz, cy, cx = (IR._axis_counts(sorted({s[a] for s in starts}), roi, m, dev) for a, m in enumerate((D, Hh, W)))
        labels = torch.empty(D, Hh, W, device=dev, dtype=torch.uint8)
        acc.normal_()
        dst = torch.empty_like(acc)
        pair(out, f"finalize, whole volume, {len(starts)} windows ({tag})",
             lambda: H.call("vx_sw_blend_finalize", H.P(acc), H.P(dst), H.P(labels, torch.uint8), gc, b.floor, tab, *b.strides, K, D, Hh, W, st),
             lambda: H.call("vx_sw_finalize", H.P(acc), H.P(dst), H.P(labels, torch.uint8), H.P(cz), H.P(cy), H.P(cx), K, D, Hh, W, st), (2 * K * 4 + 1) * D * Hh * W)
        del acc, dst
    return out


def volumes(roi):
    cfg, _ = WORKLOADS["brats128" if roi == 128 else "brats96"]
    torch.manual_seed(12345)
    model = VeloxSeg(**cfg).to(dev).eval()
    vol = torch.randn(1, 4, *VOLUME, device=dev)
    modes = [(axes, blend) for axes in ((), (0, 1, 2)) for blend in ("constant", "gaussian")]

    def run(mode, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            IR.infer_volume(model, vol, (roi,) * 3, SWB, OVERLAP, mirror_axes=mode[0], blend=mode[1], sigma_scale=SIGMA)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    count, ms = {}, {m: [] for m in modes}
    with torch.inference_mode():
        for m in modes:
            run(m, 2)
            count[m] = max(3, int(args.seconds * 1e3 / run(m, 3)))
        for _ in range(args.rounds):
            for m in modes:
                ms[m].append(round(run(m, count[m]), 3))
    out = {}
    for axes in ((), (0, 1, 2)):
        c, g = ms[(axes, "constant")], ms[(axes, "gaussian")]
        base = statistics.median(c)
        out[f"mirror_axes={axes}"] = {"volumes_per_window": count[(axes, "constant")], "constant_ms_per_volume_rounds": c, "gaussian_ms_per_volume_rounds": g,
                                      "gaussian_over_constant": round(statistics.median(g) / base, 4), "constant_spread": round((max(c) - min(c)) / base, 4)}
    return out


res = {"workload": f"volume (1, 4, {', '.join(map(str, VOLUME))}), overlap {OVERLAP}, sw_batch_size {SWB}, sigma_scale {SIGMA}, brats128 / brats96 network (seeded random weights), fp32"}
for roi in args.rois:
    res[f"roi {roi}"] = {"kernels": kernels(roi), "volume": volumes(roi)}
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
