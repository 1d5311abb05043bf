#!/usr/bin/env python3
"""Mirror test-time augmentation of the sliding-window inference, timed on the bench's sliding volume: (1, 4, 240, 240, 155), roi 128^3, overlap 0.5, sw_batch_size 2
(18 windows), the brats128 network with seeded random weights, utils.inference_runtime.infer_volume (taped, two window batches in flight).

1. Time per volume for mirror_axes (), (2,) and (0, 1, 2) -- n = 1, 2, 8 forwards per window -- and the ratio to n times the n = 1 time of the same process.  Every
   mode is warmed up first (tape capture, replicas, allocator); the modes are then timed alternately, ROUNDS times, each window ending in a device synchronise;
   all rounds are printed, the ratios use the medians.  Beside every mode, in the same alternation: the same volume with SW_PIPELINE = False (one window batch at a
   time instead of two in flight).
2. The three window movers of csrc/infer.hip alone on one window batch of that workload (2 windows, 4 channels / 4 classes, 128^3), REPS back-to-back launches
   between device events, beside a device-to-device copy_ that moves the same number of bytes (read + written): vx_sw_extract_mirror for the masks 0, 3 (D and H
   mirrored: rows move, groups do not), 4 (W mirrored: the lanes of every 16-byte group reversed) and 7; vx_sw_mirror_sum as store and as add; vx_sw_mirror_accumulate
   (one window per launch), and the existing vx_sw_extract / vx_sw_accumulate for comparison.
Prints one JSON object; `--json FILE` also writes it.  Needs the GPU: there is nothing to time without one."""
import argparse
import ctypes
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
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("tta_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
ROI, OVERLAP, SWB, REPS = (128, 128, 128), 0.5, 2, 20
MODES = [(), (2,), (0, 1, 2)]


def volumes():
    cfg, _ = WORKLOADS["brats128"]
    torch.manual_seed(12345)
    model = VeloxSeg(**cfg).to(dev).eval()
    vol = torch.randn(1, 4, 240, 240, 155, device=dev)

    def run(axes, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            IR.infer_volume(model, vol, ROI, SWB, OVERLAP, mirror_axes=axes)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    count = {}
    with torch.inference_mode():
        for axes in MODES:                                  # warm-up: captures, replicas, allocator; then a first estimate to size the timed windows
            run(axes, 2)
            count[axes] = max(3, int(args.seconds * 1e3 / run(axes, 3)))
        ms = {axes: [] for axes in MODES}
        seq = {axes: [] for axes in MODES}
        for _ in range(args.rounds):
            for axes in MODES:
                ms[axes].append(round(run(axes, count[axes]), 3))
                IR.SW_PIPELINE = False                      # one window batch after the other on the caller's stream (the same tape, no replica)
                try:
                    seq[axes].append(round(run(axes, count[axes]), 3))
                finally:
                    IR.SW_PIPELINE = True
    base = statistics.median(ms[()])
    out = {}
    for axes in MODES:
        n = 2 ** len(axes)
        med = statistics.median(ms[axes])
        out[f"mirror_axes={axes}"] = {"forwards_per_window": n, "volumes_per_window": count[axes], "ms_per_volume_rounds": ms[axes], "ms_per_volume_median": round(med, 3),
                                      "ratio_to_n_times_plain": round(med / (n * base), 4),
                                      "ms_per_volume_rounds_one_batch_at_a_time": seq[axes],
                                      "two_in_flight_over_one_at_a_time": round(med / statistics.median(seq[axes]), 4)}
    return out


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


def movers():
    C = K = 4
    D, Hh, W = 240, 240, 155
    rd, rh, rw = ROI
    per = rd * rh * rw
    vol = torch.randn(1, C, D, Hh, W, device=dev)
    win = torch.empty(SWB, C, rd, rh, rw, device=dev)
    pred, wsum = torch.randn(SWB, K, rd, rh, rw, device=dev), torch.zeros(SWB, K, rd, rh, rw, device=dev)
    acc = torch.zeros(K, D, Hh, W, device=dev)
    rows = [(0, 0, 0, 0), (0, 56, 56, 27)]               # (x0 = 27: the clamped last window of the 155-voxel axis; W = 155 -- this workload takes the scalar path)
    tab = (ctypes.c_int * 8)(*[v for r in rows for v in r])
    st = H.stream_ptr()
    z0, y0, x0 = rows[1][1:]
    calls = {}
    for mask in (0, 3, 4, 7):
        calls[f"vx_sw_extract_mirror mask {mask} ({SWB} windows, one launch)"] = (
            lambda mask=mask: H.call("vx_sw_extract_mirror", H.P(vol), H.P(win), ctypes.addressof(tab), SWB, mask, 1, C, D, Hh, W, rd, rh, rw, st), 2 * SWB * C * per * 4)
    calls[f"vx_sw_extract ({SWB} windows, {SWB} launches)"] = (
        lambda: [H.call("vx_sw_extract", H.P(vol[0]), H.P(win[k]), C, D, Hh, W, rd, rh, rw, *rows[k][1:], st) for k in range(SWB)], 2 * SWB * C * per * 4)
    for mask in (0, 4, 7):
        calls[f"vx_sw_mirror_sum store mask {mask}"] = (lambda mask=mask: H.call("vx_sw_mirror_sum", H.P(pred), H.P(wsum), SWB * K, rd, rh, rw, mask, 1, st), 2 * SWB * K * per * 4)
        calls[f"vx_sw_mirror_sum add mask {mask}"] = (lambda mask=mask: H.call("vx_sw_mirror_sum", H.P(pred), H.P(wsum), SWB * K, rd, rh, rw, mask, 0, st), 3 * SWB * K * per * 4)
        calls[f"vx_sw_mirror_accumulate mask {mask} (one window)"] = (
            lambda mask=mask: H.call("vx_sw_mirror_accumulate", H.P(pred[1]), H.P(wsum[1]), H.P(acc), K, D, Hh, W, rd, rh, rw, z0, y0, x0, mask, 0.0, st), 4 * K * per * 4)
    calls["vx_sw_accumulate (one window)"] = (lambda: H.call("vx_sw_accumulate", H.P(pred[1]), H.P(acc), K, D, Hh, W, rd, rh, rw, z0, y0, x0, 0.0, st), 3 * K * per * 4)
    out = {}
    for name, (fn, nbytes) in calls.items():
        a = torch.randn(nbytes // 8, device=dev)           # a copy_ of nbytes / 2 reads and writes nbytes
        b = torch.empty_like(a)
        us, cp = timed(fn), timed(lambda: b.copy_(a))
        out[name] = {"us_per_call": us, "bytes_read_and_written": nbytes, "copy_us_same_bytes": cp, "ratio_to_copy": round(statistics.median(us) / statistics.median(cp), 2)}
        del a, b
    return out


res = {"workload": "volume (1, 4, 240, 240, 155), roi 128^3, overlap 0.5, sw_batch_size 2, 18 windows, brats128 network (seeded random weights), fp32",
       "volume": volumes(), "movers": movers()}
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
