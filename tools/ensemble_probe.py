#!/usr/bin/env python3
"""Ensemble inference (utils/ensemble.py, csrc/ensemble.hip), timed on the bench's sliding volume 240 x 240 x 155 with K = 2 and K = 4 classes.

1. The kernels alone, REPS back-to-back launches between device events, the modes timed in turn, ROUNDS rounds: vx_softmax_accumulate (first call: reads the logits,
   writes psum; later call: also reads psum) and vx_prob_finalize (labels; labels + entropy), each beside
   - the device-to-device copy_ that moves the same number of bytes (read plus written): the streaming floor of this device for that traffic, and
   - the torch eager chain a user would write instead: softmax, mul, add_ for the accumulation; argmax (+ the uint8 cast), and log, mul, sum, neg for the entropy.
2. Time per volume of an ensemble of N = 5 models on the (1, 4, 240, 240, 155) volume, roi 128^3, overlap 0.5, sw_batch_size 2 (brats128 network, seeded random weights,
   taped): five infer_volume calls alone (their logits dropped), infer_ensemble, and the five calls followed by the eager chain; every mode warmed up first (tape
   capture, replicas, allocator), then the modes timed alternately, ROUNDS times, each window ending in a device synchronise.
All rounds are printed; ratios use the medians, and the spread of the rounds stands beside them.  Prints one JSON object; `--json FILE` also writes it.
Needs the GPU: there is nothing to time without one."""
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
from veloxseg_amd.utils import ensemble as E
from veloxseg_amd.utils import inference_runtime as IR

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--seconds", type=float, default=0.7, help="length of one timed window of an ensemble mode")
ap.add_argument("--models", type=int, default=5)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("ensemble_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
VOLUME = (240, 240, 155)
V = VOLUME[0] * VOLUME[1] * VOLUME[2]
OVERLAP, SWB, ROI = 0.5, 2, (128, 128, 128)


def window(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000 / args.reps, 2)


def in_turn(modes):
    """{name: fn} -> {name: [us per call, one per round]}: every mode warmed up, then the modes timed one after the other, round by round"""
    for fn in modes.values():
        for _ in range(3):
            fn()
    runs = {k: [] for k in modes}
    for _ in range(args.rounds):
        for k, fn in modes.items():
            runs[k].append(window(fn))
    return runs


def summary(runs, kernel, nbytes):
    med = {k: statistics.median(v) for k, v in runs.items()}
    return {"bytes_read_and_written": nbytes, "us_rounds": runs, "median_us": med, "kernel_GBps": round(nbytes / med[kernel] / 1e3, 1),
            "kernel_over_copy": round(med[kernel] / med["copy"], 3), "eager_over_kernel": round(med["eager"] / med[kernel], 3),
            "spread": {k: round((max(v) - min(v)) / med[k], 3) for k, v in runs.items()}}


def kernels(K):
    st = H.stream_ptr()
    logits = torch.randn((1, K, V), device=dev) * 3
    psum = torch.empty((1, K, V), device=dev)
    labels = torch.empty((1, V), device=dev, dtype=torch.uint8)
    ent = torch.empty((1, V), device=dev)
    w = 0.2
    out = {}

    def copy_of(nbytes):
        a = torch.empty(nbytes // 2, device=dev, dtype=torch.uint8)
        b = torch.empty_like(a)
        return lambda: b.copy_(a)

    def eager_first():
        p = torch.softmax(logits, 1)
        p.mul_(w)
        return p

    def eager_add():
        p = torch.softmax(logits, 1)
        p.mul_(w)
        psum.add_(p)

    nb = 2 * K * V * 4
    out["accumulate, first call"] = summary(in_turn({"kernel": lambda: H.call("vx_softmax_accumulate", H.P(logits), H.P(psum), 1, K, V, w, 1, st),
                                                     "copy": copy_of(nb), "eager": eager_first}), "kernel", nb)
    nb = 3 * K * V * 4
    out["accumulate, later call"] = summary(in_turn({"kernel": lambda: H.call("vx_softmax_accumulate", H.P(logits), H.P(psum), 1, K, V, w, 0, st),
                                                     "copy": copy_of(nb), "eager": eager_add}), "kernel", nb)
    H.call("vx_softmax_accumulate", H.P(logits), H.P(psum), 1, K, V, 1.0, 1, st)          # a proper mean for the finalize
    nb = K * V * 4 + V
    out["finalize, labels"] = summary(in_turn({"kernel": lambda: H.call("vx_prob_finalize", H.P(psum), H.P(labels, torch.uint8), None, 1, K, V, st),
                                               "copy": copy_of(nb), "eager": lambda: psum.argmax(1).to(torch.uint8)}), "kernel", nb)

    def eager_both():
        lab = psum.argmax(1).to(torch.uint8)
        return lab, psum.log().mul_(psum).sum(1).neg_()
    nb = K * V * 4 + 5 * V
    out["finalize, labels + entropy"] = summary(in_turn({"kernel": lambda: H.call("vx_prob_finalize", H.P(psum), H.P(labels, torch.uint8), H.P(ent), 1, K, V, st),
                                                         "copy": copy_of(nb), "eager": eager_both}), "kernel", nb)
    return out


def volumes(n):
    cfg, _ = WORKLOADS["brats128"]
    models = []
    for i in range(n):
        torch.manual_seed(12345 + i)
        models.append(VeloxSeg(**cfg).to(dev).eval())
    vol = torch.randn(1, 4, *VOLUME, device=dev)
    w = E.normalise_weights(None, n)

    def alone():
        for m in models:
            IR.infer_volume(m, vol, ROI, SWB, OVERLAP)

    def ensemble():
        E.infer_ensemble(models, vol, ROI, SWB, OVERLAP, entropy=True)

    def eager():
        psum = None
        for m, wi in zip(models, w):
            p = torch.softmax(IR.infer_volume(m, vol, ROI, SWB, OVERLAP)[0], 1)
            p.mul_(wi)
            psum = p if psum is None else psum.add_(p)
        return psum.argmax(1, keepdim=True).to(torch.uint8), psum.log().mul_(psum).sum(1, keepdim=True).neg_()
    modes = {"n x infer_volume": alone, "infer_ensemble": ensemble, "n x infer_volume + eager chain": eager}

    def run(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    count, ms = {}, {k: [] for k in modes}
    with torch.inference_mode():
        for k, fn in modes.items():
            run(fn, 2)
            count[k] = max(3, int(args.seconds * 1e3 / run(fn, 3)))
        for _ in range(args.rounds):
            for k, fn in modes.items():
                ms[k].append(round(run(fn, count[k]), 3))
    med = {k: statistics.median(v) for k, v in ms.items()}
    base = med["n x infer_volume"]
    return {"models": n, "calls_per_window": count, "ms_per_ensemble_rounds": ms, "median_ms": med,
            "ensemble_over_n_infer_volume": round(med["infer_ensemble"] / base, 4), "eager_over_n_infer_volume": round(med["n x infer_volume + eager chain"] / base, 4),
            "ensemble_extra_ms_per_model": round((med["infer_ensemble"] - base) / n, 4), "eager_extra_ms_per_model": round((med["n x infer_volume + eager chain"] - base) / n, 4),
            "spread": {k: round((max(v) - min(v)) / med[k], 4) for k, v in ms.items()}}


res = {"workload": f"volume {VOLUME}, fp32; kernels on (1, K, {V}); ensemble: (1, 4, 240, 240, 155), roi 128^3, overlap {OVERLAP}, sw_batch_size {SWB}, brats128 network, seeded random weights"}
for K in (2, 4):
    res[f"K = {K}"] = kernels(K)
res["ensemble"] = volumes(args.models)
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
