#!/usr/bin/env python3
"""Batch assembly with mirror, scale, shift (and noise) in one pass, timed at the workload's batch: B = 4 samples, M = 2 modalities, 128^3 patches, fp32 images and a
float32 label per sample (what the crop / rotation chain hands over), every transform firing.

1. `fused`: utils.augment.BatchAssembler -- the draws, the table, its upload and ONE call of vx_augment_batch (two launches: images, labels); without the noise step
   (the result the eager chain can reproduce: compared on bytes before anything is timed) and with it.
2. `eager`: the torch chain the same result needs without the kernel: per sample and key torch.flip, `*`, `+`; per sample torch.cat and .long() of the flipped label;
   per batch two torch.stack.
3. `kernel`: vx_augment_batch alone on a table that is already on the device, REPS back-to-back calls between device events, without and with noise.
4. `copy`: a device copy_ that moves the same number of bytes (read plus written) as the fused pass: the streaming floor of this device for that traffic.
Modes are warmed up, then timed alternately, ROUNDS times; every window ends in a device synchronise; all rounds are printed, ratios use the medians and the spread of
the eager rounds stands beside them.  Prints one JSON object; `--json FILE` also writes it.  Needs the GPU: there is nothing to time without one."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch

from veloxseg_amd import _hip as H
from veloxseg_amd.utils import augment as A

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--modalities", type=int, default=2)
ap.add_argument("--size", type=int, default=128)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("augment_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
B, M, S = args.batch, args.modalities, args.size
spatial = (S, S, S)
V = S ** 3
keys = [f"img{m}" for m in range(M)]
g = torch.Generator(device=dev).manual_seed(1)
samples = [dict({k: torch.randn((1,) + spatial, generator=g, device=dev) for k in keys}, seg=(torch.rand((1,) + spatial, generator=g, device=dev) > 0.97).float()) for _ in range(B)]
SCALE, SHIFT = 0.1, 0.1


def transforms(noise):
    ts = [A.RandFlipd(keys + ["seg"], prob=1.0, spatial_axis=a) for a in range(3)]
    ts += [A.RandScaleIntensityd(keys, (SCALE, SCALE), prob=1.0), A.RandShiftIntensityd(keys, (SHIFT, SHIFT), prob=1.0)]
    if noise:
        ts.append(A.RandGaussianNoised(keys, prob=1.0, std=0.1))
    return ts


asm = {n: A.BatchAssembler(keys, "seg", transforms(n)).set_random_state(3) for n in (False, True)}
s32 = torch.tensor(float(np.float32(1.0 + SCALE)), device=dev)
o32 = torch.tensor(float(np.float32(SHIFT)), device=dev)


def eager():
    xs, ys = [], []
    for d in samples:
        xs.append(torch.cat([torch.flip(d[k], (1, 2, 3)) * s32 + o32 for k in keys], 0))
        ys.append(torch.flip(d["seg"], (1, 2, 3)).long())
    return torch.stack(xs), torch.stack(ys)


EAGER_LAUNCHES = B * M * 3 + B * 3 + 2          # flip, mul, add per (sample, key); cat, label flip, .long() per sample; two stacks

# the same bytes before anything is timed
fx, fy = asm[False](samples)
ex, ey = eager()
assert torch.equal(fx.view(torch.int32), ex.view(torch.int32)) and torch.equal(fy, ey), "the fused pass and the eager chain disagree"

# the kernel alone: one table on the device, kept alive
captured = {}
launch = A._launch


def table_of(noise):
    def keep(entries, x_out, y_out, Bn, Mn, sp):
        captured["entries"] = entries
    A._launch = keep
    try:
        asm[noise](samples)
    finally:
        A._launch = launch
    return A._pack(captured["entries"]).to(dev)


tables = {n: table_of(n) for n in (False, True)}
x_out = torch.empty((B, M) + spatial, device=dev)
y_out = torch.empty((B, 1) + spatial, dtype=torch.int64, device=dev)
moved = B * M * V * 8 + B * V * (4 + 8)          # images: 4 bytes read + 4 written; label: 4 read + 8 written
src_copy = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
dst_copy = torch.empty_like(src_copy)


def kernel(noise):
    H.call("vx_augment_batch", tables[noise].data_ptr(), B * M, B, x_out.data_ptr(), y_out.data_ptr(), 8, B, M, *spatial, H.stream_ptr())


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000 / args.reps, 2)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e6 / args.reps, 2)


modes = {
    "fused_us (assembler call: draws, table, upload, kernel)": (wall, lambda: asm[False](samples)),
    "fused_with_noise_us": (wall, lambda: asm[True](samples)),
    "eager_us (flip, *, +, cat, stack, .long())": (wall, eager),
    "kernel_us (vx_augment_batch alone)": (events, lambda: kernel(False)),
    "kernel_with_noise_us": (events, lambda: kernel(True)),
    "copy_us (copy_ of the same bytes read + written)": (events, lambda: dst_copy.copy_(src_copy)),
}
for how, fn in modes.values():
    for _ in range(10):
        fn()
runs = {name: [] for name in modes}
for _ in range(args.rounds):
    for name, (how, fn) in modes.items():
        runs[name].append(how(fn))
med = {name: statistics.median(v) for name, v in runs.items()}
names = list(modes)
res = {"workload": f"B {B}, M {M}, {S}^3, fp32 images + float32 label per sample, every transform firing (3 flips, scale, shift)", "reps_per_window": args.reps,
       "bytes_read_and_written": moved, "rounds": runs, "median_us": med,
       "launches": {"fused": 2, "eager (by construction)": EAGER_LAUNCHES},
       "eager_over_fused": round(med[names[2]] / med[names[0]], 3), "eager_spread": round((max(runs[names[2]]) - min(runs[names[2]])) / med[names[2]], 3),
       "kernel_over_copy": round(med[names[3]] / med[names[5]], 3), "kernel_with_noise_over_copy": round(med[names[4]] / med[names[5]], 3),
       "kernel_GBps": round(moved / med[names[3]] / 1e3, 1), "kernel_with_noise_GBps": round(moved / med[names[4]] / 1e3, 1), "copy_GBps": round(moved / med[names[5]] / 1e3, 1)}
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
