#!/usr/bin/env python3
"""Blur, fixed-mean contrast and gamma in the batch assembly, timed at the workload's batch: B = 4 samples, M = 2 modalities, 128^3 patches, fp32
images and a float32 label per sample.  Cases: nothing firing (every new transform configured with prob 0: the one-pass form), blur only, contrast only, gamma with
retain_stats, everything (noise, blur, contrast, gamma with retain_stats); parameters are fixed (degenerate ranges) so that every window does the same work.

Per case:
1. `fused`: the BatchAssembler call on the host (draws, plan, table, one upload, the launches), wall time per call;
2. `kernels`: the device time of that call's C entries, by events around each of them (veloxseg_amd._hip.profile_begin / profile_end), summed over a call (the mean of KERNEL_CALLS calls per window);
3. `eager`: a torch restatement of the same transforms (three conv3d per channel with zero padding, amin / amax / mean / std, pow, cat / stack / .long()), compared with
   the fused result within twice the tests' bars (both sides lie within one bar of the fp64 value) before anything is timed;
4. `copy`: a device copy_ that moves the bytes the one-pass assembly reads and writes.
Modes are warmed up, then timed alternately, ROUNDS times; every window ends in a device synchronise; all rounds are printed, ratios use the medians, spreads stand beside
them.  Prints one JSON object; `--json FILE` also writes it.  Needs the GPU: there is nothing to time without one."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import torch.nn.functional as F

from veloxseg_amd import _hip as H
from veloxseg_amd.utils import augment as A

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--modalities", type=int, default=2)
ap.add_argument("--size", type=int, default=128)
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("augment_stats_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
B, M, S = args.batch, args.modalities, args.size
spatial = (S, S, S)
V = S ** 3
keys = [f"img{m}" for m in range(M)]
g = torch.Generator(device=dev).manual_seed(1)
samples = [dict({k: torch.randn((1,) + spatial, generator=g, device=dev) + 0.3 for k in keys}, seg=(torch.rand((1,) + spatial, generator=g, device=dev) > 0.97).float())
           for _ in range(B)]
SIGMA, FACTOR, GAMMA, U = 1.0, 0.25, 1.5, 2.0 ** -24
KERNEL_CALLS = 10          # assembler calls per kernel-time window


def transforms(blur, contrast, gamma, noise=0.0):
    return [A.RandGaussianNoised(keys, prob=noise, std=0.1), A.RandGaussianSmoothd(keys, sigma_x=SIGMA, sigma_y=SIGMA, sigma_z=SIGMA, prob=blur),
            A.RandScaleIntensityFixedMeand(keys, factors=(FACTOR, FACTOR), prob=contrast), A.RandAdjustContrastd(keys, prob=gamma, gamma=(GAMMA, GAMMA), retain_stats=True)]


CASES = {"nothing": (0.0, 0.0, 0.0), "blur": (1.0, 0.0, 0.0), "contrast": (0.0, 1.0, 0.0), "gamma_retain": (0.0, 0.0, 1.0), "everything": (1.0, 1.0, 1.0)}
asm = {n: A.BatchAssembler(keys, "seg", transforms(*c, noise=1.0 if n == "everything" else 0.0)).set_random_state(3) for n, c in CASES.items()}
w32 = torch.from_numpy(np.concatenate([A.gaussian_weights(SIGMA)[:0:-1], A.gaussian_weights(SIGMA)])).to(dev)
TAIL = (w32.numel() - 1) // 2


def e_blur(x):
    """x (1, D, H, W) -> blurred, three conv3d with zero padding, W then H then D"""
    y = x[None]
    y = F.conv3d(y, w32.view(1, 1, 1, 1, -1), padding=(0, 0, TAIL))
    y = F.conv3d(y, w32.view(1, 1, 1, -1, 1), padding=(0, TAIL, 0))
    y = F.conv3d(y, w32.view(1, 1, -1, 1, 1), padding=(TAIL, 0, 0))
    return y[0]


def e_contrast(x):
    m = x.mean()
    return (x - m) * float(np.float32(1.0 + FACTOR)) + m


def e_gamma(x):
    mn, mx, m1, s1 = x.amin(), x.amax(), x.mean(), x.std()
    r = mx - mn
    y = torch.pow((x - mn) / (r + 1e-7), GAMMA) * r + mn
    return (y - y.mean()) / (y.std() + 1e-8) * s1 + m1


def eager(case, noise_from=None):
    blur, contrast, gamma = CASES[case]
    xs, ys = [], []
    for b, d in enumerate(samples):
        chans = []
        for c, k in enumerate(keys):
            x = d[k] if noise_from is None else noise_from[b, c:c + 1]
            if blur:
                x = e_blur(x)
            if contrast:
                x = e_contrast(x)
            if gamma:
                x = e_gamma(x)
            chans.append(x)
        xs.append(torch.cat(chans, 0))
        ys.append(d["seg"].long())
    return torch.stack(xs), torch.stack(ys)


def bars(case, x):
    """twice the tests' bars, per channel, from the eager intermediates (tests/test_augment_stats_gpu.py: blur_bound, gamma_bar, retain_bar); a scalar per batch"""
    blur, contrast, gamma = CASES[case]
    bar = 0.0
    amax = float(x.abs().max())
    if blur:
        bar += 4.0 * (TAIL + 3) * U * amax
    if contrast:
        bar = bar * (1.0 + FACTOR) + 6.0 * U * amax * (1.0 + FACTOR)
    if gamma:
        r = float(x.amax() - x.amin())
        e = ((8.0 * max(GAMMA, 1.0) + 4.0) * r + 2.0 * amax) * U + bar * (1.0 + GAMMA) * 2.0
        bar = 8.0 * e + 64.0 * U * amax                    # retain: K and |z| are a few units on this data; the tests derive the factor per channel
    return 2.0 * bar


results = {}
for case in CASES:
    fx, fy = asm[case](samples)
    if case == "everything":                                   # the noise comes from the device generator: take it from a noise-only assembler with the same first seed
        nx, _ = A.BatchAssembler(keys, "seg", [A.RandGaussianNoised(keys, prob=1.0, std=0.1)]).set_random_state(3)(samples)
        fx, fy = A.BatchAssembler(keys, "seg", transforms(*CASES[case], noise=1.0)).set_random_state(3)(samples)
        ex, ey = eager(case, noise_from=nx)
    else:
        ex, ey = eager(case)
    err = float((fx - ex).abs().max())
    bar = bars(case, torch.stack([torch.cat([d[k] for k in keys], 0) for d in samples]))
    assert torch.equal(fy, ey) and (err <= bar if case != "nothing" else err == 0.0), f"{case}: the fused pass and the eager chain disagree: {err} > {bar}"
    results[case] = {"max_abs_difference_fused_vs_eager": err, "bar": bar}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e6 / args.reps, 2)


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(args.reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) * 1000 / args.reps, 2)


def kernels(case):
    """device time of the C entries of ONE assembler call, and the calls made"""
    torch.cuda.synchronize()
    H.profile_begin()
    for _ in range(KERNEL_CALLS):
        asm[case](samples)
    prof = H.profile_end()
    calls = {}
    for (name, _), (n, _) in prof.items():
        calls[name] = calls.get(name, 0) + n // KERNEL_CALLS
    return round(sum(ms for _, ms in prof.values()) * 1000 / KERNEL_CALLS, 2), calls


moved = B * M * V * 8 + B * V * (4 + 8)
src_copy = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
dst_copy = torch.empty_like(src_copy)
modes = {}
for case in CASES:
    modes[f"{case}: fused_us"] = (wall, lambda case=case: asm[case](samples))
    modes[f"{case}: kernels_us"] = (lambda fn: fn(), lambda case=case: kernels(case)[0])
    modes[f"{case}: eager_us"] = (wall, lambda case=case: eager(case))
modes["copy_us (copy_ of the bytes the one-pass assembly reads + writes)"] = (events, lambda: dst_copy.copy_(src_copy))
for how, fn in modes.values():
    for _ in range(3):
        fn()
runs = {name: [] for name in modes}
for _ in range(args.rounds):
    for name, (how, fn) in modes.items():
        runs[name].append(how(fn))
med = {name: statistics.median(v) for name, v in runs.items()}
spread = {name: round((max(v) - min(v)) / med[name], 3) for name, v in runs.items()}
copy = med[list(modes)[-1]]
for case in CASES:
    calls = kernels(case)[1]
    results[case].update({"calls": calls, "launches": sum({"vx_augment_stats": 2, "vx_blur_batch": 3}.get(n, 2) * c for n, c in calls.items()) - int("vx_blur_batch" in calls),
                          "fused_us": med[f"{case}: fused_us"], "kernels_us": med[f"{case}: kernels_us"], "eager_us": med[f"{case}: eager_us"],
                          "eager_over_fused": round(med[f"{case}: eager_us"] / med[f"{case}: fused_us"], 3), "kernels_over_copy": round(med[f"{case}: kernels_us"] / copy, 3)})
res = {"workload": f"B {B}, M {M}, {S}^3, fp32 images + float32 label per sample; sigma {SIGMA}, contrast factor {FACTOR}, gamma {GAMMA} with retain_stats",
       "reps_per_window": args.reps, "bytes_of_the_one_pass_assembly": moved, "copy_us": copy, "rounds": runs, "median_us": med, "window_spread": spread, "cases": results}
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
