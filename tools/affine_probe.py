#!/usr/bin/env python3
"""Spatial augmentation timed at the workload's batch: B = 4 patches of 128^3 cut from 160 x 160 x 144 volumes, M = 2 fp32 modalities plus a float32 label per
patch (what CropForegroundd hands over), every patch firing.  The crop origins are fixed beforehand: finding them (the label rank-select) is common to all paths.

a. `old`: the path before RandAffined -- per patch and key one crop copy (`.contiguous()`, the statement RandCropByPosNegLabeld runs) and RandRotated's rotate_z
   launch: the unchanged classes.
b. `affine_z`: RandAffined with the same z-rotation range, on crop VIEWS, one call of vx_affine_batch.
c. `affine_full`: rotation about all three axes plus scale.
d. `affine_context`: (c) with context=True (the sampler reads the volume around the patch).
e. `copy`: a device copy_ of the bytes (a)-(d) read and write once: the streaming yardstick.
`*_kernel`: the kernel(s) alone, REPS back-to-back launches between device events on tables that are already on the device (for `old`: the rotate_z launches on
crops that are already copied).  Every path is warmed up, then the paths are timed alternately, ROUNDS times; every window ends in a device synchronise; all
rounds are printed, ratios use the medians, the spread of each path stands beside them.  Before anything is timed (b) is compared with (a): same angles, so the
two differ by rounding only.  Prints one JSON object; `--json FILE` also writes it.  Needs the GPU: there is nothing to time without one."""
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
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--modalities", type=int, default=2)
ap.add_argument("--size", type=int, default=128)
ap.add_argument("--volume", type=int, nargs=3, default=(160, 160, 144))
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("affine_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
B, M, S = args.batch, args.modalities, args.size
vol = tuple(args.volume)
patch = (S, S, S)
V = S ** 3
keys = [f"img{m}" for m in range(M)] + ["seg"]
modes = A.image_label_modes(M)
g = torch.Generator(device=dev).manual_seed(1)
# one volume per two patches, as the loader has it (num_samples = 2)
volumes = [dict({k: torch.randn((1,) + vol, generator=g, device=dev) for k in keys[:-1]}, seg=(torch.rand((1,) + vol, generator=g, device=dev) > 0.97).float())
           for _ in range((B + 1) // 2)]
rs = np.random.RandomState(2)
starts = [[int(rs.randint(0, v - S + 1)) for v in vol] for _ in range(B)]


def views():
    out = []
    for b, st in enumerate(starts):
        d = volumes[b // 2]
        out.append(dict({k: d[k][:, st[0]:st[0] + S, st[1]:st[1] + S, st[2]:st[2] + S] for k in keys}, crop_start=list(st), crop_source_shape=list(vol)))
    return out


RANGE = A.rotation_range_from_degrees(15.0)
old_rot = A.RandRotated(keys, range_z=RANGE, mode=modes, prob=1.0)
aff = {"affine_z": A.RandAffined(keys, prob=1.0, rotate_range=(0.0, 0.0, RANGE), mode=modes),
       "affine_full": A.RandAffined(keys, prob=1.0, rotate_range=(RANGE, RANGE, RANGE), scale_range=(0.1, 0.1, 0.1), mode=modes),
       "affine_context": A.RandAffined(keys, prob=1.0, rotate_range=(RANGE, RANGE, RANGE), scale_range=(0.1, 0.1, 0.1), mode=modes, context=True)}


def old():
    samples = [dict(d, **{k: d[k].contiguous() for k in keys}) for d in views()]
    return old_rot(samples)


# the same result before anything is timed: the z-rotation of (b) against (a) under the same angles
old_rot.set_random_state(7)
ref = old()
R = np.random.RandomState(7)
angles = []
for _ in range(B):
    R.rand()
    R.uniform(-0.0, 0.0)
    R.uniform(-0.0, 0.0)
    angles.append(float(R.uniform(-RANGE, RANGE)))
got = A.affine_sample([(d[k][0], A.affine_matrix(rotate=(0.0, 0.0, a)), m, "border", 0.0) for d, a in zip(views(), angles) for k, m in zip(keys, modes)], patch)
torch.cuda.synchronize()
worst, flips = 0.0, 0
for i, o in enumerate(got):
    r = ref[i // len(keys)][keys[i % len(keys)]][0]
    if keys[i % len(keys)] == "seg":
        flips += int((o != r).sum())                  # nearest: a coordinate that rounds differently by one fp32 ulp picks the other voxel
    else:
        worst = max(worst, float((o - r).abs().max()))
assert worst < 1e-3 and flips < 1e-4 * B * V, f"RandAffined (z only) and RandRotated disagree: max |diff| {worst}, {flips} label voxels"

# the kernels alone
tables, outs = {}, {}
for name, t in aff.items():
    t.set_random_state(3)
    ents = []
    for d in views():
        rot, tra, sca = t.draw()
        bounds = ([-s for s in d["crop_start"]], [p - 1 - s for p, s in zip(vol, d["crop_start"])])
        for k, m in zip(keys, modes):
            ents.append((d[k][0], A.affine_matrix(rot, sca, tra), m, "border", 0.0) + ((bounds,) if t.context else ()))
    table, outs[name], _ = A._affine_pack(ents, patch)
    tables[name] = table.to(dev)
crops = [d[k].contiguous() for d in views() for k in keys]
rot_out = [torch.empty_like(c) for c in crops]
moved = 2 * B * (M + 1) * V * 4
src_copy = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
dst_copy = torch.empty_like(src_copy)


def kernel(name):
    H.call("vx_affine_batch", tables[name].data_ptr(), B * (M + 1), *patch, H.stream_ptr())


def old_kernels():
    for i, (c, o) in enumerate(zip(crops, rot_out)):
        H.call("vx_rotate_z", c.data_ptr(), o.data_ptr(), 1, *patch, 0.9659258, 0.2588190, 0 if i % (M + 1) < M else 1, H.stream_ptr())


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


paths = {"old_us (crop copies + rotate_z per key)": (wall, old), "old_kernel_us (rotate_z launches alone)": (events, old_kernels)}
for name, t in aff.items():
    paths[f"{name}_us (draws, table, upload, kernel)"] = (wall, (lambda t=t: t(views())))
    paths[f"{name}_kernel_us"] = (events, (lambda name=name: kernel(name)))
paths["copy_us (copy_ of the bytes read + written once)"] = (events, lambda: dst_copy.copy_(src_copy))
for how, fn in paths.values():
    for _ in range(5):
        fn()
runs = {name: [] for name in paths}
for _ in range(args.rounds):
    for name, (how, fn) in paths.items():
        runs[name].append(how(fn))
med = {name: statistics.median(v) for name, v in runs.items()}
spread = {name: round((max(v) - min(v)) / med[name], 3) for name, v in runs.items()}
n = list(paths)
res = {"workload": f"B {B}, M {M} + label, {S}^3 patches from {vol} volumes, fp32, every patch firing, rotation range 15 degrees, scale 0.1", "reps_per_window": args.reps,
       "bytes_read_and_written_once": moved, "rounds": runs, "median_us": med, "spread (max - min) / median": spread,
       "launches": {"old": f"{B * (M + 1)} copies + {B * (M + 1)} rotate_z", "affine": "1 (+ one table upload)"},
       "z_only_against_rotate_z": {"max_abs_diff": worst, "label_voxels_that_differ": flips},
       "old_over_affine_z": round(med[n[0]] / med[n[2]], 3), "old_kernel_over_affine_z_kernel": round(med[n[1]] / med[n[3]], 3),
       "kernel_over_copy": {k: round(med[f"{k}_kernel_us"] / med[n[-1]], 3) for k in aff},
       "kernel_GBps": {k: round(moved / med[f"{k}_kernel_us"] / 1e3, 1) for k in aff}, "copy_GBps": round(moved / med[n[-1]] / 1e3, 1)}
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
