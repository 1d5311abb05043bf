#!/usr/bin/env python3
"""Elastic deformation timed at the workload's batch: B = 4 patches of 128^3 cut from 160 x 160 x 144 volumes, M = 2 fp32 modalities plus a
float32 label per patch, every patch firing -- the geometry of tools/affine_probe.py.  Three steps, each in a fresh child process under its own time limit; the first
one that fails or runs out of time ends the probe (nothing more is started on the GPU).  A machine without a GPU fails; there is no fallback.

  batch   vx_elastic_batch alone (tables already on the device) with a field per patch and with none, against vx_affine_batch on the same matrices (rotation about
          three axes plus scale), and a device copy_ of the bytes the affine pass reads and writes once.
  field   vx_elastic_noise and each pass of the smoothing (vx_elastic_smooth_pass: W, H, D) for the B fields, as
          multiples of a device copy_ of the field's bytes (B x 3 x 128^3 floats), at sigma 5 (tail 15) and sigma 13 (tail 39); vx_elastic_smooth as a whole.
  host    the wall time of one Rand3DElasticd call on the list of patches (draws, tables, one upload, five launches) against one RandAffined call.
Every figure: WINDOWS alternating windows of 3 warm-up calls and the median of REPEATS single calls between two HIP events (wall clock with a device synchronise for
the host step); the spread between the windows of one figure is what a difference has to beat.

    python tools/elastic_probe.py [--out profiles/rNN_elastic_probe.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["batch", "field", "host"]
B, M, S, VOL = 4, 2, 128, (160, 160, 144)
STEP_LIMIT_S, WINDOWS, REPEATS = 240, 3, 15


def _time(fn, torch, wall=False):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        if wall:
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
            continue
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def _windows(fns, torch, wall=False):
    """name -> {window medians, median of them, min / max over all windows}; the windows of the different figures alternate"""
    w = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            w[k].append(_time(fn, torch, wall))
    return {k: {"window_median_ms": [round(t["median_ms"], 4) for t in v], "median_ms": round(sorted(t["median_ms"] for t in v)[len(v) // 2], 4),
                "min_ms": round(min(t["min_ms"] for t in v), 4), "max_ms": round(max(t["max_ms"] for t in v), 4)} for k, v in w.items()}


def run_step(step):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("elastic_probe: no GPU")
    from veloxseg_amd import _hip as H
    from veloxseg_amd.utils import augment as A
    dev = torch.device("cuda", 0)
    patch, V = (S, S, S), S ** 3
    keys = [f"img{m}" for m in range(M)] + ["seg"]
    modes = A.image_label_modes(M)
    g = torch.Generator(device=dev).manual_seed(1)
    volumes = [dict({k: torch.randn((1,) + VOL, generator=g, device=dev) for k in keys[:-1]}, seg=(torch.rand((1,) + VOL, generator=g, device=dev) > 0.97).float())
               for _ in range((B + 1) // 2)]
    rs = np.random.RandomState(2)
    starts = [[int(rs.randint(0, v - S + 1)) for v in VOL] for _ in range(B)]

    def views():
        out = []
        for b, st in enumerate(starts):
            d = volumes[b // 2]
            out.append(dict({k: d[k][:, st[0]:st[0] + S, st[1]:st[1] + S, st[2]:st[2] + S] for k in keys}, crop_start=list(st), crop_source_shape=list(VOL)))
        return out
    RANGE = A.rotation_range_from_degrees(15.0)
    kw = dict(prob=1.0, rotate_range=(RANGE, RANGE, RANGE), scale_range=(0.1, 0.1, 0.1), mode=modes)
    st = H.stream_ptr()
    res = {"step": step, "workload": f"B {B}, M {M} + label, {S}^3 patches from {VOL} volumes, fp32, every patch firing, rotation range 15 degrees, scale 0.1"}
    if step == "batch":
        fields = A.elastic_field(patch, list(range(11, 11 + B)), [5.0] * B)
        t = A.RandAffined(keys, **kw).set_random_state(3)
        aff, ela, none = [], [], []
        for d, f in zip(views(), fields):
            rot, tra, sca = t.draw()
            m = A.affine_matrix(rot, sca, tra)
            for k, mode in zip(keys, modes):
                aff.append((d[k][0], m, mode, "border", 0.0))
                ela.append(aff[-1] + (f, 150.0))
                none.append(aff[-1] + (None, 0.0))
        ta, oa, _ = A._affine_pack(aff, patch)
        ta = ta.to(dev)
        te, oe, _ = A._elastic_pack(ela, patch, None)
        tn, on, _ = A._elastic_pack(none, patch, None)
        te, tn = (torch.from_numpy(x.view(np.uint8).reshape(-1)).to(dev) for x in (te, tn))
        moved = 2 * B * (M + 1) * V * 4
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        n = B * (M + 1)
        times = _windows({"copy": lambda: dst.copy_(src), "affine": lambda: H.call("vx_affine_batch", ta.data_ptr(), n, *patch, st),
                          "elastic_no_field": lambda: H.call("vx_elastic_batch", tn.data_ptr(), n, *patch, st),
                          "elastic": lambda: H.call("vx_elastic_batch", te.data_ptr(), n, *patch, st)}, torch)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(oa, on)), "vx_elastic_batch without a field differs from vx_affine_batch"
        c = times["copy"]["median_ms"]
        res.update(times=times, bytes_read_and_written_once=moved, field_bytes_read=B * 3 * V * 4,
                   largest_displacement_voxels=round(150.0 * float(fields.abs().max()), 3),
                   ratios={"elastic_over_affine": round(times["elastic"]["median_ms"] / times["affine"]["median_ms"], 3),
                           "elastic_no_field_over_affine": round(times["elastic_no_field"]["median_ms"] / times["affine"]["median_ms"], 3),
                           "affine_over_copy": round(times["affine"]["median_ms"] / c, 3), "elastic_over_copy": round(times["elastic"]["median_ms"] / c, 3)})
    elif step == "field":
        planes, other = torch.empty((B, 3) + patch, device=dev), torch.empty((B, 3) + patch, device=dev)
        keys_t = torch.arange(11, 11 + B, dtype=torch.int64, device=dev)
        H.call("vx_elastic_noise", keys_t.data_ptr(), 3 * B, V, planes.data_ptr(), st)
        fns = {"copy": lambda: other.copy_(planes), "noise": lambda: H.call("vx_elastic_noise", keys_t.data_ptr(), 3 * B, V, other.data_ptr(), st)}
        tables = {}
        for sigma in (5.0, 13.0):
            w = A.elastic_weights(sigma)
            wt = np.zeros(B, dtype=A._ELW)
            wt["tail"], wt["w"][:, :w.size] = w.size - 1, w
            tables[sigma] = torch.from_numpy(wt.view(np.uint8).reshape(-1)).to(dev)
            for axis, name in ((2, "W"), (1, "H"), (0, "D")):
                fns[f"sigma{int(sigma)}_{name}"] = (
                    lambda sigma=sigma, axis=axis: H.call("vx_elastic_smooth_pass", tables[sigma].data_ptr(), 3 * B, planes.data_ptr(), other.data_ptr(), axis, *patch, st))
        times = _windows(fns, torch)
        # the whole call last: it leaves its H pass in `planes`
        times.update(_windows({f"sigma{int(s)}_smooth": (lambda s=s: H.call("vx_elastic_smooth", tables[s].data_ptr(), 3 * B, planes.data_ptr(), other.data_ptr(), *patch, st))
                               for s in tables}, torch))
        c = times["copy"]["median_ms"]
        res.update(times=times, field_bytes=B * 3 * V * 4, as_copy={k: round(v["median_ms"] / c, 3) for k, v in times.items() if k != "copy"},
                   copy_GBps=round(2 * B * 3 * V * 4 / c / 1e6, 1))
    else:
        ela = A.Rand3DElasticd(keys, (5.0, 13.0), (100.0, 200.0), **kw).set_random_state(3)
        aff = A.RandAffined(keys, **kw).set_random_state(3)
        ctx_e = A.Rand3DElasticd(keys, (5.0, 13.0), (100.0, 200.0), context=True, **kw).set_random_state(3)
        ctx_a = A.RandAffined(keys, context=True, **kw).set_random_state(3)
        times = _windows({"RandAffined": lambda: aff(views()), "Rand3DElasticd": lambda: ela(views()), "RandAffined_context": lambda: ctx_a(views()),
                          "Rand3DElasticd_context": lambda: ctx_e(views())}, torch, wall=True)
        res.update(times=times, what="wall time of one call on the list of patches, device synchronise included (draws, tables, upload, launches, kernels)",
                   ratios={"elastic_over_affine": round(times["Rand3DElasticd"]["median_ms"] / times["RandAffined"]["median_ms"], 3),
                           "elastic_over_affine_context": round(times["Rand3DElasticd_context"]["median_ms"] / times["RandAffined_context"]["median_ms"], 3)})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=str, default=None, help="(internal) run one step in this process")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step)
        return 0
    results = []
    for step in STEPS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"[probe] {step}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
            return 2
        if r.returncode != 0:
            print(f"[probe] {step}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        print(f"{step}:", flush=True)
        for k, t in res["times"].items():
            print(f"  {k:28s} {t['median_ms']:9.4f} ms, windows {t['window_median_ms']} [{t['min_ms']:.4f} .. {t['max_ms']:.4f}]", flush=True)
        for k in ("ratios", "as_copy"):
            if k in res:
                print(f"  {k}: {res[k]}", flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
