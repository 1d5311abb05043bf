#!/usr/bin/env python3
"""Bandwidth of the preprocessing kernels (csrc/preprocess.hip) on one 512 x 512 x 600 fp32 volume, each as a ratio to the device-to-device copy_ rate measured
in the same process.

Every step runs in a fresh child process under its own time limit; the first step that fails or runs out of time ends the probe (nothing more is started on the
GPU).  Per step: 3 warm-up calls, then REPEATS windows of CALLS back-to-back calls between two HIP events; the rate is the bytes the algorithm has to move (from
the shapes) over the median window, min / max windows give the spread.  A machine without a GPU fails; there is no fallback.

    python tools/preprocess_probe.py [--shape 512 512 600] [--out result.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ["moments_all", "moments_foreground", "normalize_apply", "normalize_apply_inplace", "histogram_ct_ties", "histogram_random", "histogram_refine_ct",
         "resample_trilinear", "resample_label_nearest"]
REPEATS, CALLS, STEP_LIMIT_S = 10, 10, 240


def _time(fn, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / CALLS)
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def run_step(step, shape):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("preprocess_probe: no GPU")
    from veloxseg_amd import _hip as H
    from veloxseg_amd.utils import preprocess as P
    dev = torch.device("cuda", 0)
    n = shape[0] * shape[1] * shape[2]
    g = torch.Generator(device=dev).manual_seed(5)
    ct = torch.randint(-1000, 2001, shape, generator=g, device=dev).float()
    ct[torch.rand(shape, generator=g, device=dev) < 0.6] = -1024.0             # CT: a few thousand distinct values, most voxels air
    rnd = torch.randn(shape, generator=g, device=dev) * 300.0
    st = H.stream_ptr()
    dst = torch.empty_like(ct)
    copy = _time(lambda: dst.copy_(ct), torch)
    copy_rate = 8.0 * n / (copy["median_ms"] * 1e-3)
    ws = torch.empty(H.query("vx_moments_ws_doubles"), dtype=torch.float64, device=dev)
    stats = torch.zeros(3, dtype=torch.float64, device=dev)
    hist = torch.zeros(2048, dtype=torch.int64, device=dev)
    mask = (ct > -500).to(torch.uint8)
    if step in ("moments_all", "moments_foreground"):
        thr = torch.full((1,), -1024.0, device=dev) if step == "moments_foreground" else None
        tp = None if thr is None else thr.data_ptr()
        nbytes, fn = 8.0 * n, lambda: H.call("vx_moments_stats", ct.data_ptr(), n, tp, ws.data_ptr(), stats.data_ptr(), st)          # two passes over x
    elif step in ("normalize_apply", "normalize_apply_inplace"):
        out = dst if step == "normalize_apply" else rnd
        src = ct if step == "normalize_apply" else rnd
        nbytes, fn = 8.0 * n, lambda: H.call("vx_normalize_apply", src.data_ptr(), out.data_ptr(), n, None, None, 3.0, 1.0001, 1, -1e30, 1e30, 0, 1e-8, st)
    elif step in ("histogram_ct_ties", "histogram_random"):
        x = ct if step == "histogram_ct_ties" else rnd
        nbytes, fn = 5.0 * n, lambda: H.call("vx_key_histogram", x.data_ptr(), mask.data_ptr(), 1, n, 0, 0, 11, hist.data_ptr(), None, None, st)
    elif step == "histogram_refine_ct":
        prefix = int(P.float_key([40.0])[0]) >> 21                              # a later round: only the voxels under one 11-bit prefix are counted
        nbytes, fn = 5.0 * n, lambda: H.call("vx_key_histogram", ct.data_ptr(), mask.data_ptr(), 1, n, prefix, 11, 11, hist.data_ptr(), None, None, st)
    elif step in ("resample_trilinear", "resample_label_nearest"):
        src_sp, dst_sp = (0.8, 0.8, 1.25), (1.0, 1.0, 1.0)
        mode = "bilinear" if step == "resample_trilinear" else "nearest"
        x = ct if mode == "bilinear" else mask
        so = P.output_shape(shape, src_sp, dst_sp)
        tabs = [P.axis_table(a, b, s, d, mode) for a, b, s, d in zip(shape, so, src_sp, dst_sp)]
        import numpy as np
        i0, i1, w = (torch.from_numpy(np.concatenate([t[k] for t in tabs])).to(dev) for k in range(3))
        out = torch.empty(so, dtype=x.dtype, device=dev)
        nbytes = float(x.element_size()) * (n + out.numel())                    # every input voxel read once, every output voxel written once
        if mode == "bilinear":
            fn = lambda: H.call("vx_resample_axes", x.data_ptr(), out.data_ptr(), 1, *shape, *so, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), 0, st)
        else:
            fn = lambda: H.call("vx_resample_axes_label", x.data_ptr(), out.data_ptr(), 1, 1, *shape, *so, i0.data_ptr(), st)
    else:
        raise SystemExit(f"unknown step {step}")
    t = _time(fn, torch)
    rate = nbytes / (t["median_ms"] * 1e-3)
    res = {"step": step, "shape": list(shape), "bytes": nbytes, **t, "GBps": rate / 1e9, "copy_GBps": copy_rate / 1e9, "copy_ms": copy,
           "ratio_to_copy": rate / copy_rate, "ratio_spread": [nbytes / (t["max_ms"] * 1e-3) / copy_rate, nbytes / (t["min_ms"] * 1e-3) / copy_rate]}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[512, 512, 600])
    ap.add_argument("--step", type=str, default=None, help="(internal) run one step in this process")
    ap.add_argument("--steps", type=str, nargs="*", default=STEPS)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step, tuple(a.shape))
        return 0
    results = []
    for step in a.steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--shape", *map(str, a.shape)]
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
        print(f"{step:28s} {res['GBps']:8.1f} GB/s  = {res['ratio_to_copy']:.2f} x copy_ ({res['copy_GBps']:.1f} GB/s)  "
              f"[{res['ratio_spread'][0]:.2f} .. {res['ratio_spread'][1]:.2f}]  median {res['median_ms']:.3f} ms", flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
