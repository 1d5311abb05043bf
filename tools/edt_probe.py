#!/usr/bin/env python3
"""Time of the exact distance transform (csrc/distance.hip) and of hd95 built on it, on 400 x 400 x 352 and 240 x 240 x 155, each figure as a
ratio to a device-to-device copy_ of the fp64 output measured in the same process.

Two site sets per shape: "balls" (about 50 balls of radius 3 - 12, the geometry of tools/morphology_probe.py; the sites are the balls' 6-connected surfaces, which
is what the surface metrics transform) and "corner" (one site at voxel (0, 0, 0): the worst case of the outward scan, every voxel of the x pass walks back to
x = 0).  Timed: the z pass alone, z + y, z + y + x = the whole transform (the y and x passes work in place on what the pass before left, so they are timed as
differences of these prefixes), the square root, and -- balls only -- hd95 end to end (two masks on the device in, one float out) against scipy.ndimage +
np.percentile with medpy's formula on the host, copies to the host included; the two results must be equal as floats.  Every figure: WINDOWS alternating
windows of 3 warm-up calls and the median of REPEATS single calls between two HIP events; the spread between the windows of one figure is what a difference has to
beat.  Every step runs in a fresh child process under its own time limit; the first one that fails or runs out of time ends the probe (nothing more is started on
the GPU).  A machine without a GPU fails; there is no fallback.

    python tools/edt_probe.py [--out profiles/rNN_edt_probe.json] [--no-scipy]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(400, 400, 352), (240, 240, 155)]
KINDS = ["balls", "corner"]
SPACING = (2.0364, 0.9766, 3.27)
STEP_LIMIT_S, WINDOWS = 280, 3


def _windows(fns, torch):
    """name -> {window medians, median of them, min / max over all windows}; the windows of the different figures alternate"""
    from components_probe import _time
    w = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            w[k].append(_time(fn, torch))
    return {k: {"window_median_ms": [t["median_ms"] for t in v], "median_ms": sorted(t["median_ms"] for t in v)[len(v) // 2], "min_ms": min(t["min_ms"] for t in v),
                "max_ms": max(t["max_ms"] for t in v)} for k, v in w.items()}


def _medpy_hd95(result, reference, spacing):
    """medpy 0.4's hd95 with scipy.ndimage on host arrays"""
    import numpy as np
    from scipy import ndimage

    def sd(a, b):
        fp = ndimage.generate_binary_structure(3, 1)
        ab, bb = a ^ ndimage.binary_erosion(a, structure=fp, iterations=1), b ^ ndimage.binary_erosion(b, structure=fp, iterations=1)
        return ndimage.distance_transform_edt(~bb, sampling=spacing)[ab]
    return float(np.percentile(np.hstack((sd(result, reference), sd(reference, result))), 95))


def run_step(kind, shape, use_scipy):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("edt_probe: no GPU")
    from components_probe import make_volume
    from veloxseg_amd import _hip as H
    from veloxseg_amd.utils import morphology as M
    from veloxseg_amd.utils.metric import surface as S
    dev = torch.device("cuda", 0)
    st = H.stream_ptr()
    if kind == "balls":
        lab = make_volume("balls", shape, torch, dev)
        sites = M.inner_boundary(M.pack(lab), 6)
    else:
        lab = torch.zeros(shape, dtype=torch.uint8, device=dev)
        lab[0, 0, 0] = 1
        sites = M.pack(lab)
    bits = sites.bits[0]
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    dst = torch.empty_like(out)
    one = lambda axis: H.call("vx_edt_pass", axis, bits.data_ptr(), 0, out.data_ptr(), *shape, SPACING[axis], st)
    t = _windows({"copy": lambda: dst.copy_(out), "z": lambda: one(0), "zy": lambda: (one(0), one(1)), "zyx": lambda: H.call("vx_edt_sq", bits.data_ptr(), 0, out.data_ptr(), *shape, *SPACING, st),
                  "sqrt": lambda: H.call("vx_edt_sqrt", dst.data_ptr(), dst.numel(), st)}, torch)
    copy = t["copy"]["median_ms"]
    res = {"kind": kind, "shape": list(shape), "spacing": list(SPACING), "sites": int(M.unpack(sites).sum()), "fp64_bytes": out.numel() * 8, "times": t,
           "ratio_to_copy": {"z": t["z"]["median_ms"] / copy, "y": (t["zy"]["median_ms"] - t["z"]["median_ms"]) / copy, "x": (t["zyx"]["median_ms"] - t["zy"]["median_ms"]) / copy,
                             "whole": t["zyx"]["median_ms"] / copy, "sqrt": t["sqrt"]["median_ms"] / copy}}
    if kind == "balls":
        other = torch.roll(lab, (3, -2, 4), (0, 1, 2))
        res["hd95_ms"] = _windows({"hd95": lambda: S.hd95(lab, other, SPACING)}, torch)["hd95"]
        res["hd95"] = S.hd95(lab, other, SPACING)
        if use_scipy:
            t0 = time.perf_counter()
            res["hd95_scipy"] = _medpy_hd95(lab.cpu().numpy() != 0, other.cpu().numpy() != 0, SPACING)
            res["hd95_scipy_s"] = time.perf_counter() - t0
            assert res["hd95"] == res["hd95_scipy"], f"hd95 {res['hd95']!r} on the device, {res['hd95_scipy']!r} with scipy on the host"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=str, default=None, help="(internal) run one step in this process: kind")
    ap.add_argument("--shape", type=int, nargs=3, default=None, help="(internal) the shape of that step")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step, tuple(a.shape), not a.no_scipy)
        return 0
    results = []
    for shape in SHAPES:
        for kind in KINDS:
            cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, "--shape", *map(str, shape)] + (["--no-scipy"] if a.no_scipy else [])
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
            except subprocess.TimeoutExpired:
                print(f"[probe] {kind} {shape}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
                return 2
            if r.returncode != 0:
                print(f"[probe] {kind} {shape}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                return 1
            res = json.loads(r.stdout.strip().splitlines()[-1])
            results.append(res)
            t, q = res["times"], res["ratio_to_copy"]
            print(f"{kind} {shape}: {res['sites']} sites, copy_ of fp64 {t['copy']['median_ms']:.3f} ms {[round(v, 3) for v in t['copy']['window_median_ms']]}", flush=True)
            for k in ("z", "zy", "zyx", "sqrt"):
                print(f"  {k:4s} {t[k]['median_ms']:9.3f} ms, windows {[round(v, 3) for v in t[k]['window_median_ms']]} [{t[k]['min_ms']:.3f} .. {t[k]['max_ms']:.3f}]", flush=True)
            print(f"  as copy_: z {q['z']:.2f}, y {q['y']:.2f}, x {q['x']:.2f}, whole transform {q['whole']:.2f}, sqrt {q['sqrt']:.2f}", flush=True)
            if "hd95_ms" in res:
                h = res["hd95_ms"]
                print(f"  hd95 end to end {h['median_ms']:.3f} ms, windows {[round(v, 3) for v in h['window_median_ms']]}; scipy on the host "
                      f"{res.get('hd95_scipy_s', float('nan')):.2f} s; value {res['hd95']!r}", flush=True)
            if a.out:
                with open(a.out, "w") as fh:
                    json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
