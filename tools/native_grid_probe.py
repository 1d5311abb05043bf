#!/usr/bin/env python3
"""Label map on the image's own grid: the fused kernel (vx_native_argmax) beside the composition it replaces (vx_resample_axes to a (K, D, H, W) fp32 volume on the
native grid, then vx_argmax_channels), with the device-to-device copy_ of the same output bytes next to them, on one MI355X.

Every geometry runs in a fresh child process under its own time limit; the first one that fails or runs out of time ends the probe (nothing more is started on the
GPU).  Tables and outputs are allocated once; per variant: 3 warm-up calls, then REPEATS windows of CALLS back-to-back calls between two HIP events, median window
reported with the min / max windows; each side is timed twice, in turn.  The two label maps of one geometry must agree byte for byte, or the step fails.  Rates are
the bytes the algorithm has to move (from the shapes) over the median time.  A machine without a GPU fails; there is no fallback.

    python tools/native_grid_probe.py [--out result.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# name: (K, network shape, network spacing, native shape, native spacing)
GEOMETRIES = {
    "up_2mm_to_1mm": (2, (200, 200, 176), (2.0, 2.0, 2.0), (400, 400, 352), (1.0, 1.0, 1.0)),
    "identity_k4": (4, (240, 240, 155), (1.0, 1.0, 1.0), (240, 240, 155), (1.0, 1.0, 1.0)),
    "down_1mm_to_2mm": (2, (400, 400, 352), (1.0, 1.0, 1.0), (200, 200, 176), (2.0, 2.0, 2.0)),
}
REPEATS, CALLS, STEP_LIMIT_S = 10, 50, 120


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


def run_step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("native_grid_probe: no GPU")
    from veloxseg_amd import _hip as H
    from veloxseg_amd.utils import preprocess as P
    K, sp, s_net, so, s_nat = GEOMETRIES[name]
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(5)
    logits = torch.randn((K,) + sp, generator=g, device=dev) * 4.0
    v_net, v_nat = int(np.prod(sp)), int(np.prod(so))
    tabs = P.inverse_tables(sp, so, s_net, s_nat)
    i0, i1, w = (torch.from_numpy(np.concatenate([t[k] for t in tabs])).to(dev) for k in range(3))
    full = torch.empty((K,) + so, device=dev)                                          # the composition's fp32 volume on the native grid
    lab_c = torch.empty(so, dtype=torch.uint8, device=dev)
    lab_f = torch.empty(so, dtype=torch.uint8, device=dev)
    st = H.stream_ptr()

    def composition():
        H.call("vx_resample_axes", logits.data_ptr(), full.data_ptr(), K, *sp, *so, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), 0, st)
        H.call("vx_argmax_channels", full.data_ptr(), lab_c.data_ptr(), 1, K, v_nat, st)

    def fused():
        H.call("vx_native_argmax", logits.data_ptr(), lab_f.data_ptr(), K, *sp, *so, i0.data_ptr(), i1.data_ptr(), w.data_ptr(), st)

    src = torch.randint(0, K, so, generator=g, device=dev, dtype=torch.uint8)
    res = {"geometry": name, "K": K, "net_shape": list(sp), "native_shape": list(so),
           "bytes": {"copy": 2.0 * v_nat, "composition": 4.0 * K * v_net + 8.0 * K * v_nat + v_nat, "fused": 4.0 * K * v_net + v_nat}}
    for key, fn in (("copy", lambda: lab_c.copy_(src)), ("composition", composition), ("fused", fused), ("composition_again", composition), ("fused_again", fused)):
        res[key] = _time(fn, torch)
    torch.cuda.synchronize()
    if not torch.equal(lab_f, lab_c):
        raise SystemExit(f"native_grid_probe: {name}: the fused labels differ from the composition's")
    for key in ("copy", "composition", "fused"):
        res[key]["GBps"] = res["bytes"][key] / (res[key]["median_ms"] * 1e-3) / 1e9
    res["composition_over_fused"] = res["composition"]["median_ms"] / res["fused"]["median_ms"]
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=str, default=None, help="(internal) run one geometry in this process")
    ap.add_argument("--geometries", type=str, nargs="*", default=list(GEOMETRIES))
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step)
        return 0
    results = []
    for name in a.geometries:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"[probe] {name}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
            return 2
        if r.returncode != 0:
            print(f"[probe] {name}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        print(f"{name:18s} composition {res['composition']['median_ms']:.3f} ms ({res['composition']['GBps']:.0f} GB/s)  fused {res['fused']['median_ms']:.3f} ms "
              f"({res['fused']['GBps']:.0f} GB/s) [{res['fused']['min_ms']:.3f} .. {res['fused']['max_ms']:.3f}]  "
              f"copy_ {res['copy']['median_ms']:.3f} ms ({res['copy']['GBps']:.0f} GB/s)  composition / fused = {res['composition_over_fused']:.2f}  "
              f"(repeat: {res['composition_again']['median_ms']:.3f} / {res['fused_again']['median_ms']:.3f} ms)", flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
