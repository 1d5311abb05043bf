#!/usr/bin/env python3
"""Time of vx_cc_label and vx_cc_tally (csrc/components.hip) on one 400 x 400 x 352 uint8 volume, each as a ratio to a device-to-device copy_ of an int32 tensor of
the same voxel count measured in the same process, with scipy.ndimage.label's time on the host beside it.

Two volumes: "balls" (about 50 balls of radius 3 - 12: a lesion mask) and "bernoulli" (each voxel set with probability 0.30: thousands of tiny components and,
above the percolation threshold of the wider connectivities, one giant one).  Every step runs in a fresh child process under its own time limit; the first step
that fails or runs out of time ends the probe (nothing more is started on the GPU).  Per step: 3 warm-up calls, then the median of REPEATS single calls between
two HIP events; min / max give the spread.  A machine without a GPU fails; there is no fallback.

    python tools/components_probe.py [--shape 400 400 352] [--out result.json] [--no-scipy]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOLUMES = ["balls", "bernoulli"]
CONNECTIVITIES = [6, 18, 26]
REPEATS, STEP_LIMIT_S = 20, 240


def _time(fn, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPEATS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def make_volume(kind, shape, torch, dev):
    g = torch.Generator(device=dev).manual_seed(5)
    if kind == "bernoulli":
        return (torch.rand(shape, generator=g, device=dev) < 0.30).to(torch.uint8)
    vol = torch.zeros(shape, dtype=torch.uint8, device=dev)
    cpu = torch.Generator().manual_seed(5)
    for _ in range(50):
        r = int(torch.randint(3, 13, (1,), generator=cpu))
        c = [int(torch.randint(r, n - r, (1,), generator=cpu)) for n in shape]
        ax = [torch.arange(-r, r + 1, device=dev) for _ in range(3)]
        ball = (ax[0][:, None, None] ** 2 + ax[1][None, :, None] ** 2 + ax[2][None, None, :] ** 2) <= r * r
        sl = tuple(slice(ci - r, ci + r + 1) for ci in c)
        vol[sl] |= ball.to(torch.uint8)
    return vol


def run_step(volume, shape, use_scipy):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("components_probe: no GPU")
    from veloxseg_amd import _hip as H
    dev = torch.device("cuda", 0)
    V = shape[0] * shape[1] * shape[2]
    lab = make_volume(volume, shape, torch, dev)
    st = H.stream_ptr()
    cc = torch.empty(shape, dtype=torch.int32, device=dev)
    dst = torch.empty_like(cc)
    copy = _time(lambda: dst.copy_(cc), torch)
    ws = torch.empty((H.query("vx_cc_ws_bytes", *shape) + 7) // 8, dtype=torch.int64, device=dev)
    num = torch.zeros(1, dtype=torch.int32, device=dev)
    res = {"volume": volume, "shape": list(shape), "foreground": float(lab.float().mean()), "copy_ms": copy, "label": {}, "tally": {}, "scipy_s": {}}
    for c in CONNECTIVITIES:
        fn = lambda: H.call("vx_cc_label", lab.data_ptr(), 1, cc.data_ptr(), *shape, c, ws.data_ptr(), num.data_ptr(), st)
        t = _time(fn, torch)
        n = int(num.item())
        res["label"][str(c)] = {**t, "components": n, "ratio_to_copy": t["median_ms"] / copy["median_ms"]}
        sizes = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        hits = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        t = _time(lambda: H.call("vx_cc_tally", cc.data_ptr(), lab.data_ptr(), 1, V, n, sizes.data_ptr(), hits.data_ptr(), st), torch)
        res["tally"][str(c)] = {**t, "ratio_to_copy": t["median_ms"] / copy["median_ms"]}
        assert int(sizes[1:].sum()) == (3 + REPEATS) * int(lab.sum()), "tally lost voxels"
    if use_scipy:
        import numpy as np
        from scipy import ndimage
        host = lab.cpu().numpy()
        for c, rank in zip(CONNECTIVITIES, (1, 2, 3)):
            t0 = time.perf_counter()
            _, n = ndimage.label(host, structure=ndimage.generate_binary_structure(3, rank))
            res["scipy_s"][str(c)] = time.perf_counter() - t0
            assert n == res["label"][str(c)]["components"], f"scipy counts {n} components, the kernel {res['label'][str(c)]['components']}"
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=[400, 400, 352])
    ap.add_argument("--step", type=str, default=None, help="(internal) run one volume in this process")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step, tuple(a.shape), not a.no_scipy)
        return 0
    results = []
    for volume in VOLUMES:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", volume, "--shape", *map(str, a.shape)] + (["--no-scipy"] if a.no_scipy else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f"[probe] {volume}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
            return 2
        if r.returncode != 0:
            print(f"[probe] {volume}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
            return 1
        res = json.loads(r.stdout.strip().splitlines()[-1])
        results.append(res)
        print(f"{volume} ({100 * res['foreground']:.1f} % foreground), copy_ of int32 {res['copy_ms']['median_ms']:.3f} ms", flush=True)
        for c in map(str, CONNECTIVITIES):
            lb, ty = res["label"][c], res["tally"][c]
            print(f"  connectivity {c:2s}: {lb['components']:8d} components  label {lb['median_ms']:8.3f} ms = {lb['ratio_to_copy']:6.2f} x copy_ [{lb['min_ms']:.3f} .. {lb['max_ms']:.3f}]"
                  f"   tally {ty['median_ms']:7.3f} ms = {ty['ratio_to_copy']:5.2f} x copy_   scipy {res['scipy_s'].get(c, float('nan')):.2f} s", flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(results, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
