#!/usr/bin/env python3
"""Time the data movers of csrc/pwa.hip alone at the first two PWA levels of the headline network (autopet128, B = 4, M = 2: a 32^3 grid with 4^3 windows, one head of
4 channels, four scales; a 16^3 grid with 8^3 windows, two heads of 8 channels, two scales): vx_pwa_gather_all_fwd, vx_pwa_gather_all_bwd and vx_pwa_scatter_bwd_all_w,
20 back-to-back launches, three runs, microseconds per call.  Beside each: the bytes the call has to move and that traffic at the device-to-device copy_ rate measured
here; then the scatter adjoint of every scale of a level alone (a plan of that one scale).  The scatter adjoint runs as one launch (vx_pwa_scatter_set_merged(2)), with
`--per-scale` as one launch per scale (vx_pwa_scatter_set_merged(0)); `--json FILE` writes the figures."""
import argparse, ctypes, json, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch
from veloxseg_amd import _hip as H

ap = argparse.ArgumentParser()
ap.add_argument("--per-scale", action="store_true")
ap.add_argument("--json", default=None)
args = ap.parse_args()
B, M, REPS, RUNS = 4, 2, 20, 3
dev = torch.device("cuda")


def timed(fn):
    for _ in range(5):
        fn()
    best = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(round(e0.elapsed_time(e1) * 1000 / REPS, 2))
    return best


def copy_rate():
    """bytes read + written per microsecond of a device-to-device copy_ of 64 MB (larger than the volumes of a level, smaller than the last-level cache: as they are in the step)"""
    a = torch.randn(16 << 20, device=dev)
    b = torch.empty_like(a)
    us = min(timed(lambda: b.copy_(a)))
    return 2 * a.numel() * 4 / us


def level(G, n, heads, c):
    scales = []
    s = 1
    while n * s <= G:
        scales.append(s)
        s *= 2
    nb = len(scales)
    plan = H.make_plan([G] * 3, [n] * 3, heads, [[s] * 3 for s in scales], [[G // (n * s)] * 3 for s in scales])
    pp, st = ctypes.addressof(plan), H.stream_ptr()
    src = [torch.randn(B, nb * heads * c, G, G, G, device=dev) for _ in range(3 * M)]
    dst = [torch.empty_like(t) for t in src]
    tok = [torch.empty(B, heads, plan.Ntot, M * plan.l, c, device=dev) for _ in range(3)]
    idx = [torch.zeros(t.shape, device=dev, dtype=torch.int32) for t in tok]
    arr = (ctypes.c_void_p * (3 * M))(*[H.P(t) for t in src])
    darr = (ctypes.c_void_p * (3 * M))(*[H.P(t) for t in dst])
    douts = (ctypes.c_void_p * 4)(*([H.P(t) for t in src[:M]] + [None] * (4 - M)))
    dtok = torch.empty_like(tok[0])
    vol = sum(t.numel() for t in src) * 4
    tokb = sum(t.numel() for t in tok) * 4
    pooled = tokb * (nb - 1) // nb                    # indices exist for the pooled scales only
    calls = {
        "gather_fwd": (lambda: H.call("vx_pwa_gather_all_fwd", ctypes.addressof(arr), *[H.P(t) for t in tok], *[H.P(t, torch.int32) for t in idx], pp, c, c, M, B, st), vol + tokb + pooled),
        "gather_bwd": (lambda: H.call("vx_pwa_gather_all_bwd", *[H.P(t) for t in tok], *[H.P(t, torch.int32) for t in idx], ctypes.addressof(darr), pp, c, c, M, B, st), vol + tokb + pooled),
        "scatter_bwd": (lambda: H.query("vx_pwa_scatter_bwd_all_w", ctypes.addressof(douts), H.P(dtok), pp, c, M, B, st), M * src[0].numel() * 4 + dtok.numel() * 4),
    }
    out = {}
    for name, (fn, nbytes) in calls.items():
        us = timed(fn)
        out[name] = {"us_per_call": us, "bytes": nbytes, "traffic_us_at_copy_rate": round(nbytes / RATE, 2)}
        print(f"grid {G}^3 n {n} heads {heads} c {c} ({nb} scales) {name}: {us} us per call, {nbytes / 1e6:.1f} MB = {nbytes / RATE:.1f} us at the copy_ rate", flush=True)
    return out


def scatter_scales(G, n, heads, c):
    """the scatter adjoint of each scale of a level alone (a plan of that one scale, vx_pwa_scatter_bwd_all: "+=" into the destination)"""
    out, s = {}, 1
    while n * s <= G:
        plan = H.make_plan([G] * 3, [n] * 3, heads, [[s] * 3], [[G // (n * s)] * 3])
        dout = [torch.randn(B, heads * c, G, G, G, device=dev) for _ in range(M)]
        douts = (ctypes.c_void_p * 4)(*([H.P(t) for t in dout] + [None] * (4 - M)))
        dtok = torch.zeros(B, heads, plan.Ntot, M * plan.l, c, device=dev)
        pp, st = ctypes.addressof(plan), H.stream_ptr()
        out[f"cells_{s}"] = timed(lambda: H.call("vx_pwa_scatter_bwd_all", ctypes.addressof(douts), H.P(dtok), pp, c, M, B, st))
        print(f"grid {G}^3 n {n} heads {heads} c {c} scatter_bwd, the {s}^3-cell scale alone: {out[f'cells_{s}']} us per call", flush=True)
        s *= 2
    return out


RATE = copy_rate()
print(f"device-to-device copy_: {RATE / 1e3:.0f} GB/s (read + written)", flush=True)
H.call("vx_pwa_scatter_set_merged", 0 if args.per_scale else 2)
res = {"copy_GBps": round(RATE / 1e3, 1), "scatter_adjoint": "per scale" if args.per_scale else "one launch",
       "level1": level(32, 4, 1, 4), "level2": level(16, 8, 2, 8),
       "level1_scatter_scales": scatter_scales(32, 4, 1, 4), "level2_scatter_scales": scatter_scales(16, 8, 2, 8)}
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
