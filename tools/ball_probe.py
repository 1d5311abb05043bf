#!/usr/bin/env python3
"""Time of the ball kernel (csrc/morphology.hip: vx_morph_ball), of the distance-transform route to the same bits and of the normalised surface
Dice built on them, on 240 x 240 x 155 and 400 x 400 x 352, isotropic 1 mm and the anisotropic spacing of tools/edt_probe.py.

Two masks per shape: "balls" (the 6-connected surfaces of about 50 balls of radius 3 - 12, the geometry of tools/morphology_probe.py: what the surface metrics
dilate) and "dense" (the solid balls' union with a 30 % Bernoulli field: many words are decided after a few rows).  Per mask and spacing, radii chosen so that the
element has about 7 / 33 / 123 / 515 / 2000 rows:
    ball        vx_morph_ball, dilation, border 0, no gate
    ball_gated  the same with a surface as gate (the mask rolled by (3, -2, 4): the other operand of a surface overlap)
    edt         the other route: vx_edt_sq, the comparison with q, vx_morph_pack
each as a multiple of a device-to-device copy_ of the packed mask and of the uint8 volume, measured in the same process.  Then, balls only, surface_overlap end
to end at 2 and 5 voxels of the finest spacing against the two-transform route (surface_distances twice, squared, compared with q and counted) and -- on the
smaller shape, or everywhere with --scipy-all -- against scipy.ndimage and the formula on the host; the counts must be equal.  Every figure: WINDOWS alternating
windows of 3 warm-up calls and the median of REPEATS single calls between two HIP events.  Every step runs in a fresh child process under its own time limit; the
first one that fails or runs out of time ends the probe (nothing more is started on the GPU).  A machine without a GPU fails; there is no fallback.

    python tools/ball_probe.py [--out profiles/rNN_ball_probe.json] [--no-scipy] [--scipy-all]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(240, 240, 155), (400, 400, 352)]
KINDS = ["balls", "dense"]
SPACINGS = {"iso": (1.0, 1.0, 1.0), "aniso": (2.0364, 0.9766, 3.27)}
ROW_TARGETS = (7, 33, 123, 515, 2000)
NSD_VOXELS = (2.0, 5.0)
STEP_LIMIT_S, WINDOWS = 280, 3


def _windows(fns, torch):
    from components_probe import _time
    w = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            w[k].append(_time(fn, torch))
    return {k: {"window_median_ms": [t["median_ms"] for t in v], "median_ms": sorted(t["median_ms"] for t in v)[len(v) // 2], "min_ms": min(t["min_ms"] for t in v),
                "max_ms": max(t["max_ms"] for t in v)} for k, v in w.items()}


def radius_for(rows, spacing, M):
    """the smallest radius, in steps of a tenth of the finest spacing, whose element has at least `rows` rows"""
    step, k = min(spacing) / 10.0, 0
    while True:
        el = M.BallElement(k * step, spacing)
        if el.n_rows is None or el.n_rows >= rows:
            return k * step
        k += 1 if rows < 100 else 5


def _host_counts(a, b, tau, spacing):
    import numpy as np
    from scipy import ndimage

    def sd(x, y):
        fp = ndimage.generate_binary_structure(3, 1)
        xb, yb = x ^ ndimage.binary_erosion(x, structure=fp, iterations=1), y ^ ndimage.binary_erosion(y, structure=fp, iterations=1)
        return ndimage.distance_transform_edt(~yb, sampling=spacing)[xb]
    ab, ba = sd(a, b), sd(b, a)
    return [int(np.sum(ab <= tau)), len(ab), int(np.sum(ba <= tau)), len(ba)]


def run_step(kind, shape, spacing_name, use_scipy):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ball_probe: no GPU")
    from components_probe import make_volume
    from veloxseg_amd import _hip as H
    from veloxseg_amd.utils import morphology as M
    from veloxseg_amd.utils.metric import surface as S
    dev = torch.device("cuda", 0)
    spacing = SPACINGS[spacing_name]
    lab = make_volume("balls", shape, torch, dev)
    other = torch.roll(lab, (3, -2, 4), (0, 1, 2))
    gate = M.inner_boundary(M.pack(other), 6)
    if kind == "balls":
        mask = M.inner_boundary(M.pack(lab), 6)
    else:
        mask = M.pack(lab | make_volume("bernoulli", shape, torch, dev))
    u8 = M.unpack(mask)
    bits_dst, u8_dst = torch.empty_like(mask.bits), torch.empty_like(u8)
    fns = {"copy_bits": lambda: bits_dst.copy_(mask.bits), "copy_u8": lambda: u8_dst.copy_(u8)}
    elements = {}
    for target in ROW_TARGETS:
        el = M.BallElement(radius_for(target, spacing, M), spacing)
        el.rows(dev)
        elements[target] = el
        fns[f"ball_{target}"] = lambda el=el: M._ball_kernel(mask, el, 0, 0)
        fns[f"ball_gated_{target}"] = lambda el=el: M._ball_kernel(mask, el, 0, 0, gate)
        fns[f"edt_{target}"] = lambda el=el: M._ball_edt(mask, el, 0, 0)
    t = _windows(fns, torch)
    for target, el in elements.items():                      # the two routes give the same bits
        assert torch.equal(M._ball_kernel(mask, el, 0, 0).bits, M._ball_edt(mask, el, 0, 0).bits), f"ball and edt differ at {target} rows"
    cb, cu = t["copy_bits"]["median_ms"], t["copy_u8"]["median_ms"]
    res = {"kind": kind, "shape": list(shape), "spacing": list(spacing), "set_voxels": int(u8.sum()), "words": mask.bits.numel(), "times": t,
           "elements": {str(k): {"radius": el.radius, "radii": list(el.radii), "rows": el.n_rows} for k, el in elements.items()},
           "as_copy_bits": {k: v["median_ms"] / cb for k, v in t.items()}, "as_copy_u8": {k: v["median_ms"] / cu for k, v in t.items()}}
    if kind == "balls":
        def two_transforms(tau):
            q = M.sq_threshold(tau)
            ab, ba = S.surface_distances(lab, other, spacing, squared=True), S.surface_distances(other, lab, spacing, squared=True)
            return torch.stack([(ab <= q).sum(), torch.tensor(ab.numel(), device=dev), (ba <= q).sum(), torch.tensor(ba.numel(), device=dev)]).tolist()
        res["nsd"] = {}
        for vox in NSD_VOXELS:
            tau = vox * min(spacing)
            counts = list(S.surface_overlap(lab, other, tau, spacing))
            assert counts == two_transforms(tau), f"surface_overlap {counts} against the two transforms {two_transforms(tau)}"
            r = {"tau": tau, "rows": M.BallElement(tau, spacing).n_rows, "counts": counts, "value": S.normalized_surface_dice(lab, other, tau, spacing),
                 "times": _windows({"overlap": lambda: S.surface_overlap(lab, other, tau, spacing), "two_transforms": lambda: two_transforms(tau)}, torch)}
            if use_scipy:
                t0 = time.perf_counter()
                host = _host_counts(lab.cpu().numpy() != 0, other.cpu().numpy() != 0, tau, spacing)
                r["scipy_s"] = time.perf_counter() - t0
                assert counts == host, f"surface_overlap {counts} on the device, {host} with scipy on the host"
            res["nsd"][str(vox)] = r
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=str, nargs=2, default=None, help="(internal) run one step in this process: kind spacing")
    ap.add_argument("--shape", type=int, nargs=3, default=None, help="(internal) the shape of that step")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--scipy-all", action="store_true", help="the host comparison on the larger shape too (minutes)")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    if a.step:
        run_step(a.step[0], tuple(a.shape), a.step[1], not a.no_scipy)
        return 0
    results = []
    for shape in SHAPES:
        for kind in KINDS:
            for sp in SPACINGS:
                host = not a.no_scipy and (a.scipy_all or shape == SHAPES[0])
                cmd = [sys.executable, os.path.abspath(__file__), "--step", kind, sp, "--shape", *map(str, shape)] + ([] if host else ["--no-scipy"])
                try:
                    r = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT_S)
                except subprocess.TimeoutExpired:
                    print(f"[probe] {kind} {sp} {shape}: no result within {STEP_LIMIT_S} s; stopping", file=sys.stderr)
                    return 2
                if r.returncode != 0:
                    print(f"[probe] {kind} {sp} {shape}: exit {r.returncode}; stopping\n{r.stderr[-2000:]}", file=sys.stderr)
                    return 1
                res = json.loads(r.stdout.strip().splitlines()[-1])
                results.append(res)
                t = res["times"]
                print(f"{kind} {sp} {shape}: {res['set_voxels']} set voxels; copy_ of the packed mask {t['copy_bits']['median_ms']:.4f} ms, of the uint8 volume "
                      f"{t['copy_u8']['median_ms']:.4f} ms", flush=True)
                for k, el in res["elements"].items():
                    line = f"  {el['rows']:5d} rows (radius {el['radius']:.3f}, radii {el['radii']}):"
                    for name in ("ball", "ball_gated", "edt"):
                        v = t[f"{name}_{k}"]
                        line += f"  {name} {v['median_ms']:.3f} ms [{v['min_ms']:.3f} .. {v['max_ms']:.3f}] = {res['as_copy_u8'][name + '_' + k]:.2f} x u8"
                    print(line, flush=True)
                for vox, n in res.get("nsd", {}).items():
                    print(f"  surface overlap at {vox} voxels ({n['rows']} rows): {n['times']['overlap']['median_ms']:.3f} ms, windows "
                          f"{[round(v, 3) for v in n['times']['overlap']['window_median_ms']]}; two transforms {n['times']['two_transforms']['median_ms']:.3f} ms; scipy on the "
                          f"host {n.get('scipy_s', float('nan')):.2f} s; counts {n['counts']}, value {n['value']!r}", flush=True)
                if a.out:
                    with open(a.out, "w") as fh:
                        json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
