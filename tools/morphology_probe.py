#!/usr/bin/env python3
"""Time of the mask-morphology kernels (csrc/morphology.hip) on one 400 x 400 x 352 uint8 volume, each as a ratio to a device-to-device copy_
of the uint8 volume measured in the same process.  Beside them: the torch eager statement of a 26-connected dilation (max_pool3d, kernel 3, stride 1, padding 1
on a float copy: the same bits) and scipy.ndimage on the host.

Two volumes: "balls" (about 50 balls of radius 3 - 12: a lesion mask) and "bernoulli" (each voxel set with probability 0.30).  Timed: pack, unpack, a step of 1,
max_fused and 2 max_fused + 1 iterations at connectivity 6 and 26, max_fused iterations as ONE call against the same count as chained one-iteration calls (three
alternating windows each: the spread between windows of one kind is what a difference has to beat), a packed closing of 2 iterations end to end (pack, two
steps, unpack) and fill_holes.  Every volume runs in a fresh child process under its own time limit; the first one that fails or runs out of time ends the probe
(nothing more is started on the GPU).  Per figure: 3 warm-up calls, then the median of REPEATS single calls between two HIP events; min / max give the spread.
A machine without a GPU fails; there is no fallback.

    python tools/morphology_probe.py [--shape 400 400 352] [--out result.json] [--no-scipy]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
VOLUMES = ["balls", "bernoulli"]
CONNECTIVITIES = [6, 26]
STEP_LIMIT_S, WINDOWS = 280, 3


def run_step(volume, shape, use_scipy):
    sys.path.insert(0, ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("morphology_probe: no GPU")
    from components_probe import _time, make_volume
    from veloxseg_amd import _hip as H
    from veloxseg_amd.utils import morphology as M
    dev = torch.device("cuda", 0)
    lab = make_volume(volume, shape, torch, dev)
    st = H.stream_ptr()
    F = H.query("vx_morph_max_fused")
    nw = H.query("vx_morph_words", *shape)
    dst = torch.empty_like(lab)
    copy = _time(lambda: dst.copy_(lab), torch)
    ratio = lambda t: {**t, "ratio_to_copy": t["median_ms"] / copy["median_ms"]}
    bits, out, tmp = (torch.empty(nw, dtype=torch.int64, device=dev) for _ in range(3))
    res = {"volume": volume, "shape": list(shape), "foreground": float(lab.float().mean()), "max_fused": F, "packed_bytes": nw * 8, "copy_ms": copy, "step": {},
           "fused_vs_chained": {}, "scipy_s": {}}
    res["pack"] = ratio(_time(lambda: H.call("vx_morph_pack", lab.data_ptr(), 1, 0, 0, bits.data_ptr(), *shape, st), torch))
    res["unpack"] = ratio(_time(lambda: H.call("vx_morph_unpack", bits.data_ptr(), None, dst.data_ptr(), 1, 1, 0, *shape, st), torch))
    step = lambda src, to, c, n: H.call("vx_morph_step", src.data_ptr(), to.data_ptr(), tmp.data_ptr(), *shape, 0, c, n, 0, st)

    def chained(c, n):
        src, to = bits, (out if n % 2 else tmp)          # one-iteration calls, alternating between two buffers
        for _ in range(n):
            H.call("vx_morph_step", src.data_ptr(), to.data_ptr(), None, *shape, 0, c, 1, 0, st)
            src, to = to, (tmp if to is out else out)

    for c in CONNECTIVITIES:
        res["step"][str(c)] = {str(n): ratio(_time(lambda: step(bits, out, c, n), torch)) for n in sorted({1, F, 2 * F + 1})}
        if F > 1:
            w = {"fused": [], "chained": []}
            for _ in range(WINDOWS):                      # alternating windows of the two forms
                w["fused"].append(_time(lambda: step(bits, out, c, F), torch)["median_ms"])
                w["chained"].append(_time(lambda: chained(c, F), torch)["median_ms"])
            res["fused_vs_chained"][str(c)] = {"iterations": F, "window_median_ms": w}
    res["closing2_packed"] = ratio(_time(lambda: M.unpack(M.binary_closing(M.pack(lab), 26, 2)), torch))
    res["fill_holes"] = {str(c): ratio(_time(lambda: M.fill_holes(lab, c), torch)) for c in CONNECTIVITIES}
    x = lab.float()[None, None]
    res["torch_max_pool3d_26"] = ratio(_time(lambda: torch.nn.functional.max_pool3d(x, 3, 1, 1), torch))
    res["torch_max_pool3d_26_with_casts"] = ratio(_time(lambda: torch.nn.functional.max_pool3d(lab.float()[None, None], 3, 1, 1).to(torch.uint8), torch))
    same = torch.equal(torch.nn.functional.max_pool3d(x, 3, 1, 1)[0, 0].to(torch.uint8), M.binary_dilation(lab, 26))
    assert same, "max_pool3d and the kernel disagree on a 26-connected dilation"
    if use_scipy:
        from scipy import ndimage
        host = lab.cpu().numpy() != 0
        s26 = ndimage.generate_binary_structure(3, 3)
        for name, fn, mine in (("binary_dilation_26", lambda: ndimage.binary_dilation(host, s26), lambda: M.binary_dilation(lab, 26)),
                               ("binary_closing_26_x2", lambda: ndimage.binary_closing(host, s26, 2), lambda: M.binary_closing(lab, 26, 2)),
                               ("binary_fill_holes_6", lambda: ndimage.binary_fill_holes(host), lambda: M.fill_holes(lab, 6))):
            t0 = time.perf_counter()
            want = fn()
            res["scipy_s"][name] = time.perf_counter() - t0
            assert torch.equal(mine().cpu() != 0, torch.from_numpy(want)), f"scipy and the kernels disagree on {name}"
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
        f = lambda t: f"{t['median_ms']:8.3f} ms = {t['ratio_to_copy']:6.2f} x copy_ [{t['min_ms']:.3f} .. {t['max_ms']:.3f}]"
        print(f"{volume} ({100 * res['foreground']:.1f} % foreground), copy_ of uint8 {res['copy_ms']['median_ms']:.3f} ms, packed mask {res['packed_bytes'] / 1e6:.1f} MB", flush=True)
        print(f"  pack   {f(res['pack'])}\n  unpack {f(res['unpack'])}", flush=True)
        for c in map(str, CONNECTIVITIES):
            for n, t in res["step"][c].items():
                print(f"  step, connectivity {c:2s}, {n} iteration(s): {f(t)}", flush=True)
            if c in res["fused_vs_chained"]:
                w = res["fused_vs_chained"][c]["window_median_ms"]
                print(f"  {res['max_fused']} iterations, connectivity {c:2s}: fused {[round(v, 4) for v in w['fused']]} ms, chained {[round(v, 4) for v in w['chained']]} ms", flush=True)
            print(f"  fill_holes, connectivity {c:2s}: {f(res['fill_holes'][c])}", flush=True)
        print(f"  closing x 2 (26), pack to unpack: {f(res['closing2_packed'])}", flush=True)
        print(f"  torch max_pool3d on float: {f(res['torch_max_pool3d_26'])}; with the casts: {f(res['torch_max_pool3d_26_with_casts'])}", flush=True)
        print(f"  scipy on the host: {', '.join(f'{k} {v:.2f} s' for k, v in res['scipy_s'].items()) or 'not run'}", flush=True)
        if a.out:
            with open(a.out, "w") as fh:
                json.dump(results, fh, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
