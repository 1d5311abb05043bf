#!/usr/bin/env python3
"""Time the coarse-level convolution entries alone at the shapes of the five bench workloads: vx_jlc_cl_fwd / vx_jlc_cl_bwd (csrc/jlc_cl.hip: the JLC grouped convolutions
at <= 8 voxels per axis) and the k3 s2 DownConv layers through vx_conv_mfma_fwd / vx_conv_mfma_bwd_data (csrc/conv_mfma.hip).  20 back-to-back launches of each C-ABI entry
on HIP events, microseconds per launch.

    python tools/coarse_conv_probe.py [--runs N] [--json FILE]     timing table, N passes over the rows (default 3); FILE receives the raw numbers
    python tools/coarse_conv_probe.py --npy DIR                    every row once on inputs from a fixed seed: DIR/<row>__<entry>__<tensor>.npy for every output tensor
    python tools/coarse_conv_probe.py --compare DIR_A DIR_B        the .npy files of two builds, element by element with == (exit status 1 on any difference)

Outputs are prefilled with NaN, so an element a kernel does not write shows in the files.  The rows come from bench.WORKLOADS: token grid = patch / 4, JLC at levels
3 and 4 (C = 64 / 128 in 8 groups), DownConv 16 -> 32 -> 64 -> 128 channels from the token grid down; B = the workload's batch."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


def bench_rows():
    """[(label, kind, kwargs)] without duplicates, in the order of bench.WORKLOADS"""
    from bench import WORKLOADS
    rows, seen = [], set()
    for name, (cfg, B) in WORKLOADS.items():
        grid = [s // cfg["patch_size"] for s in cfg["input_size"]]
        base = cfg["attn_base_ch"]
        for lv in (2, 3):
            sp = tuple(g >> lv for g in grid)
            C = base << lv
            G = C // cfg["min_dim_group"][lv]
            key = ("jlc", B, C, G, sp)
            if key not in seen:
                seen.add(key)
                rows.append((f"jlc B{B} C{C} G{G} {sp[0]}x{sp[1]}x{sp[2]}", "jlc", dict(B=B, C=C, G=G, sp=sp)))
        for lv in range(3):
            sp = tuple(g >> lv for g in grid)
            Cin = cfg["base_ch"] << lv
            key = ("down", B, Cin, sp)
            if key not in seen:
                seen.add(key)
                rows.append((f"down B{B} {Cin}to{2 * Cin} {sp[0]}x{sp[1]}x{sp[2]}", "down", dict(B=B, Cin=Cin, Cout=2 * Cin, sp=sp)))
    return rows


def _H():
    import veloxseg_amd  # noqa
    from veloxseg_amd import _hip
    _hip.LIB.load()
    return _hip


def run_row(kind, kw, H, seed=11):
    """-> [(entry, {name: output tensor}, launch)]; the inputs come from `seed` alone"""
    import torch
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).cuda()
    nan = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), device="cuda", dtype=dtype)
    st = H.stream_ptr()
    if kind == "jlc":
        B, C, G, (D, Hh, W) = kw["B"], kw["C"], kw["G"], kw["sp"]
        assert H.query("vx_jlc_cl_ok", C, G, D, Hh, W) == 1, kw
        Cg = C // G
        x, d_o = rnd(B, C, D, Hh, W), rnd(B, C, D, Hh, W)
        ws = [rnd(C, Cg, k, k, k, scale=1.0 / (Cg * k ** 3) ** 0.5) for k in (1, 3, 5)]
        bs = [rnd(C, scale=0.1) for _ in range(3)]
        gs = [rnd(B, C, D, Hh, W, scale=s) for s in (0.01, 7.0, 1.0)]
        img = nan(H.query("vx_jlc_cl_img_floats", C, G))
        H.call("vx_jlc_cl_prep", H.P(ws[0]), H.P(ws[1]), H.P(ws[2]), H.P(img), C, G, st)
        fo = dict(y1=nan(B, C, D, Hh, W), y3=nan(B, C, D, Hh, W), y5=nan(B, C, D, Hh, W), part=nan(3, B * C, H.query("vx_jlc_cl_ntiles", C, G, D, Hh, W), 2, dtype=torch.float64))
        bo = dict(dx=nan(B, C, D, Hh, W))
        keep = (x, d_o, ws, bs, gs, img)
        fwd = lambda keep=keep: H.call("vx_jlc_cl_fwd", H.P(x), H.P(img), H.P(bs[0]), H.P(bs[1]), H.P(bs[2]), H.P(fo["y1"]), H.P(fo["y3"]), H.P(fo["y5"]),
                                       H.P(fo["part"], torch.float64), B, C, G, D, Hh, W, st)
        bwd = lambda keep=keep: H.call("vx_jlc_cl_bwd", H.P(gs[0]), H.P(gs[1]), H.P(gs[2]), H.P(img), H.P(d_o), H.P(bo["dx"]), B, C, G, D, Hh, W, st)
        fwd(); bwd()
        return [("vx_jlc_cl_fwd", fo, fwd), ("vx_jlc_cl_bwd", bo, bwd)]
    B, Cin, Cout, (D, Hh, W) = kw["B"], kw["Cin"], kw["Cout"], kw["sp"]
    assert H.query("vx_conv_mfma_ok", Cin, Cout, D, Hh, W, 3, 2, 1, 1, 1) == 1, kw
    x, w, b = rnd(B, Cin, D, Hh, W), rnd(Cout, Cin, 3, 3, 3, scale=1.0 / (27 * Cin) ** 0.5), rnd(Cout, scale=0.1)
    dy = rnd(B, Cout, D // 2, Hh // 2, W // 2)
    wsf, wsb = nan(H.query("vx_conv_mfma_ws_floats", Cin, Cout, 3, 0)), nan(H.query("vx_conv_mfma_ws_floats", Cin, Cout, 3, 1))
    fo, bo = dict(y=nan(B, Cout, D // 2, Hh // 2, W // 2)), dict(dx=nan(B, Cin, D, Hh, W))
    keep = (x, w, b, dy, wsf, wsb)
    fwd = lambda keep=keep: H.call("vx_conv_mfma_fwd", H.P(x), H.P(w), H.P(b), H.P(fo["y"]), H.P(wsf), B, Cin, D, Hh, W, Cout, 3, 2, 1, st)
    bwd = lambda keep=keep: H.call("vx_conv_mfma_bwd_data", H.P(dy), H.P(w), H.P(bo["dx"]), H.P(wsb), B, Cin, D, Hh, W, Cout, 3, 2, 1, 0, st)
    fwd(); bwd()
    return [("vx_conv_mfma_fwd", fo, fwd), ("vx_conv_mfma_bwd_data", bo, bwd)]


def timed(launch, reps=20):
    import torch
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def _fname(label, entry, tensor):
    return f"{label.replace(' ', '_')}__{entry}__{tensor}.npy"


def compare(a, b):
    fa, fb = sorted(f for f in os.listdir(a) if f.endswith(".npy")), sorted(f for f in os.listdir(b) if f.endswith(".npy"))
    assert fa == fb and fa, f"different file sets: {len(fa)} against {len(fb)}"
    bad = []
    for f in fa:
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        same = x.shape == y.shape and bool((x == y).all())          # (==: a NaN left in either differs)
        if not same:
            bad.append(f)
    print(json.dumps({"coarse_conv_compare": {"files": len(fa), "elements": int(sum(np.load(os.path.join(a, f)).size for f in fa)), "different": bad}}))
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--json", metavar="FILE", default=None)
    ap.add_argument("--npy", metavar="DIR", default=None)
    ap.add_argument("--compare", nargs=2, metavar="DIR", default=None)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    import torch
    H = _H()
    rows = bench_rows()
    if args.npy:
        os.makedirs(args.npy, exist_ok=True)
        n = 0
        for label, kind, kw in rows:
            for entry, outs, _ in run_row(kind, kw, H):
                torch.cuda.synchronize()
                for k, t in outs.items():
                    np.save(os.path.join(args.npy, _fname(label, entry, k)), t.detach().cpu().numpy())
                    n += 1
        print(f"{n} tensors -> {args.npy}")
        return
    res = {}
    for _ in range(args.runs):
        for label, kind, kw in rows:
            for entry, _, launch in run_row(kind, kw, H):
                res.setdefault((label, entry), []).append(timed(launch))
    print(f"{'row':<34} {'entry':<22} us per launch")
    for (label, entry), us in res.items():
        print(f"{label:<34} {entry:<22} " + " ".join(f"{u:7.1f}" for u in us), flush=True)
    out = {"coarse_conv_probe": [{"row": l, "entry": e, "us": [round(u, 2) for u in us]} for (l, e), us in res.items()]}
    print(json.dumps(out))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        json.dump(out, open(args.json, "w"), indent=1)


if __name__ == "__main__":
    main()
