#!/usr/bin/env python3
"""Time the six tile-GEMM chain entries of csrc/pwa_fused.hip alone at their bench shapes (autopet128, B = 4, M = 2, fp32, dropout 0.1): 20 back-to-back launches
of each C-ABI entry on HIP events, microseconds per launch, beside the algorithmic bytes of the launch (activations read + written once; the weights are L2-resident)
and their time at the HBM peak of 8 TB/s.

    python tools/tile_chain_probe.py [--runs N]        timing table, N passes over the rows
    python tools/tile_chain_probe.py --hash DIR        every row once on inputs from a fixed seed; DIR/tile_chain_hashes.json holds the sha256 of every output tensor
                                                       (scratch operands and partial sums included), to compare two builds bit for bit

The callers below (pre_* / post_* / inmlp_*) hand the entries raw pointers exactly as veloxseg_amd/functional.py and csrc/_vxops.cpp do; tests/test_tile_chains_gpu.py
drives the same callers at small shapes.  Outputs are prefilled with NaN, so an element a kernel does not write shows in the hash and in the tests."""
import argparse, hashlib, json, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

HBM_BYTES_PER_S = 8.0e12
f64 = torch.float64


def _H():
    import veloxseg_amd  # noqa
    from veloxseg_amd import _hip
    return _hip


def _ptrs(H, vals):
    return (H.ctypes.c_void_p * len(vals))(*[(v if v else None) for v in vals])


def _nan(*shape, dev="cuda"):
    return torch.full(shape, float("nan"), device=dev, dtype=torch.float32)


def _rand(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).cuda()


def rng_tensor(seed=77, step=1):
    return torch.tensor([seed, step], dtype=torch.int64, device="cuda")


# --------------------------------------------------------------------------------------------------------------------- pre: LN + projections / PatchMerging
def pre_inputs(B, M, C, J, V=None, s2d=False, grid=None, dres=True, seed=5):
    """s2d: grid = the COARSE grid (gd, gh, gw), x is (B, C / 8, 2gd, 2gh, 2gw) and V = gd gh gw"""
    g = torch.Generator().manual_seed(seed)
    if s2d:
        V = grid[0] * grid[1] * grid[2]
        xshape = (B, C // 8, 2 * grid[0], 2 * grid[1], 2 * grid[2])
    else:
        grid = (1, 1, V)
        xshape = (B, C, V)
    mods = []
    for _ in range(M):
        mods.append(dict(x=_rand(g, *xshape), gamma=(1.0 + 0.2 * torch.randn(C, generator=g)).cuda(), beta=_rand(g, C, scale=0.1),
                         w=[_rand(g, j, C, scale=0.5 / C ** 0.5) for j in J], b=[_rand(g, j, scale=0.1) for j in J],
                         dout=[_rand(g, B, j, V) for j in J], dres=_rand(g, B, C, V) if (dres and not s2d) else None))
    return dict(B=B, M=M, C=C, J=list(J), V=V, s2d=int(s2d), grid=tuple(grid), eps=1e-5, mods=mods)


def pre_fwd(inp, H=None):
    H = H or _H()
    B, M, C, J, V, NS = inp["B"], inp["M"], inp["C"], inp["J"], inp["V"], len(inp["J"])
    outs = [dict(xn=_nan(B, C, V), out=[_nan(B, j, V) for j in J]) for _ in range(M)]
    vals = []
    for m, o in zip(inp["mods"], outs):
        w, b, ot = m["w"] + [None] * (3 - NS), m["b"] + [None] * (3 - NS), o["out"] + [None] * (3 - NS)
        vals += [H.P(m["x"]), H.P(m["gamma"]), H.P(m["beta"]), H.P(w[0]), H.P(b[0]), H.P(w[1]), H.P(b[1]), H.P(w[2]), H.P(b[2]), H.P(o["xn"]), H.P(ot[0]), H.P(ot[1]), H.P(ot[2])]
    arr, Jc, g = _ptrs(H, vals), (H.ctypes.c_int * 3)(*(J + [0] * (3 - NS))), inp["grid"]
    launch = lambda: H.call("vx_ln_pw_fwd", H.ctypes.addressof(arr), M, NS, H.ctypes.addressof(Jc), B, C, V, inp["eps"], inp["s2d"], g[0], g[1], g[2], H.stream_ptr())
    launch()
    return outs, launch


def pre_rows(inp, H=None):
    H = H or _H()
    return H.query("vx_ln_pw_tiles", inp["B"], inp["V"]) if not inp["s2d"] else inp["B"] * ((inp["V"] + 15) // 16)


def pre_bwd(inp, H=None):
    H = H or _H()
    B, M, C, J, V, NS = inp["B"], inp["M"], inp["C"], inp["J"], inp["V"], len(inp["J"])
    rows = pre_rows(inp, H)
    outs = [dict(dx=_nan(*m["x"].shape), part=_nan(rows, 2 * C)) for m in inp["mods"]]
    vals = []
    for m, o in zip(inp["mods"], outs):
        w, d = m["w"] + [None] * (3 - NS), m["dout"] + [None] * (3 - NS)
        vals += [H.P(m["x"]), H.P(m["gamma"]), H.P(w[0]), H.P(w[1]), H.P(w[2]), H.P(d[0]), H.P(d[1]), H.P(d[2]), H.P(m["dres"]), H.P(o["dx"]), H.P(o["part"])]
    arr, Jc, g = _ptrs(H, vals), (H.ctypes.c_int * 3)(*(J + [0] * (3 - NS))), inp["grid"]
    launch = lambda: H.call("vx_ln_pw_bwd", H.ctypes.addressof(arr), M, NS, H.ctypes.addressof(Jc), B, C, V, inp["eps"], inp["s2d"], g[0], g[1], g[2], H.stream_ptr())
    launch()
    return outs, launch


# --------------------------------------------------------------------------------------------------------------------- post: mix + LN + FFN
def post_inputs(B, M, C, Cv, R, V, p=0.1, alpha=0.7, seed=6):
    g = torch.Generator().manual_seed(seed)
    mods = []
    for i in range(M):
        mods.append(dict(s=_rand(g, B, Cv, V), x=_rand(g, B, C, V), wm=_rand(g, C, Cv, scale=0.5 / Cv ** 0.5), bm=_rand(g, C, scale=0.1),
                         gamma=(1.0 + 0.2 * torch.randn(C, generator=g)).cuda(), beta=_rand(g, C, scale=0.1), w1=_rand(g, R, C, scale=0.5 / C ** 0.5), b1=_rand(g, R, scale=0.1),
                         w2=_rand(g, C, R, scale=0.5 / R ** 0.5), b2=_rand(g, C, scale=0.1), dout=_rand(g, B, C, V), sites=(11 + 3 * i, 12 + 3 * i, 13 + 3 * i)))
    return dict(B=B, M=M, C=C, Cv=Cv, R=R, V=V, p=p, alpha=alpha, eps=1e-5, mods=mods, rs=rng_tensor() if p > 0 else None)


_POST_PRM = ("wm", "bm", "gamma", "beta", "w1", "b1", "w2", "b2")


def post_fwd(inp, H=None):
    H = H or _H()
    B, M, C, Cv, R, V = (inp[k] for k in ("B", "M", "C", "Cv", "R", "V"))
    outs = [dict(y=_nan(B, C, V), out=_nan(B, C, V)) for _ in range(M)]
    vals = []
    for m, o in zip(inp["mods"], outs):
        vals += [H.P(m["s"]), H.P(m["x"])] + [H.P(m[k]) for k in _POST_PRM] + [H.P(o["y"]), H.P(o["out"])] + [None] * 9 + list(m["sites"])
    arr = _ptrs(H, vals)
    launch = lambda: H.call("vx_pwa_post_fwd", H.ctypes.addressof(arr), M, B, C, Cv, R, V, inp["eps"], inp["alpha"], H.P(inp["rs"], torch.int64), inp["p"], inp["p"], H.stream_ptr())
    launch()
    return outs, launch


def post_bwd(inp, ys, H=None):
    """ys[m] = the forward's y of modality m"""
    H = H or _H()
    B, M, C, Cv, R, V = (inp[k] for k in ("B", "M", "C", "Cv", "R", "V"))
    rows = H.query("vx_pwa_post_tiles", B, V)
    outs = [dict(ds=_nan(B, Cv, V), dxres=_nan(B, C, V), part=_nan(rows, 2 * C), sc_n=_nan(B, C, V), sc_h=_nan(B, R, V), sc_da=_nan(B, R, V), sc_dz=_nan(B, C, V),
                 sc_dmix=_nan(B, C, V)) for _ in range(M)]
    vals = []
    for m, o, y in zip(inp["mods"], outs, ys):
        vals += [H.P(m["s"]), None] + [H.P(m[k]) for k in _POST_PRM] + [H.P(y), None, H.P(m["dout"]), H.P(o["ds"]), H.P(o["dxres"]), H.P(o["part"])] + \
                [H.P(o[k]) for k in ("sc_n", "sc_h", "sc_da", "sc_dz", "sc_dmix")] + list(m["sites"])
    arr = _ptrs(H, vals)
    launch = lambda: H.call("vx_pwa_post_bwd", H.ctypes.addressof(arr), M, B, C, Cv, R, V, inp["eps"], inp["alpha"], H.P(inp["rs"], torch.int64), inp["p"], inp["p"], H.stream_ptr())
    launch()
    return outs, launch


# --------------------------------------------------------------------------------------------------------------------- inmlp: channel stage of the JLC block
def inmlp_inputs(B, C, R, V, p=0.1, nparts=4, seed=7):
    """nparts = 0: no partial sums (the forward then READS stats = the fp64 statistics cast to float)"""
    g = torch.Generator().manual_seed(seed)
    o = (torch.randn(B, C, V, generator=g) * 1.5 + 0.3)
    d = dict(B=B, C=C, R=R, V=V, p=p, eps=1e-5, site=21, nparts=nparts, rs=rng_tensor() if p > 0 else None, w1=_rand(g, R, C, scale=0.5 / C ** 0.5), b1=_rand(g, R, scale=0.1),
             w2=_rand(g, C, R, scale=0.5 / R ** 0.5), b2=_rand(g, C, scale=0.1), dout=_rand(g, B, C, V))
    od = o.double().reshape(B * C, V)
    if nparts:
        bounds = [round(i * V / nparts) for i in range(nparts + 1)]
        d["part"] = torch.stack([torch.stack([od[:, a:b].sum(1), (od[:, a:b] ** 2).sum(1)], 1) for a, b in zip(bounds[:-1], bounds[1:])], 1).contiguous().cuda()      # (B C, nparts, 2)
    else:
        d["part"] = None
    d["o"] = o.cuda()
    return d


def inmlp_fwd(inp, stats=None, H=None):
    """stats: given when inp['part'] is None"""
    H = H or _H()
    B, C, R, V = (inp[k] for k in ("B", "C", "R", "V"))
    outs = dict(out=_nan(B, C, V), stats=_nan(B * C, 2) if inp["part"] is not None else stats)
    launch = lambda: H.call("vx_inmlp_fwd", H.P(inp["o"]), H.P(inp["part"], f64), inp["nparts"], H.P(outs["stats"]), H.P(inp["w1"]), H.P(inp["b1"]), H.P(inp["w2"]), H.P(inp["b2"]),
                            H.P(outs["out"]), B, C, R, V, inp["eps"], H.P(inp["rs"], torch.int64), inp["site"], inp["p"], H.stream_ptr())
    launch()
    return outs, launch


def inmlp_bwd(inp, stats, H=None):
    H = H or _H()
    B, C, R, V = (inp[k] for k in ("B", "C", "R", "V"))
    tiles = H.query("vx_inmlp_tiles", V)
    outs = dict(dn=_nan(B, C, V), part_dn=_nan(B * C, tiles, 2), sc_n=_nan(B, C, V), sc_h=_nan(B, R, V), sc_da=_nan(B, R, V), sc_dz=_nan(B, C, V))
    launch = lambda: H.call("vx_inmlp_bwd", H.P(inp["o"]), H.P(stats), H.P(inp["w1"]), H.P(inp["b1"]), H.P(inp["w2"]), H.P(inp["dout"]), H.P(outs["dn"]), H.P(outs["part_dn"]),
                            H.P(outs["sc_n"]), H.P(outs["sc_h"]), H.P(outs["sc_da"]), H.P(outs["sc_dz"]), B, C, R, V, H.P(inp["rs"], torch.int64), inp["site"], inp["p"], H.stream_ptr())
    launch()
    return outs, launch


# --------------------------------------------------------------------------------------------------------------------- the bench rows
def bench_rows():
    """(label, kind, arguments) of every launch of the family in one autopet128 step, from the bench configuration itself"""
    from bench import WORKLOADS
    from veloxseg_amd.model.components.PWA import plan_windows
    cfg, B = WORKLOADS["autopet128"]
    M, base = len(cfg["in_ch"]), cfg["attn_base_ch"]
    rows = []
    for lv in range(4):
        g, C = 32 >> lv, base << lv
        pl = plan_windows([g] * 3, cfg["min_big_window_sizes"][lv], cfg["min_small_window_sizes"][lv], 2, cfg["num_heads"][lv], cfg["min_dim_head"][lv], C)
        J, V = (pl["ch_qk"], pl["ch_qk"], pl["ch_v"]), g ** 3
        rows.append((f"pre L{lv + 1} C{C} J{J} V{V}", "pre", dict(B=B, M=M, C=C, J=J, V=V)))
        if lv < 3:
            rows.append((f"merge to {g // 2}^3 C{8 * C} J{2 * C}", "pre", dict(B=B, M=M, C=8 * C, J=(2 * C,), s2d=True, grid=(g // 2,) * 3)))
        if lv >= 1:
            rows.append((f"post L{lv + 1} C{C} Cv{pl['ch_v']} R{C * cfg['ffn_expansion_ratio'][lv]} V{V}", "post", dict(B=B, M=M, C=C, Cv=pl["ch_v"], R=C * cfg["ffn_expansion_ratio"][lv], V=V)))
            rows.append((f"inmlp {g}^3 C{C} R{C * cfg['conv_expansion_factor'][lv]}", "inmlp", dict(B=B, C=C, R=C * cfg["conv_expansion_factor"][lv], V=V)))
    return rows


def _nbytes(*trees):
    n = 0
    for t in trees:
        if torch.is_tensor(t):
            n += t.numel() * t.element_size()
        elif isinstance(t, dict):
            n += _nbytes(*t.values())
        elif isinstance(t, (list, tuple)):
            n += _nbytes(*t)
    return n


def _act_bytes_in(kind, inp, fwd):
    """activation inputs of the launch (weights, biases and statistics left out)"""
    if kind == "pre":
        return sum(_nbytes(m["x"]) + (0 if fwd else _nbytes(m["dout"], m["dres"])) for m in inp["mods"])
    if kind == "post":
        return sum(_nbytes(m["s"], m["x"]) if fwd else _nbytes(m["x"], m["dout"]) for m in inp["mods"])      # backward: y (the size of x) and dout
    return _nbytes(inp["o"]) + (0 if fwd else _nbytes(inp["dout"]))


def run_row(kind, kw, H):
    """-> [(entry, outputs, launch, bytes)] for the forward and the backward entry of the row"""
    if kind == "pre":
        inp = pre_inputs(**kw)
        fo, fl = pre_fwd(inp, H)
        bo, bl = pre_bwd(inp, H)
        names = ("vx_ln_pw_fwd", "vx_ln_pw_bwd")
    elif kind == "post":
        inp = post_inputs(**kw)
        fo, fl = post_fwd(inp, H)
        bo, bl = post_bwd(inp, [o["y"] for o in fo], H)
        names = ("vx_pwa_post_fwd", "vx_pwa_post_bwd")
    else:
        inp = inmlp_inputs(**kw)
        fo, fl = inmlp_fwd(inp, H=H)
        bo, bl = inmlp_bwd(inp, fo["stats"], H)
        names = ("vx_inmlp_fwd", "vx_inmlp_bwd")
    return [(names[0], fo, fl, _act_bytes_in(kind, inp, True) + _nbytes(fo)), (names[1], bo, bl, _act_bytes_in(kind, inp, False) + _nbytes(bo))]


def _flat(prefix, t, out):
    if torch.is_tensor(t):
        out[prefix] = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
    elif isinstance(t, dict):
        for k, v in t.items():
            _flat(f"{prefix}.{k}", v, out)
    elif isinstance(t, (list, tuple)):
        for i, v in enumerate(t):
            _flat(f"{prefix}[{i}]", v, out)


def timed(launch, reps=20):
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--hash", metavar="DIR", default=None)
    ap.add_argument("--runs", type=int, default=1)
    args = ap.parse_args()
    H = _H()
    rows = bench_rows()
    if args.hash:
        hashes = {}
        for label, kind, kw in rows:
            for entry, outs, _, _ in run_row(kind, kw, H):
                torch.cuda.synchronize()
                _flat(f"{label} | {entry}", outs, hashes)
        os.makedirs(args.hash, exist_ok=True)
        path = os.path.join(args.hash, "tile_chain_hashes.json")
        json.dump(hashes, open(path, "w"), indent=1, sort_keys=True)
        print(f"{len(hashes)} tensors hashed -> {path}; digest of all: {hashlib.sha256(json.dumps(hashes, sort_keys=True).encode()).hexdigest()[:16]}")
        return
    res = {}
    for run in range(args.runs):
        for label, kind, kw in rows:
            for entry, _, launch, nbytes in run_row(kind, kw, H):
                us = timed(launch)
                res.setdefault((label, entry), (nbytes, []))[1].append(us)
    print(f"{'row':<46} {'entry':<16} {'MB':>7} {'HBM us':>7}  us per launch")
    for (label, entry), (nbytes, us) in res.items():
        print(f"{label:<46} {entry:<16} {nbytes / 1e6:7.1f} {nbytes / HBM_BYTES_PER_S * 1e6:7.1f}  " + " ".join(f"{u:7.1f}" for u in us), flush=True)
    print(json.dumps({"tile_chain_probe": [{"row": l, "entry": e, "bytes": b, "hbm_us": round(b / HBM_BYTES_PER_S * 1e6, 2), "us": [round(u, 2) for u in us]} for (l, e), (b, us) in res.items()]}))


if __name__ == "__main__":
    main()
