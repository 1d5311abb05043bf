"""The six tile-GEMM chain entries of csrc/pwa_fused.hip called directly (raw pointers, as functional.py / _vxops.cpp call them; the callers are those of
tools/tile_chain_probe.py) against the fp64 references of tests/tile_chain_ref.py, at the tolerances of tests/test_pwa_fused_gpu.py: outputs 2e-4, gradients
2e-3 of the gradient's scale.  Dropout 0.1 on the post and channel-stage chains with the masks of oracle/philox.py.  The shapes are the smallest at which each
mechanism of the kernels can go wrong: waves sharing n-tiles and projections (one row tile), several row tiles, partial last tiles, K that is no multiple of the
64-k chunk, K beyond one chunk per row tile many times over, 4- and 8-wave blocks, the strided PatchMerging gather.
Every output and scratch buffer is a slice of ONE arena prefilled with NaN with NaN gaps between the slices: an element a kernel does not write stays NaN in the
comparison, a write beyond a buffer (columns beyond V) lands in a gap, and the slices cannot alias."""
import importlib.util
import os

import pytest
import torch

import tile_chain_ref as R
from oracle import philox

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("tile_chain_probe", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools", "tile_chain_probe.py"))
P = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(P)

SEED, STEP, PDROP = 77, 1, 0.1          # P.rng_tensor()
GAP = 64                                # floats (256 bytes: the slices stay 16-byte aligned)


class Arena:
    def __init__(self, floats=1 << 23):
        self.buf = torch.full((floats,), float("nan"), device="cuda", dtype=torch.float32)
        self.off, self.slices = GAP, []

    def __call__(self, *shape, dev="cuda"):
        n = 1
        for s in shape:
            n *= s
        assert self.off + n + GAP <= self.buf.numel()
        t = self.buf[self.off:self.off + n].view(*shape)
        self.slices.append((self.off, n))
        self.off += (n + GAP + 63) // 64 * 64
        return t

    def check(self):
        torch.cuda.synchronize()
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        ends = 0
        for off, n in self.slices:
            assert off >= ends, "slices alias"
            ends = off + n
            keep[off:off + n] = False
        assert bool(torch.isnan(self.buf[keep]).all()), "a kernel wrote outside its buffers"


@pytest.fixture
def arena(monkeypatch):
    a = Arena()
    monkeypatch.setattr(P, "_nan", a)
    yield a
    a.check()


def _close(a, b, atol, rtol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    assert not bool(torch.isnan(a).any()), f"{what}: {int(torch.isnan(a).sum())} elements were not written"
    if not bool((err <= tol).all()):
        i = int((err - tol).argmax())
        raise AssertionError(f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e}); worst idx {i}: got {float(a.flatten()[i]):.6e} "
                             f"want {float(b.flatten()[i]):.6e}; bad frac {float((err > tol).double().mean()):.3e}")


def _out(a, b, what):
    _close(a, b, 2e-4, 2e-4, what)


def _grad(a, b, what):
    _close(a, b, 2e-3 * float(b.abs().max()), 2e-3, what)


def _scales(site, shape, p=PDROP):
    n = 1
    for s in shape:
        n *= s
    return philox.site_scales(SEED, STEP, site, n, p).view(*shape).double() if p > 0 else None


# --------------------------------------------------------------------------------------------------------------------- pre
PRE = [
    ("T4_one_row_tile_dres", dict(B=2, M=2, C=16, J=(16, 16, 16), V=2100, dres=True)),          # waves share n-tiles (backward) and projections (forward); partial last tile
    ("T4_one_row_tile", dict(B=2, M=2, C=16, J=(16, 16, 16), V=2100, dres=False)),
    ("T4_row_tiles", dict(B=1, M=1, C=32, J=(32, 32, 32), V=2048)),                             # two row tiles: two n-tiles per wave in the backward
    ("T1_NW4", dict(B=3, M=2, C=64, J=(32, 32, 64), V=1000)),                                   # 378 blocks, partial tile
    ("T1_NW8_s2d", dict(B=2, M=2, C=128, J=(32,), s2d=True, grid=(3, 3, 3))),                   # fine grid 6^3, C0 = 16
    ("K48", dict(B=2, M=1, C=48, J=(16, 16, 32), V=200)),                                       # K no multiple of 64: clamped pieces; K = 16 segments in the backward
    ("K80", dict(B=2, M=1, C=80, J=(16, 16, 32), V=200)),
    ("K48_T4", dict(B=1, M=1, C=48, J=(16, 16, 32), V=2052)),
    ("K320", dict(B=1, M=1, C=320, J=(64,), V=27)),                                             # five chunks per row tile
]


@pytest.mark.parametrize("name,kw", PRE, ids=[c[0] for c in PRE])
def test_pre(name, kw, arena):
    inp = P.pre_inputs(**kw)
    fo, _ = P.pre_fwd(inp)
    bo, _ = P.pre_bwd(inp)
    gather = bool(inp["s2d"])
    for m, (md, f, b) in enumerate(zip(inp["mods"], fo, bo)):
        xn, outs = R.pre_fwd(md["x"], md["gamma"], md["beta"], md["w"], md["b"], inp["eps"], gather)
        _out(f["xn"], xn, f"{name} xn[{m}]")
        for s, (a, r) in enumerate(zip(f["out"], outs)):
            _out(a, r, f"{name} out[{m}][{s}]")
        dx, dg, db = R.pre_bwd(md["x"], md["gamma"], md["w"], md["dout"], md["dres"], inp["eps"], gather)
        _grad(b["dx"], dx, f"{name} dx[{m}]")
        part = b["part"].double().sum(0).cpu()
        _grad(part[:inp["C"]], dg, f"{name} dgamma[{m}] from the partials")
        _grad(part[inp["C"]:], db, f"{name} dbeta[{m}] from the partials")


# --------------------------------------------------------------------------------------------------------------------- post
POST = [
    ("T4", dict(B=2, M=2, C=32, Cv=32, R=96, V=2100)),
    ("T1_NW4", dict(B=3, M=2, C=64, Cv=64, R=128, V=1000)),
    ("T1_NW8", dict(B=2, M=2, C=128, Cv=128, R=256, V=27)),
    ("uneven", dict(B=1, M=1, C=16, Cv=32, R=48, V=2048)),          # one row tile in the C-row stages, K = 48
]


@pytest.mark.parametrize("name,kw", POST, ids=[c[0] for c in POST])
def test_post(name, kw, arena):
    inp = P.post_inputs(p=PDROP, **kw)
    B, C, R_, V = inp["B"], inp["C"], inp["R"], inp["V"]
    fo, _ = P.post_fwd(inp)
    bo, _ = P.post_bwd(inp, [o["y"] for o in fo])
    for m, (md, f, b) in enumerate(zip(inp["mods"], fo, bo)):
        km, k1, k2 = _scales(md["sites"][0], (B, C, V)), _scales(md["sites"][1], (B, R_, V)), _scales(md["sites"][2], (B, C, V))
        prm = [md[k] for k in ("wm", "bm", "gamma", "beta", "w1", "b1", "w2", "b2")]
        rf = R.post_fwd(md["s"], md["x"], *prm, inp["alpha"], inp["eps"], km, k1, k2)
        _out(f["y"], rf["y"], f"{name} y[{m}]")
        _out(f["out"], rf["out"], f"{name} out[{m}]")
        assert float((rf["h"] == 0).double().mean()) > 0.05, "the masks are not in play"
        rb = R.post_bwd(rf, md["s"], md["dout"], md["wm"], md["gamma"], md["w1"], md["w2"], inp["alpha"], km, k1, k2)
        for k in ("sc_n", "sc_h"):
            _out(b[k], rb[k], f"{name} {k}[{m}]")
        for k in ("ds", "dxres", "sc_da", "sc_dz", "sc_dmix"):
            _grad(b[k], rb[k], f"{name} {k}[{m}]")
        part = b["part"].double().sum(0).cpu()
        _grad(part[:C], rb["dgamma"], f"{name} dgamma[{m}] from the partials")
        _grad(part[C:], rb["dbeta"], f"{name} dbeta[{m}] from the partials")


# --------------------------------------------------------------------------------------------------------------------- channel stage
INMLP = [
    ("V2100", dict(B=2, C=32, R=96, V=2100), 4),
    ("NW8", dict(B=2, C=64, R=128, V=512), 7),
    ("small", dict(B=1, C=128, R=256, V=27), 1),
    ("stats_given", dict(B=2, C=64, R=128, V=512), 0),
]


@pytest.mark.parametrize("name,kw,nparts", INMLP, ids=[c[0] for c in INMLP])
def test_inmlp(name, kw, nparts, arena):
    inp = P.inmlp_inputs(p=PDROP, nparts=nparts, **kw)
    B, C, V = inp["B"], inp["C"], inp["V"]
    if nparts:
        want = R.fold_stats(inp["part"], V, inp["eps"])
        fo, _ = P.inmlp_fwd(inp)
        assert torch.equal(fo["stats"].cpu(), want), f"{name}: stats differ from the fp64 fold cast to float (max {float((fo['stats'].cpu() - want).abs().max()):.3e})"
        stats = fo["stats"]
    else:
        m, r = R.in_stats(inp["o"], inp["eps"])
        stats = torch.stack([m.reshape(-1), r.reshape(-1)], 1).float().cuda()
        fo, _ = P.inmlp_fwd(inp, stats=stats)
    bo, _ = P.inmlp_bwd(inp, stats)
    k = _scales(inp["site"], (B, C, V))
    rf = R.inmlp_fwd(inp["o"], inp["w1"], inp["b1"], inp["w2"], inp["b2"], inp["eps"], k, stats=stats)
    _out(fo["out"], rf["out"], f"{name} out")
    rb = R.inmlp_bwd(rf, inp["dout"], inp["w1"], inp["w2"], k)
    for key in ("sc_n", "sc_h"):
        _out(bo[key], rb[key], f"{name} {key}")
    for key in ("dn", "sc_da", "sc_dz"):
        _grad(bo[key], rb[key], f"{name} {key}")
    # part_dn: one (sum dn, sum dn nhat) pair per 16 voxels
    tiles = (V + 15) // 16
    pad = lambda t: torch.nn.functional.pad(t, (0, 16 * tiles - V)).reshape(B * C, tiles, 16)
    want = torch.stack([pad(rb["dn"]).sum(2), pad(rb["dn"] * rf["nh"]).sum(2)], 2)
    _grad(bo["part_dn"], want, f"{name} part_dn against the per-16-voxel sums")


def test_headline_shapes_reach_the_chain_entries():
    """through the `_hip` call spy of tests/test_pwa_fused_gpu.py::test_fused_paths_are_taken: the 32^3, 8^3 and 4^3 levels of the headline network"""
    import test_pwa_fused_gpu as TP
    from veloxseg_amd import _hip as H
    calls = []
    real = H.LIB.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    H.LIB.call = spy
    try:
        for case in (TP.CASES[0], TP.CASES[2], TP.CASES[3]):
            layer = TP._layer(case, 0.0).cuda().train()
            xs, gy = TP._inputs(case)
            calls.clear()
            TP._run(layer, xs, gy, True)
            pre = 2 if case[-1] else 1                      # the block's pre (+ PatchMerging)
            assert calls.count("vx_ln_pw_fwd") == pre and calls.count("vx_ln_pw_bwd") == pre, (case[0], calls)
            if case[0] != "L1_16cube_T4":
                assert calls.count("vx_pwa_post_fwd") == 1 and calls.count("vx_pwa_post_bwd") == 1, (case[0], calls)
    finally:
        H.LIB.call = real
