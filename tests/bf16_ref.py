"""Host half of the oracle of tests/test_bf16_storage_ops_gpu.py (the *_h entries of include/veloxseg_hip.h: the bf16 STORAGE mode).

Every 16-bit value a kernel reads is produced exactly on the host (`.bfloat16()` rounds to nearest even, as `(__bf16)x` does in vx_pack_bf16x2 / tz_pack), and every
16-bit value it writes is the nearest-even rounding of an fp32 result.  An fp64 reference on exactly those inputs leaves two error terms: one bf16 rounding of the
output (<= 2^-8 |v|: bf16 has 8 significant bits, so half an ulp of v is at most 2^-8 |v|) and the fp32 noise of the same kernel with fp32 storage (e32, measured).

The fp64 restatements below follow the formulas of the header comment of the JLC entries (vx_jlc_mid_fwd / _mid_bwd / _gk, vx_mlp_fwd / _bwd with norm = 0); plain
torch on whatever device the inputs live on; tests/test_bf16_ref_cpu.py holds them to oracle.veloxseg_oracle.jlc and its autograd.
"""
import math

import torch

EPS = 1e-5


def rounded(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> the fp32 values its bf16 storage holds (round to nearest, ties to even)"""
    assert t.dtype == torch.float32
    return t.bfloat16().float()


def widen(t: torch.Tensor) -> torch.Tensor:
    """any stored tensor -> fp64, exactly"""
    return t.detach().double()


def bf16_bound(ref64: torch.Tensor, e32: float) -> torch.Tensor:
    """element-wise bound of an output stored as bf16: half a bf16 ulp of the reference + 3 x the fp32 kernel's own error against the same reference"""
    return ref64.abs() * 2.0 ** -8 + 3.0 * e32


def held(got: torch.Tensor, ref64: torch.Tensor, tol, what: str) -> float:
    """every element of `got` within `tol` (tensor or number) of ref64; NaN (an element never written) fails.  Reports the worst index and the fraction of bad
    elements like close() of tests/test_hip_ops_gpu.py; returns the worst err / tol (the observed multiple of the bound)."""
    a, b = widen(got).cpu(), ref64.detach().double().cpu()
    assert a.shape == b.shape, (what, tuple(a.shape), tuple(b.shape))
    tol = tol.detach().double().cpu() if torch.is_tensor(tol) else torch.full_like(b, float(tol))
    err = (a - b).abs()
    bad = ~(err <= tol)                      # (NaN compares false: counted as bad)
    if bool(bad.any()):
        score = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err - tol)
        i = int(score.argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), a.shape)) if a.dim() else ()
        raise AssertionError(f"{what}: max abs err {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e} (ref max {float(b.abs().max()):.3e}); worst idx {i} = {idx}: "
                             f"got {float(a.flatten()[i]):.6e} want {float(b.flatten()[i]):.6e} tol {float(tol.flatten()[i]):.3e}; bad frac {float(bad.double().mean()):.3e}")
    return float((err / tol.clamp_min(1e-300)).max())


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def row_stats(t, eps=EPS):
    """(rows, V) -> (rows, 2) = (mean, rstd), biased variance: the `stats` layout of the InstanceNorm entries"""
    m = t.mean(-1)
    var = (t * t).mean(-1) - m * m
    return torch.stack([m, 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)], -1)


def partials(t, nparts, prod=None):
    """(rows, V) -> (rows, nparts, 2): (sum t, sum t * (prod or t)) over nparts ragged slices of the row: what a producer kernel hands its consumer"""
    V = t.shape[-1]
    cuts = [round(V * j / nparts) for j in range(nparts + 1)]
    u = t if prod is None else prod
    return torch.stack([torch.stack([t[..., a:b].sum(-1), (t[..., a:b] * u[..., a:b]).sum(-1)], -1) for a, b in zip(cuts[:-1], cuts[1:])], -2)


# ---- JLC spatial stage (include/veloxseg_hip.h: vx_jlc_mid_fwd / vx_jlc_mid_bwd / vx_jlc_gk); rows = (b, c) pairs, every tensor (BC, V) or (3, BC, V)
def jlc_mid_fwd(x, y, stats_y):
    """o = x + sum_k GELU((y_k - mean_k) rstd_k)"""
    o = x
    for k in range(3):
        o = o + gelu((y[k] - stats_y[k, :, 0:1]) * stats_y[k, :, 1:2])
    return o


def jlc_mid_bwd(dout, dn, mean_dn, mean_dn_nhat, o, stats_o):
    """d_o = dout + rstd_o (dn - mean(dn) - nhat mean(dn nhat)), nhat = (o - mean_o) rstd_o; the means are what the caller folded from part_dn"""
    nhat = (o - stats_o[:, 0:1]) * stats_o[:, 1:2]
    return dout + stats_o[:, 1:2] * (dn - mean_dn[:, None] - nhat * mean_dn_nhat[:, None])


def jlc_t(d_o, y, stats_y):
    """-> t (3, BC, V), yhat (3, BC, V)"""
    yh = (y - stats_y[:, :, 0:1]) * stats_y[:, :, 1:2]
    return d_o[None] * gelu_grad(yh), yh


def jlc_gk(d_o, y, stats_y, mean_t, mean_t_yh):
    """g_k = rstd_k (t_k - mean t_k - yhat_k mean(t_k yhat_k)); mean_t, mean_t_yh: (3, BC)"""
    t, yh = jlc_t(d_o, y, stats_y)
    return stats_y[:, :, 1:2] * (t - mean_t[:, :, None] - yh * mean_t_yh[:, :, None])


# ---- JLC channel stage (vx_mlp_fwd / vx_mlp_bwd, norm = 0, no dropout); x: (B, C, V), stats: (B * C, 2), w1: (R, C), w2: (C, R)
def mlp_fwd(x, stats, w1, b1, w2, b2):
    """out = x + W2 GELU(W1 n + b1) + b2, n = (x - mean) rstd.  -> out, n, a"""
    B, C, V = x.shape
    n = (x - stats[:, 0].view(B, C, 1)) * stats[:, 1].view(B, C, 1)
    a = torch.einsum("rc,bcv->brv", w1, n) + b1.view(1, -1, 1)
    out = x + torch.einsum("cr,brv->bcv", w2, gelu(a)) + b2.view(1, -1, 1)
    return out, n, a


def mlp_bwd(x, stats, w1, b1, w2, dout):
    """-> dn (the gradient at the NORMALISED input), dw1, db1, dw2, db2, nhat"""
    _, n, a = mlp_fwd(x, stats, w1, b1, w2, torch.zeros(w2.shape[0], dtype=x.dtype, device=x.device))
    h = gelu(a)
    da = torch.einsum("cr,bcv->brv", w2, dout) * gelu_grad(a)
    dn = torch.einsum("rc,brv->bcv", w1, da)
    return dn, torch.einsum("brv,bcv->rc", da, n), da.sum((0, 2)), torch.einsum("bcv,brv->cr", dout, h), dout.sum((0, 2)), n


def in_backward(dn, n, rstd):
    """InstanceNorm backward at a normalised input n: rstd (dn - mean dn - n mean(dn n)); rows on the last axis"""
    return rstd * (dn - dn.mean(-1, keepdim=True) - n * (dn * n).mean(-1, keepdim=True))


# ---- the seeded inputs of the "statistics over the ROUNDED values" case (vx_jlc_mid_fwd_h at (BC, V) = (32, 1728)): shared by the GPU test and its CPU pre-check
def mid_inputs(BC, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(BC, V, generator=g)
    y = torch.randn(3, BC, V, generator=g) * torch.tensor([0.7, 1.3, 2.1]).view(3, 1, 1) + torch.randn(3, BC, 1, generator=g) * 0.5
    return x, y.bfloat16()
