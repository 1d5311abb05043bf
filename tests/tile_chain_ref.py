"""fp64 torch references of the three tile-GEMM chains of csrc/pwa_fused.hip, forward and backward, written from the reference's formulas:

  pre    PWA.py:291-298,329-344 with attention_utils.py:29-43 (channels-first LayerNorm, u = mean, s = mean((x - u)^2)): xn = LN(x); out_s = W_s xn + b_s;
         PatchMerging, attention_utils.py:127-168: the 8-way strided gather (sub-volume index outermost in the channels), LN(8C), the 8C -> 2C reduction
  post   PWA.py:377,433-439 with attention_utils.py:45-71: y = alpha x + Drop(Wm s + bm); out = y + Drop(W2 Drop(GELU(W1 LN(y) + b1)) + b2)
  inmlp  conv_blocks.py:60-66,74: out = o + Drop(W2 GELU(W1 IN(o) + b1) + b2), IN = InstanceNorm3d (biased variance over the volume, no affine)

The backward passes are the hand-derived formulas the kernels implement (not autograd), so tests/test_tile_chain_ref_cpu.py can hold them to autograd through
oracle.veloxseg_oracle.  Dropout enters as keep-scale tensors (0 or 1 / (1 - p), the shape of the tensor they multiply; None = no dropout), so the same
functions serve p = 0 against the oracle and p > 0 with the masks of oracle/philox.py.  Activations are (B, C, V); weights (out, in)."""
import math

import torch

f64 = torch.float64


def _d(t):
    return None if t is None else t.detach().to("cpu", f64)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0))))


def gelu_grad(x):
    return 0.5 * (1.0 + torch.erf(x * (1.0 / math.sqrt(2.0)))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


def _k(scale, like):
    return torch.ones_like(like) if scale is None else _d(scale).reshape(like.shape)


def ln_fwd(x, gamma, beta, eps):
    u = x.mean(1, keepdim=True)
    s = (x - u).pow(2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(s + eps)
    xh = (x - u) * rstd
    return gamma.view(1, -1, 1) * xh + beta.view(1, -1, 1), xh, rstd


def ln_bwd(dn, xh, rstd, gamma):
    """dn = gradient at the LayerNorm output -> (dx, dgamma, dbeta)"""
    g = dn * gamma.view(1, -1, 1)
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return dx, (dn * xh).sum((0, 2)), dn.sum((0, 2))


def s2d(x):
    """(B, C0, 2d, 2h, 2w) -> (B, 8 C0, d h w), channel = sub * C0 + c with sub = 4 i + 2 j + k"""
    parts = [x[:, :, i::2, j::2, k::2] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    return torch.cat(parts, 1).flatten(2)


def s2d_adjoint(g, shape):
    B, C0, D, Hh, W = shape
    out = torch.zeros(shape, dtype=g.dtype)
    g = g.reshape(B, 8, C0, D // 2, Hh // 2, W // 2)
    n = 0
    for i in (0, 1):
        for j in (0, 1):
            for k in (0, 1):
                out[:, :, i::2, j::2, k::2] = g[:, n]
                n += 1
    return out


def pre_fwd(x, gamma, beta, ws, bs, eps, gather=False):
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    t = s2d(x) if gather else x
    xn, _, _ = ln_fwd(t, gamma, beta, eps)
    outs = [torch.einsum("jc,bcv->bjv", _d(w), xn) + (0 if b is None else _d(b).view(1, -1, 1)) for w, b in zip(ws, bs)]
    return xn, outs


def pre_bwd(x, gamma, ws, douts, dres, eps, gather=False):
    """-> dx (the shape of x), dgamma, dbeta"""
    x, gamma = _d(x), _d(gamma)
    t = s2d(x) if gather else x
    _, xh, rstd = ln_fwd(t, gamma, torch.zeros_like(gamma), eps)
    dxn = sum(torch.einsum("jc,bjv->bcv", _d(w), _d(d)) for w, d in zip(ws, douts))
    dx, dg, db = ln_bwd(dxn, xh, rstd, gamma)
    if gather:
        return s2d_adjoint(dx, x.shape), dg, db
    return dx + (0 if dres is None else _d(dres)), dg, db


def post_fwd(s, x, wm, bm, gamma, beta, w1, b1, w2, b2, alpha, eps, k_mix=None, k1=None, k2=None):
    s, x, wm, bm, gamma, beta, w1, b1, w2, b2 = map(_d, (s, x, wm, bm, gamma, beta, w1, b1, w2, b2))
    mix = torch.einsum("cv,bvn->bcn", wm, s) + bm.view(1, -1, 1)
    y = alpha * x + mix * _k(k_mix, mix)
    n, xh, rstd = ln_fwd(y, gamma, beta, eps)
    a = torch.einsum("rc,bcn->brn", w1, n) + b1.view(1, -1, 1)
    h = gelu(a) * _k(k1, a)
    z = torch.einsum("cr,brn->bcn", w2, h) + b2.view(1, -1, 1)
    return dict(y=y, out=y + z * _k(k2, z), n=n, xh=xh, rstd=rstd, a=a, h=h)


def post_bwd(f, s, dout, wm, gamma, w1, w2, alpha, k_mix=None, k1=None, k2=None):
    """f = post_fwd(...) -> ds, dxres, dgamma, dbeta and the operands the kernel leaves for the grouped weight-gradient launch"""
    s, dout, wm, gamma, w1, w2 = map(_d, (s, dout, wm, gamma, w1, w2))
    dz = dout * _k(k2, dout)
    da = torch.einsum("cr,bcn->brn", w2, dz) * _k(k1, f["a"]) * gelu_grad(f["a"])
    dn = torch.einsum("rc,brn->bcn", w1, da)
    dyl, dg, db = ln_bwd(dn, f["xh"], f["rstd"], gamma)
    dy = dout + dyl
    dmix = dy * _k(k_mix, dy)
    return dict(ds=torch.einsum("cv,bcn->bvn", wm, dmix), dxres=alpha * dy, dgamma=dg, dbeta=db, sc_n=f["n"], sc_h=f["h"], sc_da=da, sc_dz=dz, sc_dmix=dmix)


def in_stats(o, eps):
    o = _d(o)
    mean = o.mean(2, keepdim=True)
    var = (o * o).mean(2, keepdim=True) - mean * mean          # (the kernels fold sum and sum of squares)
    return mean, 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)


def fold_stats(part, V, eps):
    """the fp64 fold of vx_inmlp_fwd over the producer's partial sums, in its order: part (B C, nparts, 2) -> (B C, 2) mean, rstd as float32"""
    part = part.detach().to("cpu", f64)
    s, q = torch.zeros(part.shape[0], dtype=f64), torch.zeros(part.shape[0], dtype=f64)
    for i in range(part.shape[1]):
        s = s + part[:, i, 0]
        q = q + part[:, i, 1]
    m = s / V
    var = (q / V - m * m).clamp_min(0.0)
    return torch.stack([m, 1.0 / torch.sqrt(var + eps)], 1).float()


def inmlp_fwd(o, w1, b1, w2, b2, eps, k=None, stats=None):
    """stats: (B C, 2) mean, rstd to use instead of the volume's own"""
    o, w1, b1, w2, b2 = map(_d, (o, w1, b1, w2, b2))
    if stats is None:
        mean, rstd = in_stats(o, eps)
    else:
        st = _d(stats).view(o.shape[0], o.shape[1], 2)
        mean, rstd = st[..., 0:1], st[..., 1:2]
    nh = (o - mean) * rstd
    a = torch.einsum("rc,bcn->brn", w1, nh) + b1.view(1, -1, 1)
    z = torch.einsum("cr,brn->bcn", w2, gelu(a)) + b2.view(1, -1, 1)
    return dict(out=o + z * _k(k, z), nh=nh, a=a, mean=mean, rstd=rstd)


def inmlp_bwd(f, dout, w1, w2, k=None):
    """f = inmlp_fwd(...) -> dn (gradient at the normalised input; the residual and the InstanceNorm backward are the caller's) and its operands"""
    dout, w1, w2 = map(_d, (dout, w1, w2))
    dz = dout * _k(k, dout)
    da = torch.einsum("cr,bcn->brn", w2, dz) * gelu_grad(f["a"])
    dn = torch.einsum("rc,brn->bcn", w1, da)
    return dict(dn=dn, sc_n=f["nh"], sc_h=gelu(f["a"]), sc_da=da, sc_dz=dz)


def in_bwd_from_dn(dn, nh, rstd):
    """InstanceNorm backward from dn and the two sums the kernel returns per (b, c): rstd (dn - mean(dn) - nhat mean(dn nhat))"""
    return rstd * (dn - dn.mean(2, keepdim=True) - nh * (dn * nh).mean(2, keepdim=True))
