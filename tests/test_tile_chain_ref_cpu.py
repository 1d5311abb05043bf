"""The fp64 chain references of tests/tile_chain_ref.py (forward AND the hand-derived backward formulas) against autograd through oracle.veloxseg_oracle with
dropout off: `pwa_block` (pre -> the oracle's own window attention -> post), `patch_merging`, and the channel stage of `jlc` (spatial convolutions zeroed, so
that the block IS its channel stage).  Everything runs in fp64 on the host; the references then serve tests/test_tile_chains_gpu.py as the GPU kernels' yardstick."""
import torch

import tile_chain_ref as R
from oracle import veloxseg_oracle as O

f64 = torch.float64
TOL = 1e-9


def _close(a, b, what):
    a, b = a.detach().to(f64), b.detach().to(f64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= TOL * (1.0 + float(b.abs().max())), f"{what}: max abs err {err:.3e} (ref max {float(b.abs().max()):.3e})"


def _leaf(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g, dtype=f64) * scale + shift).requires_grad_(True)


def test_patch_merging_fwd_bwd():
    g = torch.Generator().manual_seed(1)
    B, C0, grid = 2, 4, (4, 6, 4)
    C = 8 * C0
    x = _leaf(g, B, C0, *grid)
    sd = {"d.norm.weight": _leaf(g, C, scale=0.2, shift=1.0), "d.norm.bias": _leaf(g, C, scale=0.1), "d.reduction.weight": _leaf(g, 2 * C0, C, 1, 1, 1, scale=0.3)}
    ref = O.patch_merging(x, sd, "d.")
    gy = torch.randn(ref.shape, generator=g, dtype=f64)
    ref.backward(gy)
    w = sd["d.reduction.weight"].flatten(1)
    xn, outs = R.pre_fwd(x, sd["d.norm.weight"], sd["d.norm.bias"], [w], [None], 1e-6, gather=True)
    _close(outs[0], ref.flatten(2), "merge out")
    dx, dg, db = R.pre_bwd(x, sd["d.norm.weight"], [w], [gy.flatten(2)], None, 1e-6, gather=True)
    _close(dx, x.grad, "merge dx")
    _close(dg, sd["d.norm.weight"].grad, "merge dgamma")
    _close(db, sd["d.norm.bias"].grad, "merge dbeta")
    _close(torch.einsum("bjv,bcv->jc", gy.flatten(2), xn), sd["d.reduction.weight"].grad.flatten(1), "merge dW from xn")


def test_pwa_block_fwd_bwd():
    """the oracle's window scatter is fp32 by construction (its interpolation matrices restate aten's fp32 arithmetic), so this one runs the oracle in fp32 and
    compares at FP32_TOL = 64 fp32 roundings of the largest value: sums of <= 48 products per output, chained through five stages"""
    global TOL
    TOL = 64 * 2.0 ** -24
    try:
        _pwa_block_fwd_bwd()
    finally:
        TOL = 1e-9


def _pwa_block_fwd_bwd():
    g = torch.Generator().manual_seed(2)
    _leaf = lambda g_, *shape, scale=1.0, shift=0.0: (torch.randn(*shape, generator=g_) * scale + shift).requires_grad_(True)
    B, M, C, grid, win, heads, dh, ratio = 2, 2, 16, (4, 4, 4), (2, 2, 2), 1, 4, 3
    plan = O.plan_pwa(list(grid), list(win), [1, 1, 1], 2, heads, dh, C)
    cq, cv, V = plan["c_qk"], plan["c_v"], grid[0] * grid[1] * grid[2]          # per (scale, head) widths of the window gather
    Jq, Jv = plan["ch_qk"], plan["ch_v"]                                           # widths of the projections
    n = plan["n"]
    sd = {"b.attn.position_embedding.relative_position_bias_table": _leaf(g, (2 * n[0] - 1) * (2 * n[1] - 1) * (2 * n[2] - 1), plan["heads"], scale=0.3),
          "b.attn.position_embedding.relative_position_index": O.relative_position_index(n)}
    for m in range(M):
        sd[f"b.attn.input_norms.{m}.weight"], sd[f"b.attn.input_norms.{m}.bias"] = _leaf(g, C, scale=0.2, shift=1.0), _leaf(g, C, scale=0.1)
        for j, co in enumerate((Jq, Jq, Jv)):
            sd[f"b.attn.qkv_proj.{m}.{j}.weight"], sd[f"b.attn.qkv_proj.{m}.{j}.bias"] = _leaf(g, co, C, 1, 1, 1, scale=0.3), _leaf(g, co, scale=0.1)
        sd[f"b.attn.mix_channels.{m}.weight"], sd[f"b.attn.mix_channels.{m}.bias"] = _leaf(g, C, Jv, 1, 1, 1, scale=0.3), _leaf(g, C, scale=0.1)
        sd[f"b.norms.{m}.weight"], sd[f"b.norms.{m}.bias"] = _leaf(g, C, scale=0.2, shift=1.0), _leaf(g, C, scale=0.1)
        sd[f"b.ffns.{m}.linear1.weight"], sd[f"b.ffns.{m}.linear1.bias"] = _leaf(g, ratio * C, C, 1, 1, 1, scale=0.3), _leaf(g, ratio * C, scale=0.1)
        sd[f"b.ffns.{m}.linear2.weight"], sd[f"b.ffns.{m}.linear2.bias"] = _leaf(g, C, ratio * C, 1, 1, 1, scale=0.2), _leaf(g, C, scale=0.1)
    xs = [_leaf(g, B, C, *grid) for _ in range(M)]
    gy = [torch.randn(B, C, *grid, generator=g) for _ in range(M)]
    ref = O.pwa_block(xs, sd, "b.", plan, {"attn": 0.0, "proj": 0.0}, True)
    torch.autograd.backward(ref, gy)

    # the same block from the chain references, with the oracle's window attention between them
    W = lambda k: sd[k].detach().flatten(1) if sd[k].dim() > 1 else sd[k].detach()
    qkv, xns = [], []
    for m in range(M):
        xn, outs = R.pre_fwd(xs[m].flatten(2), W(f"b.attn.input_norms.{m}.weight"), W(f"b.attn.input_norms.{m}.bias"),
                             [W(f"b.attn.qkv_proj.{m}.{j}.weight") for j in range(3)], [W(f"b.attn.qkv_proj.{m}.{j}.bias") for j in range(3)], 1e-6)
        xns.append(xn)
        qkv.append([o.float().reshape(B, -1, *grid).requires_grad_(True) for o in outs])
    q = torch.cat([O.gather_windows(qkv[m][0], plan, cq) for m in range(M)], 3)
    k = torch.cat([O.gather_windows(qkv[m][1], plan, cq) for m in range(M)], 3)
    v = torch.cat([O.gather_windows(qkv[m][2], plan, cv) for m in range(M)], 3)
    l = q.shape[3] // M
    bias = O.relative_bias(sd["b.attn.position_embedding.relative_position_bias_table"].detach(), sd["b.attn.position_embedding.relative_position_index"], l)
    a = O.window_attention(q, k, v, bias, M, 0.0, True, None, "site")
    ss = [O.scatter_windows(a[:, :, :, m * l:(m + 1) * l], plan, cv).flatten(2) for m in range(M)]
    post_w = lambda m: (W(f"b.attn.mix_channels.{m}.weight"), W(f"b.attn.mix_channels.{m}.bias"), W(f"b.norms.{m}.weight"), W(f"b.norms.{m}.bias"),
                        W(f"b.ffns.{m}.linear1.weight"), W(f"b.ffns.{m}.linear1.bias"), W(f"b.ffns.{m}.linear2.weight"), W(f"b.ffns.{m}.linear2.bias"))
    fs, pbs = [], []
    for m in range(M):
        f = R.post_fwd(ss[m], xs[m].flatten(2), *post_w(m), alpha=2.0, eps=1e-6)          # y = x + (x + mix)
        _close(f["out"], ref[m].flatten(2), f"block out[{m}]")
        wm, _, gam, _, w1, _, w2, _ = post_w(m)
        pb = R.post_bwd(f, ss[m], gy[m].flatten(2), wm, gam, w1, w2, 2.0)
        fs.append(f); pbs.append(pb)
        _close(pb["dgamma"], sd[f"b.norms.{m}.weight"].grad, f"post dgamma[{m}]")
        _close(pb["dbeta"], sd[f"b.norms.{m}.bias"].grad, f"post dbeta[{m}]")
        _close(torch.einsum("brn,bcn->rc", pb["sc_da"], pb["sc_n"]), sd[f"b.ffns.{m}.linear1.weight"].grad.flatten(1), f"dW1[{m}] from the scratch operands")
        _close(torch.einsum("bcn,brn->cr", pb["sc_dz"], pb["sc_h"]), sd[f"b.ffns.{m}.linear2.weight"].grad.flatten(1), f"dW2[{m}] from the scratch operands")
        _close(torch.einsum("bcn,bvn->cv", pb["sc_dmix"], ss[m].detach().double()), sd[f"b.attn.mix_channels.{m}.weight"].grad.flatten(1), f"dWm[{m}] from the scratch operands")
    leaves = [t for m in range(M) for t in qkv[m]]
    dqkv = torch.autograd.grad(ss, leaves, [pb["ds"].float() for pb in pbs])
    for m in range(M):
        dx, dg, db = R.pre_bwd(xs[m].flatten(2), W(f"b.attn.input_norms.{m}.weight"), [W(f"b.attn.qkv_proj.{m}.{j}.weight") for j in range(3)],
                               [d.flatten(2) for d in dqkv[3 * m:3 * m + 3]], pbs[m]["dxres"], 1e-6)
        _close(dx, xs[m].grad.flatten(2), f"block dx[{m}]")
        _close(dg, sd[f"b.attn.input_norms.{m}.weight"].grad, f"pre dgamma[{m}]")
        _close(db, sd[f"b.attn.input_norms.{m}.bias"].grad, f"pre dbeta[{m}]")
        _close(torch.einsum("bjv,bcv->jc", dqkv[3 * m + 2].flatten(2).double(), xns[m]), sd[f"b.attn.qkv_proj.{m}.2.weight"].grad.flatten(1), f"dWv[{m}] from xn")


def test_jlc_channel_stage_fwd_bwd():
    g = torch.Generator().manual_seed(3)
    B, C, r, grid, groups = 2, 32, 3, (4, 4, 2), 4
    V = grid[0] * grid[1] * grid[2]
    sd = {}
    for i, k in enumerate((1, 3, 5)):          # zero spatial convolutions: conv = 0 -> IN(0) = 0 -> GELU(0) = 0, so acc = x and the block is its channel stage
        sd[f"j.spatial_convs.{i}.0.weight"], sd[f"j.spatial_convs.{i}.0.bias"] = torch.zeros(C, C // groups, k, k, k, dtype=f64), torch.zeros(C, dtype=f64)
    sd["j.channel_conv.1.weight"], sd["j.channel_conv.1.bias"] = _leaf(g, r * C, C, 1, 1, 1, scale=0.3), _leaf(g, r * C, scale=0.1)
    sd["j.channel_conv.3.weight"], sd["j.channel_conv.3.bias"] = _leaf(g, C, r * C, 1, 1, 1, scale=0.2), _leaf(g, C, scale=0.1)
    x = _leaf(g, B, C, *grid, scale=1.5, shift=0.3)
    ref = O.jlc(x, sd, "j.", groups, 0.0, True)
    gy = torch.randn(ref.shape, generator=g, dtype=f64)
    ref.backward(gy)
    w1, b1, w2, b2 = (sd[k].detach().flatten(1) if sd[k].dim() > 1 else sd[k].detach() for k in ("j.channel_conv.1.weight", "j.channel_conv.1.bias", "j.channel_conv.3.weight", "j.channel_conv.3.bias"))
    f = R.inmlp_fwd(x.flatten(2), w1, b1, w2, b2, 1e-5)
    _close(f["out"], ref.flatten(2), "jlc channel stage out")
    pb = R.inmlp_bwd(f, gy.flatten(2), w1, w2)
    _close(gy.flatten(2) + R.in_bwd_from_dn(pb["dn"], f["nh"], f["rstd"]), x.grad.flatten(2), "jlc channel stage dx from dn and its two sums")
    _close(torch.einsum("brn,bcn->rc", pb["sc_da"], pb["sc_n"]), sd["j.channel_conv.1.weight"].grad.flatten(1), "dW1 from the scratch operands")
    _close(torch.einsum("bcn,brn->cr", pb["sc_dz"], pb["sc_h"]), sd["j.channel_conv.3.weight"].grad.flatten(1), "dW2 from the scratch operands")
    # the partial-sum fold gives the same statistics (to float32)
    o = x.detach().flatten(2).reshape(B * C, V)
    part = torch.stack([torch.stack([o[:, a:b].sum(1), (o[:, a:b] ** 2).sum(1)], 1) for a, b in ((0, 5), (5, 17), (17, V))], 1)
    st = R.fold_stats(part, V, 1e-5)
    assert torch.equal(st[:, 0], f["mean"].reshape(-1).float()) or float((st[:, 0].double() - f["mean"].reshape(-1)).abs().max()) < 1e-6
    assert float((st[:, 1].double() - f["rstd"].reshape(-1)).abs().max()) < 1e-5 * float(f["rstd"].max())


def test_keep_scales_enter_where_the_kernels_draw_them():
    """p > 0: the references with keep-scale tensors equal autograd through the same chain written with explicit masks"""
    g = torch.Generator().manual_seed(4)
    B, C, Cv, Rr, V = 2, 16, 32, 48, 10
    s, x = _leaf(g, B, Cv, V), _leaf(g, B, C, V)
    wm, bm, gam, bet = _leaf(g, C, Cv, scale=0.3), _leaf(g, C, scale=0.1), _leaf(g, C, scale=0.2, shift=1.0), _leaf(g, C, scale=0.1)
    w1, b1, w2, b2 = _leaf(g, Rr, C, scale=0.3), _leaf(g, Rr, scale=0.1), _leaf(g, C, Rr, scale=0.2), _leaf(g, C, scale=0.1)
    km, k1, k2 = [(torch.rand(B, n_, V, generator=g, dtype=f64) > 0.1).double() / 0.9 for n_ in (C, Rr, C)]
    y = 0.7 * x + (torch.einsum("cv,bvn->bcn", wm, s) + bm.view(1, -1, 1)) * km
    n = O.layernorm_cf(y, gam, bet, 1e-5)
    h = O.gelu(torch.einsum("rc,bcn->brn", w1, n) + b1.view(1, -1, 1)) * k1
    out = y + (torch.einsum("cr,brn->bcn", w2, h) + b2.view(1, -1, 1)) * k2
    gy = torch.randn(out.shape, generator=g, dtype=f64)
    out.backward(gy)
    f = R.post_fwd(s, x, wm, bm, gam, bet, w1, b1, w2, b2, 0.7, 1e-5, km, k1, k2)
    _close(f["out"], out, "post out with masks")
    pb = R.post_bwd(f, s, gy, wm, gam, w1, w2, 0.7, km, k1, k2)
    _close(pb["ds"], s.grad, "post ds with masks")
    _close(pb["dxres"], x.grad, "post dxres with masks")
    _close(torch.einsum("brn,bcn->rc", pb["sc_da"], pb["sc_n"]), w1.grad, "dW1 with masks")
