"""Second pass over the 32^3 streaming kernels and the loss join, through the C ABI: the long-row InstanceNorm apply kernels (16-byte path, scalar
path of misaligned rows, row tails), the Gram matrix on the matrix pipe and its LDS-staged backward, the patch-embedding weight gradient (its kernel stayed as it was: both rewrites lost
to it, the cases hold whatever comes next), and the lane-per-cell loss finalisation.  Shapes are the smallest that reach every path: a tail shorter than a block's span, rows that start off a 16-byte boundary, several blocks per row."""
import os
import re

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu
F64 = torch.float64


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(tuple(shape), generator=g) * scale


def ulp32(t):
    a = t.abs()
    return torch.nextafter(a, torch.full_like(a, float("inf"))) - a


# ---------------------------------------------------------------------------------------------------------------------- InstanceNorm, long rows
IN_V = [4100, 5002, 4096 * 3 + 4]       # tail shorter than a block's span | V % 4 = 2: rows 1 and 2 start off a 16-byte boundary | three blocks per row plus one quad
BC = 3


def _in_separate(H, ys, res, dout, act, V):
    d, st, nk = dev(), H.stream_ptr(), len(ys)
    pad = [None] * (3 - nk)
    stats = [torch.empty(BC * 2, device=d) for _ in range(nk)]
    for y, s in zip(ys, stats):
        part = torch.empty(BC * 32, device=d, dtype=F64)
        H.call("vx_in_stats", H.P(y), H.P(s), H.P(part, F64), BC, V, 1e-5, st)
    ref = torch.empty(BC, V, device=d)
    H.call("vx_in_apply_fwd", *([H.P(y) for y in ys] + pad), *([H.P(s) for s in stats] + pad), nk, act, H.P(res), H.P(ref), BC, V, st)
    rgrads = []
    for y, s in zip(ys, stats):
        g, ws, part = torch.empty(BC, V, device=d), torch.empty(BC * 2, device=d), torch.empty(BC * 32, device=d, dtype=F64)
        H.call("vx_in_bwd", H.P(dout), H.P(y), H.P(s), act, H.P(ws), H.P(part, F64), H.P(g), BC, V, st)
        rgrads.append(g)
    return stats, ref, rgrads


@gpu
@pytest.mark.parametrize("with_res", [0, 1], ids=["nores", "res"])
@pytest.mark.parametrize("V", IN_V)
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("nk", [1, 2, 3])
def test_instance_norm_split_apply_equals_separate_launches(nk, act, V, with_res):
    """vx_in_fwd_split / vx_in_bwd_split == vx_in_stats + vx_in_apply_fwd / vx_in_bwd bit for bit (statistics included); input 1, where present, gets dy1 = NULL and
    its gradient buffer (filled with a sentinel) must stay untouched"""
    from veloxseg_amd import _hip as H
    d = dev()
    ys = [(rnd(BC, V, seed=10 + k) * (1.0 + k) + 0.3 * k).to(d) for k in range(nk)]
    res = rnd(BC, V, seed=5).to(d) if with_res else None
    dout = rnd(BC, V, seed=6).to(d)
    st = H.stream_ptr()
    pad = [None] * (3 - nk)
    stats, ref, rgrads = _in_separate(H, ys, res, dout, act, V)
    stats2 = [torch.empty(BC * 2, device=d) for _ in range(nk)]
    part = torch.empty(nk * BC * 32, device=d, dtype=F64)
    out = torch.full((BC, V), float("nan"), device=d)
    H.call("vx_in_fwd_split", *([H.P(y) for y in ys] + pad), *([H.P(s) for s in stats2] + pad), H.P(part, F64), nk, act, H.P(res), H.P(out), BC, V, 1e-5, st)
    grads = [torch.full((BC, V), float("nan"), device=d) if k != 1 else None for k in range(nk)]
    H.call("vx_in_bwd_split", H.P(dout), *([H.P(y) for y in ys] + pad), *([H.P(s) for s in stats2] + pad), H.P(part, F64), nk, act,
           *([H.P(g) for g in grads] + pad), None, BC, V, st)
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    for s2, s in zip(stats2, stats):
        assert torch.equal(s2, s)
    for k in range(nk):
        if grads[k] is not None:
            assert torch.equal(grads[k], rgrads[k]), k


@gpu
@pytest.mark.parametrize("V", IN_V)
def test_instance_norm_split_backward_add0(V):
    """add0 is added last: dy0 with add0 == add0 + (dy0 without add0) to 1 ulp; dy1 is unchanged by it.  The kernel's `add0 + rstd * (...)` is one fused multiply-add,
    which skips the rounding of the product: the two differ by half an ulp of the PRODUCT plus the final rounding, so the ulp is taken at the larger of |sum| and
    |product| (where add0 cancels the product, an ulp of the sum alone is smaller than the product's own rounding: 4 ulp of the sum were measured there)"""
    from veloxseg_amd import _hip as H
    d, nk, act = dev(), 2, 1
    ys = [(rnd(BC, V, seed=20 + k) * (1.0 + k)).to(d) for k in range(nk)]
    dout, add0 = rnd(BC, V, seed=7).to(d), rnd(BC, V, seed=8).to(d)
    st = H.stream_ptr()
    stats = [torch.empty(BC * 2, device=d) for _ in range(nk)]
    part = torch.empty(nk * BC * 32, device=d, dtype=F64)
    out = torch.empty(BC, V, device=d)
    H.call("vx_in_fwd_split", H.P(ys[0]), H.P(ys[1]), None, H.P(stats[0]), H.P(stats[1]), None, H.P(part, F64), nk, act, None, H.P(out), BC, V, 1e-5, st)
    g = [[torch.full((BC, V), float("nan"), device=d) for _ in range(nk)] for _ in range(2)]
    for i, a in enumerate((None, add0)):
        H.call("vx_in_bwd_split", H.P(dout), H.P(ys[0]), H.P(ys[1]), None, H.P(stats[0]), H.P(stats[1]), None, H.P(part, F64), nk, act,
               H.P(g[i][0]), H.P(g[i][1]), None, H.P(a), BC, V, st)
    torch.cuda.synchronize()
    assert torch.equal(g[0][1], g[1][1])
    want = add0 + g[0][0]
    assert bool(((g[1][0] - want).abs() <= ulp32(torch.maximum(want.abs(), g[0][0].abs()))).all()), float((g[1][0] - want).abs().max())


# ---------------------------------------------------------------------------------------------------------------------- Gram matrix
@gpu
@pytest.mark.parametrize("V", [64, 1000, 4096 + 4])
@pytest.mark.parametrize("C", [8, 12, 16, 32])
def test_gram_against_fp64(C, V):
    """G = x x^T / (C V) and dx = (dG + dG^T) x / (C V) against torch fp64.  Bounds: 2e-6 max|ref| forward, 1e-6 max|ref| backward: fp32 accumulation over at most 4100
    terms of unit-scale data.  An fp32 restatement of the same sums on the CPU (sequential fp32 chains of 256 voxels per wave, waves and blocks added in fp32; a chain of
    C fused multiply-adds backward) stays inside them: forward 3.0e-7 max|ref| at worst over these shapes, backward 2.2e-7 max|ref|."""
    from veloxseg_amd import _hip as H
    d, B = dev(), 2
    x, dG = rnd(B, C, V, seed=1).to(d), rnd(B, C, C, seed=2).to(d)
    G = torch.full((B, C, C), float("nan"), device=d)
    dx = torch.full((B, C, V), float("nan"), device=d)
    st = H.stream_ptr()
    H.call("vx_gram_fwd", H.P(x), H.P(G), B, C, V, st)
    H.call("vx_gram_bwd", H.P(x), H.P(dG), H.P(dx), B, C, V, st)
    torch.cuda.synchronize()
    xd, gd = x.double(), dG.double()
    G_ref = xd @ xd.transpose(1, 2) / (C * V)
    dx_ref = (gd + gd.transpose(1, 2)) @ xd / (C * V)
    ef, eb = float((G.double() - G_ref).abs().max()), float((dx.double() - dx_ref).abs().max())
    print(f"[gram] C={C} V={V}: fwd err {ef / float(G_ref.abs().max()):.2e} max|ref|, bwd err {eb / float(dx_ref.abs().max()):.2e} max|ref|")
    assert ef <= 2e-6 * float(G_ref.abs().max())
    assert eb <= 1e-6 * float(dx_ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------- patch-embedding weight gradient
@gpu
@pytest.mark.parametrize("B,Cin,Cout,grid", [(3, 2, 32, (8, 8, 8)), (1, 1, 16, (4, 8, 12)), (2, 1, 16, (16, 16, 16))],
                         ids=["ragged_chunks", "below_one_block_span", "several_chunks"])
def test_patch_embed_weight_gradient(B, Cin, Cout, grid):
    """dw += dy (patchified x)^T against an fp64 einsum at 1e-5 max|ref|; the call accumulates into dw (a non-zero start, and a second call with db = NULL)"""
    from veloxseg_amd import _hip as H
    d = dev()
    Do, Ho, Wo = grid
    x = rnd(B, Cin, 4 * Do, 4 * Ho, 4 * Wo, seed=3).to(d)
    dy = rnd(B, Cout, Do, Ho, Wo, seed=4).to(d)
    dw0 = rnd(Cout, Cin * 64, seed=5).to(d)
    dw, db = dw0.clone(), torch.zeros(Cout, device=d)
    st = H.stream_ptr()
    args = (x.data_ptr(), Cin * 64 * Do * Ho * Wo, H.P(dy), H.P(dw))
    H.call("vx_patch_embed_bwd_weight", *args, H.P(db), B, Cin, Cout, Do, Ho, Wo, st)
    torch.cuda.synchronize()
    dw1, db1 = dw.clone(), db.clone()
    H.call("vx_patch_embed_bwd_weight", *args, None, B, Cin, Cout, Do, Ho, Wo, st)
    torch.cuda.synchronize()
    xp = x.double().view(B, Cin, Do, 4, Ho, 4, Wo, 4)
    ref = torch.einsum("bodhw,bcdihjwk->ocijk", dy.double(), xp).reshape(Cout, Cin * 64)
    db_ref = dy.double().sum((0, 2, 3, 4))
    tol = 1e-5 * float(ref.abs().max())
    e1 = float((dw1.double() - dw0.double() - ref).abs().max())
    e2 = float((dw.double() - dw0.double() - 2 * ref).abs().max())
    eb = float((db1.double() - db_ref).abs().max())
    print(f"[patch4 wgrad] B={B} Cin={Cin} Cout={Cout} grid={grid}: first call {e1 / tol * 1e-5:.2e} max|ref|, two calls {e2 / tol * 1e-5:.2e}, db {eb / float(db_ref.abs().max()):.2e}")
    assert e1 <= tol
    assert e2 <= 2 * tol
    assert eb <= 1e-5 * float(db_ref.abs().max())
    assert torch.equal(db, db1), "db = NULL: the bias gradient of the first call must stay as it was"


# ---------------------------------------------------------------------------------------------------------------------- loss finalisation
def _finalize_restated(acc, nh, B, C, V, wds, rc, n_rc, w_rc, gs, gm, w_f):
    """the formulas of vx_loss_finalize_k's comment in fp64 (numpy scalars), in the kernel's order"""
    eps = np.float64(1e-5)
    acc = acc.reshape(nh, 1 + B * C * 3)
    coef = np.zeros((nh, 1 + B * C * 2), np.float32)
    total = np.float64(0.0)
    for h in range(nh):
        w = np.float64(wds[h])
        ce = acc[h, 0] / (np.float64(B) * np.float64(V))
        wd = w / (np.float64(B) * np.float64(C - 1))
        coef[h, 0] = np.float32(w / (np.float64(B) * np.float64(V)))
        dice = np.float64(0.0)
        for b in range(B):
            for c in range(C):
                I, P, T = acc[h, 1 + (b * C + c) * 3: 4 + (b * C + c) * 3]
                U = P + T + eps
                if c >= 1:
                    dice += 1.0 - (2.0 * I + eps) / U
                    coef[h, 1 + (b * C + c) * 2] = np.float32(-2.0 * wd / U)
                    coef[h, 2 + (b * C + c) * 2] = np.float32(wd * (2.0 * I + eps) / (U * U))
        dice /= np.float64(B) * np.float64(C - 1)
        total += w * (ce + dice)
    misc = np.zeros(2, np.float32)
    if rc is not None:
        total += np.float64(w_rc) * rc / np.float64(n_rc)
        misc[0] = np.float32(2.0 * np.float64(w_rc) / np.float64(n_rc))
    if gm:
        ng = gs.size
        feat = sum(((gs.astype(np.float64) - g.astype(np.float64)) ** 2).sum() / ng for g in gm)
        total += np.float64(w_f) * feat / len(gm)
        misc[1] = np.float32(2.0 * np.float64(w_f) / (np.float64(len(gm)) * np.float64(ng)))
    return total, np.concatenate([coef.reshape(-1), misc])


@gpu
@pytest.mark.parametrize("M", [0, 2], ids=["nogram", "gram2"])
@pytest.mark.parametrize("with_rc", [0, 1], ids=["norc", "rc"])
@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("B", [1, 4])
@pytest.mark.parametrize("nh", [1, 4])
def test_loss_finalize_against_fp64_restatement(nh, B, C, with_rc, M):
    """one lane per (head, b, c) cell, lane 0 adds the Dice terms in the serial order: every coefficient equals the fp64 restatement after the cast to float32,
    the loss agrees to 1 ulp of float32 (the 64-lane Gram sum and fused multiply-adds of the total may differ in the last fp64 bits)"""
    from veloxseg_amd import _hip as H
    d = dev()
    V, Cg, w_rc, w_f = 32 ** 3, 16, 0.7, 0.3
    g = torch.Generator().manual_seed(100 * nh + 10 * B + C)
    acc = (torch.rand(nh * (1 + B * C * 3), generator=g, dtype=F64) + 0.05) * V          # positive accumulators: ce_sum, (I, P, T) x (b, c)
    rc = (torch.rand(1, generator=g, dtype=F64) + 0.1) * 1000.0
    wds = torch.tensor([1.0, 0.5, 0.25, 0.125][:nh])
    gs = rnd(B, Cg, Cg, seed=1)
    gm = [rnd(B, Cg, Cg, seed=2 + m) for m in range(M)]
    n_rc = B * 2 * V
    coef = torch.full((nh * (1 + B * C * 2) + 2,), float("nan"), device=d)
    loss = torch.full((1,), float("nan"), device=d)
    gsd, gmd, accd, wdsd, rcd = gs.to(d), [t.to(d) for t in gm], acc.to(d), wds.to(d), rc.to(d)
    H.call("vx_loss_finalize", H.P(accd, F64), nh, B, C, V, H.P(wdsd), H.P(rcd, F64) if with_rc else None, n_rc, w_rc,
           H.P(gsd) if M else None, *([H.P(t) for t in gmd] + [None] * (4 - M)), M, Cg, w_f, H.P(loss), H.P(coef), H.stream_ptr())
    torch.cuda.synchronize()
    total, coef_ref = _finalize_restated(acc.numpy(), nh, B, C, V, wds.numpy(), rc.numpy()[0] if with_rc else None, n_rc, np.float32(w_rc),
                                         gs.numpy(), [t.numpy() for t in gm], np.float32(w_f))
    assert np.array_equal(coef.cpu().numpy(), coef_ref), np.abs(coef.cpu().numpy() - coef_ref).max()
    want = torch.tensor([np.float32(total)])
    assert bool(((loss.cpu() - want).abs() <= ulp32(want)).all()), (float(loss), float(total))


# ---------------------------------------------------------------------------------------------------------------------- register budget (needs only the build)
def test_stream_kernel_register_budget():
    """vx_patch4_wgrad_k (64 sums and 20 loads of 16 bytes per lane), the Gram kernels (up to 32 rows of 16 bytes per thread backward), the InstanceNorm apply kernels
    (up to 16 loads of 16 bytes in flight per thread) and the finalisation: no scratch, no spilled VGPRs, VGPRs + AGPRs within one wave per SIMD (512).  Reads the
    resource metadata only."""
    obj = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "veloxseg_amd", "lib", "obj")
    want = {"pointwise.s": ["vx_patch4_wgrad_k"], "loss.s": ["vx_gram_fwd_k", "vx_gram_bwd_k", "vx_loss_finalize_k"], "norm.s": ["vx_in_apply_fwd_fin_k", "vx_in_bwd_apply_fin_k"]}
    if not all(os.path.exists(os.path.join(obj, f)) for f in want):
        pytest.skip("the build left no assembly (veloxseg_amd/lib/obj/*.s)")
    for f, kernels in want.items():
        text = open(os.path.join(obj, f)).read()
        entries = re.split(r"\n  - ", text[text.index("amdhsa.kernels:"):])
        seen = set()
        for ent in entries:
            name = re.search(r"\.name:\s+(\S+)", ent)
            hit = [k for k in kernels if name is not None and k in name.group(1)]
            if not hit:
                continue
            seen.add(hit[0])
            num = lambda key: (lambda m_: None if m_ is None else int(m_.group(1)))(re.search(r"\." + key + r":\s+(\d+)", ent))
            assert num("private_segment_fixed_size") == 0, (name.group(1), "scratch", num("private_segment_fixed_size"))
            assert num("vgpr_spill_count") == 0, (name.group(1), "spilled VGPRs", num("vgpr_spill_count"))
            assert num("vgpr_count") + (num("agpr_count") or 0) <= 512, (name.group(1), "registers", num("vgpr_count"), num("agpr_count"))
        assert seen == set(kernels), f"{f}: expected {kernels} in the metadata, found {sorted(seen)}"
