"""The channel-MLP backward kernel (csrc/mlp.hip, vx_mlp_bwd_k) at the volumes where a wave owns 64 voxels (TPW = 4, V >= 16384): blocks of four waves below
V = 32768 and of eight waves from there on, h = gelu(a) mask1 and da formed once and handed to the weight-gradient products through per-wave LDS tiles.

  - V = 16384 (the smallest TPW = 4 volume), R = 48 and 32: the FFN tail (the NORM = 1 instance, which no other test file reaches with TPW = 4) against the
    oracle with dropout off, and against the per-operator kernels with dropout on (the masks of both sites are the same bits in both layouts);
  - V = 32916 = 32768 + 148 (a multiple of 4, not of 64 or 512: a partly live wave, lanes redirected to V - 4, waves past the end) through the C ABI with
    norm = 0 against the fp64 restatement tests/bf16_ref.py::mlp_bwd;
  - a sample's dn / part_out do not depend on what it is batched with, and two calls give the same bits (no atomics feed them);
  - (no GPU) the register budget of every vx_mlp_bwd_k instance, from the assembly build() leaves: no scratch, no spills, two waves per SIMD."""
import os
import re

import pytest
import torch

import bf16_ref as R

C = 16


def _close(a, b, atol, rtol, what):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    print(f"[mlp-wide] {what}: max abs err {float(err.max()):.3e}, ref max {float(b.abs().max()):.3e}, worst err / tol {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    if not bool((err <= tol).all()):
        i = int((err - tol).argmax())
        raise AssertionError(f"{what}: max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e}); worst idx {i}: got {float(a.flatten()[i]):.6e} "
                             f"want {float(b.flatten()[i]):.6e}; bad frac {float((err > tol).double().mean()):.3e}")


def _ffn_modules(r, p, seed):
    from veloxseg_amd.model.components.attention_utils import FFN, LayerNorm
    from veloxseg_amd import functional as VF
    torch.manual_seed(seed)
    VF.reset_dropout_sites()
    ffn = FFN(C, expansion_ratio=r, dropout_rate=p)
    ln = LayerNorm(C)
    with torch.no_grad():
        for q in list(ffn.parameters()) + list(ln.parameters()):
            q.copy_(torch.randn_like(q) * 0.3 + (1.0 if q is ln.weight else 0.0))
    return ffn, ln


FFN_SP = (16, 32, 32)          # V = 16384


@pytest.mark.gpu
@pytest.mark.parametrize("r", [3, 2], ids=["R48", "R32"])
def test_ffn_tail_at_the_smallest_wide_volume_vs_oracle(r):
    """y + FFN(LN(y)) fused == oracle (p = 0); pattern and tolerances of test_fused_blocks_gpu.py::test_fused_ffn_tail_vs_oracle"""
    from oracle import veloxseg_oracle as O
    from veloxseg_amd import functional as VF
    from veloxseg_amd import _hip as H
    assert H.query("vx_mlp_supported", C, C * r, 16384) == 1
    cm = VF.cpp_module()
    cm.set_fuse_blocks(True)
    ffn, ln = _ffn_modules(r, 0.0, 4)
    ffn, ln = ffn.cuda().train(), ln.cuda().train()
    y = torch.randn(2, C, *FFN_SP, generator=torch.Generator().manual_seed(8))
    yg = y.cuda().requires_grad_(True)
    out = VF.ffn_tail(yg, ln, ffn, 0.0)
    gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    out.backward(gy.cuda())
    torch.cuda.synchronize()
    sd = {"f." + k: v.detach().clone().cpu().requires_grad_(True) for k, v in ffn.state_dict().items()}
    lw, lb = ln.weight.detach().clone().cpu().requires_grad_(True), ln.bias.detach().clone().cpu().requires_grad_(True)
    yc = y.clone().requires_grad_(True)
    ref = yc + O.ffn(O.layernorm_cf(yc, lw, lb), sd, "f.", 0.0, True)
    ref.backward(gy)
    _close(out, ref, 2e-4, 2e-4, "ffn out")
    _close(yg.grad, yc.grad, 1e-3 * float(yc.grad.abs().max()), 1e-3, "ffn dy")
    for k, p in ffn.named_parameters():
        g = sd["f." + k].grad
        _close(p.grad, g, 2e-3 * float(g.abs().max()) + 1e-6, 2e-3, f"ffn d{k}")
    _close(ln.weight.grad, lw.grad, 2e-3 * float(lw.grad.abs().max()), 2e-3, "dgamma")
    _close(ln.bias.grad, lb.grad, 2e-3 * float(lb.grad.abs().max()), 2e-3, "dbeta")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [3, 2], ids=["R48", "R32"])
def test_ffn_tail_at_the_smallest_wide_volume_equals_per_operator_kernels_with_dropout(r):
    """pattern and tolerances of test_fused_blocks_gpu.py::test_fused_ffn_tail_equals_per_operator_kernels_with_dropout"""
    from veloxseg_amd import functional as VF
    cm = VF.cpp_module()
    res = {}
    try:
        for fused in (True, False):
            cm.set_fuse_blocks(fused)
            ffn, ln = _ffn_modules(r, 0.1, 4)
            ffn, ln = ffn.cuda().train(), ln.cuda().train()
            VF.manual_seed(91, "cuda")
            y = torch.randn(2, C, *FFN_SP, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_(True)
            out = VF.ffn_tail(y, ln, ffn, 0.1)
            gy = torch.randn(out.shape, generator=torch.Generator().manual_seed(9)).cuda()
            out.backward(gy)
            torch.cuda.synchronize()
            res[fused] = (out.detach().clone(), y.grad.clone(), {k: p.grad.clone() for k, p in list(ffn.named_parameters()) + [("ln." + n, q) for n, q in ln.named_parameters()]})
    finally:
        cm.set_fuse_blocks(True)
    _close(res[True][0], res[False][0], 1e-4, 1e-4, "out")
    _close(res[True][1], res[False][1], 1e-3 * float(res[False][1].abs().max()), 1e-3, "dy")
    for k in res[True][2]:
        g = res[False][2][k]
        _close(res[True][2][k], g, 2e-3 * float(g.abs().max()) + 1e-6, 2e-3, f"d{k}")


# ---------------------------------------------------------------------------------------------------------------------- C ABI, norm = 0
V_RAGGED = 32768 + 148


def _abi_inputs(B, Rr, V, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, V, generator=g) * 1.2 + 0.8).cuda()
    w1 = (torch.randn(Rr, C, generator=g) * 0.3).cuda()
    b1 = (torch.randn(Rr, generator=g) * 0.1).cuda()
    w2 = (torch.randn(C, Rr, generator=g) * 0.3).cuda()
    dout = torch.randn(B, C, V, generator=g).cuda()
    stats = R.row_stats(x.double().view(B * C, V)).float().contiguous()
    return x, stats, w1, b1, w2, dout


def _abi_bwd(x, stats, w1, b1, w2, dout, p, seed_t, grads=None):
    """vx_mlp_bwd (norm = 0) -> dn, part_out (B * C, nparts, 2), [dw1, db1, dw2, db2]; the outputs are pre-filled with NaN, the gradients with `grads` or zero"""
    from veloxseg_amd import _hip as H
    B, _, V = x.shape
    Rr = w1.shape[0]
    npo = H.query("vx_mlp_bwd_nparts", B, C, V)
    dn = torch.full_like(x, float("nan"))
    part = torch.full((B * C, npo, 2), float("nan"), device="cuda")
    gr = [torch.zeros(s, device="cuda") if grads is None else grads[i].clone() for i, s in enumerate(((Rr, C), (Rr,), (C, Rr), (C,)))]
    H.call("vx_mlp_bwd", H.P(x), 0, H.P(stats), None, None, H.P(w1), H.P(b1), H.P(w2), H.P(dout), H.P(dn), H.P(part), None, None,
           H.P(gr[0]), H.P(gr[1]), H.P(gr[2]), H.P(gr[3]), B, C, Rr, V, R.EPS, seed_t.data_ptr(), 1, p, 2, p, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dn, part, gr


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("Rr", [48, 32], ids=["R48", "R32"])
def test_ragged_volume_through_the_c_abi_vs_fp64(Rr):
    """V = 32916, norm = 0, no dropout.
    dn bound: dn = W1^T da is the end of three chained fp32 products (K = 16, 16 and Rr) with GELU' (absolute error <= 2e-7 of the Abramowitz-Stegun form in vx_common.h)
    between them.  Worst-case rounding of a K-term fp32 dot product is K 2^-24 of the sum of |terms|; (16 + 16 + 48) 2^-24 = 4.8e-6, and for these inputs the sum of
    |terms| of the last product reaches ~10 x the largest |dn|: 1e-4 of the scale of dn, plus 1e-4 |ref| for what the errors of the inner products carry through.
    The weight and bias gradients use the bars of test_bf16_storage_ops_gpu.py (2e-3 scale + 1e-6 + 2e-3 |ref|), part_out its _sum_tol."""
    from veloxseg_amd import _hip as H
    B, V = 2, V_RAGGED
    assert H.query("vx_mlp_supported", C, Rr, V) == 1
    x, stats, w1, b1, w2, dout = _abi_inputs(B, Rr, V, 51)
    seed_t = torch.zeros(2, dtype=torch.int64, device="cuda")
    g = torch.Generator().manual_seed(52)
    inits = [torch.randn(s, generator=g).cuda() for s in ((Rr, C), (Rr,), (C, Rr), (C,))]
    dn, part, gr = _abi_bwd(x, stats, w1, b1, w2, dout, 0.0, seed_t, inits)
    dn_ref, dw1r, db1r, dw2r, db2r, nhat = R.mlp_bwd(x.double(), stats.double(), w1.double(), b1.double(), w2.double(), dout.double())
    sc = float(dn_ref.abs().max())
    mult = R.held(dn, dn_ref, 1e-4 * sc + 1e-4 * dn_ref.abs(), "dn vs fp64")
    print(f"[mlp-wide] C-ABI R={Rr} dn: worst err / tol {mult:.3f}")
    for i, (ref, what) in enumerate(((dw1r, "dw1"), (db1r, "db1"), (dw2r, "dw2"), (db2r, "db2"))):
        s = float(ref.abs().max())
        mult = R.held(gr[i], inits[i].double() + ref, 2e-3 * s + 1e-6 + 2e-3 * ref.abs(), f"{what} vs fp64")
        print(f"[mlp-wide] C-ABI R={Rr} {what}: worst err / tol {mult:.3f}")
    assert part.shape[1] == H.query("vx_mlp_bwd_nparts", B, C, V)
    dxs = dn.double().view(B * C, V)
    nh = nhat.reshape(B * C, V)
    fold = part.double().sum(1)
    sum_tol = lambda terms, ref: 1e-5 * ref.abs() + 2e-6 * terms.abs().sum(-1)      # (_sum_tol of test_bf16_storage_ops_gpu.py)
    R.held(fold[:, 0], dxs.sum(-1), sum_tol(dxs, dxs.sum(-1)), "part_out: sum dn over the stored dn")
    R.held(fold[:, 1], (dxs * nh).sum(-1), sum_tol(dxs * nh, (dxs * nh).sum(-1)), "part_out: sum dn nhat over the stored dn")


@pytest.mark.gpu
@pytest.mark.parametrize("V", [16384, V_RAGGED], ids=["4waves", "8waves_ragged"])
def test_a_sample_does_not_depend_on_its_batch_and_calls_repeat(V):
    """sample 0 alone (B = 1) and as sample 0 of B = 3 (dropout on: its masks are indexed by (b, row, voxel)): bit-identical dn and part_out rows; and the B = 3 call
    twice: bit-identical dn and part_out"""
    Rr = 48
    x, stats, w1, b1, w2, dout = _abi_inputs(3, Rr, V, 61)
    seed_t = torch.tensor([1234, 5], dtype=torch.int64, device="cuda")
    dn3, part3, _ = _abi_bwd(x, stats, w1, b1, w2, dout, 0.1, seed_t)
    dn3b, part3b, _ = _abi_bwd(x, stats, w1, b1, w2, dout, 0.1, seed_t)
    dn1, part1, _ = _abi_bwd(x[:1].contiguous(), stats[:C].contiguous(), w1, b1, w2, dout[:1].contiguous(), 0.1, seed_t)
    assert not bool(torch.isnan(dn3).any()) and not bool(torch.isnan(part3).any()), "an element of dn / part_out was never written"
    assert float((dn3 == 0).float().mean()) < 0.01, "dropout is on: dn must not be trivially zero"
    assert torch.equal(_bits(dn3), _bits(dn3b)) and torch.equal(_bits(part3), _bits(part3b)), "two calls with the same inputs differ"
    assert torch.equal(_bits(dn1[0]), _bits(dn3[0])), "dn of a sample depends on its batch"
    assert torch.equal(_bits(part1), _bits(part3[:C])), "part_out of a sample depends on its batch"


# ---------------------------------------------------------------------------------------------------------------------- register budget (needs only the build)
def test_backward_kernel_register_budget():
    """every vx_mlp_bwd_k instance: no scratch, no spilled VGPRs, and VGPRs + AGPRs <= 256 (two waves per SIMD).  Reads the resource metadata only."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "veloxseg_amd", "lib", "obj", "mlp.s")
    if not os.path.exists(path):
        pytest.skip("the build left no assembly for mlp (veloxseg_amd/lib/obj/mlp.s)")
    text = open(path).read()
    meta = text[text.index("amdhsa.kernels:"):]
    entries = re.split(r"\n  - ", meta)
    seen = 0
    for ent in entries:
        name = re.search(r"\.name:\s+(\S+)", ent)
        if name is None or "vx_mlp_bwd_k" not in name.group(1):
            continue
        seen += 1
        num = lambda key: (lambda m_: None if m_ is None else int(m_.group(1)))(re.search(r"\." + key + r":\s+(\d+)", ent))
        vg, ag = num("vgpr_count"), num("agpr_count")
        assert num("private_segment_fixed_size") == 0, (name.group(1), "scratch", num("private_segment_fixed_size"))
        assert num("vgpr_spill_count") == 0, (name.group(1), "spilled VGPRs", num("vgpr_spill_count"))
        assert vg is not None and vg + (ag or 0) <= 256, (name.group(1), "registers", vg, ag)
    assert seen >= 12, f"expected every vx_mlp_bwd_k instance in the metadata, found {seen}"
