"""The bf16 STORAGE mode's own C-ABI entries (the 17 `*_h` entries of include/veloxseg_hip.h, round 6; BASELINE configs[1]) against element-wise fp64 oracles.

The oracle (tests/bf16_ref.py; its host half is checked by tests/test_bf16_ref_cpu.py):
  - inputs are drawn as fp32 on the CPU and rounded with `.bfloat16()` (nearest even, what the kernels' `(__bf16)x` does); the kernel gets the bf16 tensor, the
    reference the same values in fp64.  Matrix-pipe kernels that round operands themselves (the Toeplitz entries with pieces = 1, the patch-expand `_bf16_h`
    entries) get the same rounding on the host, so that the reference's products are the kernel's products;
  - an output stored as bf16 is held to |got - ref64| <= 2^-8 |ref64| + 3 e32, element-wise: half a bf16 ulp + 3 x the error e32 of the SAME entry with
    h16 = 0 on the widened inputs (measured in the test, printed);
  - an output that stays fp32 is held to the tolerance of the sibling fp32 test (the inputs are identical: bf16 contributes nothing);
  - 16-bit outputs are pre-filled with NaN (an element that is never written fails), every output sits between two 64-element canaries (a store of fp32-sized
    elements, or one past a ragged end, fails), `*_h(h16 = 0)` must be bit-identical to the plain fp32 entry, and one case per element-wise kernel runs with its
    16-bit base pointers 8-byte but not 16-byte aligned (element 4 of a larger buffer: how the engine carves y1 / y3 / y5 out of one allocation).
Every line printed with the tag [bf16-ops] carries e32 and the worst observed multiple of the bound."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

import bf16_ref as R
from exact_ref import CANARY, NAN, Guard      # (the canary-fenced output buffer lives with the exact oracles: tests/exact_ref.py)

pytestmark = pytest.mark.gpu


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _h16_in(t32, shift=0):
    """CPU fp32 -> (bf16 device tensor the kernel reads [optionally at element `shift` of a larger buffer], the same values in fp64 on the device)"""
    tb = t32.bfloat16()
    if shift:
        buf = torch.zeros(tb.numel() + shift, dtype=torch.bfloat16, device="cuda")
        dev = buf[shift:].view(tb.shape)
        dev.copy_(tb)
        assert dev.data_ptr() % 16 == 8
    else:
        dev = tb.cuda()
    return dev, R.widen(dev)


def _report(kernel, case, what, e32, mult):
    print(f"[bf16-ops] {kernel} {case} {what}: e32 = {e32:.3e}, worst multiple of the bf16 bound = {mult:.3f}")


def _held_bf16(got, ref64, got32, kernel, case, what):
    """the bf16 bound with e32 measured from the fp32-storage run of the same entry; got32 = None: the fp32 run does not exist (e32 = 0)"""
    assert got.dtype == torch.bfloat16
    e32 = float((R.widen(got32) - ref64).abs().max()) if got32 is not None else 0.0
    mult = R.held(got, ref64, R.bf16_bound(ref64, e32), f"{kernel} {case} {what}")
    _report(kernel, case, what, e32, mult)
    return e32


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------- 1. vx_patchify_bs_h
@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("B,C,Ctot,c_off,grid,shift", [(2, 2, 5, 2, (3, 5, 6), 0), (1, 4, 6, 1, (2, 2, 2), 0), (2, 2, 5, 2, (3, 5, 6), 4)], ids=["b2c2_3x5x6", "b1c4_2x2x2", "b2c2_8byte_base"])
def test_patchify_16bit_copy_is_the_rounded_fp32_copy(K, B, C, Ctot, c_off, grid, shift):
    """vx_patchify_bs_h (out_h16 = 1) of a channel slice of a wider tensor == .bfloat16() of vx_patchify_bs, bit for bit; and both == the permutation itself"""
    H = _H()
    d, h, w = grid
    x = torch.randn(B, Ctot, d * K, h * K, w * K, generator=_gen(7)).cuda()
    Vin = d * h * w * K ** 3
    xp, bstride = x.data_ptr() + 4 * c_off * Vin, Ctot * Vin
    o32, o32h, o16 = Guard((B, C * K ** 3, d, h, w)), Guard((B, C * K ** 3, d, h, w)), Guard((B, C * K ** 3, d, h, w), torch.bfloat16, shift=shift)
    H.call("vx_patchify_bs", xp, bstride, o32.ptr, B, C, d, h, w, K, _st())
    H.call("vx_patchify_bs_h", xp, bstride, o32h.ptr, B, C, d, h, w, K, 0, _st())
    H.call("vx_patchify_bs_h", xp, bstride, o16.ptr, B, C, d, h, w, K, 1, _st())
    torch.cuda.synchronize()
    for g_, n_ in ((o32, "fp32"), (o32h, "_h fp32"), (o16, "_h bf16")):
        g_.check(f"patchify {n_}")
    xs = x[:, c_off:c_off + C]
    want = xs.view(B, C, d, K, h, K, w, K).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(B, C * K ** 3, d, h, w)
    assert torch.equal(o32.t, want), "vx_patchify_bs is not the permutation"
    assert torch.equal(_bits(o32h.t), _bits(o32.t)), "vx_patchify_bs_h(out_h16 = 0) differs from vx_patchify_bs"
    bad = _bits(o16.t) != _bits(o32.t.bfloat16())
    assert not bool(bad.any()), f"16-bit patchify: {int(bad.sum())} of {bad.numel()} elements differ from bf16(fp32 copy); first flat index {int(bad.flatten().nonzero()[0])}"


# ---------------------------------------------------------------------------------------------------------------------- 2. vx_pw_conv_fwd_h / vx_pw_conv_bwd_weight_h
PW_CASES = [
    # name, Cin, Cout, V, shift   (B = 2)
    ("v4_cinb16", 64, 16, 16384, 0),          # one-wave 16-byte kernel, <16> instance
    ("v4_cinb32", 32, 32, 16384, 0),          # ... <32> instance
    ("v4_8byte_base", 64, 16, 16384, 4),
    ("general_c128", 128, 16, 1000, 0),
    ("general_odd_v", 256, 6, 1001, 0),       # odd V: the scalar loop of the weight gradient; Cout no multiple of 4
    ("general_c8_v60", 8, 16, 60, 0),
    ("general_8byte_base", 128, 16, 1000, 4),
]


@pytest.mark.parametrize("case", PW_CASES, ids=[c[0] for c in PW_CASES])
def test_pw_conv_with_16bit_input_vs_fp64(case):
    """y = W x + b and dW += dy x^T, db += sum dy with x a bf16 array: against fp64 on the same x to the tolerances of test_conv3d's run_pair (y: 2e-5 + 2e-4 |ref|;
    parameters: 1e-4 max(1, max|g|) + 4e-3 |ref|), and against the x_h16 = 0 entry on the widened x (the same products: 2e-6 of the maximum, the v4-vs-scalar bound)"""
    H = _H()
    name, Cin, Cout, V, shift = case
    B = 2
    xh, x64 = _h16_in(torch.randn(B, Cin, V, generator=_gen(11)), shift)
    x32 = xh.float()
    w = (torch.randn(Cout, Cin, generator=_gen(12)) * Cin ** -0.5).cuda()
    b = (torch.randn(Cout, generator=_gen(13)) * 0.1).cuda()
    dy = torch.randn(B, Cout, V, generator=_gen(14)).cuda()
    y_h, y_0, y_p = Guard((B, Cout, V)), Guard((B, Cout, V)), Guard((B, Cout, V))
    H.call("vx_pw_conv_fwd_h", H.P(xh, None), H.P(w), H.P(b), y_h.ptr, B, Cin, Cout, V, 1, _st())
    H.call("vx_pw_conv_fwd_h", H.P(x32), H.P(w), H.P(b), y_0.ptr, B, Cin, Cout, V, 0, _st())
    H.call("vx_pw_conv_fwd", H.P(x32), None, 0, H.P(w), H.P(b), y_p.ptr, B, Cin, Cout, V, _st())
    dw0 = torch.randn(Cout, Cin, generator=_gen(15)).cuda()
    db0 = torch.randn(Cout, generator=_gen(16)).cuda()
    dw_h, dw_0, dw_p = Guard((Cout, Cin), fill=dw0), Guard((Cout, Cin), fill=dw0), Guard((Cout, Cin), fill=dw0)
    db_h, db_0, db_p = Guard((Cout,), fill=db0), Guard((Cout,), fill=db0), Guard((Cout,), fill=db0)
    H.call("vx_pw_conv_bwd_weight_h", H.P(xh, None), H.P(dy), dw_h.ptr, db_h.ptr, B, Cin, Cout, V, 1, _st())
    H.call("vx_pw_conv_bwd_weight_h", H.P(x32), H.P(dy), dw_0.ptr, db_0.ptr, B, Cin, Cout, V, 0, _st())
    H.call("vx_pw_conv_bwd_weight", H.P(x32), None, 0, H.P(dy), dw_p.ptr, db_p.ptr, B, Cin, Cout, V, _st())
    torch.cuda.synchronize()
    for g_ in (y_h, y_0, y_p, dw_h, dw_0, dw_p, db_h, db_0, db_p):
        g_.check(f"pw {name}")
    yref = torch.einsum("oi,biv->bov", w.double(), x64) + b.double().view(1, -1, 1)
    R.held(y_h.t, yref, 2e-5 + 2e-4 * yref.abs(), f"pw fwd {name} vs fp64")
    ymax = float(yref.abs().max())
    R.held(y_h.t, R.widen(y_0.t), 2e-6 * ymax, f"pw fwd {name}: 16-bit x vs the widened x")
    assert torch.equal(_bits(y_0.t), _bits(y_p.t)), "vx_pw_conv_fwd_h(x_h16 = 0) differs from vx_pw_conv_fwd"
    dwref = dw0.double() + torch.einsum("bov,biv->oi", dy.double(), x64)
    dbref = db0.double() + dy.double().sum((0, 2))
    for got, got0, gotp, ref, what in ((dw_h.t, dw_0.t, dw_p.t, dwref, "dw"), (db_h.t, db_0.t, db_p.t, dbref, "db")):
        sc = max(1.0, float(ref.abs().max()))
        R.held(got, ref, 1e-4 * sc + 4e-3 * ref.abs(), f"pw {what} {name} vs fp64")
        R.held(got, R.widen(got0), 2e-6 * float(ref.abs().max()), f"pw {what} {name}: 16-bit x vs the widened x")
        R.held(got0, R.widen(gotp), 2e-6 * float(ref.abs().max()), f"pw {what} {name}: _h(x_h16 = 0) vs the plain entry (atomics: summation order only)")


# ---------------------------------------------------------------------------------------------------------------------- 3. vx_sqdiff_sum_grad_bs_h
@pytest.mark.parametrize("n,shift", [(3 * 4096 + 20, 0), (8, 0), (4099, 0), (3 * 4096 + 20, 4)], ids=["vector_pairs_and_tail", "vector_n8", "scalar_odd_n", "scalar_8byte_base"])
def test_sqdiff_sum_grad_16bit_reconstruction(n, shift):
    """acc += sum (a - b)^2, da = bf16(scale (a - b)) with a, da bf16 arrays and b a batch-strided fp32 slice: da bit-exact (one fp32 subtraction, one fp32
    product, one rounding), acc to 1e-6 of the fp64 sum on top of its non-zero start value"""
    H = _H()
    B, bstride = 2, n + 12
    ah, a64 = _h16_in(torch.randn(B, n, generator=_gen(21)), shift)
    bfull = torch.randn(B, bstride, generator=_gen(22)).cuda()
    scale = float(torch.tensor(2.0 * 0.3 / 12345.0, dtype=torch.float32))
    acc0 = 7.25
    want_da = (torch.tensor(scale, device="cuda") * (ah.float() - bfull[:, :n])).bfloat16()
    want_acc = acc0 + float(((a64 - bfull[:, :n].double()) ** 2).sum())
    da_h = Guard((B, n), torch.bfloat16, shift=shift)
    acc_h = Guard((1,), torch.float64, fill=acc0)
    H.call("vx_sqdiff_sum_grad_bs_h", H.P(ah, None), H.P(bfull), n, bstride, B, acc_h.ptr, scale, da_h.ptr, 1, _st())
    a32 = ah.float()
    da_0, da_p = Guard((B, n)), Guard((B, n))
    acc_0, acc_p = Guard((1,), torch.float64, fill=acc0), Guard((1,), torch.float64, fill=acc0)
    H.call("vx_sqdiff_sum_grad_bs_h", H.P(a32), H.P(bfull), n, bstride, B, acc_0.ptr, scale, da_0.ptr, 0, _st())
    H.call("vx_sqdiff_sum_grad_bs", H.P(a32), H.P(bfull), n, bstride, B, acc_p.ptr, scale, da_p.ptr, _st())
    torch.cuda.synchronize()
    for g_ in (da_h, acc_h, da_0, da_p, acc_0, acc_p):
        g_.check(f"sqdiff n={n}")
    bad = _bits(da_h.t) != _bits(want_da)
    assert not bool(bad.any()), (f"da: {int(bad.sum())} of {bad.numel()} elements are not bf16(scale (a - b)); first flat index {int(bad.flatten().nonzero()[0])}: "
                                 f"got {float(da_h.t.flatten()[int(bad.flatten().nonzero()[0])])} want {float(want_da.flatten()[int(bad.flatten().nonzero()[0])])}")
    assert abs(float(acc_h.t) - want_acc) <= 1e-6 * abs(want_acc), (float(acc_h.t), want_acc)
    assert torch.equal(_bits(da_0.t), _bits(da_p.t)), "vx_sqdiff_sum_grad_bs_h(a_h16 = 0) differs from vx_sqdiff_sum_grad_bs"
    assert abs(float(acc_0.t) - float(acc_p.t)) <= 1e-12 * abs(want_acc)          # (double atomics of identical block sums: order only)
    assert abs(float(acc_0.t) - want_acc) <= 1e-6 * abs(want_acc)


# ---------------------------------------------------------------------------------------------------------------------- 4. vx_jlc_mid_fwd_h / vx_jlc_mid_bwd_h / vx_jlc_gk_h
MID_CASES = [("bc32_v1728", 32, 1728, 0), ("bc16_v1920", 16, 1920, 0), ("bc8_v68", 8, 68, 0), ("bc16_v32768_8chunks", 16, 32768, 0), ("bc16_v1920_8byte_base", 16, 1920, 4)]


def _sum_tol(terms64, ref):
    """a fp32 sum of the given terms against its fp64 value: 1e-5 relative, + 2e-6 of sum |terms| where the sum cancels (the conditioning of the sum: every term
    carries up to ~3e-7 relative error of the fp32 GELU' / normalisation in front of it, and the fp32 partial sums up to a few 2^-24 of sum |terms| more)"""
    return 1e-5 * ref.abs() + 2e-6 * terms64.abs().sum(-1)


@pytest.mark.parametrize("case", MID_CASES, ids=[c[0] for c in MID_CASES])
def test_jlc_spatial_stage_with_16bit_tensors_vs_fp64(case):
    """o, d_o, g_k (stored bf16) to the bf16 bound; stats_y to fp32 rounding; part_o / part_t fold to the sums over the values the kernel STORED"""
    H = _H()
    name, BC, V, shift = case
    nch = H.query("vx_jlc_nchunks", BC, V)
    assert nch == (8 if V == 32768 else 2 if V > 1024 else 1)
    x, y = R.mid_inputs(BC, V, 41)
    g = _gen(42)
    x = x.cuda()
    yh_, y64 = _h16_in(y.float(), shift)
    nty = 3
    part_y = R.partials(y64, nty).contiguous()                       # (3, BC, nty, 2) doubles: exact sums of the values the kernel reads
    stats_y64 = torch.stack([R.row_stats(y64[k]) for k in range(3)])
    ps = [yh_[k].data_ptr() for k in range(3)]
    y32 = yh_.float()
    # ---- forward
    o_ref = R.jlc_mid_fwd(x.double(), y64, stats_y64)
    res = {}
    for h16 in (1, 0):
        o = Guard((BC, V), torch.bfloat16 if h16 else torch.float32, shift=shift if h16 else 0)
        st_y, p_o = Guard((3, BC, 2)), Guard((BC, nch, 2), torch.float64)
        yp = ps if h16 else [y32[k].data_ptr() for k in range(3)]
        H.call("vx_jlc_mid_fwd_h", H.P(x), *yp, part_y.data_ptr(), nty, st_y.ptr, o.ptr, p_o.ptr, BC, V, R.EPS, h16, _st())
        res[h16] = (o, st_y, p_o)
    o_p, st_p, p_p = Guard((BC, V)), Guard((3, BC, 2)), Guard((BC, nch, 2), torch.float64)
    H.call("vx_jlc_mid_fwd", H.P(x), *[y32[k].data_ptr() for k in range(3)], part_y.data_ptr(), nty, st_p.ptr, o_p.ptr, p_p.ptr, BC, V, R.EPS, _st())
    torch.cuda.synchronize()
    for h16 in (1, 0):
        for g_ in res[h16]:
            g_.check(f"mid_fwd {name} h16={h16}")
    o_h, o_0 = res[1][0].t, res[0][0].t
    assert torch.equal(_bits(o_0), _bits(o_p.t)) and torch.equal(_bits(res[0][1].t), _bits(st_p.t)) and torch.equal(res[0][2].t, p_p.t), "vx_jlc_mid_fwd_h(h16 = 0) differs from vx_jlc_mid_fwd"
    _held_bf16(o_h, o_ref, o_0, "vx_jlc_mid_fwd_h", name, "o")
    R.held(res[1][1].t, stats_y64, 1e-6 + 1e-5 * stats_y64.abs(), f"mid_fwd {name} stats_y")
    oh64 = R.widen(o_h)
    fold = res[1][2].t.sum(1)
    want = torch.stack([oh64.sum(-1), (oh64 * oh64).sum(-1)], -1)
    R.held(fold, want, 1e-5 * want.abs(), f"mid_fwd {name} part_o vs the sums of the STORED o")
    if name == "bc32_v1728":
        # ... and NOT the sums of the unrounded fp32 o: where the two differ clearly (tests/test_bf16_ref_cpu.py: a quarter of the rows for this seed), part_o sides with the rounded one
        o064 = R.widen(o_0)
        other = torch.stack([o064.sum(-1), (o064 * o064).sum(-1)], -1)
        clear = (want - other).abs() > 3e-5 * want.abs()
        assert int(clear[:, 0].sum()) >= BC // 4 and int(clear[:, 1].sum()) >= BC // 4
        assert bool(((fold - other).abs() > 1e-5 * other.abs())[clear].all()), "part_o folds to the statistics of the UNROUNDED o"
    # ---- backward: d_o and the partial sums of t_k
    dout = torch.randn(BC, V, generator=g).cuda()
    dnh, dn64 = _h16_in(torch.randn(BC, V, generator=g) * 0.5, shift)
    oin, o64 = _h16_in(o_h.float().cpu(), shift)                      # (the o the forward stored)
    stats_o = R.row_stats(o64).float()
    stats_y = stats_y64.float().contiguous()
    so64, sy64 = stats_o.double(), stats_y.double()
    nhat = (o64 - so64[:, 0:1]) * so64[:, 1:2]
    npd = 2
    part_dn = R.partials(dn64, npd, prod=nhat).float().contiguous()  # (BC, npd, 2) floats
    mean_dn, mean_dnn = part_dn.double()[:, :, 0].sum(1) / V, part_dn.double()[:, :, 1].sum(1) / V
    do_ref = R.jlc_mid_bwd(dout.double(), dn64, mean_dn, mean_dnn, o64, so64)
    res = {}
    for h16 in (1, 0):
        d_o = Guard((BC, V), torch.bfloat16 if h16 else torch.float32, shift=shift if h16 else 0)
        p_t = Guard((3, BC, nch, 2))
        cv = (lambda t: t) if h16 else (lambda t: t.float())
        keep = [cv(dnh), cv(oin), cv(yh_)]
        H.call("vx_jlc_mid_bwd_h", H.P(dout), keep[0].data_ptr(), H.P(part_dn), npd, keep[1].data_ptr(), H.P(stats_o), *[keep[2][k].data_ptr() for k in range(3)],
               H.P(stats_y), d_o.ptr, p_t.ptr, BC, V, h16, _st())
        torch.cuda.synchronize()
        res[h16] = (d_o, p_t)
    d_p, pt_p = Guard((BC, V)), Guard((3, BC, nch, 2))
    dn32, o32 = dnh.float(), oin.float()
    H.call("vx_jlc_mid_bwd", H.P(dout), H.P(dn32), H.P(part_dn), npd, H.P(o32), H.P(stats_o), *[y32[k].data_ptr() for k in range(3)], H.P(stats_y), d_p.ptr, pt_p.ptr, BC, V, _st())
    torch.cuda.synchronize()
    for h16 in (1, 0):
        for g_ in res[h16]:
            g_.check(f"mid_bwd {name} h16={h16}")
    assert torch.equal(_bits(res[0][0].t), _bits(d_p.t)) and torch.equal(_bits(res[0][1].t), _bits(pt_p.t)), "vx_jlc_mid_bwd_h(h16 = 0) differs from vx_jlc_mid_bwd"
    do_h = res[1][0].t
    _held_bf16(do_h, do_ref, res[0][0].t, "vx_jlc_mid_bwd_h", name, "d_o")
    t64, yhat64 = R.jlc_t(R.widen(do_h), y64, sy64)
    fold = res[1][1].t.double().sum(2)                               # (3, BC, 2)
    R.held(fold[..., 0], t64.sum(-1), _sum_tol(t64, t64.sum(-1)), f"mid_bwd {name} part_t: sum t_k over the STORED d_o")
    R.held(fold[..., 1], (t64 * yhat64).sum(-1), _sum_tol(t64 * yhat64, (t64 * yhat64).sum(-1)), f"mid_bwd {name} part_t: sum t_k yhat_k over the STORED d_o")
    # ---- g_k from the stored d_o and caller-folded partial sums
    din, d64 = _h16_in(do_h.float().cpu(), shift)
    t64, yhat64 = R.jlc_t(d64, y64, sy64)
    wts = torch.linspace(1.0, 2.0, nch, dtype=torch.float64, device="cuda")
    wts = wts / wts.sum()
    part_t = (torch.stack([t64.sum(-1), (t64 * yhat64).sum(-1)], -1)[:, :, None, :] * wts.view(1, 1, nch, 1)).float().contiguous()
    mt, mty = part_t.double()[..., 0].sum(2) / V, part_t.double()[..., 1].sum(2) / V
    g_ref = R.jlc_gk(d64, y64, sy64, mt, mty)
    res = {}
    for h16 in (1, 0):
        gk = Guard((3, BC, V), torch.bfloat16 if h16 else torch.float32, shift=shift if h16 else 0)
        cv = (lambda t: t) if h16 else (lambda t: t.float())
        keep = [cv(din), cv(yh_)]
        H.call("vx_jlc_gk_h", keep[0].data_ptr(), *[keep[1][k].data_ptr() for k in range(3)], H.P(stats_y), H.P(part_t), *[gk.t[k].data_ptr() for k in range(3)], BC, V, h16, _st())
        torch.cuda.synchronize()
        res[h16] = gk
    g_p = Guard((3, BC, V))
    d32 = din.float()
    H.call("vx_jlc_gk", H.P(d32), *[y32[k].data_ptr() for k in range(3)], H.P(stats_y), H.P(part_t), *[g_p.t[k].data_ptr() for k in range(3)], BC, V, _st())
    torch.cuda.synchronize()
    res[1].check(f"gk {name}")
    res[0].check(f"gk {name} fp32")
    assert torch.equal(_bits(res[0].t), _bits(g_p.t)), "vx_jlc_gk_h(h16 = 0) differs from vx_jlc_gk"
    for k in range(3):
        _held_bf16(res[1].t[k], g_ref[k], res[0].t[k], "vx_jlc_gk_h", name, f"g{2 * k + 1}")


# ---------------------------------------------------------------------------------------------------------------------- 5. vx_mlp_fwd_h / vx_mlp_bwd_h
MLP_CASES = [(16, Rr, V, 0) for Rr in (48, 32) for V in (64, 1728, 4100)] + [(16, 48, 1728, 4)]      # V = 64: the minimum; 4100: a multiple of 4, not of a block's 64 voxels


@pytest.mark.parametrize("C,Rr,V,shift", MLP_CASES, ids=[f"c{c[0]}_r{c[1]}_v{c[2]}" + ("_8byte_base" if c[3] else "") for c in MLP_CASES])
def test_jlc_channel_stage_with_16bit_tensors_vs_fp64(C, Rr, V, shift):
    """out = x + W2 GELU(W1 IN(x) + b1) + b2 with x (= the block's o) a bf16 array, and its backward with dx (= dn) stored bf16: out and the weight gradients to the
    fp32 tolerances of test_fused_jlc_block_vs_oracle (and to 2e-6 of the maximum against the h16 = 0 entry: the same products on the same values), dx to the
    bf16 bound, part_out against the fp64 sums over the STORED dx"""
    H = _H()
    B = 2
    BC = B * C
    name = f"c{C}_r{Rr}_v{V}" + ("_8byte_base" if shift else "")
    assert H.query("vx_mlp_supported", C, Rr, V) == 1
    g = _gen(51)
    xh, x64 = _h16_in(torch.randn(B, C, V, generator=g) * 1.2 + 0.8, shift)
    w1 = (torch.randn(Rr, C, generator=g) * 0.3).cuda()
    b1 = (torch.randn(Rr, generator=g) * 0.1).cuda()
    w2 = (torch.randn(C, Rr, generator=g) * 0.3).cuda()
    b2 = (torch.randn(C, generator=g) * 0.1).cuda()
    dout = torch.randn(B, C, V, generator=g).cuda()
    seed = torch.zeros(2, dtype=torch.int64, device="cuda")          # {seed, step}: passed as the C++ operator bodies do, with p = 0
    nparts = 2
    part = R.partials(x64.view(BC, V), nparts).contiguous()
    stats64 = R.row_stats(x64.view(BC, V))
    out_ref, _, _ = R.mlp_fwd(x64, stats64, w1.double(), b1.double(), w2.double(), b2.double())
    x32 = xh.float()
    res = {}
    for h16 in (1, 0):
        out, st_o = Guard((B, C, V)), Guard((BC, 2))
        H.call("vx_mlp_fwd_h", (xh if h16 else x32).data_ptr(), 0, part.data_ptr(), nparts, st_o.ptr, None, None, H.P(w1), H.P(b1), H.P(w2), H.P(b2), out.ptr, B, C, Rr, V, R.EPS,
               seed.data_ptr(), 0, 0.0, 0, 0.0, h16, _st())
        res[h16] = (out, st_o)
    out_p, st_p = Guard((B, C, V)), Guard((BC, 2))
    H.call("vx_mlp_fwd", H.P(x32), 0, part.data_ptr(), nparts, st_p.ptr, None, None, H.P(w1), H.P(b1), H.P(w2), H.P(b2), out_p.ptr, B, C, Rr, V, R.EPS, seed.data_ptr(), 0, 0.0, 0, 0.0, _st())
    torch.cuda.synchronize()
    for h16 in (1, 0):
        for g_ in res[h16]:
            g_.check(f"mlp_fwd {name} h16={h16}")
    assert torch.equal(_bits(res[0][0].t), _bits(out_p.t)) and torch.equal(_bits(res[0][1].t), _bits(st_p.t)), "vx_mlp_fwd_h(h16 = 0) differs from vx_mlp_fwd"
    R.held(res[1][0].t, out_ref, 2e-4 + 2e-4 * out_ref.abs(), f"mlp_fwd {name} out vs fp64")
    R.held(res[1][0].t, R.widen(res[0][0].t), 2e-6 * float(out_ref.abs().max()), f"mlp_fwd {name} out: 16-bit x vs the widened x")
    R.held(res[1][1].t, stats64, 1e-6 + 1e-5 * stats64.abs(), f"mlp_fwd {name} stats")
    # ---- backward
    stats = stats64.float().contiguous()
    s64 = stats.double()
    dn_ref, dw1r, db1r, dw2r, db2r, nhat = R.mlp_bwd(x64, s64, w1.double(), b1.double(), w2.double(), dout.double())
    npo = H.query("vx_mlp_bwd_nparts", B, C, V)
    inits = [torch.randn(s_, generator=g).cuda() for s_ in ((Rr, C), (Rr,), (C, Rr), (C,))]
    res = {}
    for h16 in (1, 0):
        dx = Guard((B, C, V), torch.bfloat16 if h16 else torch.float32, shift=shift if h16 else 0)
        p_out = Guard((BC, npo, 2))
        gr = [Guard(t.shape, fill=t) for t in inits]
        H.call("vx_mlp_bwd_h", (xh if h16 else x32).data_ptr(), 0, H.P(stats), None, None, H.P(w1), H.P(b1), H.P(w2), H.P(dout), dx.ptr, p_out.ptr, None, None,
               gr[0].ptr, gr[1].ptr, gr[2].ptr, gr[3].ptr, B, C, Rr, V, R.EPS, seed.data_ptr(), 0, 0.0, 0, 0.0, h16, _st())
        res[h16] = (dx, p_out, gr)
    dx_p, po_p = Guard((B, C, V)), Guard((BC, npo, 2))
    gr_p = [Guard(t.shape, fill=t) for t in inits]
    H.call("vx_mlp_bwd", H.P(x32), 0, H.P(stats), None, None, H.P(w1), H.P(b1), H.P(w2), H.P(dout), dx_p.ptr, po_p.ptr, None, None, gr_p[0].ptr, gr_p[1].ptr, gr_p[2].ptr, gr_p[3].ptr,
           B, C, Rr, V, R.EPS, seed.data_ptr(), 0, 0.0, 0, 0.0, _st())
    torch.cuda.synchronize()
    for h16 in (1, 0):
        for g_ in [res[h16][0], res[h16][1]] + res[h16][2]:
            g_.check(f"mlp_bwd {name} h16={h16}")
    assert torch.equal(_bits(res[0][0].t), _bits(dx_p.t)) and torch.equal(_bits(res[0][1].t), _bits(po_p.t)), "vx_mlp_bwd_h(h16 = 0) differs from vx_mlp_bwd"
    _held_bf16(res[1][0].t, dn_ref, res[0][0].t, "vx_mlp_bwd_h", name, "dx")
    for i, (ref, what) in enumerate(((dw1r, "dw1"), (db1r, "db1"), (dw2r, "dw2"), (db2r, "db2"))):
        sc = float(ref.abs().max())
        want = inits[i].double() + ref
        R.held(res[1][2][i].t, want, 2e-3 * sc + 1e-6 + 2e-3 * ref.abs(), f"mlp_bwd {name} {what} vs fp64")
        R.held(res[1][2][i].t, R.widen(res[0][2][i].t), 1e-5 * sc, f"mlp_bwd {name} {what}: 16-bit x vs the widened x (float atomics: summation order)")
        R.held(res[0][2][i].t, R.widen(gr_p[i].t), 1e-5 * sc, f"mlp_bwd {name} {what}: _h(h16 = 0) vs the plain entry")
    dxs = R.widen(res[1][0].t).view(BC, V)
    nh = nhat.reshape(BC, V)
    fold = res[1][1].t.double().sum(1)
    R.held(fold[:, 0], dxs.sum(-1), _sum_tol(dxs, dxs.sum(-1)), f"mlp_bwd {name} part_out: sum dn over the STORED dx")
    R.held(fold[:, 1], (dxs * nh).sum(-1), _sum_tol(dxs * nh, (dxs * nh).sum(-1)), f"mlp_bwd {name} part_out: sum dn nhat over the STORED dx")


# ---------------------------------------------------------------------------------------------------------------------- 6. vx_jlc_tz_fwd_h / _bwd_h / vx_jlc_wgrad_tz_h
TZ_H_CASES = [
    # name, B, C, groups, spatial (forward + input gradient), spatial of the weight gradient (needs H % 4 == 0), element shift of the 16-bit base pointers
    ("L2_w8_16cube", 2, 32, 4, (16, 16, 16), (16, 16, 16), 0),
    ("L3_w8_8cube", 2, 64, 8, (8, 8, 8), (8, 8, 8), 0),
    ("L4_w16_4cube", 2, 128, 8, (4, 4, 4), (4, 4, 4), 0),
    ("hecktor_L1", 1, 16, 4, (32, 32, 16), (32, 32, 16), 0),
    ("aniso_ragged", 1, 16, 4, (10, 9, 20), (10, 8, 20), 0),
    ("aniso_ragged_8byte_base", 1, 16, 4, (10, 9, 20), (10, 8, 20), 4),
]


def _tz_operands(B, C, G, sp, seed):
    Cg = C // G
    g = _gen(seed)
    x = torch.randn(B, C, *sp, generator=g).cuda()
    ws = [(torch.randn(C, Cg, k, k, k, generator=g) * (1.0 / (Cg * k ** 3) ** 0.5)).cuda() for k in (1, 3, 5)]
    bs = [(torch.randn(C, generator=g) * 0.1).cuda() for _ in range(3)]
    return x, ws, bs, g


@pytest.mark.parametrize("case", TZ_H_CASES, ids=[c[0] for c in TZ_H_CASES])
def test_jlc_toeplitz_convs_with_16bit_tensors_vs_fp64(case):
    """vx_jlc_tz_fwd_h / vx_jlc_tz_bwd_h (pieces = 1, h16 = 1): y_k (stored bf16) to the bf16 bound against the fp64 convolution of the host-rounded x and w; `part`
    folds to the statistics of the stored y_k; dx (fp32) to the pieces = 3 tolerance max(3 e_old, 2e-6) against the fp64 adjoint of the stored g_k, d_o and the
    rounded w3 / w5 (w1 and d_o enter dx in fp32, unrounded)"""
    H = _H()
    name, B, C, G, (D, Hh, W), _, shift = case
    H.call("vx_jlc_tz_set_min_voxels", 0)
    H.call("vx_jlc_tz_set_pieces", 1)
    try:
        assert H.query("vx_jlc_tz_ok", C, G, D, Hh, W) == 1
        x, ws, bs, g = _tz_operands(B, C, G, (D, Hh, W), 61)
        BC, V = B * C, D * Hh * W
        nt = H.query("vx_jlc_tz_ntiles", C, G, D, Hh, W)
        img = torch.empty(H.query("vx_jlc_tz_img_floats_ns", C, G, 1), device="cuda")
        H.call("vx_jlc_tz_prep_ns", H.P(ws[0]), H.P(ws[1]), H.P(ws[2]), H.P(img), C, G, 1, _st())
        res = {}
        for h16 in (1, 0):
            y = Guard((3, B, C, D, Hh, W), torch.bfloat16 if h16 else torch.float32, shift=shift if h16 else 0)
            part = Guard((3, BC, nt, 2), torch.float64)
            H.call("vx_jlc_tz_fwd_h", H.P(x), H.P(img), H.P(bs[0]), H.P(bs[1]), H.P(bs[2]), y.t[0].data_ptr(), y.t[1].data_ptr(), y.t[2].data_ptr(), part.ptr,
                   B, C, G, D, Hh, W, 1, h16, _st())
            res[h16] = (y, part)
        y_p, part_p = Guard((3, B, C, D, Hh, W)), Guard((3, BC, nt, 2), torch.float64)
        H.call("vx_jlc_tz_fwd_ns", H.P(x), H.P(img), H.P(bs[0]), H.P(bs[1]), H.P(bs[2]), y_p.t[0].data_ptr(), y_p.t[1].data_ptr(), y_p.t[2].data_ptr(), part_p.ptr, B, C, G, D, Hh, W, 1, _st())
        torch.cuda.synchronize()
        for h16 in (1, 0):
            for g_ in res[h16]:
                g_.check(f"tz_fwd {name} h16={h16}")
        assert torch.equal(_bits(res[0][0].t), _bits(y_p.t)) and torch.equal(res[0][1].t, part_p.t), "vx_jlc_tz_fwd_h(h16 = 0) differs from vx_jlc_tz_fwd_ns"
        xr = R.rounded(x).double()
        for i, k in enumerate((1, 3, 5)):
            ref = TF.conv3d(xr, R.rounded(ws[i]).double(), bs[i].double(), padding=k // 2, groups=G)
            _held_bf16(res[1][0].t[i], ref, res[0][0].t[i], "vx_jlc_tz_fwd_h", name, f"y{k}")
            sc = float(ref.abs().max())
            yk = R.widen(res[1][0].t[i])
            s_new = res[1][1].t[i].sum(1).view(B, C, 2)
            R.held(s_new[..., 0], yk.sum((2, 3, 4)), 1e-3 * sc + 1e-5 * yk.sum((2, 3, 4)).abs(), f"tz_fwd {name} part (sum) of y{k} vs the STORED y")
            R.held(s_new[..., 1], (yk * yk).sum((2, 3, 4)), 1e-3 * sc * sc + 1e-5 * (yk * yk).sum((2, 3, 4)), f"tz_fwd {name} part (sum of squares) of y{k} vs the STORED y")
        # ---- input gradient
        gh, g64 = _h16_in(torch.randn(3, B, C, D, Hh, W, generator=g), shift)
        dh, d64 = _h16_in(torch.randn(B, C, D, Hh, W, generator=g), shift)
        g32, d32 = gh.float(), dh.float()
        dx_h, dx_0, dx_p, dx_old = Guard(x.shape), Guard(x.shape), Guard(x.shape), Guard(x.shape)
        H.call("vx_jlc_tz_bwd_h", gh[0].data_ptr(), gh[1].data_ptr(), gh[2].data_ptr(), H.P(img), H.P(ws[0]), dh.data_ptr(), dx_h.ptr, B, C, G, D, Hh, W, 1, 1, _st())
        H.call("vx_jlc_tz_bwd_h", g32[0].data_ptr(), g32[1].data_ptr(), g32[2].data_ptr(), H.P(img), H.P(ws[0]), H.P(d32), dx_0.ptr, B, C, G, D, Hh, W, 1, 0, _st())
        H.call("vx_jlc_tz_bwd_ns", g32[0].data_ptr(), g32[1].data_ptr(), g32[2].data_ptr(), H.P(img), H.P(ws[0]), H.P(d32), dx_p.ptr, B, C, G, D, Hh, W, 1, _st())
        H.call("vx_jlc_conv_bwd", g32[0].data_ptr(), g32[1].data_ptr(), g32[2].data_ptr(), H.P(ws[0]), H.P(ws[1]), H.P(ws[2]), H.P(d32), dx_old.ptr, B, C, G, D, Hh, W, _st())
        torch.cuda.synchronize()
        for g_ in (dx_h, dx_0, dx_p, dx_old):
            g_.check(f"tz_bwd {name}")
        assert torch.equal(_bits(dx_0.t), _bits(dx_p.t)), "vx_jlc_tz_bwd_h(h16 = 0) differs from vx_jlc_tz_bwd_ns"
        ref, ref_old = d64.clone(), d64.clone()
        for i, k in enumerate((1, 3, 5)):
            ref = ref + TF.conv_transpose3d(g64[i], (ws[i] if k == 1 else R.rounded(ws[i])).double(), None, padding=k // 2, groups=G)
            ref_old = ref_old + TF.conv_transpose3d(g64[i], ws[i].double(), None, padding=k // 2, groups=G)
        sc = float(ref.abs().max())
        e_old = float((R.widen(dx_old.t) - ref_old).abs().max()) / sc
        tol = max(3.0 * e_old, 2e-6)
        mult = R.held(dx_h.t, ref, tol * sc, f"tz_bwd {name} dx (16-bit g_k, d_o)")
        R.held(dx_0.t, ref, tol * sc, f"tz_bwd {name} dx (fp32 arrays holding the same values)")
        print(f"[bf16-ops] vx_jlc_tz_bwd_h {name} dx: e_old = {e_old:.3e}, bound {tol:.3e} of the maximum, worst multiple of it = {mult:.3f}")
    finally:
        H.call("vx_jlc_tz_set_pieces", 22)          # (the library defaults)
        H.call("vx_jlc_tz_set_min_voxels", 1024)


@pytest.mark.parametrize("case", TZ_H_CASES[:5], ids=[c[0] for c in TZ_H_CASES[:5]])
def test_jlc_toeplitz_weight_gradients_with_16bit_gradients_vs_fp64(case):
    """vx_jlc_wgrad_tz_h (pieces = 1, h16 = 1): dw_k += x (*) g_k with g_k bf16 arrays and x rounded on its way into the matrix pipe, accumulated into non-zero
    buffers, to the pieces = 3 tolerance max(3 e_old, 3e-6) of the sibling test against torch's fp64 weight gradient of the host-rounded x and the stored g_k"""
    H = _H()
    name, B, C, G, _, (D, Hh, W), _ = case
    H.call("vx_jlc_wgrad_tz_set_min_voxels", 0)
    H.call("vx_jlc_tz_set_pieces", 1)              # (vx_jlc_wgrad_tz_ok answers for the process-wide mode)
    try:
        assert H.query("vx_jlc_wgrad_tz_ok", C, G, D, Hh, W) == 1
        x, ws, _, g = _tz_operands(B, C, G, (D, Hh, W), 71)
        gh, g64 = _h16_in(torch.randn(3, B, C, D, Hh, W, generator=g))
        g32 = gh.float()
        shapes = [tuple(w_.shape) for w_ in ws]
        inits = [torch.randn(s_, generator=g).cuda() for s_ in shapes]
        d_h, d_0, d_p = ([Guard(s_, fill=t) for s_, t in zip(shapes, inits)] for _ in range(3))
        d_old = [torch.zeros(s_, device="cuda") for s_ in shapes]
        H.call("vx_jlc_wgrad_tz_h", H.P(x), gh[0].data_ptr(), gh[1].data_ptr(), gh[2].data_ptr(), d_h[0].ptr, d_h[1].ptr, d_h[2].ptr, B, C, G, D, Hh, W, 1, 1, _st())
        H.call("vx_jlc_wgrad_tz_h", H.P(x), g32[0].data_ptr(), g32[1].data_ptr(), g32[2].data_ptr(), d_0[0].ptr, d_0[1].ptr, d_0[2].ptr, B, C, G, D, Hh, W, 1, 0, _st())
        H.call("vx_jlc_wgrad_tz_ns", H.P(x), g32[0].data_ptr(), g32[1].data_ptr(), g32[2].data_ptr(), d_p[0].ptr, d_p[1].ptr, d_p[2].ptr, B, C, G, D, Hh, W, 1, _st())
        H.call("vx_conv3d_bwd_weight_tiled", H.P(x), None, 0, g32[1].data_ptr(), H.P(d_old[1]), None, B, C, D, Hh, W, C, 3, 1, 1, G, 1, _st())
        H.call("vx_conv3d_bwd_weight_tiled", H.P(x), None, 0, g32[2].data_ptr(), H.P(d_old[2]), None, B, C, D, Hh, W, C, 5, 1, 2, G, 1, _st())
        torch.cuda.synchronize()
        xr = R.rounded(x).double()
        for i, k in enumerate((1, 3, 5)):
            for g_ in (d_h[i], d_0[i], d_p[i]):
                g_.check(f"wgrad_tz {name} dw{k}")
            ref = torch.nn.grad.conv3d_weight(xr, shapes[i], g64[i], padding=k // 2, groups=G)
            ref_old = torch.nn.grad.conv3d_weight(x.double(), shapes[i], g64[i], padding=k // 2, groups=G)
            sc = float(ref.abs().max())
            e_old = float((d_old[i].double() - ref_old).abs().max()) / sc if i else 0.0
            tol = max(3.0 * e_old, 3e-6)
            # (the start value is part of the fp32 sum: its rounding, 2^-24 of |init + dw|, is inside the 3e-6 floor)
            mult = R.held(d_h[i].t, inits[i].double() + ref, tol * sc, f"wgrad_tz {name} dw{k} (16-bit g_k)")
            R.held(d_0[i].t, inits[i].double() + ref, tol * sc, f"wgrad_tz {name} dw{k} (fp32 arrays holding the same values)")
            R.held(d_0[i].t, R.widen(d_p[i].t), 2e-6 * sc, f"wgrad_tz {name} dw{k}: _h(h16 = 0) vs vx_jlc_wgrad_tz_ns (float atomics: summation order)")
            print(f"[bf16-ops] vx_jlc_wgrad_tz_h {name} dw{k}: e_old = {e_old:.3e}, bound {tol:.3e} of the maximum, worst multiple of it = {mult:.3f}")
    finally:
        H.call("vx_jlc_tz_set_pieces", 22)
        H.call("vx_jlc_wgrad_tz_set_min_voxels", 0)


# ---------------------------------------------------------------------------------------------------------------------- 8. the patch-expand entries
def _coarse(dy, B, Cc, D, Hh, W):
    """fine (B, Cc, 4D, 4H, 4W) -> the conv's (B, 64 Cc, D, H, W) layout (the inverse of PixelShuffle(4), superpixel.py:16)"""
    return dy.view(B, Cc, D, 4, Hh, 4, W, 4).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(B, 64 * Cc, D, Hh, W)


@pytest.mark.parametrize("B,Cc,sp", [(1, 1, (4, 4, 24)), (2, 2, (4, 8, 32)), (2, 1, (4, 4, 40)), (1, 3, (4, 4, 4))], ids=["w24", "w32", "w40", "w4"])
def test_patch_expand_with_16bit_fine_tensors_vs_fp64(B, Cc, sp):
    """vx_expand_fwd_mfma_bf16_h / vx_expand_bwd_data_mfma_bf16_h / vx_expand_wgrad_mfma_split_h (ns = 1) with the fine tensors (y, dy) as bf16 arrays: y to the
    bf16 bound against the fp64 convolution of the host-rounded x and w; dx, dw, db (fp32) to the ns = 3 tolerances of the split tests (4e-6 of the maximum;
    3e-6; 3e-6 + 1e-5) against fp64 on the stored dy and the rounded x / w; accumulate = 1 doubles dx"""
    from oracle import veloxseg_oracle as O
    H = _H()
    D, Hh, W = sp
    name = f"b{B}_cc{Cc}_{D}x{Hh}x{W}"
    g = _gen(81)
    x = torch.randn(B, 16, D, Hh, W, generator=g).cuda()
    w = (torch.randn(64 * Cc, 16, 3, 3, 3, generator=g) * (16 * 27) ** -0.5).cuda()
    b = (torch.randn(64 * Cc, generator=g) * 0.1).cuda()
    fine = (B, Cc, 4 * D, 4 * Hh, 4 * W)
    ws = torch.empty(64 * Cc * 16 * 27, device="cuda")
    y_h, y_0, y_p = Guard(fine, torch.bfloat16), Guard(fine), Guard(fine)
    assert H.query("vx_expand_fwd_mfma_bf16_h", H.P(x), H.P(w), H.P(b), H.P(ws), y_h.ptr, B, Cc, D, Hh, W, 1, _st()) == 0
    assert H.query("vx_expand_fwd_mfma_bf16_h", H.P(x), H.P(w), H.P(b), H.P(ws), y_0.ptr, B, Cc, D, Hh, W, 0, _st()) == 0
    assert H.query("vx_expand_fwd_mfma_bf16", H.P(x), H.P(w), H.P(b), H.P(ws), y_p.ptr, B, Cc, D, Hh, W, _st()) == 0
    torch.cuda.synchronize()
    for g_ in (y_h, y_0, y_p):
        g_.check(f"expand fwd {name}")
    assert torch.equal(_bits(y_0.t), _bits(y_p.t)), "vx_expand_fwd_mfma_bf16_h(y_h16 = 0) differs from vx_expand_fwd_mfma_bf16"
    xr, wr = R.rounded(x).double(), R.rounded(w).double()
    yref = O.pixel_shuffle3d(TF.conv3d(xr, wr, b.double(), padding=1), 4)
    _held_bf16(y_h.t, yref, y_0.t, "vx_expand_fwd_mfma_bf16_h", name, "y")
    # ---- input gradient
    dyh, dy64 = _h16_in(torch.randn(*fine, generator=g))
    dy32 = dyh.float()
    dyc = _coarse(dy64, B, Cc, D, Hh, W)
    dx_h, dx_0, dx_p = Guard(x.shape), Guard(x.shape), Guard(x.shape)
    assert H.query("vx_expand_bwd_data_mfma_bf16_h", H.P(dyh, None), H.P(w), H.P(ws), dx_h.ptr, B, Cc, D, Hh, W, 0, 1, _st()) == 0
    assert H.query("vx_expand_bwd_data_mfma_bf16_h", H.P(dy32), H.P(w), H.P(ws), dx_0.ptr, B, Cc, D, Hh, W, 0, 0, _st()) == 0
    assert H.query("vx_expand_bwd_data_mfma_bf16", H.P(dy32), H.P(w), H.P(ws), dx_p.ptr, B, Cc, D, Hh, W, 0, _st()) == 0
    torch.cuda.synchronize()
    for g_ in (dx_h, dx_0, dx_p):
        g_.check(f"expand bwd_data {name}")
    assert torch.equal(_bits(dx_0.t), _bits(dx_p.t)), "vx_expand_bwd_data_mfma_bf16_h(dy_h16 = 0) differs from vx_expand_bwd_data_mfma_bf16"
    dxref = TF.conv_transpose3d(dyc, wr, None, padding=1)
    sc = float(dxref.abs().max())
    mult = R.held(dx_h.t, dxref, 4e-6 * sc, f"expand bwd_data {name} dx (16-bit dy)")
    R.held(dx_0.t, dxref, 4e-6 * sc, f"expand bwd_data {name} dx (fp32 array holding the same values)")
    print(f"[bf16-ops] vx_expand_bwd_data_mfma_bf16_h {name} dx: worst multiple of 4e-6 max = {mult:.3f}")
    keep = dx_h.t.clone()
    assert H.query("vx_expand_bwd_data_mfma_bf16_h", H.P(dyh, None), H.P(w), H.P(ws), dx_h.ptr, B, Cc, D, Hh, W, 1, 1, _st()) == 0
    torch.cuda.synchronize()
    dx_h.check(f"expand bwd_data {name} accumulate")
    R.held(dx_h.t, 2.0 * keep.double(), 1e-6 * sc, f"expand bwd_data {name}: accumulate = 1 doubles dx")
    # ---- weight + bias gradient
    nws = H.query("vx_expand_wgrad_split_ws_floats", B, Cc, D, Hh, W)
    wref = torch.nn.grad.conv3d_weight(xr, tuple(w.shape), dyc, padding=1)
    bref = dyc.sum((0, 2, 3, 4))
    outs = {}
    for h16 in (1, 0, -1):
        pws = torch.full((nws,), NAN, device="cuda")                  # (every row that is folded must have been written)
        dw, db = Guard(w.shape, fill=1.0), Guard(b.shape, fill=2.0)
        if h16 >= 0:
            rc = H.query("vx_expand_wgrad_mfma_split_h", H.P(x), (dyh if h16 else dy32).data_ptr(), dw.ptr, db.ptr, H.P(pws), nws, B, Cc, D, Hh, W, 1, h16, _st())
        else:
            rc = H.query("vx_expand_wgrad_mfma_split", H.P(x), H.P(dy32), dw.ptr, db.ptr, H.P(pws), nws, B, Cc, D, Hh, W, 1, _st())
        assert rc == 0
        torch.cuda.synchronize()
        dw.check(f"expand wgrad {name} dw")
        db.check(f"expand wgrad {name} db")
        outs[h16] = (dw.t, db.t)
    assert torch.equal(_bits(outs[0][0]), _bits(outs[-1][0])), "vx_expand_wgrad_mfma_split_h(dy_h16 = 0) differs from vx_expand_wgrad_mfma_split"
    wsc, bsc = float(wref.abs().max()), float(bref.abs().max())
    for h16 in (1, 0):
        mult = R.held(outs[h16][0] - 1.0, wref, 3e-6 * wsc + 3e-6 * wref.abs(), f"expand wgrad {name} dw (dy_h16 = {h16})")
        R.held(outs[h16][1] - 2.0, bref, 3e-6 * bsc + 1e-5 + 1e-5 * bref.abs(), f"expand wgrad {name} db (dy_h16 = {h16})")
    print(f"[bf16-ops] vx_expand_wgrad_mfma_split_h {name} dw: worst multiple of the 3e-6 bound (fp32 run) = {mult:.3f}")


def test_patch_expand_16bit_entries_decline_shapes_they_do_not_cover():
    """D % 4, H % 4 or W % 4 != 0: the forward and input-gradient entries return 1 and launch nothing (the dispatcher then takes vx_conv_s1); the output stays as it was"""
    H = _H()
    B, Cc, D, Hh, W = 2, 1, 3, 5, 40
    x = torch.randn(B, 16, D, Hh, W, generator=_gen(82)).cuda()
    w = torch.randn(64 * Cc, 16, 3, 3, 3, generator=_gen(83)).cuda()
    ws = torch.empty(64 * Cc * 16 * 27, device="cuda")
    fine = (B, Cc, 4 * D, 4 * Hh, 4 * W)
    y, dx = Guard(fine, torch.bfloat16), Guard(x.shape)
    dy = torch.randn(*fine, generator=_gen(84)).bfloat16().cuda()
    assert H.query("vx_expand_fwd_mfma_bf16_h", H.P(x), H.P(w), None, H.P(ws), y.ptr, B, Cc, D, Hh, W, 1, _st()) == 1
    assert H.query("vx_expand_bwd_data_mfma_bf16_h", H.P(dy, None), H.P(w), H.P(ws), dx.ptr, B, Cc, D, Hh, W, 0, 1, _st()) == 1
    torch.cuda.synchronize()
    y.check("declined forward")
    dx.check("declined input gradient")
    assert bool(torch.isnan(y.t).all()) and bool(torch.isnan(dx.t).all()), "a declined call wrote to its output"


# ---------------------------------------------------------------------------------------------------------------------- 9. vx_seg_loss_ds_fwd_h / _bwd_h
DS_CASES = [
    # name, classes, B, full-resolution grid, label dtype, factors: the geometries of test_loss_with_fused_deep_supervision_upsampling
    ("c2", 2, 2, (32, 32, 32), torch.int64, (2, 4, 8)),
    ("c4_w48", 4, 1, (16, 24, 48), torch.uint8, (2, 4, 8)),
    ("c3_ragged_rows", 3, 1, (16, 40, 64), torch.int64, (4, 8, 16)),
    ("c2_model_ratios", 2, 2, (32, 64, 128), torch.uint8, (8, 16, 32)),
]
_LAB_KIND = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}


def _ds_run(H, l0, lows, lab, B, C, S, h16):
    """forward (accumulators) -> vx_loss_finalize (loss, Dice coefficients) -> backward through the C ABI, as functional.StagedLoss does.  -> loss, [dl0 .. dl3] guards"""
    nh = 1 + len(lows)
    D_, H_, W_ = S
    V = D_ * H_ * W_
    dims = (ctypes.c_int * (3 * (nh - 1)))(*[int(v) for t in lows for v in t.shape[2:]])
    acc = torch.empty(nh * (1 + B * C * 3), device="cuda", dtype=torch.float64)
    lp = [l0.data_ptr()] + [H.P(t) for t in lows] + [None] * (4 - nh)
    kind = _LAB_KIND[lab.dtype]
    H.call("vx_seg_loss_ds_fwd_h", *lp, ctypes.addressof(dims), nh, H.P(lab, None), kind, H.P(acc, torch.float64), B, C, D_, H_, W_, h16, _st())
    hw = torch.full((nh,), 0.25, device="cuda")
    coef = torch.empty(nh * (1 + B * C * 2) + 2, device="cuda")
    loss = torch.empty(1, device="cuda")
    H.call("vx_loss_finalize", H.P(acc, torch.float64), nh, B, C, V, H.P(hw), None, 1, 0.0, None, None, None, None, None, 0, 0, 0.0, H.P(loss), H.P(coef), _st())
    gr = [Guard(l0.shape, torch.bfloat16 if h16 else torch.float32)] + [Guard(t.shape) for t in lows]
    nws = H.query("vx_seg_loss_ds_ws_floats", ctypes.addressof(dims), nh, B, C, D_)
    ws = torch.empty(max(nws, 1), device="cuda")
    H.call("vx_seg_loss_ds_bwd_h", *lp, ctypes.addressof(dims), nh, H.P(lab, None), kind, H.P(coef), 1 + B * C * 2, None, *([g_.ptr for g_ in gr] + [None] * (4 - nh)), H.P(ws),
           B, C, D_, H_, W_, h16, _st())
    torch.cuda.synchronize()
    for i, g_ in enumerate(gr):
        g_.check(f"seg_loss_ds dl{i} (h16 = {h16})")
    return float(loss), gr


def test_deep_supervision_loss_with_16bit_head0_vs_oracle():
    """vx_seg_loss_ds_fwd_h / _bwd_h (l0_h16 = 1, column-owner kernels) at every geometry vx_seg_loss_ds_h16_ok covers (at least three of the four): loss 1e-5
    relative against O.seg_loss on the widened logits, dl1..dl3 (fp32) to 1e-4 of their maximum, dl0 (stored bf16) to the bf16 bound"""
    from oracle import veloxseg_oracle as O
    H = _H()
    ran = []
    for name, C, B, S, labdtype, factors in DS_CASES:
        g = _gen(91)
        lows_cpu = [torch.randn(B, C, *[max(s // f, 2) for s in S], generator=g) for f in factors]
        dims = (ctypes.c_int * 9)(*[int(v) for t in lows_cpu for v in t.shape[2:]])
        if H.query("vx_seg_loss_ds_h16_ok", ctypes.addressof(dims), 4, B, C, *S) != 1:
            continue
        ran.append(name)
        l0h, l064 = _h16_in(torch.randn(B, C, *S, generator=g))
        lab = torch.randint(0, C, (B, 1, *S), generator=g).to(labdtype)
        lows = [t.cuda() for t in lows_cpu]
        loss_h, gr_h = _ds_run(H, l0h, lows, lab.cuda(), B, C, S, 1)
        loss_0, gr_0 = _ds_run(H, l0h.float(), lows, lab.cuda(), B, C, S, 0)
        hc = [l064.cpu().requires_grad_(True)] + [t.double().requires_grad_(True) for t in lows_cpu]
        up = [hc[0]] + [TF.interpolate(h_, size=S, mode="trilinear", align_corners=True) for h_ in hc[1:]]
        ref = sum(0.25 * O.seg_loss(u, lab.long()) for u in up)
        ref.backward()
        assert abs(loss_h - float(ref)) <= 1e-5 * abs(float(ref)), (name, loss_h, float(ref))
        assert abs(loss_0 - float(ref)) <= 1e-5 * abs(float(ref)), (name, loss_0, float(ref))
        for k in range(1, 4):
            gk = hc[k].grad
            R.held(gr_h[k].t, gk, 1e-4 * float(gk.abs().max()) + 1e-4 * gk.abs(), f"seg_loss_ds {name} dl{k}")
        _held_bf16(gr_h[0].t, hc[0].grad.cuda(), gr_0[0].t, "vx_seg_loss_ds_bwd_h", name, "dl0")
        print(f"[bf16-ops] vx_seg_loss_ds_fwd_h {name}: loss {loss_h:.7f} (fp32 arrays: {loss_0:.7f}) vs oracle {float(ref):.7f}")
    assert len(ran) >= 3, f"vx_seg_loss_ds_h16_ok covers only {ran}"
