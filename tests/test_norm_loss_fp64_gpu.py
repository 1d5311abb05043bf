"""The non-linear reduction kernels against fp64 at their path and conditioning edges: InstanceNorm, channels-first LayerNorm, the loss
(plain and with fused deep supervision), the Gram matrix and trilinear up-sampling, each row of tests/stable_ref.py once through veloxseg_amd.functional, forward and
backward, every output and gradient held to

    max |got - ref64| <= 8 max |ref32 - ref64| + 16 * 2^-24 max |ref64|

with ref64 / ref32 the CPU oracle in double / single precision on the same input (tests/test_stable_ref_cpu.py proves the premise of every row without a GPU).
The pointer-alignment fallbacks of the InstanceNorm kernels and the vectorised loss / Gram backward kernels, which the public surface cannot reach with an unaligned
base, run through the C ABI into canary-fenced buffers."""
import pytest
import torch

import stable_ref as S
from exact_ref import Guard

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _vf():
    from veloxseg_amd import functional as VF
    return VF


def _run(fn_gpu, c):
    """the kernel once, forward and backward, on the row's inputs -> the tensors under the names of stable_ref.ref64"""
    d = dev()
    ts = [t.clone().to(d).requires_grad_(True) for t in c["tensors"]]
    ps = [p.clone().to(d).requires_grad_(True) for p in c["params"]]
    outs = fn_gpu(*ts, *ps)
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    torch.autograd.backward(outs, [g.to(d) for g in c["cots"]])
    torch.cuda.synchronize()
    got = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    got.update({f"d_in{i}": t.grad for i, t in enumerate(ts)})
    got.update({f"d_par{i}": p.grad for i, p in enumerate(ps)})
    return got


def _hold(op, row, got, c, tag=""):
    """every output and gradient of the row to the bound; the figures are printed (pytest -s) before anything is asserted"""
    assert set(got) == set(c["r64"]), (sorted(got), sorted(c["r64"]))
    bad = []
    for name in sorted(got):
        assert got[name] is not None, f"{op} {row['id']}{tag}: no gradient {name}"
        e, e32, M = S.figures(got[name], c["r64"][name], c["r32"][name])
        print(f"[fp64] {op} {row['id']}{tag} {name}: err {e:.3e} ref32 {e32:.3e} M {M:.3e} ratio {e / e32 if e32 > 0 else float('nan'):.2f} floor-units {e / (S.FLOOR * M) if M > 0 else float('nan'):.2f}")
        m = S.violation(got[name], c["r64"][name], c["r32"][name], f"{op} {row['id']}{tag} {name} [{row['branch']}]", op)
        if m:
            bad.append(m)
    assert not bad, "\n".join(bad)


# ---------------------------------------------------------------------------------------------------------------------- the tables through the public surface
@pytest.mark.parametrize("row", S.rows("instnorm"), ids=S.ids("instnorm"))
def test_instnorm_sum(row):
    VF = _vf()
    c = S.case("instnorm", row)
    n, act, res = row["n"], row["act"], row["res"]

    def g(*t):
        return VF.instnorm_sum(list(t[:n]), act=act, res=t[n] if res else None)

    _hold("instnorm", row, _run(g, c), c)
    sp = row["sp"]
    if sp[0] * sp[1] * sp[2] <= 4096:                   # short rows a second time on the split-statistics kernels
        try:
            VF.set_host_flags(USE_IN_ROW=False)
            got = _run(g, c)
        finally:
            VF.set_host_flags(USE_IN_ROW=True)
        _hold("instnorm", row, got, c, tag=" (USE_IN_ROW=False)")


@pytest.mark.parametrize("row", S.rows("layernorm"), ids=S.ids("layernorm"))
def test_layernorm_cf(row):
    VF = _vf()
    c = S.case("layernorm", row)
    _hold("layernorm", row, _run(lambda x, w, b: VF.layernorm_cf(x, w, b), c), c)


@pytest.mark.parametrize("row", S.rows("loss"), ids=S.ids("loss"))
def test_loss(row):
    VF = _vf()
    d = dev()
    c = S.case("loss", row)
    lab = c["labels"].to(d).to(S.LAB_DTYPES[row["lab"]])
    if row["M"] == 0:
        fn = lambda *t: VF.seg_only_loss(list(t), lab, c["weights"])
    else:
        sr = c["sr"].to(d)
        fn = lambda *t: VF.veloxseg_loss(list(t), lab, sr, c["weights"], S.W_RC, S.W_F, row["M"])
    _hold("loss", row, _run(fn, c), c)


@pytest.mark.parametrize("row", S.rows("loss_ds"), ids=S.ids("loss_ds"))
def test_loss_with_fused_deep_supervision(row):
    VF = _vf()
    from veloxseg_amd import _hip as H
    d = dev()
    c = S.case("loss_ds", row)
    lab = c["labels"].to(d).to(S.LAB_DTYPES[row["lab"]])
    H.call("vx_seg_loss_ds_set_columns", row["columns"])
    try:
        got = _run(lambda *t: VF.seg_only_loss(list(t), lab, c["weights"]), c)
    finally:
        H.call("vx_seg_loss_ds_set_columns", 1)
    _hold("loss_ds", row, got, c)


@pytest.mark.parametrize("row", S.rows("gram"), ids=S.ids("gram"))
def test_gram(row):
    VF = _vf()
    c = S.case("gram", row)
    _hold("gram", row, _run(lambda x: VF.gram(x), c), c)


@pytest.mark.parametrize("row", S.rows("upsample"), ids=S.ids("upsample"))
def test_upsample_trilinear(row):
    VF = _vf()
    c = S.case("upsample", row)
    _hold("upsample", row, _run(lambda x: VF.upsample_trilinear(x, row["hi"]), c), c)


# ---------------------------------------------------------------------------------------------------------------------- InstanceNorm: unaligned base pointers (C ABI)
def _in_abi(row, c, shift):
    """the row (two inputs + residual) through vx_in_row_fwd / _bwd (V <= vx_in_row_max) or vx_in_fwd_split / vx_in_bwd_split, every float tensor in a Guard
    whose base is `shift` floats past a 16-byte boundary -> (out, dy0, dy1), canaries checked"""
    from veloxseg_amd import _hip as H
    d = dev()
    BC = S.IN_B * S.IN_C
    V = row["sp"][0] * row["sp"][1] * row["sp"][2]
    n, act = row["n"], int(row["act"])
    assert n == 2 and row["res"]
    ys = [Guard((BC, V), fill=c["tensors"][k].reshape(BC, V), shift=shift) for k in range(n)]
    res = Guard((BC, V), fill=c["tensors"][n].reshape(BC, V), shift=shift)
    dout = Guard((BC, V), fill=c["cots"][0].reshape(BC, V), shift=shift)
    out = Guard((BC, V), shift=shift)
    dys = [Guard((BC, V), shift=shift) for _ in range(n)]
    for g in ys + [res, dout, out] + dys:
        assert g.ptr % 16 == 4 * shift
    stats = [torch.empty(BC * 2, device=d) for _ in range(n)]
    part = torch.empty(n * BC * 32, device=d, dtype=torch.float64)
    st = H.stream_ptr()
    yp, sp_, dp = [H.P(g.t) for g in ys] + [None], [H.P(s) for s in stats] + [None], [H.P(g.t) for g in dys] + [None]
    if V <= H.query("vx_in_row_max"):
        H.call("vx_in_row_fwd", *yp, *sp_, n, act, H.P(res.t), H.P(out.t), BC, V, S.IN_EPS, st)
        H.call("vx_in_row_bwd", H.P(dout.t), *yp, *sp_, n, act, *dp, BC, V, st)
    else:
        H.call("vx_in_fwd_split", *yp, *sp_, H.P(part, torch.float64), n, act, H.P(res.t), H.P(out.t), BC, V, S.IN_EPS, st)
        H.call("vx_in_bwd_split", H.P(dout.t), *yp, *sp_, H.P(part, torch.float64), n, act, *dp, None, BC, V, st)
    torch.cuda.synchronize()
    for i, g in enumerate(ys + [res, dout, out] + dys):
        g.check(f"instnorm {row['id']} shift {shift} (buffer {i})")
    return [out.t.clone()] + [g.t.clone() for g in dys]


@pytest.mark.parametrize("V", [257, 4097, 8381])
def test_instnorm_unaligned_base_pointers_take_the_scalar_path(V):
    """a base pointer 4 bytes past a 16-byte boundary: the long-row kernels must fall back to their scalar loops (every block), the row kernels have no 16-byte
    access to begin with; same bound, canaries intact, and bit for bit the results of the aligned call"""
    row = next(r for r in S.rows("instnorm") if r["id"] == f"v{V}-n2r-offset")
    c = S.case("instnorm", row)
    shp = c["tensors"][0].shape
    res = {}
    for shift in (0, 1):
        o = _in_abi(row, c, shift)
        res[shift] = o
        got = {"out0": o[0].view(shp), "d_in0": o[1].view(shp), "d_in1": o[2].view(shp), "d_in2": c["cots"][0]}          # (the residual's gradient is the cotangent itself)
        _hold("instnorm", row, got, c, tag=f" (C ABI, shift {shift})")
    for a, b in zip(res[0], res[1]):
        assert torch.equal(a, b), f"instnorm {row['id']}: the unaligned call differs from the aligned one"


# ---------------------------------------------------------------------------------------------------------------------- vectorised backward kernels into fenced buffers
@pytest.mark.parametrize("rid", ["c2_h4_int64_8x8x8_common_offset_m0", "c4_h4_uint8_5x7x9_confident_wrong_m0"], ids=["v512_vectorised", "v315_ragged"])
def test_loss_backward_writes_only_its_gradients(rid):
    """vx_seg_loss_fwd -> vx_loss_finalize -> vx_seg_loss_bwd4 through the C ABI with every head's gradient between canaries: V % 4 == 0 runs the 16-byte kernel,
    the ragged volume must take the one-voxel kernel; same bound as the public surface"""
    from veloxseg_amd import _hip as H
    d = dev()
    row = next(r for r in S.rows("loss") if r["id"] == rid)
    assert row["M"] == 0 and row["nh"] == 4
    c = S.case("loss", row)
    B, C, nh = S.LOSS_B, row["C"], row["nh"]
    V = row["vol"][0] * row["vol"][1] * row["vol"][2]
    logits = [t.to(d) for t in c["tensors"]]
    lab = c["labels"].to(d).to(S.LAB_DTYPES[row["lab"]])
    kind = {"int64": 0, "int32": 1, "uint8": 2}[row["lab"]]
    st = H.stream_ptr()
    lp = [H.P(t) for t in logits]
    acc = torch.empty(nh * (1 + B * C * 3), device=d, dtype=torch.float64)
    H.call("vx_seg_loss_fwd", *lp, nh, H.P(lab, None), kind, H.P(acc, torch.float64), B, C, V, st)
    hw = torch.tensor(c["weights"], device=d)
    stride = 1 + B * C * 2
    coef = torch.empty(nh * stride + 2, device=d)
    loss = torch.empty(1, device=d)
    H.call("vx_loss_finalize", H.P(acc, torch.float64), nh, B, C, V, H.P(hw), None, 1, 0.0, None, None, None, None, None, 0, 0, 0.0, H.P(loss), H.P(coef), st)
    grads = [Guard((B, C) + row["vol"]) for _ in range(nh)]
    H.call("vx_seg_loss_bwd4", *lp, nh, H.P(lab, None), kind, H.P(coef), stride, None, *[H.P(g.t) for g in grads], B, C, V, st)
    torch.cuda.synchronize()
    for h, g in enumerate(grads):
        g.check(f"loss {rid} head {h}")
    got = {"out0": loss.view(())}
    got.update({f"d_in{h}": g.t for h, g in enumerate(grads)})
    _hold("loss", row, got, c, tag=" (C ABI)")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("rid", ["c16_v1024_x1", "c17_v1029_x1"], ids=["v1024_vectorised", "v1029_ragged"])
def test_gram_backward_writes_only_its_gradient(rid, shift):
    """vx_gram_bwd through the C ABI, x and dx between canaries: V % 4 == 0 on an aligned base runs the 16-byte kernel; a ragged V, or a base 4 bytes past a 16-byte
    boundary, must take the one-voxel kernel"""
    from veloxseg_amd import _hip as H
    d = dev()
    row = next(r for r in S.rows("gram") if r["id"] == rid)
    c = S.case("gram", row)
    B, C = S.GRAM_B, row["C"]
    V = row["sp"][0] * row["sp"][1] * row["sp"][2]
    x = Guard((B, C, V), fill=c["tensors"][0].reshape(B, C, V), shift=shift)
    dG = c["cots"][0].to(d).contiguous()
    G = torch.empty(B, C, C, device=d)
    dx = Guard((B, C, V), shift=shift)
    st = H.stream_ptr()
    H.call("vx_gram_fwd", H.P(x.t), H.P(G), B, C, V, st)
    H.call("vx_gram_bwd", H.P(x.t), H.P(dG), H.P(dx.t), B, C, V, st)
    torch.cuda.synchronize()
    x.check(f"gram {rid} x")
    dx.check(f"gram {rid} dx")
    _hold("gram", row, {"out0": G, "d_in0": dx.t.view(c["tensors"][0].shape)}, c, tag=f" (C ABI, shift {shift})")
