"""torch.ops.veloxseg.* (veloxseg_amd/ops.py): the operators are registered dispatcher ops; on CPU they fail loudly (no fallback); on the GPU they
are the operators of veloxseg_amd.functional (same values, same gradients)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))


def test_ops_are_registered_and_have_no_cpu_kernel():
    from veloxseg_amd import functional as VF
    assert VF.cpp_module() is not None
    import veloxseg_amd.ops as O
    for name in O.OPS:
        op = getattr(torch.ops.veloxseg, name)
        assert op.default._schema.name == f"veloxseg::{name}"
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.veloxseg.gram(torch.randn(1, 4, 4, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.veloxseg.conv3d(torch.randn(1, 4, 4, 4, 4), torch.randn(4, 4, 1, 1, 1), None, 1, 0, 1, 1)


@pytest.mark.gpu
def test_ops_equal_the_functional_operators():
    import veloxseg_amd.ops  # noqa: F401
    from veloxseg_amd import functional as VF
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from oracle import veloxseg_oracle as Or
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(0)
    x = torch.randn(2, 16, 8, 8, 8, device=d, generator=g)
    w = torch.randn(16, 4, 3, 3, 3, device=d, generator=g) * 0.1
    b = torch.randn(16, device=d, generator=g) * 0.1

    def both(f_op, f_vf, tensors):
        outs = []
        for f in (f_op, f_vf):
            ts = [t.clone().requires_grad_(True) for t in tensors]
            y = f(*ts)
            ys = list(y) if isinstance(y, (list, tuple)) else [y]
            sum((o * o).sum() for o in ys).backward()
            outs.append(([o.detach() for o in ys], [t.grad for t in ts]))
        for a, r in zip(outs[0][0] + outs[0][1], outs[1][0] + outs[1][1]):
            assert torch.allclose(a, r, rtol=1e-5, atol=1e-5 * float(r.abs().max()))

    both(lambda x, w, b: torch.ops.veloxseg.conv3d(x, w, b, 1, 1, 4, 1), lambda x, w, b: VF.conv3d(x, w, b, stride=1, padding=1, groups=4), [x, w, b])
    both(lambda a, c: torch.ops.veloxseg.instance_norm_sum([a, c], True, None), lambda a, c: VF.instnorm_sum([a, c], act=True), [x, x * 0.5 + 1.0])
    gam, bet = torch.randn(16, device=d, generator=g), torch.randn(16, device=d, generator=g)
    both(lambda x, ga, be: torch.ops.veloxseg.layer_norm_cf(x, ga, be), lambda x, ga, be: VF.layernorm_cf(x, ga, be), [x, gam, bet])
    both(lambda x: torch.ops.veloxseg.gram(x), lambda x: VF.gram(x), [x])
    both(lambda x: torch.ops.veloxseg.upsample_trilinear(x, [16, 16, 16]), lambda x: VF.upsample_trilinear(x, (16, 16, 16)), [x])
    both(lambda x: torch.ops.veloxseg.space_to_depth2(x), lambda x: VF.space_to_depth2(x), [x])
    # paired-window attention through the op (plan built from the integer lists) against the functional core
    from veloxseg_amd import _hip as H
    grid, heads = [8, 8, 8], 2
    pl = Or.plan_pwa(grid, [4, 4, 4], [1, 1, 1], 2, heads, 8, 32)
    plan = H.make_plan(grid, pl["n"], heads, pl["small"], pl["nwin"])
    n = pl["n"]
    table = torch.randn((2 * n[0] - 1) * (2 * n[1] - 1) * (2 * n[2] - 1), heads, device=d, generator=g) * 0.5
    qkv = [torch.randn(2, pl["ch_qk"] if k < 2 else pl["ch_v"], *grid, device=d, generator=g) for k in range(3)]
    flat = lambda ll: [int(v) for row in ll for v in row]
    both(lambda t, q, k, v: torch.ops.veloxseg.pwa_attention(t, [q, k, v], grid, list(n), heads, flat(pl["small"]), flat(pl["nwin"]), pl["c_qk"], pl["c_v"], 0.0, 3),
         lambda t, q, k, v: VF.pwa_core(t, plan, pl["c_qk"], pl["c_v"], [q, k, v], p_attn=0.0, site=3), [table] + qkv)
    # loss
    heads4 = [torch.randn(2, 2, 16, 16, 16, device=d, generator=g) for _ in range(2)]
    lab = (torch.rand(2, 1, 16, 16, 16, device=d, generator=g) > 0.8).long()
    both(lambda a, c: torch.ops.veloxseg.seg_loss([a, c], lab, None, [0.6, 0.4], 0.0, 0.0, 0), lambda a, c: VF.seg_only_loss([a, c], lab, [0.6, 0.4]), heads4)
    # the full loss (deep supervision + reconstruction MSE + Gram distillation): the op against its functional wrapper, which calls it (one host body, as for conv3d above;
    # the oracle holds this configuration in tests/test_hip_ops_gpu.py::test_loss)
    rcs, srl = torch.randn(2, 2, 16, 16, 16, device=d, generator=g), torch.randn(2, 2, 16, 16, 16, device=d, generator=g)
    grams = [torch.randn(2, 8, 8, device=d, generator=g) for _ in range(3)]
    both(lambda a, c, r, g0, g1, g2: torch.ops.veloxseg.seg_loss([a, c, r, g0, g1, g2], lab, srl, [0.6, 0.4], 0.7, 0.3, 2),
         lambda a, c, r, g0, g1, g2: VF.veloxseg_loss([a, c, r, g0, g1, g2], lab, srl, [0.6, 0.4], 0.7, 0.3, 2), heads4 + [rcs] + grams)
    # the JLC block and the FFN tail: dispatcher op (parameters, dropout site and the {seed, step} RNG-state tensor as arguments) against the module's composite node
    from veloxseg_amd.model.components.conv_blocks import JLC
    from veloxseg_amd.model.components.attention_utils import FFN, LayerNorm
    torch.manual_seed(4)
    blk = JLC(16, groups=4, dropout=0.1).to(d).train()
    rs = VF.rng_state(d)
    convs = [seq[0] for seq in blk.spatial_convs]
    l1, l2 = blk.channel_conv[1], blk.channel_conv[3]

    def grads_of(fn):
        for p_ in blk.parameters():
            p_.grad = None
        xx = x.clone().requires_grad_(True)
        y = fn(xx)
        (y * y).sum().backward()
        torch.cuda.synchronize()
        return [y.detach(), xx.grad] + [p_.grad.clone() for p_ in blk.parameters()]
    a = grads_of(lambda xx: torch.ops.veloxseg.jlc_block(xx, [c_.weight for c_ in convs], [c_.bias for c_ in convs], 4, l1.weight, l1.bias, l2.weight, l2.bias, 0.1, blk.site, rs))
    b_ = grads_of(lambda xx: blk(xx))
    for u, v in zip(a, b_):
        assert torch.allclose(u, v, rtol=1e-5, atol=1e-5 * float(v.abs().max())), float((u - v).abs().max())
    norm, ffn = LayerNorm(16).to(d), FFN(16, dropout_rate=0.1).to(d).train()
    prm = list(norm.parameters()) + list(ffn.parameters())

    def grads_ffn(fn):
        for p_ in prm:
            p_.grad = None
        yy = x.clone().requires_grad_(True)
        o = fn(yy)
        (o * o).sum().backward()
        torch.cuda.synchronize()
        return [o.detach(), yy.grad] + [p_.grad.clone() for p_ in prm]
    a = grads_ffn(lambda yy: torch.ops.veloxseg.ffn_tail(yy, norm.weight, norm.bias, ffn.linear1.weight, ffn.linear1.bias, ffn.linear2.weight, ffn.linear2.bias, 0.1, ffn.site1, ffn.site2, rs))
    b_ = grads_ffn(lambda yy: VF.ffn_tail(yy, norm, ffn, 0.1))
    for u, v in zip(a, b_):
        assert torch.allclose(u, v, rtol=1e-5, atol=1e-5 * float(v.abs().max())), float((u - v).abs().max())
    with pytest.raises(RuntimeError, match="rng_state"):
        torch.ops.veloxseg.ffn_tail(x, norm.weight, norm.bias, ffn.linear1.weight, ffn.linear1.bias, ffn.linear2.weight, ffn.linear2.bias, 0.1, ffn.site1, ffn.site2)


@pytest.mark.gpu
def test_cpp_registered_ops_pass_opcheck_and_have_meta_kernels():
    """The eleven C++-registered operators (csrc/_vxops.cpp: TORCH_LIBRARY(veloxseg), keys Autograd / CUDA / Meta / CPU-raises): torch.library.opcheck (schema,
    autograd registration, FakeTensor agreement with the real kernel), the Meta kernel's shape for every op, and the CUDA key reached directly in inference mode."""
    import veloxseg_amd.ops as O
    from torch.library import opcheck
    d = torch.device("cuda:0")
    g = torch.Generator(device=d).manual_seed(1)
    x = torch.randn(2, 16, 8, 8, 8, device=d, generator=g)
    cases = {
        "conv3d": (x, torch.randn(16, 4, 3, 3, 3, device=d, generator=g) * 0.1, torch.randn(16, device=d, generator=g) * 0.1, 1, 1, 4, 1),
        "conv_transpose_k2s2": (x, torch.randn(16, 8, 2, 2, 2, device=d, generator=g) * 0.1, torch.randn(8, device=d, generator=g) * 0.1),
        "instance_norm_sum": ([x, x * 0.5 + 1.0], True, None),
        "layer_norm_cf": (x, torch.randn(16, device=d, generator=g), torch.randn(16, device=d, generator=g)),
        "space_to_depth2": (x,),
        "upsample_trilinear": (x, [16, 16, 16]),
        "gram": (x,),
    }
    # (round 5) the four operators north_star names: window plan as integer lists, dropout off here (opcheck re-runs the op: masks would have to repeat)
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from oracle import veloxseg_oracle as Or
    grid, heads = [8, 8, 8], 2
    pl = Or.plan_pwa(grid, [4, 4, 4], [1, 1, 1], 2, heads, 8, 32)
    n = pl["n"]
    flat = lambda ll: [int(v) for row in ll for v in row]
    table = torch.randn((2 * n[0] - 1) * (2 * n[1] - 1) * (2 * n[2] - 1), heads, device=d, generator=g) * 0.5
    qkv = [torch.randn(2, pl["ch_qk"] if k < 2 else pl["ch_v"], *grid, device=d, generator=g) for k in range(3)]
    cases["pwa_attention"] = (table, qkv, grid, list(n), heads, flat(pl["small"]), flat(pl["nwin"]), pl["c_qk"], pl["c_v"], 0.0, 3, None)
    ws = [torch.randn(16, 4, k, k, k, device=d, generator=g) * 0.1 for k in (1, 3, 5)]
    bs = [torch.randn(16, device=d, generator=g) * 0.1 for _ in range(3)]
    cases["jlc_block"] = (x, ws, bs, 4, torch.randn(64, 16, 1, 1, 1, device=d, generator=g) * 0.1, torch.zeros(64, device=d), torch.randn(16, 64, 1, 1, 1, device=d, generator=g) * 0.1,
                          torch.zeros(16, device=d), 0.0, 5, None)
    cases["ffn_tail"] = (x, torch.ones(16, device=d), torch.zeros(16, device=d), torch.randn(64, 16, 1, 1, 1, device=d, generator=g) * 0.1, torch.zeros(64, device=d),
                         torch.randn(16, 64, 1, 1, 1, device=d, generator=g) * 0.1, torch.zeros(16, device=d), 0.0, 6, 7, None)
    lab = (torch.rand(2, 1, 16, 16, 16, device=d, generator=g) > 0.8).long()
    cases["seg_loss"] = ([torch.randn(2, 2, 16, 16, 16, device=d, generator=g) for _ in range(2)], lab, None, [0.6, 0.4], 0.0, 0.0, 0)
    assert set(cases) == set(O.CPP_OPS)
    for name, args in cases.items():
        op = getattr(torch.ops.veloxseg, name).default
        keys = torch._C._dispatch_dump(f"veloxseg::{name}")
        for k in ("CUDA", "Meta", "Autograd"):
            assert k in keys, (name, k, keys)
        assert "CompositeImplicitAutograd" not in keys, (name, keys)
        grad_args = tuple(a.clone().requires_grad_(True) if (isinstance(a, torch.Tensor) and a.is_floating_point()) else
                          ([t.clone().requires_grad_(True) for t in a] if (isinstance(a, list) and a and isinstance(a[0], torch.Tensor)) else a) for a in args)
        res = opcheck(op, grad_args, test_utils=("test_schema", "test_autograd_registration", "test_faketensor"), raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (name, res)
        with torch.inference_mode():
            y = op(*args)                                        # Autograd keys excluded: the CUDA key kernel
        meta_args = tuple(a.to("meta") if isinstance(a, torch.Tensor) else ([t.to("meta") for t in a] if (isinstance(a, list) and a and isinstance(a[0], torch.Tensor)) else a) for a in args)
        ym = op(*meta_args)
        if isinstance(y, (list, tuple)):
            assert len(ym) == len(y) and all(a.device.type == "meta" and tuple(a.shape) == tuple(b.shape) for a, b in zip(ym, y)), name
        else:
            assert ym.device.type == "meta" and tuple(ym.shape) == tuple(y.shape) and ym.dtype == y.dtype, (name, ym.shape, y.shape)
