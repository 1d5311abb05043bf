"""The host half of the oracle of tests/test_bf16_storage_ops_gpu.py (tests/bf16_ref.py): the rounding helper is round-to-nearest-even, 2^-8 |v| bounds one bf16
rounding, and the fp64 restatements of the JLC spatial / channel stages are oracle.veloxseg_oracle.jlc and its autograd."""
import struct

import torch
import torch.nn.functional as F

import bf16_ref as R
from oracle import veloxseg_oracle as O


def _f(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _bits16(v):
    return int(torch.tensor([v], dtype=torch.float32).bfloat16().view(torch.int16).item()) & 0xffff


def test_bfloat16_conversion_is_round_to_nearest_even():
    """hand-picked fp32 bit patterns -> the upper 16 bits the kernels' `(__bf16)x` stores (vx_pack_bf16x2 / tz_pack)"""
    cases = [
        (0x3F800000, 0x3F80),      # 1.0: exact
        (0x3F808000, 0x3F80),      # a tie between 0x3F80 (even) and 0x3F81: to even = down
        (0x3F818000, 0x3F82),      # a tie between 0x3F81 and 0x3F82 (even): to even = up
        (0x3F808001, 0x3F81),      # just above a tie: up
        (0x3F807FFF, 0x3F80),      # just below a tie: down
        (0x3FFFFFFF, 0x4000),      # one fp32 ulp below 2.0: rounds INTO the next binade (2.0)
        (0x3F7FFFFF, 0x3F80),      # one fp32 ulp below 1.0
        (0xBF808000, 0xBF80),      # the first tie, negative: sign-symmetric
        (0xC0490FDB, 0xC049),      # -pi
        (0x00000000, 0x0000),
        (0x80000000, 0x8000),      # -0.0 keeps its sign
    ]
    for b32, b16 in cases:
        assert _bits16(_f(b32)) == b16, (hex(b32), hex(_bits16(_f(b32))), hex(b16))
    # truncation (what a store that drops the low half would give) differs on four of them: the table can tell the two apart
    assert sum(1 for b32, b16 in cases if (b32 >> 16) != b16) >= 4
    t = torch.tensor([_f(c[0]) for c in cases])
    r = R.rounded(t)
    assert r.dtype == torch.float32 and torch.equal(r.view(torch.int32) & 0xffff, torch.zeros(len(cases), dtype=torch.int32))
    assert torch.equal(R.widen(t.bfloat16()), r.double()) and torch.equal(R.rounded(r), r)


def test_half_ulp_bound_of_one_bf16_rounding():
    g = torch.Generator().manual_seed(1)
    v = torch.cat([torch.randn(200000, generator=g), torch.randn(200000, generator=g) * 1e-3, torch.randn(200000, generator=g) * 3e4,
                   torch.tensor([_f(0x3FFFFFFF), _f(0x3F808000), _f(0x3F80FFFF), 1.0, -255.5])])
    err = (R.rounded(v).double() - v.double()).abs()
    bound = v.double().abs() * 2.0 ** -8
    assert bool((err <= bound).all())
    assert float((err / bound).max()) > 0.49          # ... and it is not slack by more than the factor 2 between 2^-8 |v| and half an ulp at the top of a binade
    assert R.held(R.rounded(v), v.double(), R.bf16_bound(v.double(), 0.0), "rounding") <= 1.0


def test_held_reports_unwritten_and_wrong_elements():
    ref = torch.arange(12, dtype=torch.float64).view(3, 4)
    assert R.held(ref.float(), ref, 1e-6, "same") == 0.0
    for bad in (float("nan"), 7.5):
        got = ref.float().clone()
        got[2, 1] = bad
        try:
            R.held(got, ref, 1e-6, "x")
        except AssertionError as e:
            assert "worst idx 9 = (2, 1)" in str(e) and "bad frac 8.333e-02" in str(e), str(e)
        else:
            raise AssertionError("a wrong element passed")


def _jlc_sd(C, G, r, seed):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i, k in enumerate((1, 3, 5)):
        sd[f"b.spatial_convs.{i}.0.weight"] = torch.randn(C, C // G, k, k, k, generator=g) * 0.3
        sd[f"b.spatial_convs.{i}.0.bias"] = torch.randn(C, generator=g) * 0.1
    sd["b.channel_conv.1.weight"] = torch.randn(r * C, C, 1, 1, 1, generator=g) * 0.3
    sd["b.channel_conv.1.bias"] = torch.randn(r * C, generator=g) * 0.1
    sd["b.channel_conv.3.weight"] = torch.randn(C, r * C, 1, 1, 1, generator=g) * 0.3
    sd["b.channel_conv.3.bias"] = torch.randn(C, generator=g) * 0.1
    return {k: v.double().requires_grad_(True) for k, v in sd.items()}


def test_fp64_restatements_equal_the_oracle_block_and_its_autograd():
    """bf16_ref.jlc_mid_fwd / jlc_mid_bwd / jlc_gk / mlp_fwd / mlp_bwd chained through the three grouped convolutions == O.jlc (conv_blocks.py:41-75) forward and
    autograd on fp32 inputs, in fp64, to 1e-6 of each tensor's scale"""
    B, C, G, r, sp = 2, 16, 4, 3, (4, 5, 6)
    V, BC = sp[0] * sp[1] * sp[2], B * C
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, *sp, generator=g).double().requires_grad_(True)
    dout = torch.randn(B, C, *sp, generator=g).double()
    sd = _jlc_sd(C, G, r, 4)
    ref = O.jlc(x, sd, "b.", G, 0.0, True)
    ref.backward(dout)

    def close(a, b, what):
        e = float((a - b.detach()).abs().max())
        assert e <= 1e-6 * float(b.detach().abs().max()), (what, e)

    with torch.no_grad():
        ws = [sd[f"b.spatial_convs.{i}.0.weight"] for i in range(3)]
        ys = torch.stack([F.conv3d(x, ws[i], sd[f"b.spatial_convs.{i}.0.bias"], padding=k // 2, groups=G).reshape(BC, V) for i, k in enumerate((1, 3, 5))])
        stats_y = torch.stack([R.row_stats(ys[k]) for k in range(3)])
        o = R.jlc_mid_fwd(x.reshape(BC, V), ys, stats_y)
        stats_o = R.row_stats(o)
        w1, b1 = sd["b.channel_conv.1.weight"].view(r * C, C), sd["b.channel_conv.1.bias"]
        w2, b2 = sd["b.channel_conv.3.weight"].view(C, r * C), sd["b.channel_conv.3.bias"]
        out, _, _ = R.mlp_fwd(o.view(B, C, V), stats_o, w1, b1, w2, b2)
        close(out.view_as(ref), ref, "out")
        # the partial sums a producer hands over fold to the row statistics
        p = R.partials(o, 3)
        close(torch.stack([p[:, :, 0].sum(1) / V, 1.0 / torch.sqrt(p[:, :, 1].sum(1) / V - (p[:, :, 0].sum(1) / V) ** 2 + R.EPS)], -1), stats_o, "folded partials")
        dn, dw1, db1, dw2, db2, n = R.mlp_bwd(o.view(B, C, V), stats_o, w1, b1, w2, dout.view(B, C, V))
        close(dw1, sd["b.channel_conv.1.weight"].grad.view(r * C, C), "dw1")
        close(db1, sd["b.channel_conv.1.bias"].grad, "db1")
        close(dw2, sd["b.channel_conv.3.weight"].grad.view(C, r * C), "dw2")
        close(db2, sd["b.channel_conv.3.bias"].grad, "db2")
        dn = dn.reshape(BC, V)
        nh = n.reshape(BC, V)
        d_o = R.jlc_mid_bwd(dout.view(BC, V), dn, dn.mean(-1), (dn * nh).mean(-1), o, stats_o)
        close(d_o, dout.view(BC, V) + R.in_backward(dn, nh, stats_o[:, 1:2]), "d_o, two spellings")
        t, yh = R.jlc_t(d_o, ys, stats_y)
        gk = R.jlc_gk(d_o, ys, stats_y, t.mean(-1), (t * yh).mean(-1))
        dx = d_o.view(B, C, *sp).clone()
        for i, k in enumerate((1, 3, 5)):
            gi = gk[i].view(B, C, *sp)
            dx += F.conv_transpose3d(gi, ws[i], None, padding=k // 2, groups=G)
            close(torch.nn.grad.conv3d_weight(x, ws[i].shape, gi, padding=k // 2, groups=G), ws[i].grad, f"dw of the k={k} conv (from g_k)")
        close(dx, x.grad, "dx")


def test_rounded_and_unrounded_statistics_differ_for_the_seed_of_the_gpu_test():
    """the GPU test asserts that part_o of vx_jlc_mid_fwd_h folds to the sums of the ROUNDED o and NOT to those of the unrounded one (rtol 1e-5) at (32, 1728): for
    its seed the two differ by more than 3e-5 relative in at least a quarter of the rows"""
    BC, V = 32, 1728
    x, y = R.mid_inputs(BC, V, 41)
    yd = R.widen(y)
    o = R.jlc_mid_fwd(x.double(), yd, torch.stack([R.row_stats(yd[k]) for k in range(3)])).float()
    a, b = R.rounded(o).double(), o.double()
    rel1 = ((a.sum(-1) - b.sum(-1)).abs() / b.sum(-1).abs())
    rel2 = (((a * a).sum(-1) - (b * b).sum(-1)).abs() / (b * b).sum(-1))
    assert int((rel1 > 3e-5).sum()) >= BC // 4 and int((rel2 > 3e-5).sum()) >= BC // 4, (rel1, rel2)
