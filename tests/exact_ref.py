"""Bit-exact oracles for the LINEAR kernels on integer-valued data.

Rounding and indexing are tested apart: x, w, dy and bias are drawn as integers in [-3, 3] (stored as fp32), `+=` destinations are prefilled with integers in
[-8, 8].  Every product and every partial sum is then an integer far below 2^24, so fp32 arithmetic is exact in ANY summation order (float atomics included), and
so is a product formed from 16-bit pieces whose scales are powers of two.  A kernel must therefore reproduce the fp64 oracle value for value; a dropped, doubled
or misplaced contribution cannot hide behind a tolerance.

This module is CPU-only at import: the integer generators, the fp64 oracles (torch's own double convolution + its autograd, and oracle/veloxseg_oracle.py for
pixel-shuffle, Gram, trilinear and space-to-depth), the case table CASES (plain data: tests/test_exact_ref_cpu.py proves the premise for every row,
tests/test_exact_linear_gpu.py runs the kernels on the same rows) and `Guard`, the canary-fenced device buffer the GPU tests write into."""
import functools

import torch
import torch.nn.functional as F

from oracle import veloxseg_oracle as O

NAN = float("nan")
CANARY = 1.5            # (exact in bf16, fp32 and fp64)
LIMIT = float(1 << 24)  # integers below 2^24 are exact in fp32


class Guard:
    """an output tensor between two 64-element canaries; `shift` elements of slack in front move its base pointer (shift = 4 bf16 elements: 8-byte aligned, not 16);
    `canary` for integer dtypes, which cannot hold 1.5"""

    def __init__(self, shape, dtype=torch.float32, fill=NAN, shift=0, canary=CANARY):
        n = 1
        for s in shape:
            n *= int(s)
        self.lo = 64 + shift
        self.canary = canary
        self.buf = torch.full((self.lo + n + 64,), canary, device="cuda", dtype=dtype)
        self.t = self.buf[self.lo:self.lo + n].view(*shape)
        if torch.is_tensor(fill):
            self.t.copy_(fill.to(device="cuda", dtype=dtype))
        else:
            self.t.fill_(fill)
        if dtype == torch.bfloat16 and shift == 4:
            assert self.t.data_ptr() % 16 == 8

    @property
    def ptr(self):
        return self.t.data_ptr()

    def check(self, what):
        n = self.t.numel()
        c = self.canary
        ok = bool((self.buf[:self.lo] == c).all()) and bool((self.buf[self.lo + n:] == c).all())
        assert ok, f"{what}: the kernel wrote outside its output ({int((self.buf[:self.lo] != c).sum())} elements before, {int((self.buf[self.lo + n:] != c).sum())} after)"


# ---------------------------------------------------------------------------------------------------------------------- integer generators
def ints(*shape, seed, lo=-3, hi=3):
    """seeded, uniform integers in [lo, hi] as fp32 (CPU)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, tuple(int(s) for s in shape), generator=g).float()


def prefill(*shape, seed):
    """what a `+=` destination holds before the call: integers in [-8, 8]"""
    return ints(*shape, seed=seed, lo=-8, hi=8)


def mismatch(got, ref, what):
    """by VALUE (-0.0 == 0.0; a NaN left in `got` differs from everything): None, or the report of the first mismatch"""
    g = got.detach().double().cpu().reshape(-1)
    r = ref.detach().double().cpu().reshape(-1)
    assert g.numel() == r.numel(), f"{what}: {g.numel()} elements against {r.numel()}"
    bad = ~(g == r)
    if not bool(bad.any()):
        return None
    i = int(bad.nonzero()[0])
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first flat index {i}: got {float(g[i])!r}, want {float(r[i])!r}"


def exact(got, ref, what):
    m = mismatch(got, ref, what)
    assert m is None, m


# ---------------------------------------------------------------------------------------------------------------------- the case table
def _conv(id, B, Cin, sp, Cout, K, S=1, P=0, G=1, ps=1, C1=0, **kw):
    return dict(id=id, kind="conv", B=B, Cin=Cin, sp=tuple(sp), Cout=Cout, K=K, S=S, P=P, G=G, ps=ps, C1=C1, **kw)


def _pw(id, B, Cin, Cout, V, C1=0, **kw):
    return _conv(id, B, Cin, (1, 1, V), Cout, 1, C1=C1, **kw)


def _expand(id, B, Cc, sp, **kw):
    return _conv(id, B, 16, sp, 64 * Cc, 3, P=1, ps=4, Cc=Cc, **kw)


CASES = {
    # A. the direct kernels (csrc/conv.hip) and the tiled weight gradients (csrc/conv_wgrad.hip)
    "direct": [
        _conv("g4_k3_16_5x6x7", 2, 16, (5, 6, 7), 16, 3, P=1, G=4),
        _conv("g8_k5_64_3x4x5", 2, 64, (3, 4, 5), 64, 5, P=2, G=8),                       # the kernel reaches past the volume on every side
        _conv("k3s2_12to20_7x5x9", 3, 12, (7, 5, 9), 20, 3, S=2, P=1),                    # odd extents (vx_conv_mfma_ok declines them); B = 3
        _conv("k7s4_3to16_9x10x13", 2, 3, (9, 10, 13), 16, 7, S=4, P=3),
        _conv("concat8of24_k1", 2, 24, (3, 4, 5), 16, 1, C1=8),
        _conv("concat8of24_k3", 2, 24, (3, 4, 5), 16, 3, P=1, C1=8),
        _conv("ps2_k3_16to64_3x5x6", 2, 16, (3, 5, 6), 64, 3, P=1, ps=2),
        _conv("ps4_k3_16to64_3x5x6", 2, 16, (3, 5, 6), 64, 3, P=1, ps=4),
        _conv("k2s2_4to16_3x4x5", 2, 4, (6, 8, 10), 16, 2, S=2),
        _conv("k4s4_2to16_2x3x2", 2, 2, (8, 12, 8), 16, 4, S=4),
        _conv("extents_of_one_1x1x4", 2, 8, (1, 1, 4), 8, 3, P=1),
        _conv("g4_k3_16_4x5x16_rows", 2, 16, (4, 5, 16), 16, 3, P=1, G=4),                # rows of 16: the row-sliding weight gradient (vx_wgrad_set_rows)
    ],
    # B. vx_conv_s1 (csrc/conv_s1.hip): forward (wmode 0, out_ps) and input gradient (wmode 1, in_ps)
    "s1": [
        _conv("g4_k3_16_4x5x6", 2, 16, (4, 5, 6), 16, 3, P=1, G=4),
        _conv("g4_k5_16_4x5x6", 2, 16, (4, 5, 6), 16, 5, P=2, G=4),
        _conv("g8_k5_64_3x3x3", 2, 64, (3, 3, 3), 64, 5, P=2, G=8),
        _conv("g8_k3_64_3x3x3", 3, 64, (3, 3, 3), 64, 3, P=1, G=8),                       # B = 3
        _conv("g1_k3_ps4_16to64_5x9x32", 2, 16, (5, 9, 32), 64, 3, P=1, ps=4),
        _conv("g1_k3_ps4_16to128_4x8x24", 2, 16, (4, 8, 24), 128, 3, P=1, ps=4),
        _conv("g1_k3_ps4_16to64_3x5x40", 2, 16, (3, 5, 40), 64, 3, P=1, ps=4),
        _conv("g1_k5_8to8_3x3x3", 2, 8, (3, 3, 3), 8, 5, P=2),
    ],
    # C. dense strided convolutions on MFMA (csrc/conv_mfma.hip): forward, forward with max |x|, input gradient
    "mfma": [
        _conv("k3s2_16to32_8x8x8", 3, 16, (8, 8, 8), 32, 3, S=2, P=1),                    # B = 3
        _conv("k3s2_12to20_6x4x10", 2, 12, (6, 4, 10), 20, 3, S=2, P=1),                  # 81 k-steps: the tail of the 8-way unrolled loop
        _conv("k3s2_64to128_4x4x4", 2, 64, (4, 4, 4), 128, 3, S=2, P=1),                  # the K-split block
        _conv("k3s2_16to32_2x2x2", 2, 16, (2, 2, 2), 32, 3, S=2, P=1),                    # one output voxel per axis
        _conv("k5s2_8to16_8x8x8", 2, 8, (8, 8, 8), 16, 5, S=2, P=2),
        _conv("k3s3_4to8_9x6x12", 2, 4, (9, 6, 12), 8, 3, S=3, P=1),
        _conv("k7s2_2to8_4x6x8", 2, 2, (4, 6, 8), 8, 7, S=2, P=3),
        _conv("k7s4_3to16_8x12x16", 2, 3, (8, 12, 16), 16, 7, S=4, P=3),                  # the fp32 stem path (3 input channels)
    ],
    # ... the stem on the f16 pipe (k7 s4 p3, 16 output channels, W % 64 == 0, H % 16 == 0): knobs = (stem_f16, stem_pieces)
    "stem": [
        _conv("c1_4x16x64", 2, 1, (4, 16, 64), 16, 7, S=4, P=3, knobs=(1, 2)),
        _conv("c2_4x16x64", 2, 2, (4, 16, 64), 16, 7, S=4, P=3, knobs=(1, 2)),
        _conv("c1_8x32x128", 2, 1, (8, 32, 128), 16, 7, S=4, P=3, knobs=(1, 2)),
        _conv("c2_8x32x128", 3, 2, (8, 32, 128), 16, 7, S=4, P=3, knobs=(1, 2)),          # B = 3
        _conv("c2_4x16x64_one_piece", 2, 2, (4, 16, 64), 16, 7, S=4, P=3, knobs=(1, 1)),
        _conv("c4_4x16x64_one_piece", 2, 4, (4, 16, 64), 16, 7, S=4, P=3, knobs=(1, 1)),
        _conv("c2_4x16x64_f16_off", 2, 2, (4, 16, 64), 16, 7, S=4, P=3, knobs=(0, 2)),
    ],
    # D. weight gradients on MFMA (csrc/conv_wgrad.hip): the gather-GEMM of a dense conv
    "gather": [
        _conv("k3s2p1_12to32_7x5x9_b1", 1, 12, (7, 5, 9), 32, 3, S=2, P=1),
        _conv("k3s2p1_32to64_8x8x8_b3", 3, 32, (8, 8, 8), 64, 3, S=2, P=1),
        _conv("k1s1p0_32to128_7x5x9_b1", 1, 32, (7, 5, 9), 128, 1),                       # 315 output voxels: rows that are no multiple of 4
        _conv("k1s1p0_12to32_8x8x8_b3", 3, 12, (8, 8, 8), 32, 1),
        _conv("k3s1p1_12to64_7x5x9_b3", 3, 12, (7, 5, 9), 64, 3, P=1),
        _conv("k3s1p1_32to32_8x8x8_b1", 1, 32, (8, 8, 8), 32, 3, P=1),
        _conv("k5s2p2_12to128_7x5x9_b3", 3, 12, (7, 5, 9), 128, 5, S=2, P=2),
        _conv("k5s2p2_32to64_8x8x8_b1", 1, 32, (8, 8, 8), 64, 5, S=2, P=2),
        _conv("k1s2p0_32to32_7x5x9_b3", 3, 32, (7, 5, 9), 32, 1, S=2),
        _conv("k1s2p0_12to128_8x8x8_b1", 1, 12, (8, 8, 8), 128, 1, S=2),
    ],
    # ... the stem weight gradient (k7 s4 p3): f16 = 0 the fp32 MFMA kernel (vx_down_wgrad_set_f16(0)), f16 = 1 the f16-pipe kernel (16 output channels, rows of 64 / 96 / 128)
    "down_wgrad": [_conv(f"c{ci}to{co}_{'x'.join(map(str, sp))}_b{B}_{'f16' if f else 'fp32'}", B, ci, sp, co, 7, S=4, P=3, f16=f)
                   for ci, co, sp, B, f in ((1, 16, (4, 16, 40), 2, 0), (2, 32, (4, 16, 40), 2, 0), (3, 32, (4, 16, 40), 3, 0), (4, 16, (4, 16, 40), 2, 0),
                                            (1, 32, (8, 16, 64), 2, 0), (2, 16, (8, 16, 64), 2, 0), (3, 16, (8, 16, 64), 2, 0), (4, 32, (8, 16, 64), 2, 0),
                                            (1, 16, (4, 16, 64), 2, 1), (2, 16, (4, 16, 64), 3, 1), (2, 16, (8, 16, 96), 2, 1), (3, 16, (8, 16, 96), 2, 1))],
    # ... the three grouped weight gradients of a JLC block in one launch (group width 4 / 8 / 16)
    "jlc_gather": [dict(id=f"w{cg}_{'x'.join(map(str, sp))}_b{B}", kind="jlc3", B=B, C=C, G=G, sp=sp)
                   for cg, C, G in ((4, 16, 4), (8, 32, 4), (16, 32, 2))
                   for sp, B in (((8, 8, 8), 2), ((3, 3, 3), 3), ((4, 6, 5), 2), ((1, 1, 2), 2))],
    # ... the 1x1x1 grouped weight gradient
    "gconv1": [_conv(f"w{cg}_v{V}_b{B}", B, C, (1, 1, V), C, 1, G=G) for cg, C, G in ((4, 16, 4), (8, 32, 4), (16, 32, 2)) for V, B in ((4, 2), (60, 3), (512, 2))],
    # E. 1x1 products (csrc/pointwise.hip); `on` = the entries a row is run through
    "pw": [
        _pw("general_8to6_v60", 2, 8, 6, 60, on=("fwd", "bwd_data", "bwd_weight", "mfma", "fused")),
        _pw("general_128to16_v1001", 2, 128, 16, 1001, on=("fwd", "bwd_data", "bwd_weight")),
        _pw("general_8to16_v1001_b3", 3, 8, 16, 1001, on=("fwd", "bwd_data", "bwd_weight")),
        _pw("v4_16to16_v16384", 2, 16, 16, 16384, on=("fwd", "bwd_weight")),               # the 16-byte forward kernel (and vx_pw_conv_set_v4(0))
        _pw("v4_64to16_v16384", 2, 64, 16, 16384, on=("fwd",)),
        _pw("concat8of24_to20_v60", 2, 24, 20, 60, C1=8, on=("fwd", "bwd_data", "bwd_weight", "mfma", "fused")),
        _pw("v27_32to48", 2, 32, 48, 27, on=("mfma", "fused")),
        _pw("concat8of24_to20_v27", 3, 24, 20, 27, C1=8, on=("mfma", "fused")),
        _pw("v125_64to32", 2, 64, 32, 125, on=("mfma",)),                                  # a reduction of 64: the K-split block
        _pw("v512_32to16", 2, 32, 16, 512, on=("mfma",)),
        _pw("concat8of24_to20_v64", 2, 24, 20, 64, C1=8, on=("fused",)),
        _pw("concat8of24_to20_v216", 2, 24, 20, 216, C1=8, on=("fused",)),
        _pw("v216_64to64", 2, 64, 64, 216, on=("fused",)),
        _pw("concat8of24_to20_v5000", 2, 24, 20, 5000, C1=8, on=("fused_big",)),
        _pw("v8192_16to48_b3", 3, 16, 48, 8192, on=("fused_big",)),
        _pw("concat8of24_to20_v8192", 2, 24, 20, 8192, C1=8, on=("fused_big",)),
    ],
    # ... vx_pw_wgrad_group: three jobs with different (Cin, Cout, V, B) and one fold of integer partial rows in one launch
    "pw_group": [dict(id="three_jobs_one_fold", kind="group", jobs=((8, 6, 60, 2), (32, 48, 27, 3), (24, 20, 1001, 1)), fold=(16, 150))],
    # F. ConvTranspose3d k2 s2 (csrc/pointwise.hip); knob = vx_upconv_set_mfma4
    "upconv": [
        dict(id="32to16_3x4x5", kind="convT", B=2, Ci=32, Co=16, sp=(3, 4, 5), wgrad=True),
        dict(id="24to8_3x3x3", kind="convT", B=2, Ci=24, Co=8, sp=(3, 3, 3), wgrad=False),
        dict(id="20to6_2x3x12", kind="convT", B=2, Ci=20, Co=6, sp=(2, 3, 12), wgrad=False),
        dict(id="48to24_3x5x8", kind="convT", B=2, Ci=48, Co=24, sp=(3, 5, 8), wgrad=False),
        dict(id="16to16_3x4x5", kind="convT", B=2, Ci=16, Co=16, sp=(3, 4, 5), wgrad=True),
        dict(id="128to64_2x2x2_b3", kind="convT", B=3, Ci=128, Co=64, sp=(2, 2, 2), wgrad=True),
    ],
    # G. patch-expand (Conv3d 16 -> 64 Cc, k3 p1, PixelShuffle 4; csrc/expand_mfma.hip)
    "expand": [_expand(f"cc{cc}_{'x'.join(map(str, sp))}_b{B}", B, cc, sp)
               for sp in ((4, 4, 4), (4, 8, 24), (4, 4, 40), (8, 4, 16)) for cc in (1, 2, 3) for B in ((3,) if (cc, sp) == (1, (8, 4, 16)) else (2,))]
              + [_expand("cc1_3x5x6_declined", 2, 1, (3, 5, 6))],                          # D, H, W no multiples of 4: the entries documented to decline return 1
    # H. patch embedding
    "patchify": [dict(id=f"k{K}_c{C}of{Ct}_{'x'.join(map(str, g))}_b{B}", kind="patchify", B=B, C=C, Ctot=Ct, c_off=co, grid=g, K=K)
                 for K in (2, 3, 4) for B, C, Ct, co, g in ((2, 2, 2, 0, (3, 5, 6)), (3, 2, 5, 2, (2, 3, 4)))],
    "patch_embed": [dict(id=f"c{Cin}of{Ct}_to{Cout}_{'x'.join(map(str, g))}_b{B}", kind="patch_embed", B=B, Cin=Cin, Ctot=Ct, c_off=co, Cout=Cout, grid=g)
                    for B, Cin, Ct, co, Cout, g in ((2, 1, 1, 0, 16, (2, 3, 4)), (2, 3, 5, 1, 48, (1, 2, 12)), (3, 8, 9, 1, 16, (1, 2, 12)), (2, 3, 3, 0, 16, (2, 3, 4)))],
    # I. small linear pieces
    "add": [dict(id="sixteen_tensors", kind="add", n=(1, 5, 1023, 1024, 4, 8, 4100, 60, 2, 3, 256, 257, 16, 12, 7, 4096), no_c=(1, 4, 6, 11, 15))],
    "channel_sum": [dict(id="b2_c5_v1001", kind="chansum", B=2, C=5, V=1001), dict(id="b3_c16_v60", kind="chansum", B=3, C=16, V=60)],
    "s2d": [dict(id="b2_c3_3x5x7", kind="s2d", B=2, C=3, sp=(3, 5, 7)), dict(id="b3_c4_1x1x3", kind="s2d", B=3, C=4, sp=(1, 1, 3))],
    "gram": [dict(id="c16_4x4x4", kind="gram", B=2, C=16, sp=(4, 4, 4)), dict(id="c8_2x4x8_b3", kind="gram", B=3, C=8, sp=(2, 4, 8))],
    "trilinear": [dict(id="3to5", kind="tri", BC=6, lo=(3, 3, 3), hi=(5, 5, 5)), dict(id="2to9", kind="tri", BC=4, lo=(2, 2, 2), hi=(9, 9, 9)),
                  dict(id="5to17", kind="tri", BC=3, lo=(5, 5, 5), hi=(17, 17, 17)), dict(id="mixed_3x2x5_to_5x9x17", kind="tri", BC=4, lo=(3, 2, 5), hi=(5, 9, 17)),
                  dict(id="mixed_2x5x1_to_9x17x8", kind="tri", BC=2, lo=(2, 5, 1), hi=(9, 17, 8)),                     # rows of 8: the 16-byte store kernel
                  dict(id="w4_kept_3x3x4_to_5x5x4", kind="tri", BC=3, lo=(3, 3, 4), hi=(5, 5, 4))],
    "sqdiff": [dict(id=f"n{n}_b{B}", kind="sqdiff", B=B, n=n, pad=pad) for n, B, pad in ((4100, 2, 12), (1023, 3, 1), (8, 2, 0))],
    "axpy": [dict(id=f"alpha{a}_n{n}", kind="axpy", n=n, alpha=float(a)) for a, n in ((1, 1023), (2, 4100))],
}

ROWS = [(fam, row) for fam, rows in CASES.items() for row in rows]
ROW_IDS = [f"{fam}-{row['id']}" for fam, row in ROWS]


def rows(family):
    return CASES[family]


def ids(family):
    return [r["id"] for r in CASES[family]]


# ---------------------------------------------------------------------------------------------------------------------- inputs
def _seed(row):
    return sum(ord(c) * (i + 1) for i, c in enumerate(row["id"])) % 100003


def conv_out_shape(r):
    D, H, W = ((n + 2 * r["P"] - r["K"]) // r["S"] + 1 for n in r["sp"])
    ps = r["ps"]
    return (r["B"], r["Cout"] // ps ** 3, D * ps, H * ps, W * ps)


@functools.lru_cache(maxsize=None)
def _inputs(fam, rid):
    r = next(x for x in CASES[fam] if x["id"] == rid)
    s, k = _seed(r), r["kind"]
    if k == "conv":
        return dict(x=ints(r["B"], r["Cin"], *r["sp"], seed=s), w=ints(r["Cout"], r["Cin"] // r["G"], r["K"], r["K"], r["K"], seed=s + 1), b=ints(r["Cout"], seed=s + 2),
                    dy=ints(*conv_out_shape(r), seed=s + 3))
    if k == "convT":
        d, h, w = r["sp"]
        return dict(x=ints(r["B"], r["Ci"], d, h, w, seed=s), w=ints(r["Ci"], r["Co"], 2, 2, 2, seed=s + 1), b=ints(r["Co"], seed=s + 2), dy=ints(r["B"], r["Co"], 2 * d, 2 * h, 2 * w, seed=s + 3))
    if k == "jlc3":
        shp = (r["B"], r["C"], *r["sp"])
        return dict(x=ints(*shp, seed=s), g1=ints(*shp, seed=s + 1), g3=ints(*shp, seed=s + 2), g5=ints(*shp, seed=s + 3))
    if k == "group":
        d = {}
        for j, (ci, co, V, B) in enumerate(r["jobs"]):
            d[f"x{j}"], d[f"dy{j}"] = ints(B, ci, V, seed=s + 2 * j), ints(B, co, V, seed=s + 2 * j + 1)
        C, nrows = r["fold"]
        d["part"] = ints(nrows, 2 * C, seed=s + 50)
        return d
    if k == "patchify":
        d, h, w = r["grid"]
        return dict(x=ints(r["B"], r["Ctot"], d * r["K"], h * r["K"], w * r["K"], seed=s))
    if k == "patch_embed":
        d, h, w = r["grid"]
        return dict(x=ints(r["B"], r["Ctot"], 4 * d, 4 * h, 4 * w, seed=s), w=ints(r["Cout"], r["Cin"], 4, 4, 4, seed=s + 1), b=ints(r["Cout"], seed=s + 2), dy=ints(r["B"], r["Cout"], d, h, w, seed=s + 3))
    if k == "add":
        d = {}
        for j, n in enumerate(r["n"]):
            d[f"a{j}"], d[f"b{j}"] = ints(n, seed=s + 3 * j), ints(n, seed=s + 3 * j + 1)
            if j not in r["no_c"]:
                d[f"c{j}"] = ints(n, seed=s + 3 * j + 2)
        return d
    if k == "chansum":
        return dict(dy=ints(r["B"], r["C"], r["V"], seed=s))
    if k == "s2d":
        d, h, w = r["sp"]
        return dict(x=ints(r["B"], r["C"], 2 * d, 2 * h, 2 * w, seed=s), z=ints(r["B"], 8 * r["C"], d, h, w, seed=s + 1))
    if k == "gram":
        return dict(x=ints(r["B"], r["C"], *r["sp"], seed=s), dG=ints(r["B"], r["C"], r["C"], seed=s + 1))
    if k == "tri":
        return dict(x=ints(r["BC"], 1, *r["lo"], seed=s), dout=ints(r["BC"], 1, *r["hi"], seed=s + 1))
    if k == "sqdiff":
        return dict(a=ints(r["B"], r["n"], seed=s), b=ints(r["B"], r["n"] + r["pad"], seed=s + 1))
    if k == "axpy":
        return dict(x=ints(r["n"], seed=s), z=ints(r["n"], seed=s + 1), dout=ints(r["n"], seed=s + 2))
    raise KeyError(k)


def inputs(fam, row):
    """the row's operands: integer-valued fp32 CPU tensors (never modified)"""
    return _inputs(fam, row["id"])


# ---------------------------------------------------------------------------------------------------------------------- the operations, dtype-generic
def _grads(outs, wrt, cots):
    return torch.autograd.grad(outs, wrt, cots, allow_unused=False)


def patchify(x, K):
    """out[b, c K^3 + (kd K + kh) K + kw, z, y, x] = x[b, c, z K + kd, y K + kh, x K + kw] (include/veloxseg_hip.h: vx_patchify)"""
    B, C, D, H, W = x.shape
    d, h, w = D // K, H // K, W // K
    return x.reshape(B, C, d, K, h, K, w, K).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(B, C * K ** 3, d, h, w)


def upsample(x, size):
    """oracle.veloxseg_oracle.upsample_trilinear in the dtype of x (its interpolation matrices are fp32: at dyadic ratios exact)"""
    Ad, Ah, Aw = (O.interp_matrix(x.shape[2 + i], size[i]).to(x.dtype) for i in range(3))
    x = torch.einsum("bcdhw,Dd->bcDhw", x, Ad)
    x = torch.einsum("bcdhw,Hh->bcdHw", x, Ah)
    return torch.einsum("bcdhw,Ww->bcdhW", x, Aw)


def operate(r, t):
    """the row's operation on the operand dict t (any dtype): every output the GPU test compares, WITHOUT prefills"""
    k = r["kind"]
    if k == "conv":
        x, w, b = (t[n].clone().requires_grad_(True) for n in ("x", "w", "b"))
        y = F.conv3d(x, w, b, stride=r["S"], padding=r["P"], groups=r["G"])
        if r["ps"] > 1:
            y = O.pixel_shuffle3d(y, r["ps"])
        dx, dw, db = _grads(y, (x, w, b), t["dy"])
        return dict(y=y.detach(), dx=dx, dw=dw, db=db)
    if k == "convT":
        x, w, b = (t[n].clone().requires_grad_(True) for n in ("x", "w", "b"))
        y = F.conv_transpose3d(x, w, b, stride=2)
        dx, dw, db = _grads(y, (x, w, b), t["dy"])
        return dict(y=y.detach(), dx=dx, dw=dw, db=db)
    if k == "jlc3":
        out, cg = {}, r["C"] // r["G"]
        for kk in (1, 3, 5):
            w = torch.zeros(r["C"], cg, kk, kk, kk, dtype=t["x"].dtype, requires_grad=True)
            out[f"dw{kk}"] = _grads(F.conv3d(t["x"], w, None, padding=kk // 2, groups=r["G"]), (w,), t[f"g{kk}"])[0]
        return out
    if k == "group":
        out = {}
        for j in range(len(r["jobs"])):
            out[f"dw{j}"] = torch.einsum("bov,biv->oi", t[f"dy{j}"], t[f"x{j}"])
            out[f"db{j}"] = t[f"dy{j}"].sum((0, 2))
        C = r["fold"][0]
        s = t["part"].sum(0)
        out["dgamma"], out["dbeta"] = s[:C], s[C:]
        return out
    if k == "patchify":
        return dict(out=patchify(t["x"][:, r["c_off"]:r["c_off"] + r["C"]], r["K"]))
    if k == "patch_embed":
        xs = t["x"][:, r["c_off"]:r["c_off"] + r["Cin"]]
        w, b = (t[n].clone().requires_grad_(True) for n in ("w", "b"))
        y = F.conv3d(xs, w, b, stride=4)
        dw, db = _grads(y, (w, b), t["dy"])
        return dict(y=y.detach(), dw=dw, db=db)
    if k == "add":
        return {f"out{j}": t[f"a{j}"] + t[f"b{j}"] + (t[f"c{j}"] if f"c{j}" in t else 0) for j in range(len(r["n"]))}
    if k == "chansum":
        return dict(db=t["dy"].sum((0, 2)))
    if k == "s2d":
        x = t["x"].clone().requires_grad_(True)
        out = O.space_to_depth2(x)
        return dict(out=out.detach(), inv=_grads(out, (x,), t["z"])[0])         # (the inverse of a permutation is its adjoint)
    if k == "gram":
        x = t["x"].clone().requires_grad_(True)
        G = O.gram(x)
        return dict(G=G.detach(), dx=_grads(G, (x,), t["dG"])[0])
    if k == "tri":
        x = t["x"].clone().requires_grad_(True)
        out = upsample(x, r["hi"])
        return dict(out=out.detach(), dx=_grads(out, (x,), t["dout"])[0])
    if k == "sqdiff":
        d = t["a"] - t["b"][:, :r["n"]]
        return dict(acc=(d * d).sum().reshape(1))
    if k == "axpy":
        return dict(out=r["alpha"] * t["x"] + t["z"], dx=r["alpha"] * t["dout"], dz=t["dout"].clone())
    raise KeyError(k)


@functools.lru_cache(maxsize=None)
def _reference(fam, rid):
    r = next(x for x in CASES[fam] if x["id"] == rid)
    return operate(r, {n: v.double() for n, v in _inputs(fam, rid).items()})


def reference(fam, row):
    """the fp64 oracle of every output of the row (computed once, shared, never modified)"""
    return _reference(fam, row["id"])


def magnitude(fam, row):
    """sum |x_i| |w_i| per output element, in fp64: the same operation on the absolute values of the operands (sqdiff: a and b of opposite signs)"""
    t = {n: v.double().abs() for n, v in inputs(fam, row).items()}
    if row["kind"] == "sqdiff":
        t["b"] = -t["b"]
    return operate(row, t)
