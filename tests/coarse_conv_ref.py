"""fp64 oracles on integer-valued data for the coarse-level convolutions: the JLC grouped convolutions of csrc/jlc_cl.hip (k = 1, 3, 5 from one
input, their per-slot InstanceNorm partial sums, and the summed input gradient) and the k3 s2 DownConv path of csrc/conv_mfma.hip (forward and input gradient).

x, the three output gradients and dy are integers in [-2, 2], the weights are in {-1, 0, 1}, biases and d_o are integers in [-3, 3].  Every product and every partial sum
is then an integer far below 2^24 (`cl_magnitude` / `cm_magnitude` compute the bound from |x| * |w|; the tests assert it), the block maximum of every staged volume is 1
or 2, so the two fp16 pieces of v * 2^e are (v * 2^e, 0) exactly, and a correct kernel returns the fp64 result VALUE FOR VALUE in any summation order.

CPU-only at import.  The references are computed once per case (lru_cache) and must not be modified by their users."""
import functools

import torch
import torch.nn.functional as F

LIMIT = float(1 << 24)

# (B, C, groups, spatial): the smallest shapes at which the ring / staging code of jlc_cl.hip can go wrong
CL_CASES = {
    "w8_8cube_two_tiles_per_wave": (2, 64, 8, (8, 8, 8)),      # <8, 2>; the ring (8 entries) is longer than the K = 3 stream (7)
    "w16_4cube": (2, 128, 8, (4, 4, 4)),                        # <16, 1>, rows of 4 voxels at the padded stride
    "w16_3cube_idle_waves": (3, 128, 8, (3, 3, 3)),             # 2 tiles: two waves have none but take part in every barrier; ragged tile
    "w8_5x7x3_ragged": (1, 32, 4, (5, 7, 3)),                   # ragged tile, W < 4
    "w8_8x4x6_aniso": (1, 64, 8, (8, 4, 6)),
}
# (B, Cin, Cout, spatial) of the k3 s2 p1 layers
CM_CASES = {
    "16to32_8cube": (2, 16, 32, (8, 8, 8)),
    "64to128_4cube_ksplit": (2, 64, 128, (4, 4, 4)),
    "32to64_6x4x8_b3": (3, 32, 64, (6, 4, 8)),
    "12to20_4x6x4_81_ksteps": (2, 12, 20, (4, 6, 4)),           # 81 forward k-steps, 5 per tap in the input gradient: neither a multiple of the group of 8
}


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, tuple(shape), generator=g).float()


# ---------------------------------------------------------------------------------------------------------------------- JLC coarse convolutions
def cl_slots(V):
    """(slots per (b, c), tiles per wave) of the partial sums: slot s = the wave that owns the 16-voxel tiles [s * tpw, (s + 1) * tpw); 4 waves per block"""
    nt = (V + 15) // 16
    tpw = 2 if nt >= 32 else 1
    nchunk = (nt + 4 * tpw - 1) // (4 * tpw)
    return 4 * nchunk, tpw


@functools.lru_cache(maxsize=None)
def cl_inputs(name):
    B, C, G, sp = CL_CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CL_CASES).index(name))
    Cg = C // G
    t = dict(x=_ints(g, -2, 2, B, C, *sp), d_o=_ints(g, -3, 3, B, C, *sp))
    for k in (1, 3, 5):
        t[f"w{k}"] = _ints(g, -1, 1, C, Cg, k, k, k)
        t[f"b{k}"] = _ints(g, -3, 3, C)
        t[f"g{k}"] = _ints(g, -2, 2, B, C, *sp)
    return t


@functools.lru_cache(maxsize=None)
def cl_reference(name):
    """fp64: y1, y3, y5 (B, C, D, H, W); part (3, B * C, slots, 2) = per-slot (sum, sum of squares) of y1 / y3 / y5; dx"""
    B, C, G, sp = CL_CASES[name]
    t = {k: v.double() for k, v in cl_inputs(name).items()}
    V = sp[0] * sp[1] * sp[2]
    nslot, tpw = cl_slots(V)
    ref, parts = {}, []
    dx = t["d_o"].clone()
    for k in (1, 3, 5):
        y = F.conv3d(t["x"], t[f"w{k}"], t[f"b{k}"], padding=k // 2, groups=G)
        ref[f"y{k}"] = y
        yv = y.reshape(B * C, V)
        p = torch.zeros(B * C, nslot, 2, dtype=torch.float64)
        for s in range(nslot):
            seg = yv[:, 16 * tpw * s:16 * tpw * (s + 1)]          # (empty for the slots of waves without a tile: they hold zeros)
            p[:, s, 0], p[:, s, 1] = seg.sum(1), (seg * seg).sum(1)
        parts.append(p)
        dx = dx + F.conv_transpose3d(t[f"g{k}"], t[f"w{k}"], None, padding=k // 2, groups=G)
    ref["part"], ref["dx"] = torch.stack(parts), dx
    return ref


def cl_magnitude(name):
    """the largest value any summation order can reach on the way to an output: sums of |operand| products (+ |bias| / |d_o|), and the per-slot sums of |y|"""
    B, C, G, sp = CL_CASES[name]
    t = {k: v.double().abs() for k, v in cl_inputs(name).items()}
    m, dx = 0.0, t["d_o"].clone()
    for k in (1, 3, 5):
        y = F.conv3d(t["x"], t[f"w{k}"], t[f"b{k}"], padding=k // 2, groups=G)
        m = max(m, float(y.max()), float(y.reshape(B * C, -1).sum(1).max()))
        dx = dx + F.conv_transpose3d(t[f"g{k}"], t[f"w{k}"], None, padding=k // 2, groups=G)
    return max(m, float(dx.max()))


# ---------------------------------------------------------------------------------------------------------------------- k3 s2 DownConv on MFMA
@functools.lru_cache(maxsize=None)
def cm_inputs(name):
    B, Cin, Cout, sp = CM_CASES[name]
    g = torch.Generator().manual_seed(2000 + sorted(CM_CASES).index(name))
    so = tuple(s // 2 for s in sp)
    return dict(x=_ints(g, -2, 2, B, Cin, *sp), w=_ints(g, -1, 1, Cout, Cin, 3, 3, 3), b=_ints(g, -3, 3, Cout), dy=_ints(g, -2, 2, B, Cout, *so),
                dx0=_ints(g, -8, 8, B, Cin, *sp))


@functools.lru_cache(maxsize=None)
def cm_reference(name):
    """fp64: y = conv(x, w, b; k3 s2 p1); dx = conv^T(dy, w) (accumulate = 0) and dx_acc = dx0 + conv^T(dy, w) (accumulate = 1)"""
    t = {k: v.double() for k, v in cm_inputs(name).items()}
    dx = F.conv_transpose3d(t["dy"], t["w"], None, stride=2, padding=1, output_padding=1)
    return dict(y=F.conv3d(t["x"], t["w"], t["b"], stride=2, padding=1), dx=dx, dx_acc=t["dx0"] + dx)


def cm_magnitude(name):
    t = {k: v.double().abs() for k, v in cm_inputs(name).items()}
    y = F.conv3d(t["x"], t["w"], t["b"], stride=2, padding=1)
    dx = t["dx0"] + F.conv_transpose3d(t["dy"], t["w"], None, stride=2, padding=1, output_padding=1)
    return max(float(y.max()), float(dx.max()))
