"""Oracle of the elastic deformation (csrc/augment_elastic.hip through utils/augment.py): a numpy restatement of the three rules of
include/veloxseg_hip.h, each evaluated in a chosen dtype, the exact case table, the bounds, and the restatement of Rand3DElasticd's draw order.  It shares with
tests/affine_ref.py what the two rules share (the record values, the matrices, the data of a row, the lerp, gamma, the neighbour difference, the affine draw order) and
restates the sampling from the source coordinate on, because there the coordinates are its own; tests/test_elastic_cpu.py holds that restatement to affine_ref's on
every exact row of affine_ref with a zero field and with none.

  * noise: element e of a field uses word e & 3 of philox4x32(counter e >> 2, stream STREAM, key); u = (float)((int)(r >> 8) - 2^23) * 2^-23;
  * weights: tail = int(max(3 sigma, 0.5) + 0.5), w_k = (erf((k + 1/2) / (sigma sqrt 2)) - erf((k - 1/2) / (sigma sqrt 2))) / 2 in fp64, not normalised;
  * smoothing: augment_stats_ref's blur (passes W, H, D, zeros outside, y = w_0 x_0 + sum_k w_k (x_-k + x_+k), k ascending, the pair first) with ONE weight vector;
  * sampling: p_a = o_a - 0.5 (Out_a - 1);  p'_a = p_a + m u_a[o];  s_a = ((A[a][0] p'_0 + A[a][1] p'_1) + A[a][2] p'_2) + c_a, then affine_ref's rule;
  * the draw order (modelled on MONAI 1.x, UNPINNED against MONAI itself, which is not installed): R.rand() < prob first; only if that fires seed = R.randint(2^31 - 1),
    magnitude = R.uniform(*magnitude_range), sigma = R.uniform(*sigma_range), then RandAffined's nine uniforms.
CPU-only at import."""
import functools
import math

import numpy as np

import affine_ref as R
import augment_stats_ref as SR
import exact_ref as X
from oracle.philox import philox4x32

STREAM = 0x454C4153544943                        # "ELASTIC"
MAX_TAIL, MAX_SIGMA = 48, 16.0


# ====================================================================================================================== noise
def uniforms(key, n, e0=0):
    """fp32 (n,): the uniforms of elements e0 .. e0 + n - 1 of the field drawn under `key`"""
    lo, hi = e0 >> 2, (e0 + n - 1) >> 2
    w = philox4x32(np.arange(lo, hi + 1, dtype=np.uint64), STREAM, key).reshape(-1)[e0 - 4 * lo: e0 - 4 * lo + n]
    return ((w >> np.uint32(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23)


def noise_planes(keys, n_planes, V):
    """fp32 (n_planes, V): plane j belongs to field j / 3 (key keys[j / 3]) and holds its elements (j % 3) V .. (j % 3) V + V - 1"""
    return np.stack([uniforms(keys[j // 3], V, (j % 3) * V) for j in range(n_planes)])


# ====================================================================================================================== weights, smoothing
def tail_of(sigma):
    return int(max(3.0 * sigma, 0.5) + 0.5)


def weights64(sigma):
    """fp64 half vector w_0 .. w_tail"""
    t = 1.0 / (sigma * math.sqrt(2.0))
    return np.array([0.5 * (math.erf((k + 0.5) * t) - math.erf((k - 0.5) * t)) for k in range(tail_of(sigma) + 1)], dtype=np.float64)


def full(half):
    """half vector w_0 .. w_tail -> the full symmetric vector"""
    half = np.asarray(half)
    return np.concatenate([half[:0:-1], half])


def smooth64(x, half):
    """x (D, H, W), the fp32 half weights the kernel gets -> fp64, nothing rounded in between"""
    w = full(np.asarray(half, dtype=np.float32))
    return SR.blur64(x, (w, w, w))


def smooth32(x, half, fma):
    """the kernel's fp32 rule step by step (augment_stats_ref.blur32), with or without fma in the accumulation"""
    w = full(np.asarray(half, dtype=np.float32))
    return SR.blur32(x, (w, w, w), fma)


def smooth_bound(x, half):
    """augment_stats_ref.blur_bound at this tail: 4 (tail + 3) 2^-24 times the fp64 smoothing of |x|.  Each pass is a (tail + 2)-rounding dot product plus the rounding
    of the pair add, three passes, weights that sum to at most 1: (1 + u)^(3 (tail + 3)) - 1 <= 4 (tail + 3) u, also at tail 48 (153 u against 204 u)"""
    w = full(np.asarray(half, dtype=np.float32))
    return SR.blur_bound(x, (w, w, w))


# ---- the exact smoothing cases: dyadic weights, integer data -----------------------------------------------------------------------------------------------------------
SMOOTH_TAILS = (0, 1, 16, 17, 48)


def dyadic_half(tail, seed):
    """w_0 = 1/2 and up to six taps of 1/4 or 1/8 (the first two, the middle one, the last two, one more), zeros between: a pass multiplies the largest value by at most
    3.5 and adds three fractional bits, so integer data of |v| <= 64 stays below 2^12 with nine fractional bits through the three passes and every product and sum is
    exact in fp32, fused or not (tests/test_elastic_cpu.py evaluates the rule both ways)"""
    rs = np.random.RandomState(seed)
    w = np.zeros(tail + 1, dtype=np.float32)
    w[0] = 0.5
    for k in sorted({1, 2, tail // 2, tail - 1, tail, int(rs.randint(1, tail + 1)) if tail else 0}):
        if 1 <= k <= tail:
            w[k] = (0.25, 0.125)[int(rs.randint(2))]
    return w


def dyadic_data(shape, n_planes, seed):
    """fp32 (n_planes, D, H, W) integers of |v| <= 64, non-zero at both ends of every axis"""
    x = np.stack([X.ints(*shape, seed=seed + j, lo=-64, hi=64).numpy() for j in range(n_planes)])
    x[:, 0, 0, 0], x[:, -1, -1, -1] = 64.0, -63.0
    return x


def smooth_shapes(rows, tile_w, strip, tile_line):
    """one voxel; shorter than the tails 17 and 48; one row past a W-pass block and one output past its chunk; one output past the H (then the D) pass's tile along the
    axis and one column past its strip"""
    return [(1, 1, 1), (5, 5, 5), (3, (rows + 1 + 2) // 3, tile_w + 1), (3, tile_line + 1, strip + 1), (tile_line + 1, 2, strip + 1)]


# ====================================================================================================================== the sampling rule
def displaced(out, field, m, dtype=np.float64):
    """p'[3], each of shape `out`: p_a = o_a - 0.5 (Out_a - 1), p'_a = p_a + m u_a, every operation rounded to `dtype`; field None: p itself"""
    t = dtype
    p = [(np.arange(out[a]).astype(t) - (t(0.5) * t(out[a] - 1)).astype(t)).astype(t) for a in range(3)]
    p = [np.broadcast_to(q, tuple(out)).astype(t) for q in (p[0][:, None, None], p[1][None, :, None], p[2][None, None, :])]
    if field is None:
        return p
    u = np.asarray(field).astype(t)
    return [(p[a] + (t(np.float32(m)) * u[a]).astype(t)).astype(t) for a in range(3)]


def coords(A, c, out, field=None, m=0.0, dtype=np.float64):
    """source coordinates s[3] BEFORE any clamp: s_a = ((A[a][0] p'_0 + A[a][1] p'_1) + A[a][2] p'_2) + c_a, every operation rounded to `dtype`"""
    t = dtype
    A, c = np.asarray(A).astype(t), np.asarray(c).astype(t)
    p = displaced(out, field, m, t)
    s = []
    for a in range(3):
        q = ((A[a, 0] * p[0]).astype(t) + (A[a, 1] * p[1]).astype(t)).astype(t)
        q = (q + (A[a, 2] * p[2]).astype(t)).astype(t)
        s.append((q + c[a]).astype(t))
    return s


def sample(x, A, c, out, mode, pad, cval=0.0, field=None, m=0.0, lo=None, hi=None, origin=(0, 0, 0), dtype=np.float64):
    """affine_ref.sample with the displaced coordinates: x is the array the window lives in, window index i is x[i + origin]; mode 0 trilinear / 1 nearest, pad 0
    border / 1 constant.  Trilinear evaluates in `dtype` and returns `dtype`; nearest returns x's dtype."""
    t = dtype
    x = np.asarray(x)
    lo = [0, 0, 0] if lo is None else list(lo)
    hi = [x.shape[a] - 1 for a in range(3)] if hi is None else list(hi)
    k = 0 if pad == 0 else 1
    s = [np.minimum(np.maximum(sa, t(lo[a] - k)), t(hi[a] + k)) for a, sa in enumerate(coords(A, c, out, field, m, t))]

    def gather(src, idx, fill):
        ok = np.ones(tuple(out), dtype=bool)
        for a in range(3):
            ok &= (idx[a] >= lo[a]) & (idx[a] <= hi[a])
        safe = [np.clip(idx[a], lo[a], hi[a]) + origin[a] for a in range(3)]
        return np.where(ok, src[safe[0], safe[1], safe[2]], fill)

    if mode == 1:
        idx = [np.rint(sa).astype(np.int64) for sa in s]
        return gather(x, idx, np.array(cval).astype(x.dtype)).astype(x.dtype)
    i0 = [np.floor(sa).astype(np.int64) for sa in s]
    l = [(sa - ia.astype(t)).astype(t) for sa, ia in zip(s, i0)]
    i1 = [np.minimum(ia + 1, hi[a]) if pad == 0 else ia + 1 for a, ia in enumerate(i0)]
    xt = x.astype(t)
    v = {(a, b, cc): gather(xt, [(i0, i1)[a][0], (i0, i1)[b][1], (i0, i1)[cc][2]], t(cval)).astype(t) for a in (0, 1) for b in (0, 1) for cc in (0, 1)}
    with np.errstate(invalid="ignore"):
        r = {(a, b): R._lerp(v[a, b, 0], v[a, b, 1], l[2], t) for a in (0, 1) for b in (0, 1)}          # along W first,
        q = {a: R._lerp(r[a, 0], r[a, 1], l[1], t) for a in (0, 1)}                                     # then H,
        return R._lerp(q[0], q[1], l[0], t)                                                             # then D


def coord_bound(A, c, out, field, m):
    """bound on |fp32 coordinate - exact coordinate| for the record values (A, c) and the fp32 field: affine_ref.coord_bound with the coordinate term extended by the
    displacement, eps = gamma(5) max_a (sum_i |A[a][i]| |p'_i|max + |c_a|): a term A[a][i] p'_i passes through the rounding of p'_i = p_i + m u_i, its product and three
    additions (the rounding of m u_i alone is relative to a displacement of a few voxels, far below |p'_i|max, and is not counted apart)"""
    A, c = np.abs(np.asarray(A, dtype=np.float64)), np.abs(np.asarray(c, dtype=np.float64))
    pmax = np.array([float(np.abs(q).max()) for q in displaced(out, field, m, np.float64)])
    return float(R.gamma(5) * ((A @ pmax) + c).max())


def near_tie(A, c, out, field, m, lo, hi, pad, eps):
    """affine_ref.near_tie on the displaced coordinates"""
    s = coords(A, c, out, field, m, np.float64)
    k = 0 if pad == 0 else 1
    bad = np.zeros(tuple(out), dtype=bool)
    for a in range(3):
        sa = np.clip(s[a], lo[a] - k, hi[a] + k)
        bad |= np.abs((sa - np.floor(sa)) - 0.5) <= eps
    return bad


# ====================================================================================================================== exact rows
# output -> source extents: one brick exactly, odd extents, more than one brick along W, a one-voxel-thick source; the same extents on both sides and across
EXTENTS = (((9, 7, 5), (9, 7, 5)), ((8, 8, 8), (8, 8, 8)), ((5, 6, 17), (5, 6, 17)), ((1, 1, 3), (1, 1, 3)), ((9, 7, 5), (8, 8, 8)), ((5, 6, 17), (1, 1, 3)))
MAGNITUDES = (1.0, 2.0, 0.5)
CVAL = R.CVAL
EXACT_ROWS = [dict(id=f"{name}_{'x'.join(map(str, o))}_from_{'x'.join(map(str, n))}", matrix=name, out=o, n=n, m=MAGNITUDES[(i + j) % 3])
              for i, name in enumerate(R.MATRICES) for j, (o, n) in enumerate(EXTENTS)]


@functools.lru_cache(maxsize=None)
def _field(out, seed):
    f = (np.random.RandomState(seed).randint(-12, 13, size=(3,) + tuple(out)) / 4.0).astype(np.float32)
    f.setflags(write=False)
    return f


def field(row):
    """fp32 (3, Do, Ho, Wo): multiples of 1/4, |u| <= 3; read-only, computed once"""
    return _field(tuple(row["out"]), R._seed(row["id"]) + 1)


@functools.lru_cache(maxsize=None)
def _reference(rid, mode, pad, code):
    row = next(r for r in EXACT_ROWS if r["id"] == rid)
    A, c = R.record_values(R.row_matrix(row), row["n"])
    x = R.image(row) if code == 0 else R.label(row, code)
    out = sample(x, A, c, row["out"], mode, pad, CVAL, field(row), row["m"])
    out.setflags(write=False)
    return out


def reference(row, mode, pad, code=0):
    """the fp64 oracle of an exact row (code 0: the image) or the nearest oracle of its labels of type `code`; computed once, shared, never modified"""
    return _reference(row["id"], mode, pad, code)


# ====================================================================================================================== off the dyadic rows
OFF_SEED, OFF_N, OFF_SIGMA, OFF_FIELD_SEED, OFF_DISPLACEMENT = 11, R.OFF_N, 5.0, 77, 3.0


def off_magnitude(field):
    """the magnitude that makes the largest displacement of `field` OFF_DISPLACEMENT voxels, as the fp32 value the record holds"""
    return float(np.float32(OFF_DISPLACEMENT / float(np.abs(field).max())))


# ====================================================================================================================== Rand3DElasticd: the draw order
def pair(v):
    return (float(v), float(v)) if np.isscalar(v) else (float(min(v)), float(max(v)))


def draws(seed, prob, sigma_range, magnitude_range, rotate_range, scale_range, translate_range, count):
    """what `count` successive samples draw from RandomState(seed) -> [None | (seed, magnitude, sigma, rotate, translate, scale)]"""
    G = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        if not G.rand() < prob:
            out.append(None)
            continue
        s = int(G.randint(2 ** 31 - 1))
        mag = float(G.uniform(*pair(magnitude_range)))
        sg = float(G.uniform(*pair(sigma_range)))
        rot = [float(G.uniform(lo, hi)) for lo, hi in R.ranges(rotate_range)]
        tra = [float(G.uniform(lo, hi)) for lo, hi in R.ranges(translate_range)]
        sca = [1.0 + float(G.uniform(lo, hi)) for lo, hi in R.ranges(scale_range)]
        out.append((s, mag, sg, rot, tra, sca))
    return out
