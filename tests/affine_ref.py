"""Oracle of the affine resampler (csrc/augment_affine.hip through utils/augment.py): a numpy restatement of the rule of
include/veloxseg_hip.h, evaluated in a chosen dtype like eval_ref.rotate_exact, the exact case table, and the restatement of RandAffined's draw order and matrix.

Exact rows: the data is integer-valued (|v| <= 64) and the matrices are dyadic, so every coordinate, weight and lerp is exactly representable in fp32, with or
without fused multiply-adds, and the kernel must return the oracle VALUE FOR VALUE.  tests/test_affine_cpu.py proves that premise for every row (fp32 and fp64
evaluation agree in both modes and both paddings); tests/test_affine_gpu.py runs the kernel on the same rows.  CPU-only at import."""
import functools
import math

import numpy as np

import exact_ref as E

U = 2.0 ** -24                                   # unit roundoff of fp32


def gamma(k):
    """k roundings in a row: |(1 + d_1) .. (1 + d_k) - 1| <= k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


# ====================================================================================================================== the rule
def record_values(matrix, n):
    """what the host puts into the record: A = fp32(matrix[:, :3]), c_a = fp32(0.5 (n_a - 1) + t_a), the sum formed in fp64 and rounded once"""
    m = np.asarray(matrix, dtype=np.float64)
    A = m[:, :3].astype(np.float32)
    c = np.array([0.5 * (n[a] - 1) + m[a, 3] for a in range(3)], dtype=np.float64).astype(np.float32)
    return A, c


def coords(A, c, out, dtype=np.float64):
    """source coordinates s[3] (each of shape `out`) BEFORE any clamp, every operation rounded to `dtype`:
    p_a = o_a - 0.5 (Out_a - 1);  s_a = ((A[a][0] p_0 + A[a][1] p_1) + A[a][2] p_2) + c_a"""
    t = dtype
    A, c = np.asarray(A).astype(t), np.asarray(c).astype(t)
    p = [(np.arange(out[a]).astype(t) - (t(0.5) * t(out[a] - 1)).astype(t)).astype(t) for a in range(3)]
    p = [p[0][:, None, None], p[1][None, :, None], p[2][None, None, :]]
    s = []
    for a in range(3):
        q = ((A[a, 0] * p[0]).astype(t) + (A[a, 1] * p[1]).astype(t)).astype(t)
        q = (q + (A[a, 2] * p[2]).astype(t)).astype(t)
        s.append(np.broadcast_to((q + c[a]).astype(t), tuple(out)).astype(t))
    return s


def _lerp(u, v, l, t):
    return (((t(1) - l).astype(t) * u).astype(t) + (l * v).astype(t)).astype(t)


def sample(x, A, c, out, mode, pad, cval=0.0, lo=None, hi=None, origin=(0, 0, 0), dtype=np.float64):
    """x: the array the window lives in; window index i is x[i + origin].  [lo, hi] (window coordinates) defaults to the whole of a window that IS x.
    mode 0 trilinear / 1 nearest, pad 0 border / 1 constant.  Trilinear evaluates in `dtype` and returns `dtype`; nearest returns x's dtype."""
    t = dtype
    x = np.asarray(x)
    lo = [0, 0, 0] if lo is None else list(lo)
    hi = [x.shape[a] - 1 for a in range(3)] if hi is None else list(hi)
    m = 0 if pad == 0 else 1
    s = [np.minimum(np.maximum(sa, t(lo[a] - m)), t(hi[a] + m)) for a, sa in enumerate(coords(A, c, out, t))]

    def gather(src, idx, fill):
        ok = np.ones(tuple(out), dtype=bool)
        for a in range(3):
            ok &= (idx[a] >= lo[a]) & (idx[a] <= hi[a])
        safe = [np.clip(idx[a], lo[a], hi[a]) + origin[a] for a in range(3)]
        return np.where(ok, src[safe[0], safe[1], safe[2]], fill)

    if mode == 1:
        idx = [np.rint(sa).astype(np.int64) for sa in s]                 # round half to even (nearbyintf in the default rounding mode)
        return gather(x, idx, np.array(cval).astype(x.dtype)).astype(x.dtype)
    i0 = [np.floor(sa).astype(np.int64) for sa in s]
    l = [(sa - ia.astype(t)).astype(t) for sa, ia in zip(s, i0)]
    i1 = [np.minimum(ia + 1, hi[a]) if pad == 0 else ia + 1 for a, ia in enumerate(i0)]
    xt = x.astype(t)
    v = {(a, b, cc): gather(xt, [(i0, i1)[a][0], (i0, i1)[b][1], (i0, i1)[cc][2]], t(cval)).astype(t) for a in (0, 1) for b in (0, 1) for cc in (0, 1)}
    with np.errstate(invalid="ignore"):
        r = {(a, b): _lerp(v[a, b, 0], v[a, b, 1], l[2], t) for a in (0, 1) for b in (0, 1)}          # along W first,
        q = {a: _lerp(r[a, 0], r[a, 1], l[1], t) for a in (0, 1)}                                       # then H,
        return _lerp(q[0], q[1], l[0], t)                                                               # then D


def shares(A, c, out, lo, hi, pad):
    """(share of output voxels with a coordinate on an exact .5 tie, share with a coordinate outside [lo, hi]), from the fp64 coordinates; under `pad` = 0 the
    ties are counted after the clamp (a clamped coordinate is an integer)"""
    s = coords(A, c, out, np.float64)
    outside = np.zeros(tuple(out), dtype=bool)
    tie = np.zeros(tuple(out), dtype=bool)
    for a in range(3):
        outside |= (s[a] < lo[a]) | (s[a] > hi[a])
        sa = np.clip(s[a], lo[a], hi[a]) if pad == 0 else s[a]
        tie |= (sa - np.floor(sa)) == 0.5
    return float(tie.mean()), float(outside.mean())


# ====================================================================================================================== exact rows
MATRICES = {
    "rot3": [[.75, -.5, .25], [.5, .75, -.25], [-.25, .5, 1]],
    "zoom": [[1.25, 0, 0], [0, .75, 0], [0, 0, .5]],
    "shear": [[1, .5, 0], [0, 1, .25], [.5, 0, 1]],
    "half": [[.5, .5, 0], [-.5, .5, 0], [0, 0, 1]],
    "identity": [[1, 0, 0], [0, 1, 0], [0, 0, 1]],
    "permute": [[0, 0, 1], [1, 0, 0], [0, -1, 0]],
    "big": [[1.5, -.5, .25], [.5, 1.25, 0], [0, .25, 1.5]],
}
EXTENTS = (((9, 7, 5), (9, 7, 5)), ((8, 6, 4), (8, 6, 4)), ((6, 10, 7), (11, 9, 13)), ((13, 11, 9), (7, 5, 6)), ((16, 16, 16), (16, 16, 16)))      # output -> source
CVAL = 7.0
EXACT_ROWS = [dict(id=f"{name}_{'x'.join(map(str, o))}_from_{'x'.join(map(str, n))}", matrix=name, out=o, n=n) for name in MATRICES for o, n in EXTENTS]
LABEL_DTYPES = {1: np.uint8, 4: np.int32, 8: np.int64, -4: np.float32}


def _seed(text):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(text)) % 100003


def row_matrix(row):
    """the (3, 4) matrix of an exact row: no translation"""
    return np.concatenate([np.array(MATRICES[row["matrix"]], dtype=np.float64), np.zeros((3, 1))], axis=1)


@functools.lru_cache(maxsize=None)
def _image(n, seed):
    x = E.ints(*n, seed=seed, lo=-64, hi=64).numpy()
    x.setflags(write=False)
    return x


def image(row):
    """integer-valued fp32 (D, H, W), |v| <= 64; read-only, computed once"""
    return _image(tuple(row["n"]), _seed(row["id"]))


@functools.lru_cache(maxsize=None)
def _label(n, seed, code):
    """labels of element type `code`: small values, and the extremes of the type planted at seeded places (a narrowing copy would change them)"""
    lo = 0 if code == 1 else -64
    x = E.ints(*n, seed=seed + 7 * abs(code), lo=lo, hi=64).numpy().astype(np.float64 if code == -4 else np.int64)
    wild = {1: [255, 200], 4: [2 ** 31 - 1, -2 ** 31], 8: [2 ** 40 + 3, -(2 ** 40) - 5, 2 ** 63 - 1], -4: [0.5, -1024.0]}[code]
    rs = np.random.RandomState(seed)
    flat = x.reshape(-1)
    at = rs.choice(flat.size, size=min(flat.size, 4 * len(wild)), replace=False)
    flat[at] = np.resize(np.array(wild, dtype=flat.dtype), at.size)
    x = x.astype(LABEL_DTYPES[code])
    x.setflags(write=False)
    return x


def label(row, code):
    return _label(tuple(row["n"]), _seed(row["id"]), code)


@functools.lru_cache(maxsize=None)
def _reference(rid, mode, pad, code):
    row = next(r for r in EXACT_ROWS if r["id"] == rid)
    A, c = record_values(row_matrix(row), row["n"])
    x = image(row) if code == 0 else label(row, code)
    out = sample(x, A, c, row["out"], mode, pad, CVAL)
    out.setflags(write=False)
    return out


def reference(row, mode, pad, code=0):
    """the fp64 oracle of an exact row (code 0: the image) or the nearest oracle of its labels of type `code`; computed once, shared, never modified"""
    return _reference(row["id"], mode, pad, code)


# ====================================================================================================================== off the dyadic rows
OFF_SEED, OFF_N = 11, (24, 24, 24)


def off_dyadic_case(seed=OFF_SEED):
    """three random angles about x, y and z at once, scale 0.8 .. 1.2 per axis, 24^3 -> 24^3; data = a linear ramp plus small integers
    -> (x fp32, (3, 4) fp64 matrix)"""
    rs = np.random.RandomState(seed)
    ang = rs.uniform(-math.pi, math.pi, size=3)
    sc = rs.uniform(0.8, 1.2, size=3)
    d, h, w = np.meshgrid(*(np.arange(v, dtype=np.float64) for v in OFF_N), indexing="ij")
    x = (0.37 * d - 0.21 * h + 0.13 * w + rs.randint(-2, 3, size=OFF_N)).astype(np.float32)
    return x, matrix(ang, sc, (0.0, 0.0, 0.0))


def coord_bound(A, c, out):
    """bound on |fp32 coordinate - exact coordinate| for the record values (A, c), largest over the output voxels: every term A[a][i] p_i passes through at most four
    roundings (its product and three additions), c_a through one, and p_i is exact (a half-integer below 2^23): <= gamma(4) (sum_i |A[a][i]| |p_i| + |c_a|)"""
    A, c = np.abs(np.asarray(A, dtype=np.float64)), np.abs(np.asarray(c, dtype=np.float64))
    pmax = np.array([0.5 * (v - 1) for v in out])
    return float(gamma(4) * ((A @ pmax) + c).max())


def neighbour_difference(x, cval=None):
    """largest |difference| of adjacent voxels along any axis: the steepest slope of the trilinear interpolant.  With `cval` (constant padding) the volume is taken
    with its one-voxel frame of cval, where the interpolant runs from the outermost voxels to cval"""
    x = np.asarray(x, dtype=np.float64)
    if cval is not None:
        x = np.pad(x, 1, constant_values=float(cval))
    return float(max(np.abs(np.diff(x, axis=a)).max() for a in range(3) if x.shape[a] > 1))


def near_tie(A, c, out, lo, hi, pad, eps):
    """output voxels whose fp64 coordinate lies within eps of a .5 tie on some axis (after the clamp of the rule: a clamped coordinate is an integer and rounds the same
    way in either precision)"""
    s = coords(A, c, out, np.float64)
    m = 0 if pad == 0 else 1
    bad = np.zeros(tuple(out), dtype=bool)
    for a in range(3):
        sa = np.clip(s[a], lo[a] - m, hi[a] + m)
        bad |= np.abs((sa - np.floor(sa)) - 0.5) <= eps
    return bad


# ====================================================================================================================== RandAffined: matrix and draw order
def matrix(rotate, scale, translate):
    """MONAI 1.x AffineGrid without shear, restated with 4 x 4 homogeneous matrices: R @ T @ S, R = Rx @ Ry @ Rz, over (D, H, W) = (x, y, z) -> the top (3, 4)"""
    def rot(i, j, a):
        m = np.eye(4)
        m[i, i], m[i, j], m[j, i], m[j, j] = math.cos(a), -math.sin(a), math.sin(a), math.cos(a)
        return m
    Rx, Ry, Rz = rot(1, 2, rotate[0]), rot(2, 0, rotate[1]), rot(0, 1, rotate[2])       # Ry: [[c, 0, s], [0, 1, 0], [-s, 0, c]]
    T = np.eye(4)
    T[:3, 3] = translate
    S = np.diag([scale[0], scale[1], scale[2], 1.0])
    return (Rx @ Ry @ Rz @ T @ S)[:3]


def ranges(v):
    """a range argument as three (low, high) pairs: None -> zeros; a bare number is the first axis only; a number r means (-|r|, |r|), a pair (min, max)"""
    if v is None:
        return [(0.0, 0.0)] * 3
    seq = [v] if np.isscalar(v) else list(v)
    out = [(-abs(float(e)), abs(float(e))) if np.isscalar(e) else (float(min(e)), float(max(e))) for e in seq]
    return out + [(0.0, 0.0)] * (3 - len(out))


def draws(seed, prob, rotate_range, scale_range, translate_range, count):
    """what `count` successive samples draw from RandomState(seed): R.rand() < prob first; only if that fires three rotation uniforms, then three translation
    uniforms, then three scale uniforms (each drawn even where its range is zero; the scale is 1 + its draw) -> [None | (rotate, translate, scale)]"""
    R = np.random.RandomState(seed)
    out = []
    for _ in range(count):
        if not R.rand() < prob:
            out.append(None)
            continue
        rot = [float(R.uniform(lo, hi)) for lo, hi in ranges(rotate_range)]
        tra = [float(R.uniform(lo, hi)) for lo, hi in ranges(translate_range)]
        sca = [1.0 + float(R.uniform(lo, hi)) for lo, hi in ranges(scale_range)]
        out.append((rot, tra, sca))
    return out
