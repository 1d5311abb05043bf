"""Pure-numpy restatement of the distance-transform kernels (csrc/distance.hip) and of the surface metrics built on them: the oracle of
tests/test_distance_gpu.py.  tests/test_distance_cpu.py holds it to the brute-force definition, to scipy.ndimage.distance_transform_edt on every input the GPU file
uses, and to medpy's formulas restated with scipy; the GPU tests need no scipy.

    t_a(d) = fl(fl(d * s_a) * fl(d * s_a))            sq[v] = min over the sites s of fl(fl(t_z(dz) + t_y(dy)) + t_x(dx))

numpy rounds every product and sum on its own (it has no fused multiply-add on this path), which is what the definition asks for.  This module also owns the inputs
(seeded, CPU-only) so that both test files see the same arrays."""
import functools

import numpy as np

import morphology_ref as MR

SPACINGS = ((1.0, 1.0, 1.0), (1.5, 0.75, 2.0), (2.0364, 0.9766, 3.27), (0.9765625, 0.9765625, 3.0))
SHAPES = ((1, 1, 1), (1, 1, 70), (5, 1, 3), (9, 33, 65), (17, 40, 130), (40, 36, 70))
PATTERNS = ("corner", "last", "none", "all", "bern2", "bern30", "bern97", "plane", "balls")
INF = np.inf


def term(d, s):
    """t(d) for integer offsets d (an array or a number) and the spacing s: two roundings"""
    a = np.abs(np.asarray(d)).astype(np.float64) * np.float64(s)
    return a * a


def brute_sq(sites, sampling):
    """the definition, site by site: for small volumes"""
    sites = np.asarray(sites) != 0
    D, H, W = sites.shape
    out = np.full(sites.shape, INF)
    z, y, x = np.meshgrid(np.arange(D), np.arange(H), np.arange(W), indexing="ij")
    for sz_, sy_, sx_ in zip(*np.nonzero(sites)):
        out = np.minimum(out, (term(z - sz_, sampling[0]) + term(y - sy_, sampling[1])) + term(x - sx_, sampling[2]))
    return out


def _pass(f, s):
    """g[..., p] = min over q of fl(f[..., q] + t(p - q)) along the last axis, in chunks of at most ~4M candidates"""
    n = f.shape[-1]
    T = term(np.arange(n)[:, None] - np.arange(n)[None, :], s)
    flat = f.reshape(-1, n)
    out = np.empty_like(flat)
    step = max(1, (1 << 22) // (n * n))
    for i in range(0, flat.shape[0], step):
        out[i:i + step] = (flat[i:i + step, None, :] + T[None]).min(-1)
    return out.reshape(f.shape)


def edt_sq(sites, sampling=(1.0, 1.0, 1.0)):
    """the three passes of the kernels: z (integer distance to the nearest site of the column, then t_z), y, x"""
    sites = np.asarray(sites) != 0
    D = sites.shape[0]
    idx = np.arange(D)[:, None, None]
    far = 4 * D + 4
    prev = np.maximum.accumulate(np.where(sites, idx, -far), axis=0)
    nxt = np.minimum.accumulate(np.where(sites, idx, far)[::-1], axis=0)[::-1]
    d = np.minimum(idx - prev, nxt - idx)
    p = np.where(d < far // 2, term(d, sampling[0]), INF)
    p = np.moveaxis(_pass(np.moveaxis(p, 1, 2), sampling[1]), 2, 1)
    return _pass(p, sampling[2])


# ---------------------------------------------------------------------------------------------------------------------- inputs of the transform tests
def ball(shape, centre, radius):
    z, y, x = np.meshgrid(*(np.arange(n) for n in shape), indexing="ij")
    return (z - centre[0]) ** 2 + (y - centre[1]) ** 2 + (x - centre[2]) ** 2 <= radius ** 2


def sites(shape, pattern, seed=0):
    m = np.zeros(shape, dtype=bool)
    if pattern == "corner":
        m[0, 0, 0] = True
    elif pattern == "last":
        m[-1, -1, -1] = True
    elif pattern == "all":
        m[:] = True
    elif pattern.startswith("bern"):
        m = np.random.default_rng(seed).random(shape) < int(pattern[4:]) / 100.0
    elif pattern == "plane":
        m[shape[0] // 2] = True
    elif pattern == "balls":
        r = max(min(shape) // 3, 0)
        m = ball(shape, [n // 4 for n in shape], r) | ball(shape, [(3 * n) // 4 for n in shape], r)
    elif pattern != "none":
        raise ValueError(pattern)
    return m


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (read-only site mask, spacing): every shape with every pattern; the spacing rotates so that every shape and every pattern meets all four"""
    out = {}
    for i, shape in enumerate(SHAPES):
        for j, pattern in enumerate(PATTERNS):
            m = sites(shape, pattern, 100 + 16 * i + j)
            m.setflags(write=False)
            out["x".join(map(str, shape)) + "_" + pattern] = (m, SPACINGS[(i + j) % 4])
    return out


def cap_cases(cap):
    """a line of exactly `cap` voxels along each axis, two lines of it: name -> (site mask, spacing)"""
    out = {}
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = cap
        shape[(axis + 1) % 3] = 2
        m = np.zeros(shape, dtype=bool)
        m[0, 0, 0] = True                                   # the first line: a site at one end only, every other voxel scans the whole way
        far = [0, 0, 0]
        far[(axis + 1) % 3] = 1
        for pos in (cap // 3, cap - 1):                     # the second line: two sites
            far[axis] = pos
            m[tuple(far)] = True
        out[f"cap_axis{axis}"] = (m, SPACINGS[1 + axis])
    return out


@functools.lru_cache(maxsize=None)
def oracle_sq(name):
    m, s = cases()[name]
    out = edt_sq(m, s)
    out.setflags(write=False)
    return out


def lattice_sq(shape, period, sampling):
    """sites where every coordinate is a multiple of its period: the squared distance by arithmetic (per axis the nearest multiple inside the extent)"""
    axes = []
    for n, p, s in zip(shape, period, sampling):
        c = np.arange(n)
        below = c % p
        above = np.where(c - below + p < n, p - below, n + p)          # no multiple above inside the extent: further than any voxel
        axes.append(term(np.minimum(below, above), s))
    return (axes[0][:, None, None] + axes[1][None, :, None]) + axes[2][None, None, :]


def lattice_sites(shape, period):
    z, y, x = (np.arange(n) % p == 0 for n, p in zip(shape, period))
    return z[:, None, None] & y[None, :, None] & x[None, None, :]


def grid_cap_shapes(cap):
    """the smallest volumes at which each kernel's grid-stride loop takes a second trip: name -> (shape, lattice period)
    z: one thread per column, 256 a block; x, count, gather, sqrt: W = 1 makes a row, a word and a tile of 256 rows out of every voxel / 256 voxels; y: one tile per
    z and strip of 32 columns"""
    return {"z": ((2, 256 * cap // 1024 + 1, 1024), (1, 9, 11)), "x": ((256 * cap // 1024 + 1, 1024, 1), (7, 5, 1)), "y": ((cap // 5 + 1, 2, 130), (6, 2, 9))}


# ---------------------------------------------------------------------------------------------------------------------- surface metrics (medpy restated)
def surface(mask):
    return MR.inner_boundary(mask, 6) != 0


def surface_sq(result, reference, spacing=(1.0, 1.0, 1.0)):
    """medpy's __surface_distances, squared: the squared distance map of the reference's surface at the result's surface voxels, in flat-index order"""
    result, reference = np.asarray(result) != 0, np.asarray(reference) != 0
    if not result.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not reference.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return edt_sq(surface(reference), spacing)[surface(result)]


def surface_distances(result, reference, spacing=(1.0, 1.0, 1.0)):
    return np.sqrt(surface_sq(result, reference, spacing))


def hd(a, b, spacing=(1.0, 1.0, 1.0)):
    return float(max(surface_distances(a, b, spacing).max(), surface_distances(b, a, spacing).max()))


def hd95(a, b, spacing=(1.0, 1.0, 1.0)):
    return float(np.percentile(np.hstack((surface_distances(a, b, spacing), surface_distances(b, a, spacing))), 95))


def asd(a, b, spacing=(1.0, 1.0, 1.0)):
    return float(surface_distances(a, b, spacing).mean())


def assd(a, b, spacing=(1.0, 1.0, 1.0)):
    return float(np.mean((asd(a, b, spacing), asd(b, a, spacing))))


def reference_hd95(gt, pred, spacing=(1.0, 1.0, 1.0)):
    """the reference's get_hausdorff / HD95"""
    if gt.max() == 0 or pred.max() == 0:
        return float("nan")
    return hd95(pred, gt, spacing)


def cal_hd95(output, target, spacing=(1.0, 1.0, 1.0)):
    et = reference_hd95(output == 3, target == 3, spacing)
    tc = reference_hd95((output == 1) | (output == 3), (target == 1) | (target == 3), spacing)
    wt = reference_hd95(output != 0, target != 0, spacing)
    return float((et + tc + wt) / 3), et, tc, wt


SURFACE_SPACINGS = (SPACINGS[0], SPACINGS[2])


def box(shape, lo, hi):
    m = np.zeros(shape, dtype=np.uint8)
    m[tuple(slice(a, b + 1) for a, b in zip(lo, hi))] = 1
    return m


@functools.lru_cache(maxsize=None)
def surface_cases():
    """name -> (result, reference) uint8 masks, 24 x 28 x 40 and smaller"""
    s = (24, 28, 40)
    one_a, one_b = np.zeros((5, 6, 7), dtype=np.uint8), np.zeros((5, 6, 7), dtype=np.uint8)
    one_a[1, 2, 3] = one_b[4, 0, 6] = 1
    faces = box(s, (0, 0, 0), (23, 27, 20))                # touches five faces of the volume
    v = {"offset_balls": (ball(s, (10, 12, 15), 7).astype(np.uint8), ball(s, (13, 15, 22), 8).astype(np.uint8)),
         "nested_boxes": (box(s, (3, 4, 5), (20, 22, 33)), box(s, (8, 9, 12), (14, 16, 25))),
         "one_voxel_each": (one_a, one_b),
         "identical": (ball(s, (12, 14, 20), 9).astype(np.uint8), ball(s, (12, 14, 20), 9).astype(np.uint8)),
         "touches_faces": (faces, box(s, (2, 3, 4), (23, 20, 39)))}
    for a, b in v.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return v


def brats_maps():
    """a small BraTS label map pair with classes 0..3 (prediction, target), (10, 12, 14) int64"""
    s = (10, 12, 14)
    tgt, out = np.zeros(s, dtype=np.int64), np.zeros(s, dtype=np.int64)
    tgt[box(s, (1, 1, 1), (8, 9, 11)) != 0] = 2
    tgt[box(s, (2, 3, 3), (6, 7, 8)) != 0] = 1
    tgt[box(s, (3, 4, 4), (5, 6, 6)) != 0] = 3
    out[box(s, (1, 2, 2), (7, 10, 12)) != 0] = 2
    out[box(s, (3, 3, 4), (6, 8, 9)) != 0] = 1
    out[box(s, (4, 4, 5), (5, 6, 8)) != 0] = 3
    return out, tgt
