"""Numpy / scipy oracle of the ball element, of the dilation and erosion by it and of the normalised surface Dice (csrc/morphology.hip: vx_morph_ball,
utils/morphology.py, utils/metric/surface.py).  Nothing here is shared with the code under test: the element is found by brute force from
the definition, the morphology is scipy.ndimage's with that boolean structure, the metric is scipy's binary_erosion and distance_transform_edt with nnU-Net's
formula.

    f(o) = fl(fl(t_z(dz) + t_y(dy)) + t_x(dx)),  t_a(d) = fl(fl(d * s_a) * fl(d * s_a))            B(tau, s) = {o : f(o) <= q(tau)}
    q(tau) = the largest double whose correctly rounded square root is <= tau"""
import functools
import math

import numpy as np

import distance_ref as DR

ANISO = DR.SPACINGS[2]                                      # (2.0364, 0.9766, 3.27)


def sq_threshold(tau):
    tau = np.float64(tau)
    with np.errstate(over="ignore", under="ignore"):
        q = tau * tau
        while np.sqrt(q) > tau:
            q = np.nextafter(q, -np.inf)
        while np.sqrt(np.nextafter(q, np.inf)) <= tau:
            q = np.nextafter(q, np.inf)
    return float(q)


def f(dz, dy, dx, spacing):
    return (DR.term(dz, spacing[0]) + DR.term(dy, spacing[1])) + DR.term(dx, spacing[2])


def radii(tau, spacing):
    """per axis the largest d with t(d) <= q, walking up from 0"""
    q, out = sq_threshold(tau), []
    for s in spacing:
        d = 0
        while float(DR.term(d + 1, s)) <= q:
            d += 1
        out.append(d)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def element(tau, spacing=(1.0, 1.0, 1.0)):
    """-> (boolean structure of shape (2 r_z + 3, 2 r_y + 3, 2 r_x + 3), centred: a box one voxel beyond each radius, every offset tested on its own)"""
    q = sq_threshold(tau)
    rz, ry, rx = (r + 1 for r in radii(tau, spacing))
    dz, dy, dx = np.meshgrid(np.arange(-rz, rz + 1), np.arange(-ry, ry + 1), np.arange(-rx, rx + 1), indexing="ij")
    s = f(dz, dy, dx, spacing) <= q
    s.setflags(write=False)
    return s


def half_widths(structure):
    """(rows, row half-widths) of a centred boolean structure, trimmed to the box of its radii: -1 for an absent row; asserts every row a symmetric interval"""
    s = np.asarray(structure)
    cz, cy, cx = (n // 2 for n in s.shape)
    hw = np.full(s.shape[:2], -1, dtype=np.int64)
    for z in range(s.shape[0]):
        for y in range(s.shape[1]):
            xs = np.nonzero(s[z, y])[0] - cx
            if xs.size:
                assert xs[0] == -xs[-1] and xs.size == 2 * xs[-1] + 1, "a row that is no symmetric interval"
                hw[z, y] = xs[-1]
    keep_z, keep_y = np.nonzero((hw >= 0).any(1))[0], np.nonzero((hw >= 0).any(0))[0]
    rz, ry = max(cz - keep_z[0], keep_z[-1] - cz), max(cy - keep_y[0], keep_y[-1] - cy)
    return hw[cz - rz:cz + rz + 1, cy - ry:cy + ry + 1]


def pack_rows(hw):
    """the record list, in no particular order: dz in bits 0 - 7, dy in bits 8 - 15 (two's complement bytes), hw in bits 16 - 21"""
    hw = np.asarray(hw)
    rz, ry = hw.shape[0] // 2, hw.shape[1] // 2
    return np.array([((z - rz) & 0xff) | (((y - ry) & 0xff) << 8) | (int(hw[z, y]) << 16) for z in range(hw.shape[0]) for y in range(hw.shape[1]) if hw[z, y] >= 0],
                    dtype=np.int32)


def unpack_rows(rows):
    """what the kernel reads out of ANY int32s: [(dz, dy, hw)] with dz, dy the signed bytes and hw the 6-bit field"""
    sb = lambda v: v - 256 if v >= 128 else v
    return [(sb(int(r) & 0xff), sb((int(r) >> 8) & 0xff), (int(r) >> 16) & 63) for r in np.asarray(rows).astype(np.int64)]


def apply_rows(mask, rows, op=0, border_value=0):
    """the kernel's contract on a record list, offset by offset (small volumes): op 0 the OR, op 1 the AND, outside the volume reads border_value"""
    m = np.asarray(mask) != 0
    D, H, W = m.shape
    out = np.zeros_like(m) if op == 0 else np.ones_like(m)
    for dz, dy, hw in unpack_rows(rows):
        for dx in range(-hw, hw + 1):
            v = np.full(m.shape, bool(border_value))          # v[p] = m[p + o] where p + o lies in the volume
            dst, src = [], []
            for n, d in zip(m.shape, (dz, dy, dx)):
                dst.append(slice(max(0, -d), min(n, n - d)))
                src.append(slice(max(0, -d) + d, min(n, n - d) + d))
            if all(s.start < s.stop for s in dst):
                v[tuple(dst)] = m[tuple(src)]
            out = (out | v) if op == 0 else (out & v)
    return out.astype(np.uint8)


def _ndi():
    from scipy import ndimage
    return ndimage


def dilate(mask, tau, spacing=(1.0, 1.0, 1.0), border_value=0):
    return _ndi().binary_dilation(np.asarray(mask) != 0, structure=element(float(tau), tuple(spacing)), border_value=border_value).astype(np.uint8)


def erode(mask, tau, spacing=(1.0, 1.0, 1.0), border_value=0):
    return _ndi().binary_erosion(np.asarray(mask) != 0, structure=element(float(tau), tuple(spacing)), border_value=border_value).astype(np.uint8)


def opening(mask, tau, spacing=(1.0, 1.0, 1.0), border_value=0):
    return dilate(erode(mask, tau, spacing, border_value), tau, spacing, border_value)


def closing(mask, tau, spacing=(1.0, 1.0, 1.0), border_value=0):
    return erode(dilate(mask, tau, spacing, border_value), tau, spacing, border_value)


def _scipy_surface_distances(result, reference, spacing):
    ndi = _ndi()
    result, reference = np.asarray(result) != 0, np.asarray(reference) != 0
    if not result.any():
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if not reference.any():
        raise RuntimeError("The second supplied array does not contain any binary object.")
    fp = ndi.generate_binary_structure(3, 1)
    rb, fb = result ^ ndi.binary_erosion(result, structure=fp, iterations=1), reference ^ ndi.binary_erosion(reference, structure=fp, iterations=1)
    return ndi.distance_transform_edt(~fb, sampling=spacing)[rb]


def surface_overlap(a, b, tau, spacing=(1.0, 1.0, 1.0)):
    """(tp_a, n_a, tp_b, n_b) from scipy's distances, compared with tau itself"""
    ab, ba = _scipy_surface_distances(a, b, spacing), _scipy_surface_distances(b, a, spacing)
    return int(np.sum(ab <= tau)), len(ab), int(np.sum(ba <= tau)), len(ba)


def nsd_from_counts(tp_a, n_a, tp_b, n_b):
    ta, tb, fp, fn = tp_a / n_a, tp_b / n_b, (n_a - tp_a) / n_a, (n_b - tp_b) / n_b
    return float((ta + tb) / (ta + tb + fp + fn + 1e-8))


def normalized_surface_dice(a, b, tau, spacing=(1.0, 1.0, 1.0)):
    return nsd_from_counts(*surface_overlap(a, b, tau, spacing))


def surface_dice_or_nan(gt, pred, tau, spacing=(1.0, 1.0, 1.0)):
    if np.asarray(gt).max() == 0 or np.asarray(pred).max() == 0:
        return float("nan")
    return normalized_surface_dice(pred, gt, tau, spacing)


# ---------------------------------------------------------------------------------------------------------------------- inputs shared by the two test files
ABI_SHAPES = ((7, 9, 11), (5, 6, 63), (3, 4, 64), (3, 4, 65), (4, 5, 130), (9, 5, 1))
# (tau, spacing): one row with hw = 0; unit-grid balls of radius 1, sqrt(3), 2; the anisotropic grid; radii (9, 9, 63), which reach from any voxel to every other
# one of LARGE_SHAPES (the kernel holds a radius to 63 voxels, so no element is larger than W = 65 or 130; scipy's time grows with the element, so the large one
# meets the three shapes it is larger than and no others)
ELEMENTS = ((0.0, (1.0, 1.0, 1.0)), (1.0, (1.0, 1.0, 1.0)), (math.sqrt(3.0), (1.0, 1.0, 1.0)), (2.0, (1.0, 1.0, 1.0)), (4.0, ANISO), (63.0, (7.0, 7.0, 1.0)))
LARGE_SHAPES = ((7, 9, 11), (3, 4, 64), (9, 5, 1))
# r_x = 63 with r_z = r_y = 1: 63 steps of 1 mm, and one step of 40 mm along z or y (1600 <= 63.5^2 = 4032.25 < 2 * 1600 and < 64^2)
WIDE = (63.5, (40.0, 40.0, 1.0))
WIDE_SHAPES = ((3, 4, 130), (2, 3, 200))
METRIC_TAUS = (0.0, 1.0, 2.5)


def mask_for(shape, seed, p=0.12):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def ball_surface(shape=(24, 40, 70)):
    """the 6-connected surfaces of two balls"""
    import morphology_ref as MR
    m = DR.ball(shape, (9, 14, 20), 7) | DR.ball(shape, (14, 25, 50), 9)
    return MR.inner_boundary(m, 6)
