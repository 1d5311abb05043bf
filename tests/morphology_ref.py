"""Pure-numpy restatement of the mask-morphology kernels (csrc/morphology.hip) and of what is built on them: the oracle of
tests/test_morphology_gpu.py.  tests/test_morphology_cpu.py holds it to scipy.ndimage on every input the GPU file uses; the GPU tests need no scipy.

dilate(): the OR over the structuring element's offsets of the mask, shifted, inside a frame of `border_value`.  erode(): the complement of the dilation of the
complement with the border value flipped.  fill_holes(): loops over the ids of the background's components (components_ref.label).  This module also owns the
inputs (seeded, CPU-only at import) so that both test files see the same arrays."""
import functools
import itertools

import numpy as np

import components_ref as CR

CONNECTIVITIES = CR.CONNECTIVITIES
MAX_NONZERO = CR.MAX_NONZERO
# The step kernel has no tile: a thread owns one 64-voxel word, a wave 64 consecutive words and a block 256 of the flat word array (the fused form with a 4 x 8-row x
# 8-word LDS tile was measured slower and is not kept).  Its seams are the word boundaries along x and, in the flat array, the wave and
# block boundaries: TILE = (rows, rows, words) keeps the seam shapes at TILE + 1 rows, and the largest volume below spans several blocks.
TILE = (4, 8, 8)


def offsets(connectivity):
    """the structuring element: (dz, dy, dx) in {-1, 0, 1}^3 with at most MAX_NONZERO[connectivity] non-zero coordinates, the centre included: 7 / 19 / 27"""
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if sum(c != 0 for c in o) <= MAX_NONZERO[connectivity]]


def dilate(mask, connectivity, iterations=1, border_value=0):
    m = np.asarray(mask) != 0
    D, H, W = m.shape
    for _ in range(iterations):
        framed = np.full((D + 2, H + 2, W + 2), bool(border_value))
        framed[1:-1, 1:-1, 1:-1] = m
        out = np.zeros_like(m)
        for dz, dy, dx in offsets(connectivity):
            out |= framed[1 + dz:1 + dz + D, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        if np.array_equal(out, m):          # stationary: further iterations change nothing
            break
        m = out
    return m.astype(np.uint8)


def erode(mask, connectivity, iterations=1, border_value=0):
    return 1 - dilate(np.asarray(mask) == 0, connectivity, iterations, 1 - int(bool(border_value)))


def opening(mask, connectivity, iterations=1):
    return dilate(erode(mask, connectivity, iterations), connectivity, iterations)


def closing(mask, connectivity, iterations=1):
    return erode(dilate(mask, connectivity, iterations), connectivity, iterations)


def inner_boundary(mask, connectivity):
    m = (np.asarray(mask) != 0).astype(np.uint8)
    return m & (1 - erode(m, connectivity))


def fill_holes(lab, connectivity=6, applied_labels=None):
    """the general rule: a background component is filled with class c when no voxel of it has a neighbour outside the volume, every non-zero neighbour of its voxels
    holds c, and applied_labels is empty or contains c"""
    lab = np.asarray(lab)
    D, H, W = lab.shape
    cc, n = CR.label((lab == 0).astype(np.uint8), connectivity)
    framed = np.zeros((D + 2, H + 2, W + 2), dtype=np.int64)
    framed[1:-1, 1:-1, 1:-1] = lab.astype(np.int64)
    inside = np.zeros(framed.shape, dtype=bool)
    inside[1:-1, 1:-1, 1:-1] = True
    out = lab.copy()
    for i in range(1, n + 1):
        zs, ys, xs = np.nonzero(cc == i)
        enclosed, seen = True, set()
        for dz, dy, dx in offsets(connectivity):
            nz, ny, nx = zs + 1 + dz, ys + 1 + dy, xs + 1 + dx
            enclosed = enclosed and bool(inside[nz, ny, nx].all())
            vals = framed[nz, ny, nx][inside[nz, ny, nx]]
            seen.update(int(v) for v in np.unique(vals[vals != 0]))
        if enclosed and len(seen) == 1:
            c = seen.pop()
            if not applied_labels or c in applied_labels:
                out[cc == i] = c
    return out


def _per_class(lab, labels_list, fn, paint):
    lab = np.asarray(lab)
    if labels_list is None:
        res = fn((lab != 0).astype(np.uint8)) != 0
        return np.where(res & (lab == 0), 1, lab).astype(lab.dtype) if paint else np.where(res, lab, 0).astype(lab.dtype)
    cur = lab.copy()
    for c in labels_list:
        res = fn((cur == c).astype(np.uint8)) != 0
        if paint:
            cur[res & (cur == 0)] = c
        else:
            cur[(cur == c) & ~res] = 0
    return cur


def dilate_labels(lab, connectivity=6, iterations=1, labels_list=None):
    return _per_class(lab, labels_list, lambda m: dilate(m, connectivity, iterations), True)


def erode_labels(lab, connectivity=6, iterations=1, labels_list=None):
    return _per_class(lab, labels_list, lambda m: erode(m, connectivity, iterations), False)


def open_labels(lab, connectivity=6, iterations=1, labels_list=None):
    return _per_class(lab, labels_list, lambda m: opening(m, connectivity, iterations), False)


def close_labels(lab, connectivity=6, iterations=1, labels_list=None):
    return _per_class(lab, labels_list, lambda m: closing(m, connectivity, iterations), True)


def postprocess(lab, closing=None, fill=False, opening=None, morph_connectivity=6, labels=None, min_voxels=None, keep_largest=None, connectivity=26, binary=False):
    """the documented order: closing -> fill_holes -> opening -> min_voxels -> keep_largest"""
    out = np.asarray(lab)
    if closing:
        out = close_labels(out, morph_connectivity, closing, labels)
    if fill:
        out = fill_holes(out, morph_connectivity, labels)
    if opening:
        out = open_labels(out, morph_connectivity, opening, labels)
    if min_voxels is not None:
        out = CR.remove_small(out, min_voxels, connectivity, binary)
    if keep_largest is not None:
        out = CR.keep_largest(out, keep_largest, connectivity, binary)
    return out


# ---------------------------------------------------------------------------------------------------------------------- bit packing
def words(shape):
    return shape[0] * shape[1] * ((shape[2] + 63) // 64)


def pack(mask):
    """-> int64 array of words(shape) entries in the kernels' layout (bit i of word q of row (z, y) is voxel x = 64 q + i; tail bits zero)"""
    m = np.asarray(mask) != 0
    D, H, W = m.shape
    Wq = (W + 63) // 64
    padded = np.zeros((D, H, Wq * 64), dtype=np.uint64)
    padded[:, :, :W] = m
    w = (padded.reshape(D, H, Wq, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)          # disjoint bits: the sum is the OR
    return w.reshape(-1).view(np.int64)


def tail_ones(shape):
    """the words of an all-clear mask whose tail bits (x >= W of each row's last word) are all set"""
    D, H, W = shape
    Wq = (W + 63) // 64
    w = np.zeros((D, H, Wq), dtype=np.uint64)
    if W % 64:
        w[:, :, -1] = np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(W % 64)
    return w.reshape(-1).view(np.int64)


# ---------------------------------------------------------------------------------------------------------------------- inputs
SEAM_W = (1, 63, 64, 65, 130)
SEAM_D = (1, 2, TILE[0] + 1)
SEAM_H = (1, 2, TILE[1] + 1)


def seam_shapes():
    """every (D, H, W) of the word- and tile-seam tests"""
    return [(d, h, w) for d in SEAM_D for h in SEAM_H for w in SEAM_W]


def single_voxels(shape):
    """the positions of the single-voxel cases: the 8 corners and x = 63, x = 64 (where the volume has them) in the middle row"""
    D, H, W = shape
    pos = set(itertools.product((0, D - 1), (0, H - 1), (0, W - 1)))
    pos.update((D // 2, H // 2, x) for x in (63, 64) if x < W)
    return sorted(pos)


def clipped_element(shape, pos, connectivity):
    """the structuring element centred on pos, clipped to the volume: what the dilation of that single voxel must be"""
    out = np.zeros(shape, dtype=np.uint8)
    for o in offsets(connectivity):
        p = tuple(c + d for c, d in zip(pos, o))
        if all(0 <= c < n for c, n in zip(p, shape)):
            out[p] = 1
    return out


def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def shell(shape, lo, hi, value=1, dtype=np.uint8):
    """a closed box shell one voxel thick: the faces of the box [lo, hi] (inclusive corners)"""
    vol = np.zeros(shape, dtype=dtype)
    sl = tuple(slice(a, b + 1) for a, b in zip(lo, hi))
    vol[sl] = value
    vol[tuple(slice(a + 1, b) for a, b in zip(lo, hi))] = 0
    return vol


def hole_cases():
    """name -> label volume of the constructed hole-filling cases"""
    v = {}
    v["closed_shell"] = shell((7, 8, 9), (1, 1, 1), (5, 6, 7))
    pin = shell((7, 8, 9), (1, 1, 1), (5, 6, 7))
    pin[1, 1, 1] = 0                                         # a corner of the shell: the cavity's corner (2, 2, 2) meets the outside across it only diagonally
    v["diagonal_pinhole"] = pin
    v["cavity_at_face"] = shell((7, 8, 9), (0, 1, 1), (5, 6, 7))
    v["cavity_at_face"][0, 2:6, 2:7] = 0                     # the shell's face at z = 0 is open: the cavity touches the volume's face
    for x in (63, 64):
        one = np.zeros((3, 3, 70), dtype=np.uint8)
        one[:, :, x - 1:x + 2] = 1
        one[1, 1, x] = 0
        v[f"one_voxel_x{x}"] = one
    v["across_cc_tiles"] = shell((12, 12, 40), (2, 2, 20), (10, 10, 36))          # the cavity spans z = 8, y = 8 and x = 32: the seams of vx_cc_label's 8 x 8 x 32 tile
    two = shell((7, 8, 9), (1, 1, 1), (5, 6, 7))
    two[1:6, 1:7, 5:8][two[1:6, 1:7, 5:8] != 0] = 2          # the shell's high-x part is class 2: the cavity is bordered by two classes
    v["two_classes"] = two
    isl = shell((9, 9, 11), (1, 1, 1), (7, 7, 9))
    isl[4, 4, 5] = 2                                         # a class-2 island inside the class-1 cavity: the cavity sees two classes
    v["island"] = isl
    mixed = np.zeros((7, 8, 20), dtype=np.int32)
    mixed[:, :, :9] = shell((7, 8, 9), (1, 1, 1), (5, 6, 7), 3, np.int32)
    mixed[:, :, 10:19] = shell((7, 8, 9), (1, 1, 1), (5, 6, 7), 5, np.int32)
    v["applied_labels"] = mixed                              # one cavity in class 3, one in class 5
    v["bern_12x12x70_p80"] = bernoulli((12, 12, 70), 0.8, 21)
    for a in v.values():
        a.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def volumes():
    """name -> read-only mask / label volume: every input of the GPU tests that goes through dilate(), erode() or fill_holes()"""
    v = {f"bern_{d}x{h}x{w}_p{int(p * 100)}": bernoulli((d, h, w), p, seed) for seed, (d, h, w, p) in
         enumerate([(5, 9, 70, 0.3), (5, 9, 130, 0.6), (TILE[0] + 1, TILE[1] + 1, 65, 0.9), (1, 9, 64, 0.3), (9, 1, 65, 0.6), (3, 130, 3, 0.3), (6, 6, 6, 0.9),
                    (2 * TILE[0] + 1, 2 * TILE[1] + 3, 64 * TILE[2] + 70, 0.3)], start=30)}
    v["multiclass_10x12x70"] = np.random.default_rng(40).integers(0, 4, (10, 12, 70)).astype(np.uint8) * (bernoulli((10, 12, 70), 0.5, 41))
    v.update(hole_cases())
    for a in v.values():
        a.setflags(write=False)
    return v


STEP_VOLUMES = tuple(k for k in volumes() if k.startswith("bern_") and k != "bern_12x12x70_p80")
