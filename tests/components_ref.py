"""Pure-numpy restatement of the connected-component kernels (csrc/components.hip) and of what is built on them: the oracle of
tests/test_components_gpu.py.  tests/test_components_cpu.py holds it to scipy.ndimage.label on every input the GPU file uses; the GPU tests need no scipy.

label():  the edge list of equal-valued non-zero neighbour pairs, then rounds of scatter-min over the edges + pointer jumping until nothing changes: every voxel
ends at the smallest flat index of its component; the components are numbered by that index.  The lesion metrics and the two filters are written out as loops over
component ids.  This module also owns the inputs (seeded, CPU-only at import) so that both test files see the same arrays."""
import functools
import itertools

import numpy as np

MAX_NONZERO = {6: 1, 18: 2, 26: 3}
CONNECTIVITIES = (6, 18, 26)
TILE = (8, 8, 32)          # the LDS tile of vx_cc_label (z, y, x): the inputs below are placed against its seams


def forward_offsets(connectivity):
    """the (dz, dy, dx) in {-1, 0, 1}^3 that come lexicographically after (0, 0, 0) with at most MAX_NONZERO[connectivity] non-zero coordinates: 3 / 9 / 13"""
    return [o for o in itertools.product((-1, 0, 1), repeat=3) if o > (0, 0, 0) and sum(c != 0 for c in o) <= MAX_NONZERO[connectivity]]


def _edges(vol, connectivity):
    D, H, W = vol.shape
    idx = np.arange(vol.size, dtype=np.int64).reshape(vol.shape)
    a, b = [], []
    for off in forward_offsets(connectivity):
        src = tuple(slice(max(0, -o), n - max(0, o)) for o, n in zip(off, (D, H, W)))
        dst = tuple(slice(max(0, o), n - max(0, -o)) for o, n in zip(off, (D, H, W)))
        same = (vol[src] == vol[dst]) & (vol[src] != 0)
        a.append(idx[src][same])
        b.append(idx[dst][same])
    return np.concatenate(a), np.concatenate(b)


def label(vol, connectivity):
    """-> (cc int32 of vol's shape: 0 on background, else 1..N by ascending smallest flat index; N)"""
    vol = np.asarray(vol)
    assert vol.ndim == 3 and connectivity in MAX_NONZERO
    a, b = _edges(vol, connectivity)
    parent = np.arange(vol.size, dtype=np.int64)
    while True:
        new = parent.copy()
        m = np.minimum(parent[a], parent[b])
        for target in (a, b, parent[a], parent[b]):
            np.minimum.at(new, target, m)
        while True:                                   # pointer jumping to a fixpoint
            nxt = new[new]
            if np.array_equal(nxt, new):
                break
            new = nxt
        if np.array_equal(new, parent):
            break
        parent = new
    fg = vol.reshape(-1) != 0
    roots = np.nonzero(fg & (parent == np.arange(vol.size)))[0]          # ascending flat index
    rank = np.zeros(vol.size, dtype=np.int64)
    rank[roots] = np.arange(1, roots.size + 1)
    cc = np.where(fg, rank[parent], 0).astype(np.int32).reshape(vol.shape)
    return cc, int(roots.size)


def tally(cc, n, other=None):
    """sizes[id], hits[id] for id in 0..n (0 = background), by a loop over the ids"""
    sizes, hits = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
    for i in range(n + 1):
        sel = cc == i
        sizes[i] = int(sel.sum())
        if other is not None:
            hits[i] = int((sel & (np.asarray(other) != 0)).sum())
    return (sizes, hits) if other is not None else sizes


def remove_small(vol, min_voxels, connectivity, binary=False):
    vol = np.asarray(vol)
    cc, n = label((vol != 0).astype(np.uint8) if binary else vol, connectivity)
    out = vol.copy()
    for i in range(1, n + 1):
        sel = cc == i
        if int(sel.sum()) < min_voxels:
            out[sel] = 0
    return out


def keep_largest(vol, k, connectivity, binary=False):
    vol = np.asarray(vol)
    cc, n = label((vol != 0).astype(np.uint8) if binary else vol, connectivity)
    sizes = [int((cc == i).sum()) for i in range(1, n + 1)]
    kept = []
    for _ in range(min(k, n)):                        # k times: the largest of what is left, the lowest id among equals
        best = None
        for i in range(1, n + 1):
            if i not in kept and (best is None or sizes[i - 1] > sizes[best - 1]):
                best = i
        kept.append(best)
    out = vol.copy()
    for i in range(1, n + 1):
        if i not in kept:
            out[cc == i] = 0
    return out


def lesion_metrics(gt, pred, voxel_volume=1.0, connectivity=18):
    g, p = np.asarray(gt) != 0, np.asarray(pred) != 0
    cg, ng = label(g.astype(np.uint8), connectivity)
    cp, npred = label(p.astype(np.uint8), connectivity)
    fp = fn = det = mat = 0
    for i in range(1, npred + 1):
        sel = cp == i
        if (sel & g).any():
            mat += 1
        else:
            fp += int(sel.sum())
    for i in range(1, ng + 1):
        sel = cg == i
        if (sel & p).any():
            det += 1
        else:
            fn += int(sel.sum())
    tot = int(g.sum()) + int(p.sum())
    return {"false_pos_vol": float(fp) * float(voxel_volume), "false_neg_vol": float(fn) * float(voxel_volume), "n_gt": ng, "n_pred": npred, "n_gt_detected": det,
            "n_pred_matched": mat, "dice": 1.0 if tot == 0 else 2.0 * int((g & p).sum()) / tot}


# ---------------------------------------------------------------------------------------------------------------------- inputs
def bernoulli(shape, p, seed):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def serpentine(shape=(17, 18, 19)):
    """one voxel-wide path through the whole volume: even z planes hold a snake (rows at even y, joined at alternating ends), joined to the next plane at alternating
    ends of the snake: one 6-connected chain"""
    D, H, W = shape
    vol = np.zeros(shape, dtype=np.uint8)
    plane = snake_plane(H, W)
    rows = (H + 1) // 2
    last = (2 * (rows - 1), W - 1 if (rows - 1) % 2 == 0 else 0)          # where the snake that starts at (0, 0) ends
    for z in range(0, D, 2):
        vol[z] = plane
        if z + 2 < D:
            y, x = last if (z // 2) % 2 == 0 else (0, 0)
            vol[z + 1, y, x] = 1
    return vol


def snake_plane(H, W):
    plane = np.zeros((H, W), dtype=np.uint8)
    for y in range(0, H, 2):
        plane[y] = 1
        if y + 2 < H:
            plane[y + 1, W - 1 if (y // 2) % 2 == 0 else 0] = 1
    return plane


def twin_paths(shape=(17, 18, 19)):
    """two snakes, values 1 and 2, face-adjacent along their whole length: planes z = 7 and z = 8 (the two sides of a tile seam)"""
    vol = np.zeros(shape, dtype=np.uint8)
    vol[7] = snake_plane(shape[1], shape[2])
    vol[8] = 2 * snake_plane(shape[1], shape[2])
    return vol


def pair_cases():
    """(id, shape, voxel a, voxel b, non-zero coordinates of b - a): two voxels adjacent by face / edge / corner for each of the 13 forward offsets, once with the pair
    astride a tile seam on every axis on which it extends, once with b at the volume's last index"""
    shape = (10, 10, 34)
    out = []
    for off in forward_offsets(26):
        nz = sum(c != 0 for c in off)
        a = tuple(t - 1 if o == 1 else t for o, t in zip(off, TILE))          # o = +1: a on the low side of the seam; o = -1: a on its high side; 0: anywhere
        out.append((f"seam{off}", shape, a, tuple(c + o for c, o in zip(a, off)), nz))
        b = tuple(n - 1 for n in shape)
        if all(0 <= c - o < n for c, o, n in zip(b, off, shape)):
            out.append((f"last{off}", shape, tuple(c - o for c, o in zip(b, off)), b, nz))
    return out


@functools.lru_cache(maxsize=None)
def volumes():
    """name -> read-only label volume: every input of the GPU tests that goes through label()"""
    v = {"bern_19x21x37_p12": bernoulli((19, 21, 37), 0.12, 1), "bern_19x21x37_p30": bernoulli((19, 21, 37), 0.30, 2), "bern_33x17x70_p20": bernoulli((33, 17, 70), 0.20, 3),
         "checker_8x9x10": (np.indices((8, 9, 10)).sum(0) % 2).astype(np.uint8), "serpentine": serpentine(), "twin_paths": twin_paths(),
         "multiclass_48x50x52": np.random.default_rng(4).integers(0, 4, (48, 50, 52)).astype(np.uint8),
         "multiclass_10x12x40": np.random.default_rng(10).integers(0, 4, (10, 12, 40)).astype(np.uint8),
         "empty_5x6x7": np.zeros((5, 6, 7), dtype=np.uint8), "full_9x10x40": np.ones((9, 10, 40), dtype=np.uint8),
         "one_voxel_set": np.ones((1, 1, 1), dtype=np.uint8), "one_voxel_clear": np.zeros((1, 1, 1), dtype=np.uint8),
         "line_x_70": bernoulli((1, 1, 70), 0.6, 5), "line_y_40": bernoulli((1, 40, 1), 0.6, 6),
         "pattern_4x12x28": bernoulli((4, 12, 28), 0.25, 7),
         "blobs_gt": blobs(8), "blobs_pred": blobs(9), "ties_9x10x40": tie_volume()}
    v.update(lesion_volumes())
    for a in v.values():
        a.setflags(write=False)
    return v


def blobs(seed, shape=(20, 22, 40), n=9):
    """a few boxes of random extent: components of different sizes (filters, tallies, lesion metrics)"""
    rng = np.random.default_rng(seed)
    vol = np.zeros(shape, dtype=np.uint8)
    for _ in range(n):
        lo = [int(rng.integers(0, s - 1)) for s in shape]
        ext = [int(rng.integers(1, 6)) for _ in shape]
        vol[tuple(slice(l, l + e) for l, e in zip(lo, ext))] = 1
    return vol


def tie_volume():
    """four components, two of them equally large (filters: the lower id wins), two astride a tile seam"""
    vol = np.zeros((9, 10, 40), dtype=np.int32)
    vol[0, 0, 0:5] = 3            # id 1: 5 voxels
    vol[4, 4, 30:35] = 1          # id 2: 5 voxels, astride the x seam
    vol[7:9, 9, 10:12] = 2        # id 3: 4 voxels, astride the z seam
    vol[8, 0, 39] = 3             # id 4: 1 voxel
    return vol


def lesion_volumes():
    """inputs of the lesion-metric cases: a ground truth of two lesions (values 1 and 2: the metric binarises), a prediction that shares exactly ONE voxel with the
    first lesion, one that is face-adjacent to it without a shared voxel, and an empty map"""
    z = np.zeros((9, 10, 40), dtype=np.uint8)
    gt, one, touch = z.copy(), z.copy(), z.copy()
    gt[2:5, 2:5, 28:34] = 1                                # 54 voxels, astride the x seam
    gt[8, 9, 36:40] = 2                                    # 4 voxels
    one[4, 4, 33:37] = 1
    touch[2:5, 5, 28:34] = 1                               # 18 voxels
    return {"lesion_gt": gt, "lesion_one_voxel": one, "lesion_touching": touch, "lesion_empty": z}


# the volume above 2^26 voxels: more than 256 scan chunks, so that the one-block scan over the chunk sums carries from one 256-entry pass to the next.  Background
# but for single voxels every SPARSE_STRIDE flat indices (no two of them neighbours: checked by the CPU test against scipy), one at the last index, and one
# two-voxel component astride the boundary of two scan chunks (262144 voxels each)
SPARSE_SHAPE, SPARSE_STRIDE, SPARSE_PAIR = (2, 4096, 8704), 1000003, 260 * 262144


def sparse_big():
    """-> (shape, flat indices of the foreground voxels ascending, their expected ids, N)"""
    V = int(np.prod(SPARSE_SHAPE))
    single = np.concatenate([np.arange(0, V, SPARSE_STRIDE, dtype=np.int64), [V - 1]])
    idx = np.concatenate([single, [SPARSE_PAIR - 1, SPARSE_PAIR]])
    order = np.argsort(idx, kind="stable")
    idx = idx[order]
    assert np.all(np.diff(idx) > 0) and idx[-1] == V - 1
    ids = np.arange(1, idx.size + 1, dtype=np.int64)
    k = int(np.nonzero(idx == SPARSE_PAIR)[0][0])
    ids[k:] -= 1                                           # the pair's second voxel shares the first one's id
    return SPARSE_SHAPE, idx, ids.astype(np.int32), int(ids[-1])


@functools.lru_cache(maxsize=None)
def reference(name, connectivity):
    """(cc, N) of volumes()[name], computed once and shared (read-only)"""
    cc, n = label(volumes()[name], connectivity)
    cc.setflags(write=False)
    return cc, n


# the volume above every grid cap: CELLS copies of the verified pattern, each inside a cell with two background voxels on every side, plus one isolated voxel at flat
# index 0 and one at the last index
BIG_CELL, BIG_OFFSET, BIG_GRID = (9, 16, 36), (2, 2, 2), (58, 4, 7)


def big_volume(connectivity):
    """-> (volume uint8 (522, 64, 252), expected cc int32, N): the expectation follows from the pattern's reference by arithmetic -- the components of cell c are the
    pattern's, moved; all of them are ranked by their smallest flat index"""
    pat = volumes()["pattern_4x12x28"]
    pcc, pn = reference("pattern_4x12x28", connectivity)
    shape = tuple(c * g for c, g in zip(BIG_CELL, BIG_GRID))
    vol = np.zeros(shape, dtype=np.uint8)
    cell_of = np.zeros(shape, dtype=np.int64)          # cell number of every voxel
    local = np.zeros(shape, dtype=np.int64)            # pattern component id of every voxel (0: none)
    first = np.zeros(pn, dtype=np.int64)               # each pattern component's smallest flat index, as an offset in the big volume (flat indices are linear)
    for i in range(1, pn + 1):
        pos = np.unravel_index(int(np.nonzero(pcc.reshape(-1) == i)[0][0]), pat.shape)
        first[i - 1] = int(np.ravel_multi_index(pos, shape))
    starts = []
    for c, (cz, cy, cx) in enumerate(itertools.product(*(range(g) for g in BIG_GRID))):
        o = (cz * BIG_CELL[0] + BIG_OFFSET[0], cy * BIG_CELL[1] + BIG_OFFSET[1], cx * BIG_CELL[2] + BIG_OFFSET[2])
        sl = tuple(slice(a, a + n) for a, n in zip(o, pat.shape))
        vol[sl], cell_of[sl], local[sl] = pat, c, pcc
        starts.extend((first + int(np.ravel_multi_index(o, shape))).tolist())
    ncell = int(np.prod(BIG_GRID))
    vol[0, 0, 0] = vol[-1, -1, -1] = 1
    starts = np.array(starts + [0, vol.size - 1], dtype=np.int64)          # component (cell c, pattern id i) sits at c * pn + i - 1; then the two single voxels
    rank = np.empty(starts.size, dtype=np.int64)
    rank[np.argsort(starts, kind="stable")] = np.arange(1, starts.size + 1)
    cc = np.where(local > 0, rank[np.clip(cell_of * pn + local - 1, 0, starts.size - 1)], 0).astype(np.int32)
    cc[0, 0, 0], cc[-1, -1, -1] = rank[ncell * pn], rank[ncell * pn + 1]
    return vol, cc, int(starts.size)
