"""Exact oracles for the inference, metric and input kernels (csrc/infer.hip, csrc/augment.hip).

These kernels index, count and select; where they add or interpolate the data is integer-valued fp32 in [-3, 3] (exact_ref.ints) and the coordinates are
multiples of 1/16, so every result is exactly representable and a kernel must return the oracle VALUE FOR VALUE.  This module is CPU-only at import: plain
numpy / fp64 oracles with the rule written out (no library NaN or rounding behaviour is leaned on), seeded generators, and the case tables as plain data.
tests/test_eval_ref_cpu.py proves the premise of every row; tests/test_eval_kernels_gpu.py runs the kernels on the same rows."""
import functools

import numpy as np

import exact_ref as E

INT_MAX = 0x7FFFFFFF
OVER_CAP_V = (1 << 24) + 301                    # one element per thread no longer: 65536 blocks x 256 threads = 2^24
OVER_CAP_DHW = (73, 311, 739)                   # = OVER_CAP_V
GRID_CAP = {"vx_grid_for": 65536 * 256, "vx_confusion": 1024 * 256, "vx_min_value": 2048 * 256, "vx_bbox_gt": 2048 * 256}


def _seed(text):
    return sum(ord(c) * (i + 1) for i, c in enumerate(text)) % 100003


def ints(*shape, seed, lo=-3, hi=3):
    """exact_ref.ints as a numpy fp32 array"""
    return E.ints(*shape, seed=seed, lo=lo, hi=hi).numpy()


# ====================================================================================================================== arg-max
def argmax_first(x, axis=0):
    """over `axis`: where a column holds a NaN the index of its FIRST NaN, otherwise the index of its FIRST maximum (-0.0 == +0.0)"""
    x = np.moveaxis(np.asarray(x), axis, 0)
    best = x[0].copy()
    arg = np.zeros(best.shape, dtype=np.int64)
    best_nan = best != best
    for c in range(1, x.shape[0]):
        q = x[c]
        q_nan = q != q
        take = ~best_nan & (q_nan | (q > best))          # a NaN already found is never replaced; a NaN replaces any number; a number only a smaller number
        best = np.where(take, q, best)
        arg = np.where(take, c, arg)
        best_nan = best_nan | (take & q_nan)
    return arg


ARGMAX_KINDS = ("tie", "nan", "nans", "inf", "zeros")
ARGMAX_ROWS = [dict(id=f"b{B}_c{C}_v{V}", B=B, C=C, V=V) for B, C in ((1, 1), (3, 2), (1, 4), (3, 256), (3, 4), (1, 2)) for V in (1, 255, 256, 257, 4099)]
ARGMAX_OVER_CAP = dict(id="b1_c2_over_cap", B=1, C=2, V=OVER_CAP_V, cap="vx_grid_for")


def plant_columns(x, seed):
    """x (C, N) integer-valued fp32, changed in place: column j with j % 16 = 0..4 becomes a planted case (C >= 2; with C = 1 only the NaN and inf cases exist);
         0 tie: two channels hold 4, above every other value           1 nan: one NaN, and +inf in another channel (NaN outranks it)
         2 nans: two NaNs                                              3 inf: one +inf, one -inf
         4 zeros: every channel -1 except one -0.0 and one +0.0, in either order (equal by value: the first of the two wins)
    the other columns keep their integers in [-3, 3] (with many natural ties).  Returns kind[N] (-1 = plain)."""
    C, N = x.shape
    rs = np.random.RandomState(seed)
    kind = np.full(N, -1, dtype=np.int64)
    j = np.arange(N)
    k = j % 16
    a = rs.randint(0, C, size=N)
    b = (a + 1 + rs.randint(0, max(C - 1, 1), size=N)) % C if C > 1 else a         # a channel other than a
    for code in range(5):
        sel = j[k == code]
        if sel.size == 0:
            continue
        kind[sel] = code
        if C == 1:
            if code in (1, 2):
                x[0, sel] = np.nan
            elif code == 3:
                x[0, sel] = np.where(sel % 32 < 16, np.inf, -np.inf)
            else:
                kind[sel] = -1
            continue
        if code == 0:
            x[a[sel], sel] = 4.0
            x[b[sel], sel] = 4.0
        elif code == 1:
            x[b[sel], sel] = np.inf
            x[a[sel], sel] = np.nan
        elif code == 2:
            x[a[sel], sel] = np.nan
            x[b[sel], sel] = np.nan
        elif code == 3:
            x[a[sel], sel] = np.inf
            x[b[sel], sel] = -np.inf
        else:
            x[:, sel] = -1.0
            x[a[sel], sel] = -0.0
            x[b[sel], sel] = 0.0
    return kind


@functools.lru_cache(maxsize=None)
def _argmax_case(B, C, V, seed):
    x = ints(B, C, V, seed=seed)
    kind = np.stack([plant_columns(x[b], seed + 1 + b) for b in range(B)])
    if C > 1:                                                                       # the last voxel of the last batch item: NaN in the last two channels
        x[B - 1, :, V - 1] = 1.0
        x[B - 1, C - 2:, V - 1] = np.nan
        kind[B - 1, V - 1] = 2
    else:
        x[B - 1, 0, V - 1] = np.nan
        kind[B - 1, V - 1] = 1
    x.setflags(write=False)
    return x, kind


def argmax_case(row):
    """-> (logits (B, C, V) fp32, kind (B, V)); read-only, computed once"""
    return _argmax_case(row["B"], row["C"], row["V"], _seed(row["id"]))


@functools.lru_cache(maxsize=None)
def _argmax_ref(B, C, V, seed):
    return argmax_first(_argmax_case(B, C, V, seed)[0], axis=1)


def argmax_reference(row):
    return _argmax_ref(row["B"], row["C"], row["V"], _seed(row["id"]))


def column_shares(x):
    """x (C, N): the share of columns that hold (a tie at the maximum without NaN, exactly one NaN, several NaNs, an infinity, -0.0 and +0.0 tied at the maximum)"""
    nan = x != x
    nn = nan.sum(0)
    with np.errstate(invalid="ignore"):
        mx = np.where(nn == 0, np.max(np.where(nan, -np.inf, x), axis=0), np.nan)
        at_max = (x == mx[None]) & (nn == 0)[None]
    tie = at_max.sum(0) >= 2
    zero_pair = tie & (mx == 0) & ((at_max & np.signbit(x)).any(0)) & ((at_max & ~np.signbit(x)).any(0))
    return dict(tie=float(tie.mean()), nan=float((nn == 1).mean()), nans=float((nn >= 2).mean()), inf=float(np.isinf(x).any(0).mean()), zeros=float(zero_pair.mean()))


# ====================================================================================================================== confusion matrix
NP_LABEL = {1: np.uint8, 4: np.int32, 8: np.int64}
CONF_PAIRS = ((1, 1), (1, 8), (1, 4), (8, 8), (8, 1), (4, 4))                       # (pred bytes, gt bytes): the instances vx_confusion has
CONF_REFUSED_PAIRS = ((4, 1), (4, 8), (8, 4))
WILD = {1: (255,), 4: (-1, 255, INT_MAX, -INT_MAX - 1), 8: (-1, 255, INT_MAX, (1 << 32) + 1, -(1 << 32) - 1, (1 << 40) + 2, -(1 << 63))}
CONF_ROWS = [dict(id=f"nc{NC}_b{(1, 3)[(a + c) % 2]}_v{V}", NC=NC, B=(1, 3)[(a + c) % 2], V=V, wild=bool((a + c) % 2 == 1 and V > 1), cover=V >= 257,
                  **({"cap": "vx_confusion"} if V > 262144 else {}))
             for a, NC in enumerate((2, 4, 5, 8)) for c, V in enumerate((1, 257, 4099, 262144 + 4099))]


def confusion(pred, gt, NC):
    """pred, gt (B, V) integer arrays of any width -> int64 (B, NC, NC), conf[b, g, p]; each label is clamped IN ITS OWN WIDTH first: < 0 -> 0, >= NC -> NC-1"""
    def clamp(a):
        a = np.asarray(a)
        lo, hi = np.array(0, dtype=a.dtype), np.array(NC - 1, dtype=a.dtype)
        a = np.where(a < lo, lo, a)
        return np.where(a >= np.array(NC, dtype=a.dtype), hi, a).astype(np.int64)
    p, g = clamp(pred), clamp(gt)
    return np.stack([np.bincount(g[b] * NC + p[b], minlength=NC * NC).reshape(NC, NC) for b in range(p.shape[0])])


def labels_for(row, nbytes, which):
    """(B, V) labels of width `nbytes`: the first NC*NC voxels of every sample walk through every (gt, pred) cell (V permitting), the rest are seeded draws in
    [0, NC); a `wild` row also holds NC itself and the out-of-range values of WILD at seeded places of the tail.  which = 0 (pred) or 1 (gt)."""
    NC, B, V = row["NC"], row["B"], row["V"]
    rs = np.random.RandomState(_seed(row["id"]) + 17 * which)
    a = rs.randint(0, NC, size=(B, V)).astype(np.int64)
    cells = np.arange(min(V, NC * NC))
    a[:, :cells.size] = (cells % NC) if which == 0 else (cells // NC)
    if row["wild"]:
        vals = (NC,) + WILD[nbytes]
        free = np.arange(NC * NC, V)
        for b in range(B):
            at = rs.choice(free, size=min(free.size, 6 * len(vals)), replace=False)
            a[b, at] = np.resize(np.array(vals, dtype=np.int64), at.size)
    return a.astype(NP_LABEL[nbytes])


# ====================================================================================================================== sliding window
def sw_extract(vol, rd, rh, rw, z0, y0, x0):
    return vol[:, z0:z0 + rd, y0:y0 + rh, x0:x0 + rw].copy()


def sw_accumulate(acc, win, z0, y0, x0, weight):
    """-> fp64 copy of acc with acc[:, window] += weight * win"""
    out = np.asarray(acc, dtype=np.float64).copy()
    _, rd, rh, rw = win.shape
    out[:, z0:z0 + rd, y0:y0 + rh, x0:x0 + rw] += float(weight) * np.asarray(win, dtype=np.float64)
    return out


def sw_finalize(acc, cz, cy, cx):
    """-> (acc / ((cz*cy)*cx) in IEEE fp32, first-NaN / first-maximum arg-max over C of that quotient)"""
    f = np.float32
    cnt = (np.asarray(cz, f)[:, None, None] * np.asarray(cy, f)[None, :, None]).astype(f) * np.asarray(cx, f)[None, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = (np.asarray(acc, f) / cnt.astype(f)[None]).astype(f)
    return q, argmax_first(q, axis=0)


# (C, (D, H, W), (rd, rh, rw), (z0, y0, x0)): at the origin, at the far corner, one voxel, the whole volume; rw in {1, 3, 4, 5, 8}; odd x0
WINDOW_ROWS = [dict(id=i, C=C, vol=v, win=w, at=a) for i, C, v, w, a in (
    ("origin_rw4", 1, (5, 6, 9), (2, 3, 4), (0, 0, 0)), ("far_corner_rw5", 3, (5, 6, 9), (3, 2, 5), (2, 4, 4)), ("one_voxel", 3, (4, 5, 7), (1, 1, 1), (3, 4, 5)),
    ("whole_volume_rw8", 3, (3, 5, 8), (3, 5, 8), (0, 0, 0)), ("odd_x0_rw3", 1, (6, 7, 11), (4, 5, 3), (1, 2, 7)), ("odd_x0_rw8", 3, (4, 4, 13), (2, 3, 8), (2, 1, 3)),
    ("one_voxel_wide_column", 1, (7, 3, 5), (7, 3, 1), (0, 0, 3)))]
WINDOW_REFUSED = [((5, 6, 9), (2, 3, 4), (4, 0, 0)), ((5, 6, 9), (2, 3, 4), (0, 4, 0)), ((5, 6, 9), (2, 3, 4), (0, 0, 6)), ((5, 6, 9), (2, 3, 4), (-1, 0, 0)),
                  ((5, 6, 9), (6, 3, 4), (0, 0, 0)), ((5, 6, 9), (0, 3, 4), (0, 0, 0)), ((5, 6, 9), (2, -1, 4), (0, 0, 0)), ((5, 6, 9), (2, 3, 0), (0, 0, 0)),
                  ((5, 0, 9), (2, 3, 4), (0, 0, 0))]
WINDOW_OVER_CAP = dict(id="over_cap", C=1, vol=(258, 257, 257), win=(257, 256, 256), at=(1, 1, 1), cap="vx_grid_for")
COUNTS = (1, 2, 3, 4, 6, 8)
FINALIZE_ROWS = [dict(id=f"c{C}_{'x'.join(map(str, s))}", C=C, sp=s) for C, s in ((1, (3, 4, 5)), (2, (5, 7, 9)), (5, (4, 6, 11)), (256, (2, 3, 7)), (2, (1, 1, 1)))]
FINALIZE_OVER_CAP = dict(id="c2_over_cap", C=2, sp=OVER_CAP_DHW, cap="vx_grid_for")


@functools.lru_cache(maxsize=None)
def _finalize_case(C, sp, seed):
    D, H, W = sp
    rs = np.random.RandomState(seed)
    cz, cy, cx = (np.array(COUNTS, dtype=np.float32)[rs.randint(0, len(COUNTS), size=n)] for n in sp)
    acc = ints(C, D * H * W, seed=seed + 1)
    acc *= np.float32(2.0)                          # even integers in [-6, 6]: equal quotients across channels are planted as equal numerators (the divisor is per voxel)
    plant_columns(acc, seed + 2)
    if C > 1:
        acc[:, -1] = 1.0
        acc[C - 2:, -1] = np.nan
    acc = acc.reshape(C, D, H, W)
    for a in (cz, cy, cx, acc):
        a.setflags(write=False)
    return acc, cz, cy, cx


def finalize_case(row):
    return _finalize_case(row["C"], tuple(row["sp"]), _seed(row["id"]))


@functools.lru_cache(maxsize=None)
def _finalize_ref(C, sp, seed):
    return sw_finalize(*_finalize_case(C, sp, seed))


def finalize_reference(row):
    return _finalize_ref(row["C"], tuple(row["sp"]), _seed(row["id"]))


# ====================================================================================================================== foreground box
def min_value(x, preset=np.inf):
    """min(preset, the smallest voxel that is not NaN): NaN voxels are ignored (numpy's x.min() of oracle/augment_oracle.py would be NaN)"""
    x = np.asarray(x, dtype=np.float32).ravel()
    x = x[x == x]
    return np.float32(min(np.float32(preset), x.min())) if x.size else np.float32(preset)


def bbox_gt(x, thr, preset=(INT_MAX, INT_MAX, INT_MAX, -1, -1, -1)):
    """x (C, D, H, W): (min d, h, w, max d, h, w) of {x > thr} over all channels merged with `preset`; the preset itself when the set is empty (NaN > thr is false)"""
    with np.errstate(invalid="ignore"):
        sel = (np.asarray(x) > np.float32(thr)).any(0)
    out = list(preset)
    if sel.any():
        for ax in range(3):
            hit = np.nonzero(sel.any(axis=tuple(a for a in range(3) if a != ax)))[0]
            out[ax], out[3 + ax] = min(out[ax], int(hit[0])), max(out[3 + ax], int(hit[-1]))
    return out


MIN_N = (1, 63, 64, 65, 257, 70 * 90 * 84)
BOX_SHAPES = [(1, 1, 1, 1), (1, 1, 1, 63), (1, 2, 4, 8), (3, 5, 13, 1), (1, 1, 257, 1), (3, 3, 5, 7), (1, 70, 90, 84)]      # the last: 529,200 > 2048 x 256


# ====================================================================================================================== label rank-select
LABEL_CODES = (1, 4, 8, -4)
NP_LABEL_CODE = {1: np.uint8, 4: np.int32, 8: np.int64, -4: np.float32}
CHUNKS = (256, 768, 1000, 65536)
LABEL_N = (5003, 3 * 65536 + 259)                   # ragged against every chunk size and against 256; the last strip of the last chunk has 2 elements or more


def matches(lab, fg):
    with np.errstate(invalid="ignore"):
        m = np.asarray(lab).ravel() > 0
    return m if fg else ~m


def chunk_count(lab, chunk, fg):
    m = matches(lab, fg)
    nb = (m.size + chunk - 1) // chunk
    return np.array([int(m[c * chunk:(c + 1) * chunk].sum()) for c in range(nb)], dtype=np.int64)


def kth_in_chunk(lab, c0, chunk, fg, k):
    """flat index of the k-th match in [c0, min(c0 + chunk, n)), or None when the chunk holds k or fewer"""
    idx = np.nonzero(matches(lab, fg)[c0:c0 + chunk])[0]
    return int(c0 + idx[k]) if k < idx.size else None


@functools.lru_cache(maxsize=None)
def labels(code, n, fg):
    """seeded labels of type `code`; [1024, 3072) holds no match for `fg` (whole chunks of 256, 768 and 1000 without one).  Background values: 0, negatives where the
    type has them, for floats also NaN; foreground: 1..3, for floats 0.5, for int64 2^32 (a narrowing `> 0` would call it background)."""
    rs = np.random.RandomState(1000 * abs(code) + n % 977 + fg)
    bg = {1: [0], 4: [0, -1, -INT_MAX - 1], 8: [0, -1, -(1 << 32)], -4: [0.0, -1.0, np.nan, -0.0]}[code]
    fgv = {1: [1, 2, 3, 255], 4: [1, 2, 3, INT_MAX], 8: [1, 2, 3, 1 << 32], -4: [0.5, 1.0, 2.0, np.inf]}[code]
    is_fg = rs.rand(n) < 0.3
    is_fg[1024:3072] = not fg
    is_fg[n - 2:] = (False, True)                   # the last strip of the volume holds a match of either kind, however short it is
    lab = np.where(is_fg, np.array(fgv, dtype=np.float64 if code == -4 else np.int64)[rs.randint(0, len(fgv), size=n)],
                   np.array(bg, dtype=np.float64 if code == -4 else np.int64)[rs.randint(0, len(bg), size=n)]).astype(NP_LABEL_CODE[code])
    lab.setflags(write=False)
    return lab


def kth_queries(lab, chunk, fg, seed=5):
    """[(chunk start, k, expected flat index or None)]: in every chunk k = 0, the last k, k = the number of matches (nothing is written); every match that sits at
    thread 0 or thread 255 of a 256-strip of its chunk; every match of the ragged last strip of the volume; 64 seeded (chunk, k) draws"""
    m = matches(lab, fg)
    n, rs, out = m.size, np.random.RandomState(seed), []
    for c0 in range(0, n, chunk):
        idx = np.nonzero(m[c0:c0 + chunk])[0]
        ks = {0, idx.size}
        if idx.size:
            ks.add(idx.size - 1)
            lane = idx % 256
            ks.update(np.nonzero((lane == 0) | (lane == 255))[0].tolist())
            if c0 + chunk >= n:
                end = min(chunk, n - c0)
                ks.update(np.nonzero(idx >= (end - 1) // 256 * 256)[0].tolist())
        out += [(c0, k, int(c0 + idx[k]) if k < idx.size else None) for k in sorted(ks)]
    starts = np.arange(0, n, chunk)
    for _ in range(64):
        c0 = int(starts[rs.randint(starts.size)])
        cnt = int(m[c0:c0 + chunk].sum())
        if cnt:
            k = int(rs.randint(cnt))
            out.append((c0, k, kth_in_chunk(lab, c0, chunk, fg, k)))
    return out


# ====================================================================================================================== rotation
ROT_EXTENTS = ((9, 7), (8, 6), (33, 40), (16, 16), (5, 12))
ROT_CS_SN = ((0.75, 0.5), (0.5, -0.75), (0.875, 0.25), (1.25, 0.5), (0.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.0, -1.0), (-1.0, 0.0))
# ties: at least 10 % of the in-range samples of the row sit on an exact .5 (odd extents: the centre is an integer, .75 pd - .5 ph is a half for odd ph);
# border: at least 10 % of the samples are clamped
ROT_ROWS = [dict(id=f"{D}x{H}_cs{cs}_sn{sn}", D=D, H=H, cs=cs, sn=sn, W=(1, 3, 5)[(i + j) % 3], C=(1, 2)[(i + j) % 2],
                 ties=(D % 2 == 1 and H % 2 == 1 and (cs, sn) in ((0.75, 0.5), (0.5, -0.75), (0.5, 0.5))), border=(cs, sn) == (1.25, 0.5))
            for i, (D, H) in enumerate(ROT_EXTENTS) for j, (cs, sn) in enumerate(ROT_CS_SN)]


def rotate_coords(D, H, cs, sn, dtype=np.float64):
    """source coordinates (sd, sh), each (D, H), BEFORE the clamp, evaluated in `dtype` in the order of the kernel: cs*pd - sn*ph + cd, sn*pd + cs*ph + ch"""
    t = dtype
    cd, ch = t(0.5) * t(D - 1), t(0.5) * t(H - 1)
    pd = (np.arange(D, dtype=t) - cd)[:, None]
    ph = (np.arange(H, dtype=t) - ch)[None, :]
    cs, sn = t(cs), t(sn)
    return ((cs * pd).astype(t) - (sn * ph).astype(t)).astype(t) + cd, ((sn * pd).astype(t) + (cs * ph).astype(t)).astype(t) + ch


def rotate_exact(x, cs, sn, mode, dtype=np.float64):
    """x (C, D, H, W); out[c, d, h, w] = sample(x[c, :, :, w]) at R (d - cd, h - ch) + (cd, ch), centre (n-1)/2, the coordinate clamped to [0, n-1] and then sampled:
    mode 1 nearest with round-half-to-even (np.rint; nearbyintf in the default rounding mode), mode 0 bilinear, a direct gather and lerp in `dtype`"""
    t = dtype
    x = np.asarray(x, dtype=t)
    C, D, H, W = x.shape
    sd, sh = rotate_coords(D, H, cs, sn, t)
    sd, sh = np.clip(sd, t(0), t(D - 1)), np.clip(sh, t(0), t(H - 1))
    if mode == 1:
        return x[:, np.rint(sd).astype(np.int64), np.rint(sh).astype(np.int64), :]
    d0, h0 = np.floor(sd).astype(np.int64), np.floor(sh).astype(np.int64)
    d1, h1 = np.minimum(d0 + 1, D - 1), np.minimum(h0 + 1, H - 1)
    ld, lh = (sd - d0.astype(t))[None, :, :, None], (sh - h0.astype(t))[None, :, :, None]
    one = t(1)
    return ((one - ld) * ((one - lh) * x[:, d0, h0, :] + lh * x[:, d0, h1, :]) + ld * ((one - lh) * x[:, d1, h0, :] + lh * x[:, d1, h1, :])).astype(t)


def rotate_input(row):
    return ints(row["C"], row["D"], row["H"], row["W"], seed=_seed(row["id"]))


# ====================================================================================================================== BraTS Dice, the reference's formula
def brats_dice_reference(output, target):
    """utils/metric/metrics_brats.py of the reference restated on the CPU in fp32 (torch): Dice over dims (1, 2, 3) of (B, 1, D, H, W) masks, mean over the
    B*W planes; ET = (== 3), TC = (== 1) | (== 3), WT = (!= 0) -- a label above 3 is WT only.  -> (avg, ET, TC, WT) floats"""
    import torch

    def dice(o, t, eps=1e-6):
        inter = torch.sum(o * t, dim=(1, 2, 3)) + eps
        union = torch.sum(o, dim=(1, 2, 3)) + torch.sum(t, dim=(1, 2, 3)) + eps * 2
        return torch.mean(2 * inter / union)
    o, t = torch.as_tensor(output), torch.as_tensor(target)
    et = dice((o == 3).float(), (t == 3).float())
    tc = dice(((o == 1) | (o == 3)).float(), ((t == 1) | (t == 3)).float())
    wt = dice((o != 0).float(), (t != 0).float())
    return float((et + tc + wt) / 3), float(et), float(tc), float(wt)
