"""Surface-distance metrics on the GPU: hd, hd95, asd, assd with medpy 0.4's argument order and definitions (medpy.metric.binary, `__surface_distances` with
connectivity=1, i.e. the 6-connected structuring element).  medpy is restated here and unpinned against medpy itself, which the tests do not have; they hold the
restatement to scipy.ndimage (binary_erosion, distance_transform_edt) and np.percentile.  Device tensors only; there is no CPU fallback.

    surface of a mask   = the voxels an erosion (one iteration, border value 0) removes                    vx_morph_boundary
    surface_distances   = the distance map of the reference's surface, read at the result's surface        vx_edt_sq, vx_bits_count, vx_edt_gather
    hd95                = np.percentile(hstack((d_ab, d_ba)), 95)        hd = max(d_ab.max(), d_ba.max())
    asd                 = d_ab.mean()                                    assd = mean((asd(a, b), asd(b, a)))

hd and hd95 select their order statistics among the SQUARED distances on the device and take the square roots and numpy's interpolation on the host in fp64: the
square root is monotone and correctly rounded, so this is the percentile of the distances to the bit.  An empty mask raises RuntimeError, as medpy does."""
import math

import torch

from ... import _hip as H
from ..distance import _sampling, edt_sq, sqrt_
from ..morphology import BallElement, PackedMask, _ball_step, inner_boundary, pack
from ..preprocess import linear_lerp, linear_ranks


def _one(x, what) -> PackedMask:
    """one volume as a packed mask of x != 0: a (D, H, W) tensor, the same behind leading axes of length 1 (the reference squeezes them), or a one-sample PackedMask"""
    if isinstance(x, PackedMask):
        if x.bits.shape[0] != 1:
            raise ValueError(f"{what}: one volume expected, the packed mask holds {x.bits.shape[0]}")
        return x
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: a tensor or a PackedMask expected, got {type(x)}")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    while x.dim() > 3 and x.shape[0] == 1:
        x = x[0]
    if x.dim() != 3:
        raise ValueError(f"{what}: one (D, H, W) volume expected (leading axes of length 1 allowed), got {tuple(x.shape)}")
    if x.is_floating_point():
        x = x != 0
    return pack(x)


def _row_counts(p: PackedMask) -> torch.Tensor:
    D, Hh, W = p.shape
    counts = torch.empty(D * Hh, dtype=torch.int32, device=p.bits.device)
    H.call("vx_bits_count", p.bits[0].data_ptr(), D, Hh, W, counts.data_ptr(), H.stream_ptr())
    return counts


def _gather(values: torch.Tensor, p: PackedMask) -> torch.Tensor:
    """the values at the set voxels of p, in flat-index order (one host read: the count)"""
    D, Hh, W = p.shape
    counts = _row_counts(p)
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets = ends - counts
    out = torch.empty(int(ends[-1]), dtype=torch.float64, device=values.device)
    if out.numel():
        H.call("vx_edt_gather", values.data_ptr(), p.bits[0].data_ptr(), offsets.data_ptr(), out.data_ptr(), D, Hh, W, H.stream_ptr())
    return out


def _surfaces(result, reference, what):
    r, f = _one(result, what), _one(reference, what)
    if r.shape != f.shape:
        raise ValueError(f"{what}: the volumes differ in shape: {r.shape} and {f.shape}")
    n = torch.stack([_row_counts(r).sum(), _row_counts(f).sum()]).tolist()
    if n[0] == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if n[1] == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return inner_boundary(r, 6), inner_boundary(f, 6)


def _sq_at(surface_from: PackedMask, surface_to: PackedMask, s) -> torch.Tensor:
    return _gather(edt_sq(surface_to, False, s)[0], surface_from)


def _both_sq(result, reference, spacing, what):
    s = _sampling(spacing, what)
    br, bf = _surfaces(result, reference, what)
    return _sq_at(br, bf, s), _sq_at(bf, br, s)


def surface_distances(result, reference, spacing=None, squared: bool = False) -> torch.Tensor:
    """medpy's __surface_distances(result, reference, voxelspacing, connectivity=1): for every surface voxel of `result`, in flat-index order, its distance to the
    nearest surface voxel of `reference` -> a compact fp64 device tensor (squared=True: the squared distances)"""
    s = _sampling(spacing, "surface_distances")
    br, bf = _surfaces(result, reference, "surface_distances")
    d = _sq_at(br, bf, s)
    return d if squared else sqrt_(d)


def hd(result, reference, voxelspacing=None) -> float:
    """medpy.metric.binary.hd: the larger of the two directed maxima"""
    ab, ba = _both_sq(result, reference, voxelspacing, "hd")
    return math.sqrt(float(torch.maximum(ab.max(), ba.max())))


def hd95(result, reference, voxelspacing=None) -> float:
    """medpy.metric.binary.hd95: np.percentile(hstack((d_ab, d_ba)), 95), numpy's linear rule"""
    ab, ba = _both_sq(result, reference, voxelspacing, "hd95")
    sq = torch.sort(torch.cat([ab, ba])).values
    v, lo, hi = linear_ranks(sq.numel(), 95.0)
    a, b = sq[[lo, hi]].tolist()
    return linear_lerp(math.sqrt(a), math.sqrt(b), v, lo)


def asd(result, reference, voxelspacing=None) -> float:
    """medpy.metric.binary.asd: the mean of surface_distances(result, reference)"""
    return float(surface_distances(result, reference, voxelspacing).mean())


def assd(result, reference, voxelspacing=None) -> float:
    """medpy.metric.binary.assd: the mean of asd(result, reference) and asd(reference, result)"""
    ab, ba = _both_sq(result, reference, voxelspacing, "assd")
    a, b = torch.stack([sqrt_(ab).mean(), sqrt_(ba).mean()]).tolist()
    return (a + b) / 2


def surface_overlap(result, reference, threshold, spacing=None):
    """-> (tp_a, n_a, tp_b, n_b), Python ints: n_a / n_b = the surface voxels of `result` / `reference` (the surfaces of surface_distances), tp_a = those of
    `result` with a surface voxel of `reference` within `threshold` (sqrt(sq) <= threshold on the exact squared distances, i.e. sq <= q(threshold)), tp_b the other
    way round.  No distance map is formed: tp_a = popcount(S_a & dilate(S_b, ball)) with the gated kernel of DESIGN.md section 35 (beyond the kernel's cap the
    distance transform serves).  One host read; an empty mask raises RuntimeError, as medpy does."""
    s = _sampling(spacing, "surface_overlap")
    el = BallElement(threshold, s)
    r, f = _one(result, "surface_overlap"), _one(reference, "surface_overlap")
    if r.shape != f.shape:
        raise ValueError(f"surface_overlap: the volumes differ in shape: {r.shape} and {f.shape}")
    br, bf = inner_boundary(r, 6), inner_boundary(f, 6)
    near_b, near_a = _ball_step(bf, el, 0, 0, None, gate=br), _ball_step(br, el, 0, 0, None, gate=bf)
    m_a, m_b, tp_a, n_a, tp_b, n_b = torch.stack([_row_counts(p).sum() for p in (r, f, near_b, br, near_a, bf)]).tolist()
    if m_a == 0:
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if m_b == 0:
        raise RuntimeError("The second supplied array does not contain any binary object.")
    return tp_a, n_a, tp_b, n_b


def normalized_surface_dice(a, b, threshold, spacing=None, connectivity=1) -> float:
    """The symmetric normalised surface Dice of nnU-Net's evaluator (evaluation/surface_dice.py), restated: with the fractions tp_a = (surface voxels of a within
    `threshold` of b's surface) / n_a, tp_b likewise, fp = 1 - tp_a and fn = 1 - tp_b formed as counts over n,
        (tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8),
    summed in that order in fp64.  threshold is in the unit of `spacing` (millimetres).  Only connectivity=1 (the 6-connected surface of medpy) is accepted.  Like
    hd95 here it is unpinned against medpy and nnU-Net themselves, which the tests do not have; they hold it to scipy.ndimage.  It is NOT the surface-area-weighted
    NSD of DeepMind's surface-distance package (nnU-Net's own docstring says the same): every surface voxel counts 1."""
    if connectivity != 1:
        raise ValueError(f"normalized_surface_dice: connectivity {connectivity!r}; only 1 (the 6-connected surface) is supported")
    tp_a, n_a, tp_b, n_b = surface_overlap(a, b, threshold, spacing)
    ta, tb, fp, fn = tp_a / n_a, tp_b / n_b, (n_a - tp_a) / n_a, (n_b - tp_b) / n_b
    return (ta + tb) / (ta + tb + fp + fn + 1e-8)


def _nan_when_empty(gt, pred, what):
    if not isinstance(gt, torch.Tensor) or not isinstance(pred, torch.Tensor):
        raise TypeError(f"{what}: tensors expected")
    if not gt.is_cuda or not pred.is_cuda:
        raise RuntimeError(f"{what}: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
    top = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t).max()
    return torch.stack([top(gt) == 0, top(pred) == 0]).any().item()


def reference_surface_dice(gt, pred, threshold, spacing=(1, 1, 1)) -> float:
    """the body of get_surface_dice: nan when a side holds nothing (as get_hausdorff), else normalized_surface_dice(pred, gt, threshold, spacing)"""
    if _nan_when_empty(gt, pred, "surface Dice"):
        return float("nan")
    return normalized_surface_dice(pred, gt, threshold, spacing)


def reference_hd95(gt, pred, spacing=(1, 1, 1)) -> float:
    """the body the reference's get_hausdorff and HD95 share: nan when a side holds nothing, else hd95(pred, gt, spacing)"""
    if not isinstance(gt, torch.Tensor) or not isinstance(pred, torch.Tensor):
        raise TypeError("HD95: tensors expected")
    if not gt.is_cuda or not pred.is_cuda:
        raise RuntimeError("HD95: the HIP path needs CUDA (ROCm) tensors; there is no CPU fallback")
    top = lambda t: (t.view(torch.uint8) if t.dtype == torch.bool else t).max()
    if torch.stack([top(gt) == 0, top(pred) == 0]).any().item():
        return float("nan")
    return float(hd95(pred, gt, spacing))
