"""Connected components of label volumes on the GPU (csrc/components.hip): labelling, per-component sizes, and the two mask clean-ups built
on them (drop components below a voxel count, keep the k largest).  The reference has no counterpart: its metrics are per voxel (utils/metric/metrics.py) and a
clean-up would copy the label map to the host.  Device tensors only; there is no CPU fallback.

Two voxels belong to one component when they are neighbours under `connectivity` (6 / 18 / 26) and hold the same non-zero value; a {0, 1} map is the binary case.
Components are numbered 1..N by ascending smallest flat index (z slowest, x fastest), which is scipy.ndimage.label's numbering; samples of a batch are numbered
independently."""
import torch

from .. import _hip as H

_BYTES = {torch.bool: 1, torch.uint8: 1, torch.int32: 4, torch.int64: 8}
_KEYS = ("min_voxels", "keep_largest", "connectivity", "binary", "closing", "opening", "fill_holes", "morph_connectivity", "labels")


def _samples(labels, what):
    """-> (contiguous (B, D, H, W) view, batched?) of a (B, 1, D, H, W) or (D, H, W) device label map"""
    if not isinstance(labels, torch.Tensor) or labels.dtype not in _BYTES:
        raise TypeError(f"{what}: label dtype {getattr(labels, 'dtype', type(labels))} not supported (bool, uint8, int32, int64)")
    if labels.dim() == 5 and labels.shape[1] == 1:
        batched = True
    elif labels.dim() == 3:
        batched = False
    else:
        raise ValueError(f"{what}: expected (B, 1, D, H, W) or (D, H, W), got {tuple(labels.shape)}")
    if labels.numel() == 0:
        raise ValueError(f"{what}: empty volume")
    if not labels.is_cuda:
        raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    x = labels.contiguous()
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    return x.reshape((-1,) + tuple(x.shape[-3:])), batched


def _connectivity(connectivity):
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity {connectivity!r} is none of 6, 18, 26")
    return int(connectivity)


def connected_components(labels: torch.Tensor, connectivity: int = 26):
    """-> (cc, num): cc int32 of the input's shape (0 on background, else the component's id in 1..num[b]); num = list of the samples' component counts.
    One host read per call (the counts)."""
    connectivity = _connectivity(connectivity)
    x, _ = _samples(labels, "connected_components")
    B, D, Hh, W = x.shape
    if D * Hh * W > 2 ** 31 - 1:
        raise ValueError(f"connected_components: {D * Hh * W} voxels per sample do not fit a 32-bit component map")
    cc = torch.empty(x.shape, dtype=torch.int32, device=x.device)
    ws = torch.empty((H.query("vx_cc_ws_bytes", D, Hh, W) + 7) // 8, dtype=torch.int64, device=x.device)
    num = torch.empty(B, dtype=torch.int32, device=x.device)
    st = H.stream_ptr()
    for b in range(B):
        H.call("vx_cc_label", x[b].data_ptr(), _BYTES[x.dtype], cc[b].data_ptr(), D, Hh, W, connectivity, ws.data_ptr(), num[b].data_ptr(), st)
    return cc.reshape(labels.shape), [int(n) for n in num.tolist()]


def _sizes(cc, num, other, what):
    c, batched = _samples(cc, what)
    if cc.dtype != torch.int32:
        raise TypeError(f"{what}: a component map is int32, got {cc.dtype}")
    num = [int(n) for n in ([num] if isinstance(num, int) else num)]
    if len(num) != c.shape[0] or any(n < 0 for n in num):
        raise ValueError(f"{what}: {len(num)} component counts for {c.shape[0]} samples")
    o = None
    if other is not None:
        o, _ = _samples(other, what)
        if o.shape != c.shape:
            raise ValueError(f"{what}: component map {tuple(cc.shape)} and other {tuple(other.shape)} differ in shape")
    V, st = c[0].numel(), H.stream_ptr()
    sizes, hits = [], []
    for b, n in enumerate(num):
        s = torch.zeros(n + 1, dtype=torch.int64, device=c.device)
        h = torch.zeros(n + 1, dtype=torch.int64, device=c.device) if o is not None else None
        H.call("vx_cc_tally", c[b].data_ptr(), None if o is None else o[b].data_ptr(), 0 if o is None else _BYTES[o.dtype], V, n, s.data_ptr(),
               None if h is None else h.data_ptr(), st)
        sizes.append(s)
        hits.append(h)
    return sizes, hits, batched


def component_sizes(cc: torch.Tensor, num, other: torch.Tensor = None):
    """voxel counts of the components of a map from connected_components: int64 device tensors of num + 1 entries, entry 0 the background.  With `other` (a label map
    of the same shape) also hits, where hits[id] = #voxels of component id at which other != 0.  A (D, H, W) map gives one tensor (num an int or a one-element list),
    a (B, 1, D, H, W) map a list with one tensor per sample (their lengths differ).  No host read."""
    sizes, hits, batched = _sizes(cc, num, other, "component_sizes")
    if not batched:
        sizes, hits = sizes[0], hits[0]
    return sizes if other is None else (sizes, hits)


def _filter(labels, connectivity, binary, what, keep_of):
    x, _ = _samples(labels, what)
    cc, num = connected_components((labels != 0) if binary else labels, connectivity)
    cc = cc.reshape(x.shape)
    sizes, _, _ = _sizes(cc.reshape(labels.shape), num, None, what)
    out = torch.empty_like(x)
    V, st = x[0].numel(), H.stream_ptr()
    for b, n in enumerate(num):
        keep = keep_of(sizes[b], n)
        H.call("vx_cc_select", cc[b].data_ptr(), keep.data_ptr(), n, x[b].data_ptr(), out[b].data_ptr(), _BYTES[x.dtype], V, st)
    out = out.reshape(labels.shape)
    return out.view(torch.bool) if labels.dtype == torch.bool else out


def remove_small_components(labels: torch.Tensor, min_voxels: int, connectivity: int = 26, binary: bool = False) -> torch.Tensor:
    """labels with every component of fewer than min_voxels voxels set to 0 (a component of exactly min_voxels stays); values and dtype are the input's.
    binary: components are those of labels != 0 (all non-zero classes joined)."""
    min_voxels = int(min_voxels)
    return _filter(labels, _connectivity(connectivity), binary, "remove_small_components", lambda sizes, n: (sizes >= min_voxels).to(torch.uint8))


def keep_largest_components(labels: torch.Tensor, k: int = 1, connectivity: int = 26, binary: bool = False) -> torch.Tensor:
    """labels with all but the k largest components set to 0; among components of equal size the lower id wins; k >= N keeps everything."""
    k = int(k)
    if k < 0:
        raise ValueError("keep_largest_components: k must not be negative")

    def keep_of(sizes, n):
        keep = torch.zeros(n + 1, dtype=torch.uint8, device=sizes.device)
        if n and k:
            order = torch.sort(sizes[1:], descending=True, stable=True).indices          # stable: equal sizes stay in id order (topk promises no order among ties)
            keep[order[:k] + 1] = 1
        return keep
    return _filter(labels, _connectivity(connectivity), binary, "keep_largest_components", keep_of)


class Postprocess:
    """Mask clean-up after the arg-max, from test_config["postprocess"]: {"min_voxels": n} drops smaller components, {"keep_largest": k} keeps the k largest (both:
    the small ones go first), "connectivity" 6 / 18 / 26 (default 26), "binary" joins all non-zero classes before labelling.  Morphology (utils/morphology.py,
    DESIGN.md section 31) runs ahead of them: {"closing": n} and {"opening": n} are close_labels / open_labels with n iterations, {"fill_holes": true} is fill_holes;
    "morph_connectivity" 6 / 18 / 26 (default 6) is their structuring element, "labels" the classes they work on (a list, processed in its order; None: the
    foreground labels != 0 as one mask for closing and opening, every class for fill_holes).  The order is fixed:
    closing -> fill_holes -> opening -> min_voxels -> keep_largest.  No settings: the identity."""

    def __init__(self, min_voxels=None, keep_largest=None, connectivity=26, binary=False, closing=None, opening=None, fill_holes=False, morph_connectivity=6,
                 labels=None):
        self.min_voxels = None if min_voxels is None else int(min_voxels)
        self.keep_largest = None if keep_largest is None else int(keep_largest)
        if self.min_voxels is not None and self.min_voxels < 0 or self.keep_largest is not None and self.keep_largest < 0:
            raise ValueError("Postprocess: min_voxels and keep_largest must not be negative")
        self.connectivity, self.binary = _connectivity(connectivity), bool(binary)
        self.closing, self.opening = (int(n) if n else None for n in (closing, opening))          # 0 iterations: unset
        if any(n is not None and n < 0 for n in (self.closing, self.opening)):
            raise ValueError("Postprocess: closing and opening iterations must not be negative")
        self.fill_holes, self.morph_connectivity = bool(fill_holes), _connectivity(morph_connectivity)
        self.labels = None if labels is None else [int(c) for c in labels]

    @classmethod
    def from_config(cls, cfg):
        cfg = dict(cfg or {})
        unknown = set(cfg) - set(_KEYS)
        if unknown:
            raise ValueError(f"test_config['postprocess']: unknown keys {sorted(unknown)} (accepted: {', '.join(_KEYS)})")
        return cls(**cfg)

    @property
    def identity(self):
        return self.min_voxels is None and self.keep_largest is None and self.closing is None and self.opening is None and not self.fill_holes

    def __call__(self, labels: torch.Tensor) -> torch.Tensor:
        if self.closing is not None or self.opening is not None or self.fill_holes:
            from . import morphology as M
            if self.closing is not None:
                labels = M.close_labels(labels, self.morph_connectivity, self.closing, self.labels)
            if self.fill_holes:
                labels = M.fill_holes(labels, self.morph_connectivity, self.labels)
            if self.opening is not None:
                labels = M.open_labels(labels, self.morph_connectivity, self.opening, self.labels)
        if self.min_voxels is not None:
            labels = remove_small_components(labels, self.min_voxels, self.connectivity, self.binary)
        if self.keep_largest is not None:
            labels = keep_largest_components(labels, self.keep_largest, self.connectivity, self.binary)
        return labels
