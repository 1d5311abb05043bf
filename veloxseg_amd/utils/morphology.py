"""Binary mask morphology and hole filling on the GPU (csrc/morphology.hip): dilation, erosion, opening, closing and the inner boundary of
bit-packed masks, their per-class forms on label maps, and fill_holes.  The reference has no counterpart; the semantics are scipy.ndimage's (binary_dilation,
binary_erosion, binary_opening, binary_closing, binary_fill_holes with generate_binary_structure(3, 1 | 2 | 3)) and, for label maps, MONAI's FillHoles restated
(unpinned against MONAI, which the tests do not have).  Device tensors only; there is no CPU fallback.

`connectivity` 6 / 18 / 26 means the offsets in {-1, 0, 1}^3 with at most 1 / 2 / 3 non-zero coordinates, the centre included.  A dilation step is the OR over the
offsets, an erosion step the AND; voxels outside the volume read `border_value` (default 0: a mask erodes at the faces, and so does a closing).

A mask travels as a PackedMask (one bit per voxel, rows padded to 64-bit words).  Every binary_* function takes a label tensor (and returns a mask tensor) or a
PackedMask (and returns one), so a chain such as opening-then-closing costs one pack and one unpack:  unpack(binary_closing(binary_opening(pack(x), 26), 26)).

The ball_* functions take a structuring element given in millimetres instead: the ball of a radius on a grid of a spacing, exactly the offsets
whose rounded squared length (section 33) is <= sq_threshold(radius), so that a dilation by it equals the thresholded exact distance transform bit for bit."""
import math

import numpy as np
import torch

from .. import _hip as H
from .components import _BYTES, _connectivity, _samples

MASK, KEEP, RESTRICT, PAINT = 0, 1, 2, 3
_DILATE, _ERODE = 0, 1


class PackedMask:
    """bits: int64 (B, D * H * Wq) device tensor in the layout of include/veloxseg_hip.h; shape: (D, H, W); like: shape and dtype of the tensor it was packed from"""

    def __init__(self, bits, shape, like_shape, like_dtype):
        self.bits, self.shape, self.like_shape, self.like_dtype = bits, tuple(shape), tuple(like_shape), like_dtype

    def _new(self, bits):
        return PackedMask(bits, self.shape, self.like_shape, self.like_dtype)


def _iterations(iterations, what):
    if int(iterations) != iterations or int(iterations) < 1:
        raise ValueError(f"{what}: iterations {iterations!r}, an integer >= 1 wanted")
    return int(iterations)


def _border(border_value):
    if border_value not in (0, 1, False, True):
        raise ValueError(f"border_value {border_value!r} is neither 0 nor 1")
    return int(border_value)


def pack(x: torch.Tensor, label=None) -> PackedMask:
    """the mask x != 0 (label None) or x == label of a (B, 1, D, H, W) or (D, H, W) label tensor, one bit per voxel"""
    s, _ = _samples(x, "pack")
    B, D, Hh, W = s.shape
    if D * Hh * W > 2 ** 31 - 1:
        raise ValueError(f"pack: {D * Hh * W} voxels per sample are more than a packed mask holds")
    bits = torch.empty((B, H.query("vx_morph_words", D, Hh, W)), dtype=torch.int64, device=s.device)
    st = H.stream_ptr()
    for b in range(B):
        H.call("vx_morph_pack", s[b].data_ptr(), _BYTES[s.dtype], 0 if label is None else int(label), 0 if label is None else 1, bits[b].data_ptr(), D, Hh, W, st)
    return PackedMask(bits, (D, Hh, W), x.shape, x.dtype)


def unpack(p: PackedMask, mode: int = MASK, into: torch.Tensor = None, value: int = 1) -> torch.Tensor:
    """MASK: the mask as a tensor of the packed tensor's shape, bool for a bool input, else uint8.  KEEP / RESTRICT / PAINT combine the mask with the label tensor
    `into` (see vx_morph_unpack) and return a new tensor of its dtype."""
    D, Hh, W = p.shape
    st = H.stream_ptr()
    if mode == MASK:
        out = torch.empty((p.bits.shape[0], D, Hh, W), dtype=torch.uint8, device=p.bits.device)
        for b in range(out.shape[0]):
            H.call("vx_morph_unpack", p.bits[b].data_ptr(), None, out[b].data_ptr(), 1, 1, MASK, D, Hh, W, st)
        out = out.reshape(p.like_shape)
        return out.view(torch.bool) if p.like_dtype == torch.bool else out
    s, _ = _samples(into, "unpack")
    if tuple(s.shape[1:]) != p.shape or s.shape[0] != p.bits.shape[0]:
        raise ValueError(f"unpack: label tensor {tuple(into.shape)} does not match the packed mask {p.bits.shape[0]} x {p.shape}")
    out = torch.empty_like(s)
    for b in range(s.shape[0]):
        H.call("vx_morph_unpack", p.bits[b].data_ptr(), s[b].data_ptr(), out[b].data_ptr(), _BYTES[s.dtype], int(value), int(mode), D, Hh, W, st)
    out = out.reshape(into.shape)
    return out.view(torch.bool) if into.dtype == torch.bool else out


def _step(p, op, connectivity, iterations, border_value):
    D, Hh, W = p.shape
    out = torch.empty_like(p.bits)
    tmp = torch.empty_like(p.bits[0]) if iterations > H.query("vx_morph_max_fused") else None
    st = H.stream_ptr()
    for b in range(out.shape[0]):
        H.call("vx_morph_step", p.bits[b].data_ptr(), out[b].data_ptr(), None if tmp is None else tmp.data_ptr(), D, Hh, W, op, connectivity, iterations, border_value, st)
    return p._new(out)


def _binary(x, label, what, fn):
    if isinstance(x, PackedMask):
        if label is not None:
            raise ValueError(f"{what}: a packed mask has no labels to select from")
        return fn(x)
    return unpack(fn(pack(x, label)))


def binary_dilation(x, connectivity: int = 6, iterations: int = 1, border_value: int = 0, label=None):
    """scipy.ndimage.binary_dilation of the mask x != 0 (or x == label)"""
    c, n, bv = _connectivity(connectivity), _iterations(iterations, "binary_dilation"), _border(border_value)
    return _binary(x, label, "binary_dilation", lambda p: _step(p, _DILATE, c, n, bv))


def binary_erosion(x, connectivity: int = 6, iterations: int = 1, border_value: int = 0, label=None):
    """scipy.ndimage.binary_erosion of the mask x != 0 (or x == label)"""
    c, n, bv = _connectivity(connectivity), _iterations(iterations, "binary_erosion"), _border(border_value)
    return _binary(x, label, "binary_erosion", lambda p: _step(p, _ERODE, c, n, bv))


def binary_opening(x, connectivity: int = 6, iterations: int = 1, border_value: int = 0, label=None):
    """n erosions, then n dilations (scipy.ndimage.binary_opening; both with border_value)"""
    c, n, bv = _connectivity(connectivity), _iterations(iterations, "binary_opening"), _border(border_value)
    return _binary(x, label, "binary_opening", lambda p: _step(_step(p, _ERODE, c, n, bv), _DILATE, c, n, bv))


def binary_closing(x, connectivity: int = 6, iterations: int = 1, border_value: int = 0, label=None):
    """n dilations, then n erosions (scipy.ndimage.binary_closing; both with border_value: with the default 0 a closing erodes at the faces)"""
    c, n, bv = _connectivity(connectivity), _iterations(iterations, "binary_closing"), _border(border_value)
    return _binary(x, label, "binary_closing", lambda p: _step(_step(p, _DILATE, c, n, bv), _ERODE, c, n, bv))


def inner_boundary(x, connectivity: int = 6, label=None):
    """the mask's voxels that an erosion (one iteration, border_value 0) removes"""
    c = _connectivity(connectivity)

    def fn(p):
        out = torch.empty_like(p.bits)
        st = H.stream_ptr()
        for b in range(out.shape[0]):
            H.call("vx_morph_boundary", p.bits[b].data_ptr(), out[b].data_ptr(), *p.shape, c, st)
        return p._new(out)
    return _binary(x, label, "inner_boundary", fn)


# ---------------------------------------------------------------------------------------------------------------------- the ball
# The largest row count at which method=None still takes the ball kernel where the distance transform could serve: the largest MEASURED count at which the kernel was
# the faster route on both probe volumes (tools/ball_probe.py, one MI355X run, profiles/r17_ball_probe.json).  Ungated dilation of the
# sparse "balls" surfaces, kernel against transform + compare + pack, medians in ms:
#     240 x 240 x 155   529 rows (1 mm)  0.480 / 1.343     545 rows (anisotropic)  0.449 / 1.378     2053 rows  1.819 / 1.344     2003 rows  1.686 / 1.376
#     400 x 400 x 352   529 rows         1.156 / 10.65     545 rows                1.111 / 11.20     2053 rows  4.377 / 10.67     2003 rows  4.112 / 11.16
# Nothing was measured between 545 and 2003 rows; on the smaller volume the kernel's 0.88 us per row would cross the transform near 1500.  On the dense mask the
# kernel stops after a few rows and was 20 - 80 x faster at every count.
BALL_ROWS_SWITCH = 545
BALL_MAX_HALF_WIDTH = 63          # hw is a 6-bit field of a record; dz and dy are signed bytes, held to the same bound


def sq_threshold(tau) -> float:
    """q(tau): the largest double with sqrt(q) <= tau under the correctly rounded square root, so that  sqrt(sq) <= tau  <=>  sq <= q  for every double sq"""
    tau = float(tau)
    if not (math.isfinite(tau) and tau >= 0.0):
        raise ValueError(f"radius {tau!r}: a finite number >= 0 wanted")
    q = tau * tau
    while math.sqrt(q) > tau:
        q = math.nextafter(q, -math.inf)
    while math.sqrt(math.nextafter(q, math.inf)) <= tau:
        q = math.nextafter(q, math.inf)
    return q


def _spacing(spacing, what):
    from .distance import _sampling          # (distance imports this module)
    return _sampling(spacing, what)


def _term(d, s):
    """t(d) = fl(fl(d * s) * fl(d * s)) of section 33, for an integer array d"""
    a = np.abs(d).astype(np.float64) * np.float64(s)
    return a * a


def _axis_radius(q, s):
    """the largest integer d >= 0 with t(d) <= q"""
    t = lambda d: (float(d) * s) * (float(d) * s)          # python floats round every product on its own, as numpy does
    d = int(math.sqrt(q) / s)
    while d > 0 and t(d) > q:
        d -= 1
    while t(d + 1) <= q:
        d += 1
    return d


def pack_rows(half_widths) -> np.ndarray:
    """the record list of a half-width table: one int32 per present row, dz in bits 0 - 7, dy in bits 8 - 15 (both signed bytes), hw in bits 16 - 21; the rows nearest
    the centre first (a word stops reading rows once it is decided)"""
    hwt = np.asarray(half_widths)
    rz, ry = hwt.shape[0] // 2, hwt.shape[1] // 2
    iz, iy = np.nonzero(hwt >= 0)
    dz, dy, hw = iz - rz, iy - ry, hwt[iz, iy].astype(np.int64)
    order = np.lexsort((dy, dz, dz * dz + dy * dy))
    dz, dy, hw = dz[order], dy[order], hw[order]
    return ((dz & 0xff) | ((dy & 0xff) << 8) | (hw << 16)).astype(np.int32)


class BallElement:
    """The ball of radius `radius` (the unit of the spacing, i.e. millimetres) on a grid of `spacing` (z, y, x): the offsets o with f(o) <= q(radius), f the rounded
    squared length of section 33.  radii = the largest offset along each axis; half_widths[dz + r_z, dy + r_y] = the largest |dx| of row (dz, dy), -1 for a row the
    ball does not have (int8); n_rows = the rows it has.  An element with a radius above 63 voxels has no table (half_widths and n_rows are None): only the
    distance-transform route can apply it."""

    def __init__(self, radius, spacing=None):
        self.radius, self.spacing = float(radius), _spacing(spacing, "BallElement")
        self.q = sq_threshold(radius)
        self.radii = tuple(_axis_radius(self.q, s) for s in self.spacing)
        self.half_widths, self.n_rows, self._rows = None, None, {}
        if max(self.radii) <= BALL_MAX_HALF_WIDTH:
            rz, ry, rx = self.radii
            sz, sy, sx = self.spacing
            zy = _term(np.arange(-rz, rz + 1), sz)[:, None] + _term(np.arange(-ry, ry + 1), sy)[None, :]
            inside = (zy[:, :, None] + _term(np.arange(rx + 1), sx)[None, None, :]) <= self.q          # f is monotone in |dx|: a row is a prefix
            self.half_widths = (inside.sum(-1) - 1).astype(np.int8)
            self.n_rows = int((self.half_widths >= 0).sum())

    def rows(self, device) -> torch.Tensor:
        """the record list on `device` (made once per device)"""
        key = str(device)
        if key not in self._rows:
            self._rows[key] = torch.from_numpy(pack_rows(self.half_widths)).to(device)
        return self._rows[key]


def _ball_kernel(p, el, op, border_value, gate=None):
    """vx_morph_ball on every sample of a packed mask; gate: a PackedMask of the same samples and shape"""
    cap = H.query("vx_morph_ball_max_rows")
    if el.n_rows is None or el.n_rows > cap:
        raise ValueError(f"the ball kernel takes per-axis radii up to {BALL_MAX_HALF_WIDTH} voxels and up to {cap} rows; radius {el.radius} on spacing {el.spacing} "
                         f"has radii {el.radii}" + ("" if el.n_rows is None else f" and {el.n_rows} rows"))
    rows = el.rows(p.bits.device)
    out = torch.empty_like(p.bits)
    st = H.stream_ptr()
    for b in range(out.shape[0]):
        H.call("vx_morph_ball", p.bits[b].data_ptr(), None if gate is None else gate.bits[b].data_ptr(), out[b].data_ptr(), *p.shape, rows.data_ptr(), el.n_rows, op,
               border_value, st)
    return p._new(out)


def _ball_edt(p, el, op, border_value):
    """the same bits from the exact distance transform: a voxel is in the dilation when a set voxel lies within q, and leaves the erosion (border value 1) when a
    clear one does"""
    from .distance import edt_sq
    if border_value != op:
        raise ValueError('method="edt" serves a dilation with border_value 0 and an erosion with border_value 1; the other two need method="ball"')
    sq = edt_sq(p, bool(op), el.spacing)
    m = (sq > el.q) if op else (sq <= el.q)
    return p._new(pack(m.reshape((m.shape[0], 1) + p.shape)).bits)


def _ball_step(p, el, op, border_value, method, gate=None):
    if method not in (None, "ball", "edt"):
        raise ValueError(f'method {method!r} is none of None, "ball", "edt"')
    if method is None:
        fits = el.n_rows is not None and el.n_rows <= min(BALL_ROWS_SWITCH, H.query("vx_morph_ball_max_rows"))
        method = "ball" if border_value != op or fits else "edt"
    if method == "ball":
        return _ball_kernel(p, el, op, border_value, gate)
    r = _ball_edt(p, el, op, border_value)
    return r if gate is None else r._new(r.bits & gate.bits)


def _ball_args(radius, spacing, border_value):
    return (radius if isinstance(radius, BallElement) and spacing is None else BallElement(radius, spacing)), _border(border_value)


def ball_dilation(x, radius, spacing=None, border_value: int = 0, label=None, method=None):
    """the dilation of the mask x != 0 (or x == label) by the ball of `radius` millimetres on a grid of `spacing` (z, y, x; default 1): scipy.ndimage.binary_dilation
    with BallElement's boolean structure.  x as for binary_dilation; radius may be a BallElement (spacing None).  method "ball": the row-list kernel; "edt": the
    distance transform compared with q (border_value 0 only); None: the faster of the two by BALL_ROWS_SWITCH."""
    el, bv = _ball_args(radius, spacing, border_value)
    return _binary(x, label, "ball_dilation", lambda p: _ball_step(p, el, _DILATE, bv, method))


def ball_erosion(x, radius, spacing=None, border_value: int = 0, label=None, method=None):
    """scipy.ndimage.binary_erosion with the ball; method "edt" serves border_value 1 only"""
    el, bv = _ball_args(radius, spacing, border_value)
    return _binary(x, label, "ball_erosion", lambda p: _ball_step(p, el, _ERODE, bv, method))


def ball_opening(x, radius, spacing=None, border_value: int = 0, label=None, method=None):
    """the erosion, then the dilation, both with border_value (scipy.ndimage.binary_opening)"""
    el, bv = _ball_args(radius, spacing, border_value)
    return _binary(x, label, "ball_opening", lambda p: _ball_step(_ball_step(p, el, _ERODE, bv, method), el, _DILATE, bv, method))


def ball_closing(x, radius, spacing=None, border_value: int = 0, label=None, method=None):
    """the dilation, then the erosion, both with border_value (scipy.ndimage.binary_closing)"""
    el, bv = _ball_args(radius, spacing, border_value)
    return _binary(x, label, "ball_closing", lambda p: _ball_step(_ball_step(p, el, _DILATE, bv, method), el, _ERODE, bv, method))


def _per_class(labels, labels_list, what, fn, mode):
    """the label-map forms: per class c of labels_list, in list order, the mask labels == c goes through fn; PAINT writes c where the result is set and the current
    map holds 0, RESTRICT zeroes where the map holds c and the result is clear.  labels_list None: the foreground labels != 0, painted 1 / kept."""
    _samples(labels, what)
    if labels_list is None:
        return unpack(fn(pack(labels)), KEEP if mode == RESTRICT else PAINT, labels, 1)
    cur = labels
    for c in labels_list:
        cur = unpack(fn(pack(cur, int(c))), mode, cur, int(c))
    return cur


def dilate_labels(labels: torch.Tensor, connectivity: int = 6, iterations: int = 1, labels_list=None) -> torch.Tensor:
    """per class: the dilated mask is painted where the map holds 0 (another class is never overwritten)"""
    c, n = _connectivity(connectivity), _iterations(iterations, "dilate_labels")
    return _per_class(labels, labels_list, "dilate_labels", lambda p: _step(p, _DILATE, c, n, 0), PAINT)


def erode_labels(labels: torch.Tensor, connectivity: int = 6, iterations: int = 1, labels_list=None) -> torch.Tensor:
    """per class: the voxels an erosion (border_value 0) removes are set to 0"""
    c, n = _connectivity(connectivity), _iterations(iterations, "erode_labels")
    return _per_class(labels, labels_list, "erode_labels", lambda p: _step(p, _ERODE, c, n, 0), RESTRICT)


def open_labels(labels: torch.Tensor, connectivity: int = 6, iterations: int = 1, labels_list=None) -> torch.Tensor:
    """per class: the voxels an opening removes are set to 0"""
    c, n = _connectivity(connectivity), _iterations(iterations, "open_labels")
    return _per_class(labels, labels_list, "open_labels", lambda p: _step(_step(p, _ERODE, c, n, 0), _DILATE, c, n, 0), RESTRICT)


def close_labels(labels: torch.Tensor, connectivity: int = 6, iterations: int = 1, labels_list=None) -> torch.Tensor:
    """per class: the voxels a closing adds are painted where the map holds 0; nothing is removed"""
    c, n = _connectivity(connectivity), _iterations(iterations, "close_labels")
    return _per_class(labels, labels_list, "close_labels", lambda p: _step(_step(p, _DILATE, c, n, 0), _ERODE, c, n, 0), PAINT)


def fill_holes(labels: torch.Tensor, connectivity: int = 6, applied_labels=None) -> torch.Tensor:
    """Fill the enclosed cavities of a label map.  The background labels == 0 is cut into components under `connectivity`; a component is filled with class c when
    none of its voxels has a neighbour outside the volume, every non-zero neighbour of its voxels holds c, and applied_labels is empty / None or contains c.
    For a {0, 1} mask this is scipy.ndimage.binary_fill_holes with that structure.  One host read per sample (the component count)."""
    c = _connectivity(connectivity)
    s, _ = _samples(labels, "fill_holes")
    B, D, Hh, W = s.shape
    V = D * Hh * W
    if V > 2 ** 31 - 1:
        raise ValueError(f"fill_holes: {V} voxels per sample do not fit a 32-bit component map")
    dev, st, nb = s.device, H.stream_ptr(), _BYTES[s.dtype]
    applied = None if not applied_labels else torch.tensor([int(a) for a in applied_labels], dtype=torch.int64, device=dev)
    bg = torch.empty((D, Hh, W), dtype=torch.uint8, device=dev)
    cc = torch.empty((D, Hh, W), dtype=torch.int32, device=dev)
    ws = torch.empty((H.query("vx_cc_ws_bytes", D, Hh, W) + 7) // 8, dtype=torch.int64, device=dev)
    num = torch.empty(1, dtype=torch.int32, device=dev)
    out = torch.empty_like(s)
    for b in range(B):
        H.call("vx_morph_background", s[b].data_ptr(), nb, bg.data_ptr(), V, st)
        H.call("vx_cc_label", bg.data_ptr(), 1, cc.data_ptr(), D, Hh, W, c, ws.data_ptr(), num.data_ptr(), st)
        n = int(num.item())
        lo = torch.full((n + 1,), torch.iinfo(torch.int64).max, dtype=torch.int64, device=dev)
        hi = torch.full((n + 1,), torch.iinfo(torch.int64).min, dtype=torch.int64, device=dev)
        opn = torch.zeros(n + 1, dtype=torch.int32, device=dev)
        H.call("vx_hole_scan", s[b].data_ptr(), nb, cc.data_ptr(), n, D, Hh, W, c, lo.data_ptr(), hi.data_ptr(), opn.data_ptr(), st)
        H.call("vx_hole_fill", s[b].data_ptr(), out[b].data_ptr(), nb, cc.data_ptr(), n, lo.data_ptr(), hi.data_ptr(), opn.data_ptr(),
               None if applied is None else applied.data_ptr(), 0 if applied is None else applied.numel(), V, st)
    out = out.reshape(labels.shape)
    return out.view(torch.bool) if labels.dtype == torch.bool else out
