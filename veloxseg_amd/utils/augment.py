"""GPU stand-in for the three MONAI dictionary transforms of the reference's training pipeline (utils/train_autopet.py:132-152, utils/train_brats.py):
CropForegroundd(select_fn = x > x.min()), RandCropByPosNegLabeld and RandRotated(range_z) -- same class names, keys and argument meaning, operating on
(C, D, H, W) tensors that are already resident in HBM.  The reductions, the label rank-select and the resampling are HIP kernels (csrc/augment.hip);
random draws are taken on the host from numpy's RandomState in MONAI's order.  There is no CPU fallback.
Beyond the reference's three: RandFlipd, RandScaleIntensityd, RandShiftIntensityd, RandGaussianNoised and BatchAssembler, which applies them while ONE kernel call
(csrc/augment_batch.hip) writes the (B, M, D, H, W) batch and its int64 labels; from_config reads train_config["augment"].
RandAffined / affine_sample / affine_matrix: rotation about all three axes, scale and translation of every sample, key and channel in ONE kernel call
(csrc/augment_affine.hip); spatial_from_config reads train_config["spatial_augment"].
RandGaussianSmoothd / RandScaleIntensityFixedMeand / RandAdjustContrastd / blur_separable: a separable blur and the transforms that need a channel's min / max /
mean / std, whose statistics are reduced on the device and read there by the step program (csrc/augment_blur.hip, csrc/augment_stats.hip).
Rand3DElasticd / elastic_field / elastic_sample: a smooth random displacement field drawn and smoothed on the device from one host seed per sample, and the affine
resampler with that displacement in front of its matrix (csrc/augment_elastic.hip); the elastic_* keys of train_config["spatial_augment"]."""
import math

import numpy as np
import torch

from .. import _hip as H

_CHUNK = 1 << 16
_INT_MAX = 0x7FFFFFFF


def rotation_range_from_degrees(degrees):
    """reference: utils/runtime.py:115"""
    return math.radians(float(degrees))


def image_label_modes(image_key_count):
    """reference: utils/runtime.py:119"""
    if image_key_count <= 0:
        raise ValueError("image_key_count must be greater than 0")
    return tuple(["bilinear"] * image_key_count + ["nearest"])


def _need_cuda(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    if t.dim() != 4:
        raise ValueError(f"{what}: expected (C, D, H, W), got {tuple(t.shape)}")


def label_code(lab):
    """bytes code of a label / mask tensor for the C entries: uint8 1, int32 4, int64 8, float32 -4"""
    code = {torch.uint8: 1, torch.int32: 4, torch.int64: 8, torch.float32: -4}.get(lab.dtype)
    if code is None:
        raise TypeError(f"label dtype {lab.dtype} not supported (uint8, int32, int64, float32)")
    return code


def foreground_box(source: torch.Tensor):
    """bounding box (start[3], end[3]) of {source > source.min()} over all channels; zeros when empty"""
    _need_cuda(source, "foreground_box")
    x = source.contiguous().float()
    C, D, Hh, W = x.shape
    st = H.stream_ptr()
    mn = torch.full((1,), float("inf"), device=x.device)
    H.call("vx_min_value", x.data_ptr(), x.numel(), mn.data_ptr(), st)
    box = torch.tensor([_INT_MAX] * 3 + [-1] * 3, dtype=torch.int32, device=x.device)
    H.call("vx_bbox_gt", x.data_ptr(), float(mn.item()), C, D, Hh, W, box.data_ptr(), st)
    b = box.tolist()
    if b[3] < 0:
        return [0, 0, 0], [0, 0, 0]
    return b[:3], [v + 1 for v in b[3:]]


class _LabelIndex:
    """rank-select over the flat label volume: number of foreground / background voxels and the flat index of the k-th one"""

    def __init__(self, label: torch.Tensor):
        _need_cuda(label, "label")
        if label.shape[0] != 1:
            raise ValueError("label must have one channel")
        self.lab = label.contiguous()
        self.code = label_code(self.lab)
        self.n = self.lab.numel()
        nb = (self.n + _CHUNK - 1) // _CHUNK
        cnt = torch.empty(nb, dtype=torch.int32, device=label.device)
        H.call("vx_label_chunk_count", self.lab.data_ptr(), self.code, self.n, _CHUNK, 1, cnt.data_ptr(), H.stream_ptr())
        fg = cnt.cpu().numpy().astype(np.int64)
        sizes = np.minimum(_CHUNK, self.n - np.arange(nb, dtype=np.int64) * _CHUNK)
        self.cum = {1: np.cumsum(fg), 0: np.cumsum(sizes - fg)}
        self.out = torch.empty(1, dtype=torch.int64, device=label.device)

    def count(self, fg: int) -> int:
        return int(self.cum[fg][-1])

    def kth(self, fg: int, k: int) -> int:
        cum = self.cum[fg]
        ch = int(np.searchsorted(cum, k, side="right"))
        before = int(cum[ch - 1]) if ch else 0
        H.call("vx_label_kth_in_chunk", self.lab.data_ptr(), self.code, self.n, ch * _CHUNK, _CHUNK, fg, k - before, self.out.data_ptr(), H.stream_ptr())
        return int(self.out.item())


def _correct_center(center, spatial_size, shape, allow_smaller):
    spatial_size = list(spatial_size)
    if any(s - p < 0 for s, p in zip(shape, spatial_size)):
        if not allow_smaller:
            raise ValueError("The size of the proposed random crop ROI is larger than the image size")
        spatial_size = [min(s, p) for s, p in zip(shape, spatial_size)]
    out = []
    for c, p, s in zip(center, spatial_size, shape):
        lo = p // 2
        hi = int(s + 1 - p / 2.0)
        if hi == lo:
            hi += 1
        out.append(int(min(max(c, lo), hi - 1)))
    return out


class _Randomizable:
    def set_random_state(self, seed=None, state=None):
        self.R = state if state is not None else np.random.RandomState(seed)
        return self


class CropForegroundd:
    def __init__(self, keys, source_key, select_fn=None):
        self.keys, self.source_key = list(keys), source_key
        if select_fn is not None:      # only the reference's selector (x > x.min()) runs on the GPU: check that this is what was passed
            for probe in (torch.tensor([[-3.0, -3.0, 5.0, -1.0]]), torch.tensor([[10.0, 11.0, 10.5, 10.0]])):
                if torch.equal(torch.as_tensor(select_fn(probe)), probe > probe.min()):
                    continue
                raise NotImplementedError("CropForegroundd: only select_fn = (x > x.min()) is implemented on the HIP path")

    def __call__(self, data):
        start, end = foreground_box(data[self.source_key])
        out = dict(data)
        for k in self.keys:
            out[k] = data[k][:, start[0]:end[0], start[1]:end[1], start[2]:end[2]]
        out["foreground_start_coord"], out["foreground_end_coord"] = start, end
        return out


class RandCropByPosNegLabeld(_Randomizable):
    """copy=True (default): every crop is copied out, as MONAI does.  copy=False: the crops are VIEWS of the volume (no copy, same draws, same voxels) and every
    sample also carries `crop_start` (the window's origin in the cropped-from volume) and `crop_source_shape` (that volume's spatial shape), which
    RandAffined(context=True) reads"""

    def __init__(self, keys, label_key, spatial_size, pos=1.0, neg=1.0, num_samples=1, allow_smaller=False, copy=True):
        if pos < 0 or neg < 0 or pos + neg == 0:
            raise ValueError("pos and neg must be nonnegative and not both zero")
        self.keys, self.label_key, self.spatial_size = list(keys), label_key, list(spatial_size)
        self.pos_ratio, self.num_samples, self.allow_smaller, self.copy = pos / (pos + neg), int(num_samples), allow_smaller, bool(copy)
        self.set_random_state()

    def centers(self, label):
        index = _LabelIndex(label)
        shape = tuple(label.shape[1:])
        nfg, nbg = index.count(1), index.count(0)
        ratio = self.pos_ratio
        if nfg == 0 and nbg == 0:
            raise ValueError("No sampling location available.")
        if nfg == 0 or nbg == 0:
            ratio = 0 if nfg == 0 else 1
        out = []
        for _ in range(self.num_samples):
            fg = 1 if self.R.rand() < ratio else 0
            flat = index.kth(fg, int(self.R.randint(nfg if fg else nbg)))
            out.append(_correct_center(list(np.unravel_index(flat, shape)), self.spatial_size, shape, self.allow_smaller))
        return out

    def __call__(self, data):
        shape = tuple(data[self.label_key].shape[1:])
        res = []
        for c in self.centers(data[self.label_key]):
            sl = tuple(slice(max(ci - p // 2, 0), min(max(ci - p // 2, 0) + p, s)) for ci, p, s in zip(c, self.spatial_size, shape))
            d = dict(data)
            for k in self.keys:
                d[k] = data[k][(slice(None),) + sl].contiguous() if self.copy else data[k][(slice(None),) + sl]
            d["crop_center"] = c
            if not self.copy:
                d["crop_start"], d["crop_source_shape"] = [s.start for s in sl], list(shape)
            res.append(d)
        return res


def rotate_z(x: torch.Tensor, angle: float, mode: str = "bilinear") -> torch.Tensor:
    _need_cuda(x, "rotate_z")
    if mode not in ("bilinear", "nearest"):
        raise ValueError(f"mode {mode!r} not supported")
    xin = x.contiguous().float()
    out = torch.empty_like(xin)
    C, D, Hh, W = xin.shape
    H.call("vx_rotate_z", xin.data_ptr(), out.data_ptr(), C, D, Hh, W, math.cos(angle), math.sin(angle), 0 if mode == "bilinear" else 1, H.stream_ptr())
    return out.to(x.dtype) if x.dtype != torch.float32 else out


class RandRotated(_Randomizable):
    def __init__(self, keys, range_x=0.0, range_y=0.0, range_z=0.0, prob=0.1, mode="bilinear", padding_mode="border"):
        if range_x or range_y:
            raise NotImplementedError("RandRotated: only rotation about z (range_z) is implemented on the HIP path (the reference uses no other)")
        if padding_mode != "border":
            raise NotImplementedError("RandRotated: only padding_mode='border' (MONAI's default) is implemented")
        self.keys, self.range_z, self.prob = list(keys), float(range_z), float(prob)
        self.mode = [mode] * len(self.keys) if isinstance(mode, str) else list(mode)
        if len(self.mode) != len(self.keys):
            raise ValueError("mode must have one entry per key")
        self.set_random_state()

    def draw(self):
        do = self.R.rand() < self.prob
        self.R.uniform(low=-0.0, high=0.0)
        self.R.uniform(low=-0.0, high=0.0)
        return do, float(self.R.uniform(low=-self.range_z, high=self.range_z))

    def __call__(self, data):
        if isinstance(data, list):
            return [self(d) for d in data]
        do, angle = self.draw()
        out = dict(data)
        if do:
            for k, m in zip(self.keys, self.mode):
                out[k] = rotate_z(data[k], angle, m)
        return out


# ---- batch assembly: mirror, intensity steps and noise in one table-driven pass (csrc/augment_batch.hip) ----------------------------------
# MONAI is not installed here: the draw orders below model MONAI 1.x (RandomizableTransform.randomize draws R.rand() < prob first, the parameters only when that
# fires) and are UNPINNED against MONAI itself, like oracle/augment_oracle.py; tests/intensity_ref.py restates them.
AUG_RECORD_BYTES, AUG_MAX_STEPS, AUG_LABEL = 192, 8, -1
AUG_NOISE_STREAM = 0x564158475541          # VX_AUG_NOISE_STREAM of include/veloxseg_hip.h: dropout site ids count up from 1 and never get there
_OP_MUL, _OP_ADD, _OP_NOISE = 1, 2, 3
_OP_CONTRAST, _OP_GAMMA, _OP_RETAIN = 4, 5, 6          # read a slot of the device statistics table; known to vx_augment_batch_ext only
AUG_STAT_BYTES, AUG_STAT_JOB_BYTES, AUG_STAT_PARTIAL_BYTES, AUG_STAT_CHUNK = 32, 16, 24, 4096
BLUR_RECORD_BYTES, BLUR_MAX_TAIL, BLUR_MAX_SIGMA = 272, 16, 4.0
_REC = np.dtype([("src", "<u8"), ("stride", "<i8", (3,)), ("dtype", "<i4"), ("b", "<i4"), ("c", "<i4"), ("flip", "<i4"), ("n_steps", "<i4"), ("pad", "<i4", (3,)),
                 ("step", [("op", "<u4"), ("a", "<f4"), ("b", "<f4"), ("key", "<u4")], (AUG_MAX_STEPS,))])
assert _REC.itemsize == AUG_RECORD_BYTES
_STAT = np.dtype([("min", "<f4"), ("max", "<f4"), ("mean", "<f4"), ("std", "<f4"), ("s1", "<f8"), ("s2", "<f8")])
_JOB = np.dtype([("rec", "<i4"), ("upto", "<i4"), ("slot", "<i4"), ("frame", "<i4")])
_BLUR = np.dtype([("src", "<u8"), ("dst", "<u8"), ("stride", "<i8", (3,)), ("tail", "<i4", (3,)), ("pad", "<i4"), ("w", "<f4", (3, BLUR_MAX_TAIL + 1)), ("pad2", "<i4", (3,))])
assert (_STAT.itemsize, _JOB.itemsize, _BLUR.itemsize) == (AUG_STAT_BYTES, AUG_STAT_JOB_BYTES, BLUR_RECORD_BYTES)


def _flip_mask(spatial_axis):
    """None -> all three axes; an int or a sequence of ints -> those (0 = D, 1 = H, 2 = W; negative axes count from the end); bit a = axis a"""
    if spatial_axis is None:
        return 7
    axes = list(spatial_axis) if isinstance(spatial_axis, (list, tuple)) else [spatial_axis]
    mask = 0
    for a in axes:
        if isinstance(a, bool) or not isinstance(a, (int, np.integer)) or not -3 <= a < 3:
            raise ValueError(f"spatial_axis {spatial_axis!r}: every axis must be an int in -3..2 (0 = D, 1 = H, 2 = W)")
        mask |= 1 << (int(a) % 3)
    return mask


def _range(v, what):
    """MONAI's reading of `factors` / `offsets`: a number r means (-|r|, |r|), a pair means (min, max)"""
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
        lo, hi = min(-float(v), float(v)), max(-float(v), float(v))
    else:
        try:
            pair = [float(t) for t in v]
        except (TypeError, ValueError):
            raise ValueError(f"{what} {v!r}: a number or a pair of numbers") from None
        if len(pair) != 2:
            raise ValueError(f"{what} should be a number or pair of numbers, got {v!r}")
        lo, hi = min(pair), max(pair)
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{what} {v!r} is not finite")
    return lo, hi


def _prob(p):
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"prob {p} outside [0, 1]")
    return p


class _Program:
    """what the transforms drawn so far do to one key of one sample: a flip mask and the pointwise steps [op, a, b, key, mask of the flips that follow, noise channel]"""

    staged = False           # True once the program needs more than the one pass of vx_augment_batch: a blur, or a step that reads statistics (ops 4..6)
    blur = None              # or (number of steps in front of the blur, (wD, wH, wW) half weights, the flip mask at the time the blur was added)

    def __init__(self):
        self.flip, self.steps = 0, []

    def add_flip(self, mask):
        self.flip ^= mask
        for s in self.steps:
            s[4] ^= mask

    def add_blur(self, halves):
        if self.blur is not None:
            raise ValueError("more than one blur fired on one key: a record is materialised once")
        self.blur, self.staged = (len(self.steps), halves, self.flip), True

    def blur_post(self):
        """mask of the flips that follow the blur"""
        return self.flip ^ self.blur[2]

    def add_step(self, op, a=0.0, b=0.0, key=0, chan=0):
        if len(self.steps) == AUG_MAX_STEPS:
            raise ValueError(f"more than {AUG_MAX_STEPS} pointwise steps fired on one key: the record holds no more")
        self.steps.append([op, a, b, key, 0, chan])
        if op >= _OP_CONTRAST:
            self.staged = True


def _check_source(t, what, image):
    """raises before any GPU work: RuntimeError (not on the device), TypeError (dtype), ValueError (shape) -> the element code of the record"""
    _need_cuda(t, what)
    if image:
        if t.dtype != torch.float32:
            raise TypeError(f"{what}: image dtype {t.dtype} not supported (float32)")
        return 0
    return label_code(t)


def _pack(entries):
    """entries: [(tensor (D, H, W) view, element code, b, c, _Program)] -> the record table as a host uint8 tensor"""
    tab = np.zeros(len(entries), dtype=_REC)
    for r, (t, code, b, c, prog) in zip(tab, entries):
        r["src"], r["stride"], r["dtype"], r["b"], r["c"], r["flip"], r["n_steps"] = t.data_ptr(), t.stride(), code, b, c, prog.flip, len(prog.steps)
        for k, (op, a, sb, key, post, chan) in enumerate(prog.steps):
            r["step"][k] = (op | (post << 4) | (chan << 8), a, sb, key)
    return torch.from_numpy(tab.view(np.uint8).reshape(-1))


def _launch(entries, x_out, y_out, B, M, spatial):
    """entries as in _pack, images first -> ONE table, ONE upload, ONE call of vx_augment_batch"""
    n_image = sum(1 for e in entries if e[3] != AUG_LABEL)
    dev = (x_out if x_out is not None else y_out).device
    table = _pack(entries).to(dev)
    H.call("vx_augment_batch", table.data_ptr(), n_image, len(entries) - n_image, None if x_out is None else x_out.data_ptr(), None if y_out is None else y_out.data_ptr(),
           8, B, M, *spatial, H.stream_ptr())


# ---- staged launch: programs with a blur or with statistics steps ------------------------------------------------------------------------
class _Stage:
    """host-side plan of one staged call, made without touching the GPU.  records: the final records (images, then labels) followed by one `pre` record per blurred
    channel (the steps in front of the blur, written to a scratch channel); every record is [source or None (= the blurred scratch channel), code, b, c, flip, steps].
    rounds_pre / rounds_post: lists of job lists [(record index, upto, slot, frame)], one vx_augment_stats call each, before and after the blur.
    calls: the names of the C entries in the order they are made."""


def _plan(entries):
    """entries as in _pack, images first -> _Stage.  Round j of a phase resolves the j-th pending statistic of every record that still has one, so the number of
    vx_augment_stats calls is the depth of the deepest chain that fired and never grows with the number of records."""
    st = _Stage()
    n = len(entries)
    final, pre, st.blurs, pending_pre, pending_post, slots = [], [], [], [], [], 0
    for i, (t, code, b, c, prog) in enumerate(entries):
        steps = [list(s) for s in prog.steps]
        if prog.blur is None:
            final.append([t, code, b, c, prog.flip, steps])
            parts = [(i, steps, False)]
        else:
            if code != 0:
                raise ValueError("a blur on a label record")
            p, halves, post = prog.blur[0], prog.blur[1], prog.blur_post()
            head = [list(s) for s in steps[:p]]
            for s in head:
                s[4] ^= post                                   # the scratch channel is in the blur's frame: flips that follow the blur no longer follow these steps
            k = len(pre)
            pre.append([t, 0, k, 0, prog.flip ^ post, head])
            st.blurs.append((k, halves))
            final.append([None, 0, b, c, post, steps[p:], k])
            parts = [(n + k, head, True), (i, steps[p:], False)]
        for ri, ss, is_pre in parts:
            jobs, gamma_slot = [], None
            for k, s in enumerate(ss):
                if s[0] in (_OP_CONTRAST, _OP_GAMMA, _OP_RETAIN):
                    jobs.append((ri, k, slots, s[4]))
                    s[3] = slots
                    if s[0] == _OP_GAMMA:
                        gamma_slot = slots
                    if s[0] == _OP_RETAIN:
                        if gamma_slot is None:
                            raise ValueError("a retain-statistics step without the gamma step in front of it")
                        s[5] = gamma_slot
                    slots += 1
            if jobs:
                # a blurred record: its post-blur statistics wait for the blur; every other record starts in the first round
                (pending_post if (prog.blur is not None and not is_pre) else pending_pre).append((jobs, is_pre))
    st.records, st.n_final, st.n_slots = final + pre, n, slots
    st.n_image = sum(1 for e in entries if e[3] != AUG_LABEL)
    st.rounds_pre, st.rounds_post = [], []
    if st.blurs:
        depth = max([len(j) for j, is_pre in pending_pre if is_pre] or [0])
        st.rounds_pre = [[j[r] for j, _ in pending_pre if len(j) > r] for r in range(depth)]
        rest = [j[depth:] for j, is_pre in pending_pre if len(j) > depth] + [j for j, _ in pending_post]
    else:
        rest = [j for j, _ in pending_pre]
    st.rounds_post = [[j[r] for j in rest if len(j) > r] for r in range(max([len(j) for j in rest] or [0]))]
    ext = lambda recs: any(s[0] >= _OP_CONTRAST for r in recs for s in r[5])
    st.pre_entry = "vx_augment_batch_ext" if ext(pre) else "vx_augment_batch"
    st.final_entry = "vx_augment_batch_ext" if ext(final) else "vx_augment_batch"
    st.calls = (["vx_augment_stats"] * len(st.rounds_pre) + ([st.pre_entry, "vx_blur_batch"] if st.blurs else []) + ["vx_augment_stats"] * len(st.rounds_post)
                + [st.final_entry])
    return st


def _launch_staged(entries, x_out, y_out, B, M, spatial):
    """the staged form of _launch: ONE table (records, blur records, job lists and the statistics slots), ONE upload, then the calls of _plan in order; no device -> host
    copy and no host wait.  Statistics stay on the device."""
    st = _plan(entries)
    D, Hh, W = spatial
    V = D * Hh * W
    dev = (x_out if x_out is not None else y_out).device
    nb, nrec = len(st.blurs), len(st.records)
    rounds = st.rounds_pre + st.rounds_post
    njobs = sum(len(r) for r in rounds)
    off_blur = nrec * AUG_RECORD_BYTES
    off_jobs = off_blur + nb * BLUR_RECORD_BYTES
    off_stat = off_jobs + njobs * AUG_STAT_JOB_BYTES
    total = off_stat + st.n_slots * AUG_STAT_BYTES
    table = torch.empty(total, dtype=torch.uint8, device=dev)                       # allocated first: the records carry addresses inside it
    base = table.data_ptr()
    scratch = torch.empty((3, max(nb, 1), V), dtype=torch.float32, device=dev) if nb else None        # materialised, blurred, the blur's tmp
    host = np.zeros(total, dtype=np.uint8)
    recs = host[:off_blur].view(_REC)
    for r, rec in zip(recs, st.records):
        t, code, b, c, flip, steps = rec[:6]
        if t is None:
            r["src"], r["stride"] = scratch[1, rec[6]].data_ptr(), (Hh * W, W, 1)
        else:
            r["src"], r["stride"] = t.data_ptr(), t.stride()
        r["dtype"], r["b"], r["c"], r["flip"], r["n_steps"] = code, b, c, flip, len(steps)
        if any(s[0] >= _OP_CONTRAST for s in steps):
            r["pad"][1], r["pad"][2] = np.array([base + off_stat], dtype="<u8").view("<i4")
        for k, (op, a, sb, key, post, chan) in enumerate(steps):
            r["step"][k] = (op | (post << 4) | (chan << 8), a, sb, key)
    blur = host[off_blur:off_jobs].view(_BLUR)
    for r, (k, halves) in zip(blur, st.blurs):
        r["src"], r["dst"], r["stride"] = scratch[0, k].data_ptr(), scratch[1, k].data_ptr(), (Hh * W, W, 1)
        for a in range(3):
            r["tail"][a] = len(halves[a]) - 1
            r["w"][a, :len(halves[a])] = halves[a]
    jobs = host[off_jobs:off_stat].view(_JOB)
    jobs[:] = [j for r in rounds for j in r] or np.zeros(0, dtype=_JOB)
    table.copy_(torch.from_numpy(host), non_blocking=False)
    nchunk = (V + AUG_STAT_CHUNK - 1) // AUG_STAT_CHUNK
    widest = max([len(r) for r in rounds] or [0])
    partials = torch.empty(max(widest * nchunk * AUG_STAT_PARTIAL_BYTES, 8), dtype=torch.uint8, device=dev) if rounds else None
    stream = H.stream_ptr()
    job_at = [off_jobs]

    def stats(r):
        H.call("vx_augment_stats", base, nrec, base + job_at[0], len(r), partials.data_ptr(), partials.numel(), D, Hh, W, stream)
        job_at[0] += len(r) * AUG_STAT_JOB_BYTES
    for r in st.rounds_pre:
        stats(r)
    if nb:
        H.call(st.pre_entry, base + st.n_final * AUG_RECORD_BYTES, nb, 0, scratch[0].data_ptr(), None, 8, nb, 1, D, Hh, W, stream)
        H.call("vx_blur_batch", base + off_blur, nb, scratch[2].data_ptr(), D, Hh, W, stream)
    for r in st.rounds_post:
        stats(r)
    H.call(st.final_entry, base, st.n_image, st.n_final - st.n_image, None if x_out is None else x_out.data_ptr(), None if y_out is None else y_out.data_ptr(),
           8, B, M, D, Hh, W, stream)


def program_statistics(entries):
    """entries: [(float32 (D, H, W) CUDA view, _Program without a blur or a statistics step)], all of one shape -> a DEVICE uint8 tensor of len(entries) slots of
    AUG_STAT_BYTES bytes (_STAT: min, max, mean, std, S1, S2): the statistics of what each program gives, in the frame of the program's output, in ONE call of
    vx_augment_stats.  The low-level entry under the statistics transforms; nothing comes back to the host unless the caller copies it."""
    entries = list(entries)
    if not entries:
        raise ValueError("program_statistics: no entries")
    for i, (t, prog) in enumerate(entries):
        if not (isinstance(t, torch.Tensor) and t.is_cuda):
            raise RuntimeError(f"program_statistics: entry {i}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
        if t.dim() != 3 or 0 in t.shape or tuple(t.shape) != tuple(entries[0][0].shape):
            raise ValueError(f"program_statistics: entry {i}: expected a non-empty (D, H, W) view of the call's shape, got {tuple(t.shape)}")
        if t.dtype != torch.float32:
            raise TypeError(f"program_statistics: entry {i}: dtype {t.dtype} not supported (float32)")
        if prog.staged:
            raise ValueError(f"program_statistics: entry {i}: the program holds a blur or a statistics step")
    D, Hh, W = entries[0][0].shape
    n, dev = len(entries), entries[0][0].device
    off_jobs = n * AUG_RECORD_BYTES
    off_stat = off_jobs + n * AUG_STAT_JOB_BYTES
    table = torch.empty(off_stat + n * AUG_STAT_BYTES, dtype=torch.uint8, device=dev)
    host = np.zeros(table.numel(), dtype=np.uint8)
    recs = host[:off_jobs].view(_REC)
    recs[:] = _pack([(t, 0, 0, 0, prog) for t, prog in entries]).numpy().view(_REC)
    for r in recs:
        r["pad"][1], r["pad"][2] = np.array([table.data_ptr() + off_stat], dtype="<u8").view("<i4")
    host[off_jobs:off_stat].view(_JOB)[:] = [(i, len(prog.steps), i, 0) for i, (_, prog) in enumerate(entries)]
    table.copy_(torch.from_numpy(host))
    nchunk = (D * Hh * W + AUG_STAT_CHUNK - 1) // AUG_STAT_CHUNK
    partials = torch.empty(n * nchunk * AUG_STAT_PARTIAL_BYTES, dtype=torch.uint8, device=dev)
    H.call("vx_augment_stats", table.data_ptr(), n, table.data_ptr() + off_jobs, n, partials.data_ptr(), partials.numel(), D, Hh, W, H.stream_ptr())
    return table[off_stat:]


def _run(entries, x_out, y_out, B, M, spatial):
    """today's one call when no program needs more; the staged form otherwise"""
    if any(e[4].staged for e in entries):
        _launch_staged(entries, x_out, y_out, B, M, spatial)
    else:
        _launch(entries, x_out, y_out, B, M, spatial)


class _BatchTransform(_Randomizable):
    """common part of the four dictionary transforms below.  Draw order (modelled on MONAI 1.x, unpinned against MONAI itself, which is not installed): one RandomState
    per transform; every call draws R.rand() < prob FIRST and its parameters ONLY IF that fires; the one draw set of a call is shared by all keys of that call."""
    intensity = True
    prepares = False          # True: fold takes prepare(draw), not the draw itself

    def draw(self):
        """-> None (the call does not fire) or the parameters of this call"""
        raise NotImplementedError

    def fold(self, params, key_index, chan0, prog):
        """add what this call does to channel `chan0 + (channel within the key)` of key number `key_index` to `prog`"""
        raise NotImplementedError

    def prepare(self, params):
        """what fold takes for the parameters of one draw (made once per draw, before any GPU work); the draw itself by default"""
        return params

    def __call__(self, data):
        if isinstance(data, list):
            return [self(d) for d in data]
        params = self.draw()
        out = dict(data)
        if params is None:
            return out
        images, labels, chan0 = [], [], 0
        for ki, k in enumerate(self.keys):
            t = data[k]
            code = _check_source(t, f"{type(self).__name__}[{k!r}]", self.intensity or t.dtype == torch.float32)
            (images if code == 0 else labels).append((k, ki, chan0, t, code))
            chan0 += t.shape[0]
        spatial = {tuple(t.shape[1:]) for _, _, _, t, _ in images + labels}
        if len(spatial) != 1:
            raise ValueError(f"{type(self).__name__}: keys of different spatial shapes {sorted(spatial)} in one call")
        spatial = spatial.pop()
        if 0 in spatial:
            raise ValueError(f"{type(self).__name__}: empty spatial shape {spatial}")
        params = self.prepare(params)
        entries = []
        M = max([t.shape[0] for _, _, _, t, _ in images] or [1])           # every float32 key is one "sample" of the image output: the channels of a key stay together
        if M > 64:
            raise ValueError(f"{type(self).__name__}: {M} channels in one key (at most 64)")
        x_out = torch.empty((len(images), M) + spatial, dtype=torch.float32, device=images[0][3].device) if images else None
        nlab = sum(t.shape[0] for _, _, _, t, _ in labels)
        y_out = torch.empty((nlab, 1) + spatial, dtype=torch.int64, device=labels[0][3].device) if labels else None
        for b, (k, ki, chan0, t, code) in enumerate(images):
            for ch in range(t.shape[0]):
                prog = _Program()
                self.fold(params, ki, chan0 + ch, prog)
                entries.append((t[ch], 0, b, ch, prog))
            out[k] = x_out[b, :t.shape[0]]
        b = 0
        for k, ki, chan0, t, code in labels:
            for ch in range(t.shape[0]):
                prog = _Program()
                self.fold(params, ki, chan0 + ch, prog)
                entries.append((t[ch], code, b + ch, AUG_LABEL, prog))
            out[k] = y_out[b:b + t.shape[0], 0]
            b += t.shape[0]
        _run(entries, x_out, y_out, max(len(images), nlab, 1), M, spatial)
        return out


class RandFlipd(_BatchTransform):
    """MONAI RandFlipd(keys, prob, spatial_axis): mirror the listed spatial axes (0 = D, 1 = H, 2 = W; None = all three) of every key with probability prob.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, nothing else.  float32 keys come back as float32, bit for bit (NaN and inf included); integer keys
    (uint8, int32, int64) come back as int64 -- the value .long() gives, the label dtype of the batch."""
    intensity = False

    def __init__(self, keys, prob=0.1, spatial_axis=None):
        self.keys, self.prob, self.mask = list(keys), _prob(prob), _flip_mask(spatial_axis)
        self.set_random_state()

    def draw(self):
        return () if self.R.rand() < self.prob else None

    def fold(self, params, key_index, chan, prog):
        prog.add_flip(self.mask)


class RandScaleIntensityd(_BatchTransform):
    """MONAI RandScaleIntensityd(keys, factors, prob): v * fp32(1 + f), one fp32 multiplication.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, f = R.uniform(-factors, factors) (a pair gives low, high); one f for all keys."""

    def __init__(self, keys, factors, prob=0.1, channel_wise=False):
        if channel_wise:
            raise NotImplementedError("RandScaleIntensityd: channel_wise=True is not implemented on the HIP path")
        self.keys, self.prob, self.factors = list(keys), _prob(prob), _range(factors, "factors")
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return float(np.float32(1.0 + self.R.uniform(low=self.factors[0], high=self.factors[1])))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_MUL, params)


class RandShiftIntensityd(_BatchTransform):
    """MONAI RandShiftIntensityd(keys, offsets, prob): v + fp32(o), one fp32 addition.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, o = R.uniform(-offsets, offsets) (a pair gives low, high); one o for all keys."""

    def __init__(self, keys, offsets, prob=0.1, channel_wise=False):
        if channel_wise:
            raise NotImplementedError("RandShiftIntensityd: channel_wise=True is not implemented on the HIP path")
        self.keys, self.prob, self.offsets = list(keys), _prob(prob), _range(offsets, "offsets")
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return float(np.float32(self.R.uniform(low=self.offsets[0], high=self.offsets[1])))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_ADD, params)


class RandGaussianNoised(_BatchTransform):
    """MONAI RandGaussianNoised(keys, prob, mean, std, sample_std): v + (mean + s * n), n standard normal, independent per key and channel.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, s = R.uniform(0, std) if sample_std else std, then key = int(R.randint(2**31 - 1)).
    The normals come from the DEVICE generator (Philox4x32-7 of (key, e) under the stream AUG_NOISE_STREAM, Box-Muller; e = c * D*H*W + flat voxel index, c running
    over the channels of the keys in their listed order), not from R.normal: MONAI draws one host array per key there, so every draw AFTER this transform's
    differs from MONAI's."""

    def __init__(self, keys, prob=0.1, mean=0.0, std=0.1, sample_std=True):
        self.keys, self.prob, self.mean, self.std, self.sample_std = list(keys), _prob(prob), float(mean), float(std), bool(sample_std)
        if not (math.isfinite(self.mean) and math.isfinite(self.std)) or self.std < 0:
            raise ValueError(f"RandGaussianNoised: mean {mean!r} / std {std!r} must be finite, std >= 0")
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        s = self.R.uniform(0, self.std) if self.sample_std else self.std
        return float(np.float32(s)), int(self.R.randint(2 ** 31 - 1))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_NOISE, float(np.float32(self.mean)), params[0], params[1], chan)


# ---- blur, gamma and fixed-mean contrast (csrc/augment_blur.hip, csrc/augment_stats.hip) ---------------------------------------------------
# Modelled on MONAI 1.x (GaussianFilter(approx="erf") with zero padding, AdjustContrast, ScaleIntensityFixedMean) and UNPINNED against MONAI itself, like the transforms
# above; tests/augment_stats_ref.py restates the weights, the statistics, the three maps and the draw orders.
def gaussian_weights(sigma):
    """fp32 half vector w_0 .. w_tail of MONAI's gaussian_1d(sigma, truncated=4, approx="erf"): tail = int(max(4 sigma, 0.5) + 0.5),
    w_k = (erf((k + 1/2) / (sigma sqrt 2)) - erf((k - 1/2) / (sigma sqrt 2))) / 2, formed in fp64 and rounded once; not normalised.  0 < sigma <= 4 (tail <= 16)."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and 0.0 < sigma <= BLUR_MAX_SIGMA):
        raise ValueError(f"sigma {sigma!r} outside (0, {BLUR_MAX_SIGMA}]: the weight table holds a tail of at most {BLUR_MAX_TAIL}")
    tail = int(max(4.0 * sigma, 0.5) + 0.5)
    t = 1.0 / (sigma * math.sqrt(2.0))
    return np.array([0.5 * (math.erf((k + 0.5) * t) - math.erf((k - 0.5) * t)) for k in range(tail + 1)], dtype=np.float64).astype(np.float32)


def _half(w, what):
    """a full odd-length symmetric weight vector -> its fp32 half w_0 .. w_tail (the centre first)"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    if w.size % 2 != 1:
        raise ValueError(f"{what}: {w.size} weights: the length must be odd")
    tail = w.size // 2
    if tail > BLUR_MAX_TAIL:
        raise ValueError(f"{what}: a tail of {tail} (at most {BLUR_MAX_TAIL})")
    w32 = w.astype(np.float32)
    if not np.isfinite(w32).all():
        raise ValueError(f"{what}: weights must be finite")
    if not np.array_equal(w32, w32[::-1]):
        raise ValueError(f"{what}: the weights are not symmetric")
    return w32[tail:].copy()


def blur_separable(entries, out=None):
    """entries: [(source (D, H, W) float32 CUDA view, (wD, wH, wW))], every w an odd-length symmetric weight vector of at most 2 * 16 + 1 taps, all sources of ONE shape
    -> one contiguous (D, H, W) float32 tensor per entry, in ONE call of vx_blur_batch (three launches whatever the number of entries; the rule:
    include/veloxseg_hip.h): passes W, H, D, zeros outside the patch, y = w_0 x_0 + sum_k w_k (x_-k + x_+k) with the pair added first.  Sources may be any strided
    views (no .contiguous()).  `out`: the destinations (contiguous float32, not overlapping a source), else they are allocated.  Everything is checked before any GPU
    work; there is no CPU fallback."""
    entries = [tuple(e) for e in entries]
    if not entries:
        raise ValueError("blur_separable: no entries")
    shape, halves = None, []
    for i, e in enumerate(entries):
        if len(e) != 2:
            raise ValueError(f"blur_separable: entry {i} has {len(e)} fields (source, (wD, wH, wW))")
        src, ws = e
        if not (isinstance(src, torch.Tensor) and src.is_cuda):
            raise RuntimeError(f"blur_separable: entry {i}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
        if src.dim() != 3 or 0 in src.shape:
            raise ValueError(f"blur_separable: entry {i}: expected a non-empty (D, H, W) view, got {tuple(src.shape)}")
        if src.dtype != torch.float32:
            raise TypeError(f"blur_separable: entry {i}: dtype {src.dtype} not supported (float32)")
        shape = tuple(src.shape) if shape is None else shape
        if tuple(src.shape) != shape:
            raise ValueError(f"blur_separable: entry {i} has the shape {tuple(src.shape)}, the call {shape}")
        ws = list(ws)
        if len(ws) != 3:
            raise ValueError(f"blur_separable: entry {i}: three weight vectors (D, H, W), got {len(ws)}")
        halves.append([_half(w, f"blur_separable: entry {i} axis {a}") for a, w in enumerate(ws)])
    dev = entries[0][0].device
    if out is None:
        out = [torch.empty(shape, dtype=torch.float32, device=dev) for _ in entries]
    out = list(out)
    if len(out) != len(entries) or any(not (isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and tuple(o.shape) == shape) for o in out):
        raise ValueError(f"blur_separable: `out` must hold one contiguous float32 {shape} CUDA tensor per entry")
    for i, (src, _) in enumerate(entries):
        lo = src.data_ptr()
        hi = lo + (sum((n - 1) * abs(s) for n, s in zip(src.shape, src.stride())) + 1) * 4
        for j, o in enumerate(out):
            if o.data_ptr() < hi and lo < o.data_ptr() + o.numel() * 4:
                raise ValueError(f"blur_separable: the destination of entry {j} overlaps the source of entry {i}")
    tab = np.zeros(len(entries), dtype=_BLUR)
    for r, (src, _), o, hv in zip(tab, entries, out, halves):
        r["src"], r["dst"], r["stride"] = src.data_ptr(), o.data_ptr(), src.stride()
        for a in range(3):
            r["tail"][a] = len(hv[a]) - 1
            r["w"][a, :len(hv[a])] = hv[a]
    table = torch.from_numpy(tab.view(np.uint8).reshape(-1)).to(dev)
    tmp = torch.empty((len(entries),) + shape, dtype=torch.float32, device=dev)
    H.call("vx_blur_batch", table.data_ptr(), len(entries), tmp.data_ptr(), *shape, H.stream_ptr())
    return out


def _sigma_range(v, what):
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
        lo = hi = float(v)
    else:
        try:
            pair = [float(t) for t in v]
        except (TypeError, ValueError):
            raise ValueError(f"{what} {v!r}: a number or a pair of numbers") from None
        if len(pair) != 2:
            raise ValueError(f"{what} {v!r}: a number or a pair of numbers")
        lo, hi = (min(pair), max(pair)) if all(math.isfinite(t) for t in pair) else (float("nan"),) * 2
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo and hi <= BLUR_MAX_SIGMA):
        raise ValueError(f"{what} {v!r} outside (0, {BLUR_MAX_SIGMA}]: the weight table holds a tail of at most {BLUR_MAX_TAIL}")
    return lo, hi


class RandGaussianSmoothd(_BatchTransform):
    """MONAI RandGaussianSmoothd(keys, sigma_x, sigma_y, sigma_z, approx, prob): a separable Gaussian blur with zero padding; sigma_x is the FIRST spatial axis (D), as
    in MONAI.  Weights: gaussian_weights (erf, truncated at 4 sigma, not normalised); sigma <= 4 and approx = "erf" only.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, sigma_x, sigma_y, sigma_z = R.uniform(low, high) each; one set for all keys."""

    prepares = True

    def __init__(self, keys, sigma_x=(0.25, 1.5), sigma_y=(0.25, 1.5), sigma_z=(0.25, 1.5), approx="erf", prob=0.1):
        if approx != "erf":
            raise NotImplementedError(f"RandGaussianSmoothd: approx {approx!r} is not implemented on the HIP path (erf)")
        self.keys, self.prob = list(keys), _prob(prob)
        self.sigma = [_sigma_range(v, f"sigma_{n}") for v, n in zip((sigma_x, sigma_y, sigma_z), "xyz")]
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return tuple(float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.sigma)

    def fold(self, params, key_index, chan, prog):
        if not isinstance(params, _Weights):
            raise TypeError("RandGaussianSmoothd.fold takes the weights of its draw")
        prog.add_blur(params.halves)

    def prepare(self, params):
        return _Weights([gaussian_weights(s) for s in params])


class _Weights:
    """the three half weight vectors of one blur draw, made once per draw and shared by the keys and channels it is folded into"""

    def __init__(self, halves):
        self.halves = halves


class RandScaleIntensityFixedMeand(_BatchTransform):
    """MONAI RandScaleIntensityFixedMeand(keys, factors, fixed_mean=True, preserve_range, prob): ((v - mean) * fp32(1 + f)) + mean, then a clamp to the channel's [min, max]
    when preserve_range; every operation rounded to fp32 on its own.  mean / min / max: of the CHANNEL as it enters the step, reduced on the device.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, f = R.uniform(-factors, factors) (a pair gives low, high); one f for all keys."""

    def __init__(self, keys, factors=0, fixed_mean=True, preserve_range=False, prob=0.1, channel_wise=False):
        if not fixed_mean:
            raise NotImplementedError("RandScaleIntensityFixedMeand: fixed_mean=False is RandScaleIntensityd")
        if channel_wise:
            raise NotImplementedError("RandScaleIntensityFixedMeand: channel_wise=True (one factor per channel) is not implemented on the HIP path")
        self.keys, self.prob, self.factors, self.preserve_range = list(keys), _prob(prob), _range(factors, "factors"), bool(preserve_range)
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return float(np.float32(1.0 + self.R.uniform(low=self.factors[0], high=self.factors[1])))

    def fold(self, params, key_index, chan, prog):
        prog.add_step(_OP_CONTRAST, params, 1.0 if self.preserve_range else 0.0)


class RandAdjustContrastd(_BatchTransform):
    """MONAI RandAdjustContrastd(keys, prob, gamma, invert_image, retain_stats): v' = powf((v - min) / (r + 1e-7f), g) * r + min with r = max - min; invert_image negates the
    channel before the statistics are taken and negates the result; retain_stats then writes (v' - mean2) / (std2 + 1e-8f) * std1 + mean1 (mean1, std1 of the input, mean2,
    std2 of v').  A number g for `gamma` means (0.5, g).  The statistics are PER CHANNEL: MONAI's value for a one-channel key; for a multi-channel key MONAI's AdjustContrast
    takes min / max over the whole tensor -- a deviation.
    Draw order (MONAI 1.x, unpinned): R.rand() < prob, then, only if it fires, g = R.uniform(low, high); one g for all keys."""

    def __init__(self, keys, prob=0.1, gamma=(0.5, 4.5), invert_image=False, retain_stats=False):
        if isinstance(gamma, (int, float, np.integer, np.floating)) and not isinstance(gamma, bool):
            if gamma <= 0.5:
                raise ValueError(f"if gamma is a number, it must be greater than 0.5 and is taken as the range (0.5, gamma); got {gamma!r}")
            lo, hi = 0.5, float(gamma)
        else:
            try:
                pair = [float(t) for t in gamma]
            except (TypeError, ValueError):
                raise ValueError(f"gamma {gamma!r}: a number or a pair of numbers") from None
            if len(pair) != 2:
                raise ValueError(f"gamma should be a number or pair of numbers, got {gamma!r}")
            lo, hi = (min(pair), max(pair)) if all(math.isfinite(t) for t in pair) else (float("nan"),) * 2
        if not (math.isfinite(lo) and math.isfinite(hi)) or lo < 0:
            raise ValueError(f"gamma {gamma!r}: finite and non-negative")
        self.keys, self.prob, self.gamma, self.invert_image, self.retain_stats = list(keys), _prob(prob), (lo, hi), bool(invert_image), bool(retain_stats)
        self.set_random_state()

    def draw(self):
        if not self.R.rand() < self.prob:
            return None
        return float(np.float32(self.R.uniform(low=self.gamma[0], high=self.gamma[1])))

    def fold(self, params, key_index, chan, prog):
        if len(prog.steps) + 1 + 2 * self.invert_image + self.retain_stats > AUG_MAX_STEPS:
            raise ValueError(f"more than {AUG_MAX_STEPS} pointwise steps fired on one key: the record holds no more")
        if self.invert_image:
            prog.add_step(_OP_MUL, -1.0)
        prog.add_step(_OP_GAMMA, params)
        if self.retain_stats:
            prog.add_step(_OP_RETAIN)
        if self.invert_image:
            prog.add_step(_OP_MUL, -1.0)


class BatchAssembler:
    """the transforms above, in any order (at most one RandGaussianSmoothd), applied while the batch is assembled: samples (a list of dicts of (C, D, H, W) CUDA tensors, the output of the crop /
    rotation chain) -> (x (B, M, D, H, W) float32, y (B, 1, D, H, W) int64) with the bytes of running `transforms` as a Compose on each sample in turn and then
    torch.cat over image_keys, .long() of the label and torch.stack -- in ONE call of vx_augment_batch (one table, one upload, at most two launches).
    Draws: sample by sample, transform by transform, exactly what that Compose would draw.  Sources may be views (no .contiguous()).
    When a blur or a statistics transform FIRES in a batch, the call is staged (_plan / _launch_staged): still one table and one upload, one
    vx_augment_stats call per round of pending statistics, one materialise + vx_blur_batch pair, then the final pass; the launch count follows the deepest chain that
    fired, never B or M, and nothing comes back to the host.  When none fires, the calls and the table bytes are those of the one-pass form."""

    def __init__(self, image_keys, label_key, transforms):
        self.image_keys, self.label_key, self.transforms = list(image_keys), label_key, list(transforms)
        if not self.image_keys:
            raise ValueError("BatchAssembler: no image keys")
        known = set(self.image_keys) | {label_key}
        for t in self.transforms:
            if not isinstance(t, _BatchTransform):
                raise TypeError(f"BatchAssembler: {type(t).__name__} is not one of RandFlipd, RandScaleIntensityd, RandShiftIntensityd, RandGaussianNoised, "
                                "RandGaussianSmoothd, RandScaleIntensityFixedMeand, RandAdjustContrastd")
            if set(t.keys) - known:
                raise ValueError(f"BatchAssembler: {type(t).__name__} names keys {sorted(set(t.keys) - known)} that the batch does not hold")
            if t.intensity and label_key in t.keys:
                raise ValueError(f"BatchAssembler: {type(t).__name__} on the label key {label_key!r}")
        if sum(isinstance(t, RandGaussianSmoothd) for t in self.transforms) > 1:
            raise ValueError("BatchAssembler: more than one RandGaussianSmoothd in the transform list: a record is materialised for a blur once")

    def set_random_state(self, seed=None):
        rs = np.random.RandomState(seed)
        for t in self.transforms:
            t.set_random_state(seed=int(rs.randint(2 ** 31 - 1)))
        return self

    def __call__(self, samples):
        samples = list(samples)
        if not samples:
            raise ValueError("BatchAssembler: no samples")
        keys = self.image_keys + [self.label_key]
        spatial, device, chans = None, None, None
        for i, d in enumerate(samples):                      # every check before any GPU work
            for k in keys:
                _check_source(d[k], f"BatchAssembler: sample {i} key {k!r}", k != self.label_key)
                spatial = tuple(d[k].shape[1:]) if spatial is None else spatial
                device = d[k].device if device is None else device
                if tuple(d[k].shape[1:]) != spatial:
                    raise ValueError(f"BatchAssembler: sample {i} key {k!r} has the patch shape {tuple(d[k].shape[1:])}, the batch {spatial}")
                if d[k].device != device:
                    raise ValueError(f"BatchAssembler: sample {i} key {k!r} lives on {d[k].device}, the batch on {device}")
            if d[self.label_key].shape[0] != 1:
                raise ValueError("BatchAssembler: the label must have one channel")
            c = [d[k].shape[0] for k in self.image_keys]
            chans = c if chans is None else chans
            if c != chans:
                raise ValueError(f"BatchAssembler: sample {i} has {c} channels per image key, the batch {chans}")
        M = sum(chans)
        if 0 in spatial or not 1 <= M <= 64:
            raise ValueError(f"BatchAssembler: patch shape {spatial}, {M} channels (1..64)")
        images, labels = [], []
        for b, d in enumerate(samples):
            progs = {k: [_Program() for _ in range(d[k].shape[0])] for k in keys}
            for t in self.transforms:
                params = t.draw()
                if params is None:
                    continue
                if t.prepares:
                    params = t.prepare(params)
                chan0 = 0
                for ki, k in enumerate(t.keys):
                    for ch, prog in enumerate(progs[k]):
                        t.fold(params, ki, chan0 + ch, prog)
                    chan0 += len(progs[k])
            c = 0
            for k in self.image_keys:
                for ch, prog in enumerate(progs[k]):
                    images.append((d[k][ch], 0, b, c, prog))
                    c += 1
            labels.append((d[self.label_key][0], label_code(d[self.label_key]), b, AUG_LABEL, progs[self.label_key][0]))
        B = len(samples)
        x = torch.empty((B, M) + spatial, dtype=torch.float32, device=device)
        y = torch.empty((B, 1) + spatial, dtype=torch.int64, device=device)
        _run(images + labels, x, y, B, M, spatial)
        return x, y


_CONFIG_KEYS = ("flip_axes", "flip_prob", "scale", "scale_prob", "shift", "shift_prob", "noise_std", "noise_prob", "blur_sigma", "blur_prob", "contrast_factors",
                "contrast_prob", "contrast_preserve_range", "gamma_range", "gamma_prob", "gamma_invert", "gamma_retain_stats")


def from_config(cfg, image_keys, label_key):
    """train_config["augment"] -> BatchAssembler.  Keys (all optional; an unknown key raises ValueError): flip_axes (list of 0 = D, 1 = H, 2 = W: one RandFlipd per
    axis, each with flip_prob, default 0.5, on images and label), scale / scale_prob (RandScaleIntensityd factors, default prob 0.1), shift / shift_prob
    (RandShiftIntensityd offsets, 0.1), noise_std / noise_prob (RandGaussianNoised std with sample_std=True, 0.1), blur_sigma / blur_prob (RandGaussianSmoothd: a number
    or a (low, high) pair for all three axes, default prob 0.2), contrast_factors / contrast_prob / contrast_preserve_range (RandScaleIntensityFixedMeand, 0.15, False),
    gamma_range / gamma_prob / gamma_invert / gamma_retain_stats (RandAdjustContrastd, 0.1; gamma_invert: true puts an inverted RandAdjustContrastd in front of the plain
    one, each with gamma_prob); the order is flips, scale, shift, noise, blur, contrast, gamma."""
    if not isinstance(cfg, dict):
        raise ValueError(f"augment config must be a dict, got {type(cfg).__name__}")
    unknown = sorted(set(cfg) - set(_CONFIG_KEYS))
    if unknown:
        raise ValueError(f"augment config: unknown keys {unknown} (known: {', '.join(_CONFIG_KEYS)})")
    image_keys = list(image_keys)
    ts = []
    axes = cfg.get("flip_axes")
    if axes is not None:
        for a in ([axes] if isinstance(axes, int) else list(axes)):
            ts.append(RandFlipd(image_keys + [label_key], prob=cfg.get("flip_prob", 0.5), spatial_axis=a))
    if cfg.get("scale") is not None:
        ts.append(RandScaleIntensityd(image_keys, factors=cfg["scale"], prob=cfg.get("scale_prob", 0.1)))
    if cfg.get("shift") is not None:
        ts.append(RandShiftIntensityd(image_keys, offsets=cfg["shift"], prob=cfg.get("shift_prob", 0.1)))
    if cfg.get("noise_std") is not None:
        ts.append(RandGaussianNoised(image_keys, prob=cfg.get("noise_prob", 0.1), mean=0.0, std=cfg["noise_std"]))
    if cfg.get("blur_sigma") is not None:
        sg = cfg["blur_sigma"]
        ts.append(RandGaussianSmoothd(image_keys, sigma_x=sg, sigma_y=sg, sigma_z=sg, prob=cfg.get("blur_prob", 0.2)))
    if cfg.get("contrast_factors") is not None:
        ts.append(RandScaleIntensityFixedMeand(image_keys, factors=cfg["contrast_factors"], preserve_range=bool(cfg.get("contrast_preserve_range", False)),
                                               prob=cfg.get("contrast_prob", 0.15)))
    if cfg.get("gamma_range") is not None:
        retain = bool(cfg.get("gamma_retain_stats", False))
        if cfg.get("gamma_invert", False):
            ts.append(RandAdjustContrastd(image_keys, prob=cfg.get("gamma_prob", 0.1), gamma=cfg["gamma_range"], invert_image=True, retain_stats=retain))
        ts.append(RandAdjustContrastd(image_keys, prob=cfg.get("gamma_prob", 0.1), gamma=cfg["gamma_range"], retain_stats=retain))
    return BatchAssembler(image_keys, label_key, ts)


# ---- spatial augmentation: 3-D affine resampling of every sample, key and channel in one call (csrc/augment_affine.hip) --------------------
# Modelled on MONAI 1.x (AffineGrid's composition, RandAffined's argument names, RandomizableTransform's draw order) and UNPINNED against MONAI itself, which is not
# installed, like the transforms of section 25; tests/affine_ref.py restates the matrix and the draw order.
AFFINE_RECORD_BYTES = 144
_AFF = np.dtype([("src", "<u8"), ("dst", "<u8"), ("stride", "<i8", (3,)), ("n", "<i4", (3,)), ("lo", "<i4", (3,)), ("hi", "<i4", (3,)), ("dtype", "<i4"), ("mode", "<i4"),
                 ("pad", "<i4"), ("cval", "<f4"), ("A", "<f4", (9,)), ("c", "<f4", (3,)), ("unused", "<i4")])
assert _AFF.itemsize == AFFINE_RECORD_BYTES
_AFF_MODES = {"bilinear": 0, "trilinear": 0, "nearest": 1}
_AFF_PADS = {"border": 0, "constant": 1, "zeros": 1}
_AFF_INDEX_MAX = 1 << 24           # the kernel compares fp32 coordinates with (float)lo, (float)hi: indices must be exact in fp32


def _three(v, what):
    try:
        out = [float(t) for t in v]
    except (TypeError, ValueError):
        raise ValueError(f"{what} {v!r}: three numbers") from None
    if len(out) != 3 or not all(math.isfinite(t) for t in out):
        raise ValueError(f"{what} {v!r}: three finite numbers")
    return out


def affine_matrix(rotate=(0.0, 0.0, 0.0), scale=(1.0, 1.0, 1.0), translate=(0.0, 0.0, 0.0)):
    """fp64 (3, 4) matrix [A | t] of the map from CENTRED output coordinates to CENTRED source coordinates, s = A p + t, over the axes (D, H, W) = (x, y, z):
    MONAI 1.x AffineGrid's composition without shear, R @ T @ S with R = Rx @ Ry @ Rz (angles in radians),
        Rx = [[1, 0, 0], [0, c, -s], [0, s, c]]    Ry = [[c, 0, s], [0, 1, 0], [-s, 0, c]]    Rz = [[c, -s, 0], [s, c, 0], [0, 0, 1]]   (Rz: what vx_rotate_z does),
    T the translation by `translate` (voxels), S = diag(scale): A = R S, t = R translate.  Modelled on MONAI 1.x, unpinned against MONAI itself."""
    rx, ry, rz = _three(rotate, "rotate")
    S = np.diag(_three(scale, "scale"))
    t = np.array(_three(translate, "translate"), dtype=np.float64)
    c, s = math.cos(rx), math.sin(rx)
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, c, -s], [0.0, s, c]])
    c, s = math.cos(ry), math.sin(ry)
    Ry = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])
    c, s = math.cos(rz), math.sin(rz)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    R = Rx @ Ry @ Rz
    return np.concatenate([R @ S, (R @ t)[:, None]], axis=1)


def _affine_record(i, src, dst, matrix, mode, padding_mode, cval, bounds, seen):
    """entry i -> (the fields of its record in the order of _AFF, the byte range it may read); every check of a record's contents happens here, before the upload.
    `seen`: the matrices already checked in this call, by identity (the keys and channels of a sample share theirs)"""
    what = f"affine_sample: entry {i}"
    if not (isinstance(src, torch.Tensor) and src.is_cuda):
        raise RuntimeError(f"{what}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    if src.dim() != 3:
        raise ValueError(f"{what}: expected a (D, H, W) view, got {tuple(src.shape)}")
    if mode not in _AFF_MODES:
        raise ValueError(f"{what}: mode {mode!r} not supported (bilinear, nearest)")
    if padding_mode not in _AFF_PADS:
        raise ValueError(f"{what}: padding_mode {padding_mode!r} not supported (border, constant)")
    code = label_code(src)
    if _AFF_MODES[mode] == 0:
        if src.dtype != torch.float32:
            raise TypeError(f"{what}: mode {mode!r} on {src.dtype}: integer types take nearest only")
        code = 0
    n = [int(v) for v in src.shape]
    if 0 in n:
        raise ValueError(f"{what}: empty source {tuple(n)}")
    if id(matrix) not in seen:
        m = np.asarray(matrix, dtype=np.float64)
        if m.shape != (3, 4) or not np.isfinite(m).all():
            raise ValueError(f"{what}: the matrix must be a finite (3, 4) array")
        seen[id(matrix)] = (m[:, :3].reshape(-1), m[:, 3].tolist())
    A, t = seen[id(matrix)]
    cval = float(cval)
    if not math.isfinite(cval):
        raise ValueError(f"{what}: cval {cval!r} is not finite")
    lo, hi = ([0, 0, 0], [v - 1 for v in n]) if bounds is None else ([int(v) for v in bounds[0]], [int(v) for v in bounds[1]])
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"{what}: bounds must be (lo[3], hi[3])")
    if any(a > b for a, b in zip(lo, hi)):
        raise ValueError(f"{what}: bounds lo {lo} > hi {hi}")
    if any(abs(v) >= _AFF_INDEX_MAX for v in lo + hi + n):
        raise ValueError(f"{what}: extents / bounds beyond 2^24 are not supported")
    # the whole range [lo, hi] must lie inside the storage the view points into, and the destination must not overlap it
    st, item = list(src.stride()), src.element_size()
    if any(abs(v) > _INT_MAX for v in st):
        raise ValueError(f"{what}: strides {st} beyond 32 bits are not supported")
    first = src.storage_offset() + sum(min(a * s, b * s) for a, b, s in zip(lo, hi, st))
    last = src.storage_offset() + sum(max(a * s, b * s) for a, b, s in zip(lo, hi, st))
    if first < 0 or (last + 1) * item > src.untyped_storage().nbytes():
        raise ValueError(f"{what}: bounds lo {lo}, hi {hi} reach outside the memory the view belongs to")
    if not (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.is_contiguous() and dst.dtype == src.dtype and dst.device == src.device):
        raise ValueError(f"{what}: the destination must be a contiguous {src.dtype} tensor on {src.device}")
    base = src.data_ptr() - src.storage_offset() * item
    c = [0.5 * (n[a] - 1) + t[a] for a in range(3)]                   # formed in fp64; the table rounds it (and A) to fp32 once
    return ((src.data_ptr(), dst.data_ptr(), st, n, lo, hi, code, _AFF_MODES[mode], _AFF_PADS[padding_mode], cval, A, c, 0),
            (base + first * item, base + (last + 1) * item))


def _affine_pack(entries, out_size, out=None):
    """every check of affine_sample, then -> (the record table as a host uint8 tensor, the destinations, out_size); nothing touches the GPU but the allocation"""
    entries = [tuple(e) for e in entries]
    if not entries:
        raise ValueError("affine_sample: no entries")
    out_size = tuple(int(v) for v in out_size)
    if len(out_size) != 3 or any(v <= 0 or v >= _AFF_INDEX_MAX for v in out_size):
        raise ValueError(f"affine_sample: out_size {out_size!r} must be three positive extents")
    for i, e in enumerate(entries):
        if len(e) not in (5, 6):
            raise ValueError(f"affine_sample: entry {i} has {len(e)} fields (source, matrix, mode, padding_mode, cval[, bounds])")
        if not (isinstance(e[0], torch.Tensor) and e[0].is_cuda):
            raise RuntimeError(f"affine_sample: entry {i}: the HIP path needs a CUDA (ROCm) tensor; there is no CPU fallback")
    if out is None:
        out = [torch.empty(out_size, dtype=e[0].dtype, device=e[0].device) for e in entries]
    out = list(out)
    if len(out) != len(entries) or any(tuple(o.shape) != out_size for o in out):
        raise ValueError(f"affine_sample: `out` must hold one {out_size} tensor per entry")
    seen = {}
    recs = [_affine_record(i, e[0], o, e[1], e[2], e[3], e[4], e[5] if len(e) == 6 else None, seen) for i, (e, o) in enumerate(zip(entries, out))]
    tab = np.zeros(len(entries), dtype=_AFF)
    for f, name in enumerate(_AFF.names):                             # one assignment per field, not per record
        tab[name] = [r[0][f] for r in recs]
    # no destination may overlap what ANY record reads (the blocks of all records run side by side)
    reads = np.array([r[1] for r in recs], dtype=np.uint64)
    writes = np.array([(o.data_ptr(), o.data_ptr() + o.numel() * o.element_size()) for o in out], dtype=np.uint64)
    clash = (writes[:, None, 0] < reads[None, :, 1]) & (reads[None, :, 0] < writes[:, None, 1])
    if clash.any():
        i, j = (int(v[0]) for v in np.nonzero(clash))
        raise ValueError(f"affine_sample: the destination of entry {i} overlaps the source of entry {j}: source and destination alias")
    return torch.from_numpy(tab.view(np.uint8).reshape(-1)), out, out_size


def affine_sample(entries, out_size, out=None):
    """entries: [(source (D, H, W) CUDA view, (3, 4) matrix of affine_matrix, mode, padding_mode, cval[, bounds])] -> one (Do, Ho, Wo) tensor of the source's dtype per
    entry, out_size = (Do, Ho, Wo) for all of them, in ONE table, ONE upload, ONE call of vx_affine_batch (the rule: include/veloxseg_hip.h).  mode "bilinear"
    (float32 only) or "nearest"; padding_mode "border" or "constant" (cval outside); bounds = (lo[3], hi[3]), the valid index range in the view's coordinates (default
    0 .. n-1; -start .. parent-1-start lets a crop view read its parent).  Sources may be any strided views (no .contiguous()).  `out`: the destinations to write
    (contiguous, same dtype), else they are allocated.  Everything is checked before any GPU work; there is no CPU fallback."""
    table, out, out_size = _affine_pack(entries, out_size, out)
    table = table.to(out[0].device)
    H.call("vx_affine_batch", table.data_ptr(), len(out), *out_size, H.stream_ptr())
    return out


def _axis_ranges(v, what):
    """MONAI's reading of rotate_range / translate_range / scale_range: None -> no range; a sequence of up to three entries, one per axis (D, H, W), missing axes 0;
    an entry that is a number r means (-|r|, |r|), a pair means (min, max); a bare number is the one-entry sequence (the FIRST axis), as MONAI's ensure_tuple reads it"""
    if v is None:
        return [(0.0, 0.0)] * 3
    seq = [v] if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) else list(v)
    if len(seq) > 3:
        raise ValueError(f"{what} {v!r}: at most three entries (D, H, W)")
    return [_range(e, what) for e in seq] + [(0.0, 0.0)] * (3 - len(seq))


class RandAffined(_Randomizable):
    """MONAI RandAffined(keys, prob, rotate_range, scale_range, translate_range, spatial_size, mode, padding_mode) without shear, plus cval (the value outside under
    padding_mode="constant") and context (below).  Angles in radians about (D, H, W) = (x, y, z), translations in voxels, the scale is 1 + its draw; the matrix is
    affine_matrix(rotate, scale, translate), the map from centred output to centred source coordinates.
    Draw order (modelled on MONAI 1.x, unpinned against MONAI itself; tests/affine_ref.py restates it): one RandomState; every sample draws R.rand() < prob FIRST and
    its parameters ONLY IF that fires: three rotation uniforms (x, y, z), then three translation uniforms, then three scale uniforms, each drawn even where its range
    is zero; one draw set per sample, shared by its keys.
    Called on a dict or on a LIST of dicts (Compose hands it the list whole: takes_list), it resamples every fired sample, key and channel in ONE call of
    vx_affine_batch, straight from the tensors it is given (views are fine, nothing is copied first).  A sample that does not fire keeps its tensors and costs no
    launch (unless spatial_size differs from its shape: then it is resampled with the identity).  mode: one per key or one for all ("bilinear" float32 only,
    "nearest"); outputs keep the dtype of their source.  context=True: the samples are crop views (RandCropByPosNegLabeld(copy=False)) and the sampler may read the
    crop's parent outside the window, so a rotated patch sees the volume's real neighbours instead of clamped border values; needs the crop's `crop_start` and
    `crop_source_shape` in every sample."""
    takes_list = True

    def __init__(self, keys, prob=0.1, rotate_range=None, scale_range=None, translate_range=None, spatial_size=None, mode="bilinear", padding_mode="border", cval=0.0,
                 context=False):
        self.keys, self.prob = list(keys), _prob(prob)
        self.rotate_range, self.translate_range = _axis_ranges(rotate_range, "rotate_range"), _axis_ranges(translate_range, "translate_range")
        self.scale_range = _axis_ranges(scale_range, "scale_range")
        self.spatial_size = None if spatial_size is None else tuple(int(v) for v in spatial_size)
        if self.spatial_size is not None and (len(self.spatial_size) != 3 or min(self.spatial_size) <= 0):
            raise ValueError(f"spatial_size {spatial_size!r}: three positive extents")
        self.mode = [mode] * len(self.keys) if isinstance(mode, str) else list(mode)
        if len(self.mode) != len(self.keys):
            raise ValueError("mode must have one entry per key")
        for m in self.mode:
            if m not in _AFF_MODES:
                raise ValueError(f"mode {m!r} not supported (bilinear, nearest)")
        if padding_mode not in _AFF_PADS:
            raise ValueError(f"padding_mode {padding_mode!r} not supported (border, constant)")
        self.padding_mode, self.cval, self.context = padding_mode, float(cval), bool(context)
        self.set_random_state()

    def draw(self):
        """-> None (the sample does not fire) or (rotate[3], translate[3], scale[3])"""
        if not self.R.rand() < self.prob:
            return None
        rot = [float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.rotate_range]
        tra = [float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.translate_range]
        sca = [1.0 + float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.scale_range]
        return rot, tra, sca

    def __call__(self, data):
        if not isinstance(data, list):
            return self([data])[0]
        outs, entries, slots, out_size = [], [], [], self.spatial_size
        for i, d in enumerate(data):
            params = self.draw()
            out = dict(d)
            outs.append(out)
            if params is None and self.spatial_size is None:
                continue
            for k in self.keys:
                _need_cuda(d[k], f"RandAffined[{k!r}]")
            shapes = {tuple(d[k].shape[1:]) for k in self.keys}
            if len(shapes) != 1:
                raise ValueError(f"RandAffined: sample {i}: keys of different spatial shapes {sorted(shapes)}")
            shape = shapes.pop()
            size = self.spatial_size or shape
            if params is None and size == shape:
                continue
            if out_size is None:
                out_size = size
            if size != out_size:
                raise ValueError(f"RandAffined: sample {i} has the patch shape {shape}, the call {out_size}: set spatial_size")
            bounds = None
            if self.context:
                if "crop_start" not in d or "crop_source_shape" not in d:
                    raise ValueError("RandAffined(context=True) needs `crop_start` and `crop_source_shape` in every sample: crop with RandCropByPosNegLabeld(copy=False)")
                start, parent = [int(v) for v in d["crop_start"]], [int(v) for v in d["crop_source_shape"]]
                bounds = ([-s for s in start], [p - 1 - s for p, s in zip(parent, start)])
            m = affine_matrix() if params is None else affine_matrix(rotate=params[0], scale=params[2], translate=params[1])
            for k, mode in zip(self.keys, self.mode):
                t = d[k]
                for ch in range(t.shape[0]):
                    entries.append((t[ch], m, mode, self.padding_mode, self.cval, bounds) if bounds is not None else (t[ch], m, mode, self.padding_mode, self.cval))
                slots.append((out, k, t.shape[0], t.dtype, t.device))
        if not entries:
            return outs
        dests = [torch.empty((c,) + out_size, dtype=dt, device=dev) for _, _, c, dt, dev in slots]
        affine_sample(entries, out_size, out=[v[ch] for v in dests for ch in range(v.shape[0])])
        for (out, k, _, _, _), v in zip(slots, dests):
            out[k] = v
        return outs


# ---- elastic deformation: a device-drawn smooth displacement field and the resampler with a displacement (csrc/augment_elastic.hip) --------
# Modelled on MONAI 1.x (Rand3DElastic: uniform offsets in [-1, 1), GaussianFilter(sigma, truncated=3) with zero padding, grid += offset * magnitude, then the affine
# grid) and UNPINNED against MONAI itself, which is not installed; tests/elastic_ref.py restates the noise, the weights, the rule and the draw order.
ELASTIC_RECORD_BYTES, ELASTIC_WEIGHT_BYTES, ELASTIC_MAX_TAIL, ELASTIC_MAX_SIGMA = 160, 200, 48, 16.0
ELASTIC_STREAM = 0x454C4153544943          # VX_ELASTIC_STREAM of include/veloxseg_hip.h ("ELASTIC")
ELASTIC_ROWS, ELASTIC_TILE_W, ELASTIC_STRIP, ELASTIC_TILE_LINE = 8, 256, 32, 256          # the tiles of vx_elastic_smooth (the header's constants of the same names)
_ELA = np.dtype([("aff", _AFF), ("field", "<u8"), ("m", "<f4"), ("unused", "<i4")])
_ELW = np.dtype([("tail", "<i4"), ("w", "<f4", (ELASTIC_MAX_TAIL + 1,))])
assert (_ELA.itemsize, _ELW.itemsize) == (ELASTIC_RECORD_BYTES, ELASTIC_WEIGHT_BYTES)


def elastic_weights(sigma):
    """fp32 half vector w_0 .. w_tail of MONAI's gaussian_1d(sigma, truncated=3, approx="erf"): tail = int(max(3 sigma, 0.5) + 0.5), gaussian_weights' formula, formed in
    fp64 and rounded once; not normalised.  0 < sigma <= 16 (tail <= 48)."""
    sigma = float(sigma)
    if not (math.isfinite(sigma) and 0.0 < sigma <= ELASTIC_MAX_SIGMA):
        raise ValueError(f"sigma {sigma!r} outside (0, {ELASTIC_MAX_SIGMA}]: the weight table holds a tail of at most {ELASTIC_MAX_TAIL}")
    tail = int(max(3.0 * sigma, 0.5) + 0.5)
    t = 1.0 / (sigma * math.sqrt(2.0))
    return np.array([0.5 * (math.erf((k + 0.5) * t) - math.erf((k - 0.5) * t)) for k in range(tail + 1)], dtype=np.float64).astype(np.float32)


def _elastic_field_plan(shape, seeds, sigmas, out):
    """every check of elastic_field -> (shape, uint64 keys, the weight records, out); nothing touches the GPU but the allocation"""
    try:
        shape = tuple(int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"elastic_field: shape {shape!r} must be three positive extents") from None
    if len(shape) != 3 or any(v <= 0 for v in shape) or shape[0] * shape[1] * shape[2] > _INT_MAX:
        raise ValueError(f"elastic_field: shape {shape!r} must be three positive extents, below 2^31 voxels")
    seeds, sigmas = list(seeds), list(sigmas)
    if not seeds or len(seeds) != len(sigmas):
        raise ValueError(f"elastic_field: {len(seeds)} seeds and {len(sigmas)} sigmas: one of each per field, at least one field")
    keys = np.zeros(len(seeds), dtype="<u8")
    for i, s in enumerate(seeds):
        if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < 1 << 64:
            raise ValueError(f"elastic_field: seed {s!r} of field {i} must be an integer in [0, 2^64)")
        keys[i] = int(s)
    wts = np.zeros(len(seeds), dtype=_ELW)
    for r, s in zip(wts, sigmas):
        w = elastic_weights(s)
        r["tail"], r["w"][:w.size] = w.size - 1, w
    want = (len(seeds), 3) + shape
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == want):
        raise ValueError(f"elastic_field: `out` must be a contiguous float32 {want} CUDA tensor")
    if not torch.cuda.is_available():
        raise RuntimeError("elastic_field: the HIP path needs a CUDA (ROCm) device; there is no CPU fallback")
    return shape, keys, wts, out


def _elastic_pack(entries, out_size, out):
    """every check of elastic_sample -> (the record table as a numpy array of _ELA, the destinations, out_size): the affine part of an entry goes through _affine_pack
    (every check of affine_sample, the overlap of destinations and sources among them) and its 144 bytes are taken as they come"""
    entries = [tuple(e) for e in entries]
    try:
        size = tuple(int(v) for v in out_size)
    except (TypeError, ValueError):
        size = ()
    mags = []
    for i, e in enumerate(entries):                                  # what the record adds to an affine record first: none of it needs a device
        if len(e) not in (7, 8):
            raise ValueError(f"elastic_sample: entry {i} has {len(e)} fields (source, matrix, mode, padding_mode, cval, field, magnitude[, bounds])")
        field = e[5]
        try:
            mags.append(float(e[6]))
        except (TypeError, ValueError):
            raise ValueError(f"elastic_sample: entry {i}: magnitude {e[6]!r} is not a number") from None
        if not math.isfinite(mags[-1]):
            raise ValueError(f"elastic_sample: entry {i}: magnitude {mags[-1]!r} is not finite")
        if field is None:
            continue
        if not isinstance(field, torch.Tensor):
            raise TypeError(f"elastic_sample: entry {i}: the field must be a tensor or None, got {type(field).__name__}")
        if field.dtype != torch.float32:
            raise TypeError(f"elastic_sample: entry {i}: field dtype {field.dtype} not supported (float32)")
        if tuple(field.shape) != (3,) + size or not field.is_contiguous():
            raise ValueError(f"elastic_sample: entry {i}: the field must be a contiguous {(3,) + size} tensor, got {tuple(field.shape)} with strides {field.stride()}")
        if not field.is_cuda:
            raise RuntimeError(f"elastic_sample: entry {i}: the field must be a CUDA (ROCm) tensor; there is no CPU fallback")
    table, out, out_size = _affine_pack([e[:5] + e[7:] for e in entries], out_size, out)
    tab = np.zeros(len(entries), dtype=_ELA)
    tab["aff"] = table.numpy().view(_AFF)
    tab["m"] = mags
    writes = [(o.data_ptr(), o.data_ptr() + o.numel() * o.element_size()) for o in out]
    checked = set()
    for i, (e, r) in enumerate(zip(entries, tab)):
        field = e[5]
        if field is None:
            continue
        if field.device != e[0].device:
            raise ValueError(f"elastic_sample: entry {i}: the field lives on {field.device}, the source on {e[0].device}")
        r["field"] = field.data_ptr()
        if field.data_ptr() not in checked:                      # (the keys and channels of a sample share their field)
            checked.add(field.data_ptr())
            lo, hi = field.data_ptr(), field.data_ptr() + field.numel() * 4
            for j, (wa, wb) in enumerate(writes):
                if wa < hi and lo < wb:
                    raise ValueError(f"elastic_sample: the destination of entry {j} overlaps the field of entry {i}: field and destination alias")
    return tab, out, out_size


def _elastic_run(field_plan, sample_plan, dev):
    """ONE table (the records, the keys, the weight records), ONE upload, then vx_elastic_noise + vx_elastic_smooth for the fields of `field_plan` (or None) and
    vx_elastic_batch for the records of `sample_plan` (or None); `field_plan` carries its result tensor"""
    n_rec = 0 if sample_plan is None else len(sample_plan[0])
    n_field = 0 if field_plan is None else len(field_plan[1])
    off_keys = n_rec * ELASTIC_RECORD_BYTES
    off_wts = off_keys + n_field * 8
    host = np.zeros(off_wts + n_field * ELASTIC_WEIGHT_BYTES, dtype=np.uint8)
    if n_rec:
        host[:off_keys] = sample_plan[0].view(np.uint8).reshape(-1)
    if n_field:
        host[off_keys:off_wts] = field_plan[1].view(np.uint8)
        host[off_wts:] = field_plan[2].view(np.uint8).reshape(-1)
        scratch = torch.empty_like(field_plan[3])
    table = torch.from_numpy(host).to(dev)
    base, stream = table.data_ptr(), H.stream_ptr()
    if n_field:
        shape, result = field_plan[0], field_plan[3]
        H.call("vx_elastic_noise", base + off_keys, 3 * n_field, shape[0] * shape[1] * shape[2], scratch.data_ptr(), stream)
        H.call("vx_elastic_smooth", base + off_wts, 3 * n_field, scratch.data_ptr(), result.data_ptr(), *shape, stream)
    if n_rec:
        H.call("vx_elastic_batch", base, n_rec, *sample_plan[2], stream)


def elastic_field(shape, seeds, sigmas, out=None):
    """n smooth random displacement fields -> a (n, 3, D, H, W) float32 CUDA tensor: uniforms in [-1, 1) drawn on the DEVICE (Philox4x32-7 of (seeds[i], ELASTIC_STREAM),
    element e = plane * D*H*W + flat voxel index: include/veloxseg_hip.h) and smoothed with elastic_weights(sigmas[i]) along W, H and D with zero padding; one sigma for
    the three planes and axes of a field.  ONE vx_elastic_noise call and ONE vx_elastic_smooth call for all n fields, one table upload.  `out`: the tensor to write
    (contiguous float32), else it is allocated.  Everything is checked before any GPU work; there is no CPU fallback (RuntimeError without a device)."""
    shape, keys, wts, out = _elastic_field_plan(shape, seeds, sigmas, out)
    if out is None:
        out = torch.empty((len(keys), 3) + shape, dtype=torch.float32, device="cuda")
    _elastic_run((shape, keys, wts, out), None, out.device)
    return out


def elastic_sample(entries, out_size, out=None):
    """affine_sample with a displacement.  entries: [(source, matrix, mode, padding_mode, cval, field, magnitude[, bounds])]; `field`: a contiguous (3, Do, Ho, Wo) float32
    CUDA tensor (elastic_field's; the keys and channels of a sample share one) or None, `magnitude` a finite number: the centred output coordinate p becomes
    p + magnitude * field[:, o] BEFORE the matrix (MONAI's order); everything else is affine_sample's, checks included, and an entry whose field is None gives the bytes
    affine_sample gives.  No destination may overlap a source or a field.  ONE table, ONE upload, ONE call of vx_elastic_batch; no CPU fallback."""
    tab, out, out_size = _elastic_pack(entries, out_size, out)
    _elastic_run(None, (tab, out, out_size), out[0].device)
    return out


def _pair_range(v, what, top=None):
    """a number v -> (v, v); a pair -> (min, max); finite"""
    if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
        lo = hi = float(v)
    else:
        try:
            pair = [float(t) for t in v]
        except (TypeError, ValueError):
            raise ValueError(f"{what} {v!r}: a number or a pair of numbers") from None
        if len(pair) != 2:
            raise ValueError(f"{what} {v!r}: a number or a pair of numbers")
        lo, hi = (min(pair), max(pair)) if all(math.isfinite(t) for t in pair) else (float("nan"),) * 2
    if not (math.isfinite(lo) and math.isfinite(hi)):
        raise ValueError(f"{what} {v!r} is not finite")
    if top is not None and not (0.0 < lo and hi <= top):
        raise ValueError(f"{what} {v!r} outside (0, {top}]: the weight table holds a tail of at most {ELASTIC_MAX_TAIL}")
    return lo, hi


class Rand3DElasticd(RandAffined):
    """MONAI Rand3DElasticd(keys, sigma_range, magnitude_range, prob, rotate_range, scale_range, translate_range, spatial_size, mode, padding_mode) without shear, plus
    RandAffined's cval and context: a smooth random displacement of every output voxel, then RandAffined's matrix.  The field is elastic_field(patch shape, seed,
    sigma); a voxel samples the source at A (p + magnitude * field) + c (elastic_sample).  sigma in voxels, at most 16.
    Draw order (modelled on MONAI 1.x, unpinned against MONAI itself; tests/elastic_ref.py restates it): one RandomState; every sample draws R.rand() < prob FIRST and,
    ONLY IF that fires, seed = R.randint(2**31 - 1), magnitude = R.uniform(*magnitude_range), sigma = R.uniform(*sigma_range), then RandAffined's nine uniforms in its
    order.  The seed stands where MONAI draws the 3 D H W uniforms of the field itself on the host: the field comes from the DEVICE generator under that seed, so the
    field, and every draw after it, differ from MONAI's.
    On a list of samples: one table, one upload, ONE vx_elastic_noise, ONE vx_elastic_smooth and ONE vx_elastic_batch call for every fired sample, key and channel;
    a sample that does not fire keeps its tensors (or is resampled with the identity when spatial_size differs from its shape).  `last_draws`: what the last call
    drew, one entry per sample, None or (seed, magnitude, sigma, rotate[3], translate[3], scale[3]).
    Not implemented: shear, a coarse control grid with spline up-sampling (batchgenerators' newer form), low-resolution simulation."""

    def __init__(self, keys, sigma_range, magnitude_range, prob=0.1, rotate_range=None, scale_range=None, translate_range=None, spatial_size=None, mode="bilinear",
                 padding_mode="border", cval=0.0, context=False):
        super().__init__(keys, prob=prob, rotate_range=rotate_range, scale_range=scale_range, translate_range=translate_range, spatial_size=spatial_size, mode=mode,
                         padding_mode=padding_mode, cval=cval, context=context)
        self.sigma_range = _pair_range(sigma_range, "sigma_range", ELASTIC_MAX_SIGMA)
        self.magnitude_range = _pair_range(magnitude_range, "magnitude_range")
        self.last_draws = None

    def draw(self):
        """-> None (the sample does not fire) or (seed, magnitude, sigma, rotate[3], translate[3], scale[3])"""
        if not self.R.rand() < self.prob:
            return None
        seed = int(self.R.randint(2 ** 31 - 1))
        mag = float(self.R.uniform(low=self.magnitude_range[0], high=self.magnitude_range[1]))
        sigma = float(self.R.uniform(low=self.sigma_range[0], high=self.sigma_range[1]))
        rot = [float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.rotate_range]
        tra = [float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.translate_range]
        sca = [1.0 + float(self.R.uniform(low=lo, high=hi)) for lo, hi in self.scale_range]
        return seed, mag, sigma, rot, tra, sca

    def __call__(self, data):
        if not isinstance(data, list):
            return self([data])[0]
        outs, plans, fired, out_size, dev = [], [], [], self.spatial_size, None
        self.last_draws = []
        for i, d in enumerate(data):
            params = self.draw()
            self.last_draws.append(params)
            out = dict(d)
            outs.append(out)
            if params is None and self.spatial_size is None:
                continue
            for k in self.keys:
                _need_cuda(d[k], f"Rand3DElasticd[{k!r}]")
            shapes = {tuple(d[k].shape[1:]) for k in self.keys}
            if len(shapes) != 1:
                raise ValueError(f"Rand3DElasticd: sample {i}: keys of different spatial shapes {sorted(shapes)}")
            shape = shapes.pop()
            size = self.spatial_size or shape
            if params is None and size == shape:
                continue
            if out_size is None:
                out_size = size
            if size != out_size:
                raise ValueError(f"Rand3DElasticd: sample {i} has the patch shape {shape}, the call {out_size}: set spatial_size")
            bounds = None
            if self.context:
                if "crop_start" not in d or "crop_source_shape" not in d:
                    raise ValueError("Rand3DElasticd(context=True) needs `crop_start` and `crop_source_shape` in every sample: crop with RandCropByPosNegLabeld(copy=False)")
                start, parent = [int(v) for v in d["crop_start"]], [int(v) for v in d["crop_source_shape"]]
                bounds = ([-s for s in start], [p - 1 - s for p, s in zip(parent, start)])
            dev = d[self.keys[0]].device if dev is None else dev
            m = affine_matrix() if params is None else affine_matrix(rotate=params[3], scale=params[5], translate=params[4])
            if params is not None:
                fired.append(params)
            plans.append((out, d, m, bounds, None if params is None else (len(fired) - 1, params[1])))
        if not plans:
            return outs
        field_plan = fields = None
        if fired:
            shape, keys, wts, _ = _elastic_field_plan(out_size, [p[0] for p in fired], [p[2] for p in fired], None)
            fields = torch.empty((len(fired), 3) + shape, dtype=torch.float32, device=dev)
            field_plan = (shape, keys, wts, fields)
        entries, slots = [], []
        for out, d, m, bounds, el in plans:
            field, mag = (None, 0.0) if el is None else (fields[el[0]], el[1])
            for k, mode in zip(self.keys, self.mode):
                t = d[k]
                for ch in range(t.shape[0]):
                    entries.append((t[ch], m, mode, self.padding_mode, self.cval, field, mag) + (() if bounds is None else (bounds,)))
                slots.append((out, k, t.shape[0], t.dtype, t.device))
        dests = [torch.empty((c,) + out_size, dtype=dt, device=dv) for _, _, c, dt, dv in slots]
        tab, flat, out_size = _elastic_pack(entries, out_size, [v[ch] for v in dests for ch in range(v.shape[0])])
        _elastic_run(field_plan, (tab, flat, out_size), dev)
        for (out, k, _, _, _), v in zip(slots, dests):
            out[k] = v
        return outs


_SPATIAL_KEYS = ("rotate_degrees", "scale", "translate", "prob", "padding_mode", "context", "elastic_sigma", "elastic_magnitude")
_ELASTIC_DEFAULTS = {"elastic_sigma": (5.0, 13.0), "elastic_magnitude": (100.0, 200.0)}          # the other key's value when only one of the two is given


def spatial_from_config(cfg, keys, modes):
    """train_config["spatial_augment"] -> RandAffined.  Keys (all optional; an unknown key raises ValueError): rotate_degrees (a number: that range about each of the
    three axes; or three values, about D, H, W), scale (a number or three: the scale is 1 + U(-v, v) per axis), translate (voxels, a number or three), prob (default
    0.5, the chain's rotation probability), padding_mode ("border" default, or "constant"), context (default False: with it the crop hands views over and the
    sampler reads the volume around the patch).  With elastic_sigma and / or elastic_magnitude (each a number or a (low, high) pair; voxels, sigma at most 16; the one
    left out takes (5, 13) / (100, 200)) -> Rand3DElasticd with the same affine ranges, prob, padding_mode and context."""
    if not isinstance(cfg, dict):
        raise ValueError(f"spatial_augment config must be a dict, got {type(cfg).__name__}")
    unknown = sorted(set(cfg) - set(_SPATIAL_KEYS))
    if unknown:
        raise ValueError(f"spatial_augment config: unknown keys {unknown} (known: {', '.join(_SPATIAL_KEYS)})")

    def per_axis(v, what, f=float):
        if v is None:
            return None
        vals = [v] * 3 if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) else list(v)
        if len(vals) != 3:
            raise ValueError(f"spatial_augment config: {what} {v!r}: a number or three values")
        return [f(t) for t in vals]
    kw = dict(prob=cfg.get("prob", 0.5), rotate_range=per_axis(cfg.get("rotate_degrees"), "rotate_degrees", rotation_range_from_degrees),
              scale_range=per_axis(cfg.get("scale"), "scale"), translate_range=per_axis(cfg.get("translate"), "translate"), mode=modes,
              padding_mode=cfg.get("padding_mode", "border"), context=bool(cfg.get("context", False)))
    if cfg.get("elastic_sigma") is None and cfg.get("elastic_magnitude") is None:
        return RandAffined(keys, **kw)
    el = {k: cfg[k] if cfg.get(k) is not None else v for k, v in _ELASTIC_DEFAULTS.items()}
    return Rand3DElasticd(keys, sigma_range=el["elastic_sigma"], magnitude_range=el["elastic_magnitude"], **kw)


class Compose:
    def __init__(self, transforms):
        self.transforms = list(transforms)

    def set_random_state(self, seed=None):
        rs = np.random.RandomState(seed)
        for t in self.transforms:
            if isinstance(t, _Randomizable):
                t.set_random_state(seed=int(rs.randint(2 ** 31 - 1)))
        return self

    def __call__(self, data):
        for t in self.transforms:
            whole = isinstance(t, RandRotated) or getattr(t, "takes_list", False)          # takes_list: the transform wants the list of samples in one call
            data = [t(d) for d in data] if isinstance(data, list) and not whole else t(data)
        return data
