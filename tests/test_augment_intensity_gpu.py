"""GPU: the batch-assembly pass (csrc/augment_batch.hip through utils/augment.py) against tests/intensity_ref.py -- flips, scale and shift compared on BYTES with
torch.flip / one fp32 torch operation per step, the fused assembler against the same transforms called one at a time, the placement and the values of the noise,
guards around every written slot, the loader and one short training run.  Shapes are the ones at which the kernel can go wrong: W % 4 != 0 (one voxel per lane),
W % 4 == 0 (four per lane), rows that start off a 16-byte boundary, more than one block per record (4 x 4 x 64 is 256 quads; 16 x 32 x 64 is 32 blocks)."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import intensity_ref as IR
from test_augment_intensity_cpu import STAT_KEY, STAT_M, STAT_SHAPE

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

SHAPES = [(1, 1, 1), (2, 3, 1), (3, 2, 4), (2, 3, 5), (3, 5, 7), (2, 2, 8), (2, 3, 9), (4, 4, 64), (2, 2, 67)]
LABEL_DTYPES = [torch.uint8, torch.int32, torch.int64, torch.float32]
# relative to max(1, |n|) against the fp64 restatement.  Measured on an MI355X over the nine shapes and three channels below: see NOISE_MEASURED; the bar is four
# times that (the library bounds of logf / sincospif are per-function maxima, a sample sees less) and may never exceed 1e-5 (a larger error is a wrong word or
# formula, not rounding).
NOISE_MEASURED = 2.127e-7
NOISE_BAR = 4 * NOISE_MEASURED
assert NOISE_BAR <= 1e-5


def _dev():
    return torch.device("cuda", 0)


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _image(shape, seed, special=True):
    """fp32 CPU (C, D, H, W) with NaN and +-inf sprinkled in (they must pass through a flip bit for bit)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if special and x.numel() >= 4:
        f = x.view(-1)
        f[0], f[f.numel() // 2], f[-1] = float("nan"), float("inf"), float("-inf")
        f[1] = torch.tensor([0x7FC12345], dtype=torch.int32).view(torch.float32)[0]          # a NaN with a payload
    return x


def _label(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        return (torch.rand(shape, generator=g) * 9.0 - 3.0)                    # fractions and negatives: .long() truncates towards zero
    if dtype == torch.uint8:
        return torch.randint(0, 256, shape, generator=g).to(dtype)
    if dtype == torch.int32:
        return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g).to(dtype)
    return torch.randint(-2 ** 62, 2 ** 62, shape, generator=g)


def _place(t, layout):
    """CPU (C, D, H, W) -> a CUDA tensor of the same values: contiguous, or a crop view into a larger volume at W origin 3 (rows off a 16-byte boundary for the
    4-byte types) or 4 (aligned rows, strided)"""
    if layout == "contiguous":
        return t.to(_dev())
    ox = 3 if layout == "crop3" else 4
    C, D, Hh, W = t.shape
    big = torch.zeros((C, D + 2, Hh + 3, W + 8), dtype=t.dtype, device=_dev())
    view = big[:, 1:1 + D, 2:2 + Hh, ox:ox + W]
    view.copy_(t)
    return view


def _prog(A, flip=0, steps=()):
    p = A._Program()
    for s in steps:
        p.add_step(*s)
    p.add_flip(flip)           # after the steps: a noise step then carries the flip too, i.e. it was added before the mirror
    return p


def _prog_noise_last(A, flip, steps):
    p = A._Program()
    p.add_flip(flip)
    for s in steps:
        p.add_step(*s)
    return p


@pytest.mark.parametrize("layout", ["contiguous", "crop3", "crop4"])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_flips_are_torch_flip_on_bytes(si, layout):
    A = _A()
    spatial = SHAPES[si]
    M = 1 + si % 3
    src = _place(_image((M,) + spatial, 100 + si), layout)
    want_src = src.cpu()
    x = torch.full((8, M) + spatial, -7.0, device=_dev())
    entries = [(src[c], 0, mask, c, _prog(A, mask)) for mask in range(8) for c in range(M)]
    labs = [_place(_label((1,) + spatial, dt, 200 + si), layout) for dt in LABEL_DTYPES]
    y = torch.full((32, 1) + spatial, -7, dtype=torch.int64, device=_dev())
    entries += [(lab[0], A.label_code(lab), mask * 4 + k, A.AUG_LABEL, _prog(A, mask)) for mask in range(8) for k, lab in enumerate(labs)]
    A._launch(entries, x, y, 32, M, spatial)
    for mask in range(8):
        assert _same(x[mask], IR.flip(want_src, mask)), (spatial, layout, mask)
        for k, lab in enumerate(labs):
            assert _same(y[mask * 4 + k], IR.flip(lab.cpu(), mask).long()), (spatial, layout, mask, lab.dtype)


def _fma_sensitive(n, seed):
    """fp32 v, s, o for which round(round(v * s) + o) differs from the single rounding of an fma for a good share of the elements: v * s carries ~48 significant bits
    and o is of the same magnitude, so the low product bits decide the last place of the sum"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * 3.0 + 0.1
    s = float(np.float32(1.0 + 0.2371)), float(np.float32(-0.4173))
    return v, s[0], s[1]


@pytest.mark.parametrize("spatial", [(2, 3, 5), (4, 4, 64)])
def test_scale_and_shift_round_every_step(spatial):
    A = _A()
    B, M = 3, 3
    v, s, o = _fma_sensitive(B * M * int(np.prod(spatial)), 5)
    v = v.view((B, M) + spatial)
    s32, o32 = torch.tensor(s, dtype=torch.float32), torch.tensor(o, dtype=torch.float32)
    two = (v * s32) + o32
    fused = (v.double() * s32.double() + o32.double()).float()          # what a contracted fma would give (the fp64 product of two fp32 numbers is exact)
    differ = int((_bits(two) != _bits(fused)).sum())
    print(f"{spatial}: a contracted fma differs in {differ} of {v.numel()} elements")
    assert differ > 0, "the values do not tell an fma from two roundings"
    src = v.to(_dev())
    programs = {"mul": ([(1, s)], v * s32), "add": ([(2, o)], v + o32), "mul,add": ([(1, s), (2, o)], two), "add,mul": ([(2, o), (1, s)], (v + o32) * s32)}
    for name, (steps, want) in programs.items():
        for flip in (0, 5):
            x = torch.full((B, M) + spatial, -7.0, device=_dev())
            A._launch([(src[b, c], 0, b, c, _prog(A, flip, steps)) for b in range(B) for c in range(M)], x, None, B, M, spatial)
            assert _same(x, IR.flip(want, flip)), (spatial, name, flip)
    # and through the classes: R.uniform(f, f) is f
    d = {"a": src[0, :1], "b": src[0, 1:2]}
    out = A.RandShiftIntensityd(["a", "b"], (o, o), prob=1.0)(A.RandScaleIntensityd(["a", "b"], (s - 1.0, s - 1.0), prob=1.0)(d))
    f32 = torch.tensor(float(np.float32(1.0 + (s - 1.0))), dtype=torch.float32)
    assert _same(out["a"], (v[0, :1] * f32) + o32) and _same(out["b"], (v[0, 1:2] * f32) + o32)


def _transforms(A, image_keys, noise_first):
    keys = image_keys + ["seg"]
    flips = [A.RandFlipd(keys, prob=0.5, spatial_axis=a) for a in range(3)]
    rest = [A.RandScaleIntensityd(image_keys, 0.3, prob=0.7), A.RandShiftIntensityd(image_keys, 0.2, prob=0.7)]
    noise = [A.RandGaussianNoised(image_keys, prob=0.8, mean=0.05, std=0.4)]
    return noise + flips + rest if noise_first else flips + rest + noise


@pytest.mark.parametrize("noise_first", [False, True])
@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_fused_assembly_equals_the_transforms_one_at_a_time(si, noise_first):
    A = _A()
    spatial = SHAPES[si]
    M, B = 1 + si % 3, (1, 3)[si % 2]
    image_keys = [f"img{m}" for m in range(M)]
    layout = ("contiguous", "crop3", "crop4")[si % 3]
    samples = []
    for b in range(B):
        d = {k: _place(_image((1,) + spatial, 300 + 10 * b + m, special=False), layout) for m, k in enumerate(image_keys)}
        d["seg"] = _place(_label((1,) + spatial, LABEL_DTYPES[(si + b) % 4], 400 + b), layout)
        samples.append(d)
    plain_x = torch.stack([torch.cat([d[k] for k in image_keys], 0) for d in samples])
    fired = 0
    for seed in (11, 12):
        x, y = A.BatchAssembler(image_keys, "seg", _transforms(A, image_keys, noise_first)).set_random_state(seed)(samples)
        comp = A.Compose(_transforms(A, image_keys, noise_first)).set_random_state(seed)
        xs, ys = [], []
        for d in samples:
            o = d
            for t in comp.transforms:                      # the transforms called one at a time, each its own kernel call
                o = t(o)
            xs.append(torch.cat([o[k] for k in image_keys], 0))
            ys.append(o["seg"].long())
        assert x.shape == (B, M) + spatial and y.shape == (B, 1) + spatial and x.dtype == torch.float32 and y.dtype == torch.int64
        assert _same(x, torch.stack(xs)) and _same(y, torch.stack(ys)), (spatial, noise_first, seed)
        fired += int(not _same(x, plain_x))
    assert fired, "no transform fired: the comparison shows nothing"


def _noise_of(A, spatial, B, M, key, flip=0):
    """n[(b, c, v)]: the program noise(0, 1, key) on a zero image"""
    zero = torch.zeros((1,) + spatial, device=_dev())
    x = torch.full((B, M) + spatial, -7.0, device=_dev())
    A._launch([(zero[0], 0, b, c, _prog_noise_last(A, flip, [(3, 0.0, 1.0, key, c)])) for b in range(B) for c in range(M)], x, None, B, M, spatial)
    return x.cpu()


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_noise_placement_is_a_function_of_key_channel_and_voxel_only(si):
    A = _A()
    spatial = SHAPES[si]
    M, key = 3, 99991 + si
    base = _noise_of(A, spatial, 1, M, key)
    assert _same(base, _noise_of(A, spatial, 1, M, key)), "two runs differ"
    for flip in range(1, 8):
        assert _same(base, _noise_of(A, spatial, 1, M, key, flip)), (spatial, flip)
    three = _noise_of(A, spatial, 3, M, key, 6)
    for b in range(3):
        assert _same(three[b:b + 1], base), (spatial, b)
    if int(np.prod(spatial)) >= 4:
        assert not _same(base[:, 0], base[:, 1]), "channels share their noise"
    # one record per launch instead of all at once (how records are grouped into launches)
    zero = torch.zeros((1,) + spatial, device=_dev())
    x = torch.full((1, M) + spatial, -7.0, device=_dev())
    for c in range(M):
        A._launch([(zero[0], 0, 0, c, _prog_noise_last(A, 0, [(3, 0.0, 1.0, key, c)]))], x, None, 1, M, spatial)
    assert _same(x, base)
    # the stand-alone class and the assembler, seeded alike, draw the same key: same noise as the raw program with that key
    keys = [f"img{m}" for m in range(M)]
    d = {k: zero for k in keys}
    d["seg"] = torch.zeros((1,) + spatial, dtype=torch.uint8, device=_dev())
    t = A.RandGaussianNoised(keys, prob=1.0, std=1.0, sample_std=False).set_random_state(5)
    R = np.random.RandomState(5)
    std, k5 = IR.draw_noise(R, 1.0, 1.0, False)
    want = _noise_of(A, spatial, 1, M, k5)
    out = t(d)
    assert _same(torch.cat([out[k] for k in keys], 0)[None], want)
    asm = A.BatchAssembler(keys, "seg", [A.RandFlipd(keys + ["seg"], prob=1.0), A.RandGaussianNoised(keys, prob=1.0, std=1.0, sample_std=False).set_random_state(5)])
    x, _ = asm([d])
    assert _same(x, want)


@pytest.mark.parametrize("si", range(len(SHAPES)))
def test_noise_values_against_the_fp64_restatement(si):
    A = _A()
    spatial = SHAPES[si]
    M, key = 3, 4242 + 17 * si
    n = _noise_of(A, spatial, 1, M, key)[0].double().numpy()
    worst = 0.0
    for c in range(M):
        ref = IR.patch_normals(key, c, spatial)
        worst = max(worst, float(np.max(np.abs(n[c] - ref) / np.maximum(1.0, np.abs(ref)))))
    print(f"{spatial}: worst error of the device normals relative to max(1, |n|): {worst:.3e} (bar {NOISE_BAR:.3e})")
    assert worst <= NOISE_BAR


def test_noise_statistics_and_values_on_many_blocks():
    A = _A()
    n = _noise_of(A, STAT_SHAPE, 1, STAT_M, STAT_KEY)[0].double().numpy()
    ref = np.stack([IR.patch_normals(STAT_KEY, c, STAT_SHAPE) for c in range(STAT_M)])
    worst = float(np.max(np.abs(n - ref) / np.maximum(1.0, np.abs(ref))))
    N = n.size
    mean, var, top = float(n.mean()), float(n.var()), float(np.abs(n).max())
    print(f"N {N}: mean {mean:.3e} (bound {6 / math.sqrt(N):.3e}), var - 1 {var - 1:.3e} (bound {6 * math.sqrt(2 / N):.3e}), max |n| {top:.4f}, worst error {worst:.3e}")
    assert abs(mean) <= 6.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 6.0 * math.sqrt(2.0 / N)
    assert top <= IR.MAX_ABS_NORMAL * (1 + 2.0 ** -22)
    assert worst <= NOISE_BAR


@pytest.mark.parametrize("spatial", [(2, 3, 5), (3, 2, 4), (4, 4, 64)])
def test_guards_around_every_written_slot_and_refused_calls(spatial):
    A = _A()
    from veloxseg_amd import _hip
    B, M = 3, 2
    V = int(np.prod(spatial))
    G = (V + 3) // 4 * 4                                   # one record's worth, rounded up so that the batch stays 16-byte aligned
    xbuf = torch.full((2 * G + B * M * V,), -7.0, device=_dev())
    ybuf = torch.full((2 * G + B * V,), -7, dtype=torch.int64, device=_dev())
    x, y = xbuf[G:G + B * M * V].view((B, M) + spatial), ybuf[G:G + B * V].view((B, 1) + spatial)
    src = _image((1,) + spatial, 1, special=False)
    lab = _label((1,) + spatial, torch.int32, 2)
    s, l = src.to(_dev()), lab.to(_dev())
    written = [(0, 1), (1, 0), (2, 1)]                     # every written slot has an unwritten slot or a guard on each side
    entries = [(s[0], 0, b, c, _prog(A, 7)) for b, c in written]
    entries += [(s[0], 0, B, 0, _prog(A)), (s[0], 0, 0, M, _prog(A)), (s[0], 0, -1, 0, _prog(A)), (s[0], 5, 0, 0, _prog(A))]          # out of range: nothing is written
    entries += [(l[0], 4, 1, A.AUG_LABEL, _prog(A, 7)), (l[0], 4, B, A.AUG_LABEL, _prog(A)), (l[0], 3, 0, A.AUG_LABEL, _prog(A))]
    A._launch(entries, x, y, B, M, spatial)
    want_x = torch.full((B, M) + spatial, -7.0)
    for b, c in written:
        want_x[b, c] = IR.flip(src[0], 7)
    want_y = torch.full((B, 1) + spatial, -7, dtype=torch.int64)
    want_y[1, 0] = IR.flip(lab[0], 7).long()
    assert _same(x, want_x) and _same(y, want_y)
    for buf, n in ((xbuf, B * M * V), (ybuf, B * V)):
        assert bool((buf[:G] == -7).all()) and bool((buf[G + n:] == -7).all())
    # refused calls: everything stays as it is
    xb, yb = xbuf.clone(), ybuf.clone()
    table = torch.zeros(A.AUG_RECORD_BYTES * 2, dtype=torch.uint8, device=_dev())
    for args in ((table.data_ptr(), 1, 1, x.data_ptr(), y.data_ptr(), 4, B, M), (table.data_ptr(), 1, 1, x.data_ptr(), y.data_ptr(), 8, B, 0),
                 (table.data_ptr(), 0, 0, x.data_ptr(), y.data_ptr(), 8, B, M), (table.data_ptr(), 1, 1, None, y.data_ptr(), 8, B, M),
                 (None, 1, 1, x.data_ptr(), y.data_ptr(), 8, B, M), (table.data_ptr(), 1, 1, x.data_ptr(), y.data_ptr(), 8, 0, M)):
        with pytest.raises(RuntimeError, match="vx_augment_batch"):
            _hip.call("vx_augment_batch", *args, *spatial, _hip.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(xbuf, xb) and torch.equal(ybuf, yb)


AUG_CFG = {"flip_axes": [0, 1, 2], "flip_prob": 0.5, "scale": 0.1, "scale_prob": 0.5, "shift": 0.1, "shift_prob": 0.5, "noise_std": 0.1, "noise_prob": 0.5}


def test_loader_with_and_without_the_augment_config():
    from recipe import CASES
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    cfg, _ = CASES["g2_32_m2"]
    mk = lambda **kw: SyntheticVolumes(cfg, 2, 2, _dev(), volume=(72, 64, 56), **kw)
    plain = list(mk())
    none = list(mk(augment=None))
    # today's batch: the chain, then cat / .long() / stack
    ref, manual = mk(), []
    g = torch.Generator(device=_dev()).manual_seed(ref.seed)
    for _ in range(2):
        ds = ref.pipe(ref.case(g))
        manual.append((torch.stack([torch.cat([d[k] for k in ref.keys[:-1]], 0) for d in ds]), torch.stack([d["seg"].long() for d in ds])))
    for a, b, c in zip(plain, none, manual):
        assert _same(a[0], b[0]) and _same(a[1], b[1]) and _same(a[0], c[0]) and _same(a[1], c[1])
    aug = list(mk(augment=AUG_CFG))
    again = list(mk(augment=AUG_CFG))
    assert len(aug) == 2
    for (x, y), (x2, y2), (px, py) in zip(aug, again, plain):
        assert x.shape == px.shape and y.shape == py.shape and x.dtype == px.dtype and y.dtype == py.dtype and x.device == px.device
        assert _same(x, x2) and _same(y, y2)                                    # reproducible from its seed
        assert set(y.unique().tolist()) <= {0, 1} and int(y.sum()) == int(py.sum())        # mirrors move the lesion voxels, they do not make or lose any
    assert any(not _same(a[0], p[0]) for a, p in zip(aug, plain))
    # no transform configured: the assembler alone writes the plain loader's bytes
    for a, p in zip(list(mk(augment={})), plain):
        assert _same(a[0], p[0]) and _same(a[1], p[1])


def test_two_training_steps_with_the_augment_config(tmp_path):
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    from veloxseg_amd.utils.train_loop import run_train
    cfg, _ = CASES["g2_32_m2"]
    args = types.SimpleNamespace(model_name="VeloxSeg", dataset_name="AutoPETII", checkpoint_path=None, synthetic_steps=2, augment=True)
    h = run_train(args, dict(TRAIN_CFG, epochs=1, augment=AUG_CFG), {"VeloxSeg": cfg})
    assert len(h["loss"]) == 1 and math.isfinite(h["loss"][0])
    with pytest.raises(ValueError, match="unknown keys"):
        run_train(args, dict(TRAIN_CFG, epochs=1, augment={"gamma": 1.0}), {"VeloxSeg": cfg})
