"""CPU side of the batch-assembly transforms (utils/augment.py: RandFlipd, RandScaleIntensityd, RandShiftIntensityd, RandGaussianNoised, BatchAssembler;
csrc/augment_batch.hip): the header symbols, the argument checks of the C-ABI entry (which answers with an error code before anything is launched -- so also on a
machine without a GPU), the draw orders against tests/intensity_ref.py, every refusal of the Python surface, and the statistics of the restated normals for the key
and size the GPU statistics test uses."""
import math

import numpy as np
import pytest
import torch

import intensity_ref as IR

SEEDS = (0, 7, 12345)
STAT_KEY, STAT_SHAPE, STAT_M = 20240229, (16, 32, 64), 3          # shared with tests/test_augment_intensity_gpu.py


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def test_header_symbols_and_constants():
    import re
    from veloxseg_amd import _hip
    A = _A()
    protos = _hip.parse_header()
    assert "vx_augment_batch" in protos
    ret, args = protos["vx_augment_batch"]
    assert ret == "int" and [n for _, n in args] == ["records", "n_image", "n_label", "x_out", "y_out", "label_bytes", "B", "M", "D", "H", "W", "stream"]
    src = open(_hip.HEADER).read()
    assert "#define VX_ABI_VERSION 1" in src
    assert int(re.search(r"#define VX_AUG_RECORD_BYTES (\d+)", src).group(1)) == A.AUG_RECORD_BYTES == A._REC.itemsize
    assert int(re.search(r"#define VX_AUG_MAX_STEPS (\d+)", src).group(1)) == A.AUG_MAX_STEPS
    assert int(re.search(r"#define VX_AUG_NOISE_STREAM (0x[0-9a-fA-F]+)ull", src).group(1), 16) == A.AUG_NOISE_STREAM == IR.NOISE_STREAM
    # the record layout the header documents
    assert {n: A._REC.fields[n][1] for n in A._REC.names} == {"src": 0, "stride": 8, "dtype": 32, "b": 36, "c": 40, "flip": 44, "n_steps": 48, "pad": 52, "step": 64}
    assert A._REC.fields["step"][0].subdtype[0].itemsize == 16
    # dropout site ids count up from 1, one per site of a model: far below the noise stream
    from veloxseg_amd import functional as VF
    VF.reset_dropout_sites()
    assert VF.new_dropout_site() == 1 and A.AUG_NOISE_STREAM > 1 << 40
    VF.reset_dropout_sites()


def test_entry_refuses_bad_arguments_without_gpu():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    ok = dict(records=4096, n_image=2, n_label=1, x_out=8192, y_out=16384, label_bytes=8, B=1, M=2, D=2, H=3, W=4)      # pointers that are never dereferenced

    def call(**kw):
        a = dict(ok, **kw)
        _hip.call("vx_augment_batch", a["records"], a["n_image"], a["n_label"], a["x_out"], a["y_out"], a["label_bytes"], a["B"], a["M"], a["D"], a["H"], a["W"], None)
    for kw in (dict(records=None), dict(x_out=None), dict(y_out=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(**kw)
    for kw in (dict(n_image=0, n_label=0), dict(n_image=-1), dict(n_label=-2), dict(n_image=-1, n_label=1)):
        with pytest.raises(RuntimeError, match="no records"):
            call(**kw)
    for kw in (dict(B=0), dict(D=0), dict(H=-1), dict(W=0)):
        with pytest.raises(RuntimeError, match="non-positive extent"):
            call(**kw)
    for m in (0, -1, 65):
        with pytest.raises(RuntimeError, match="outside 1..64"):
            call(M=m)
    for lb in (0, 1, 4, -4, 16):
        with pytest.raises(RuntimeError, match="label width"):
            call(label_bytes=lb)
    for kw in (dict(records=4100), dict(x_out=8196), dict(y_out=16392)):
        with pytest.raises(RuntimeError, match="misaligned"):
            call(**kw)
    with pytest.raises(RuntimeError, match="exceed one grid"):
        call(n_image=1 << 30, D=1 << 10, H=1 << 10, W=1 << 10)


def _classes(A, seed_of):
    """(product transform, restated draw) pairs; prob 0.5 so that calls fire and do not fire"""
    keys = ["a", "b"]
    return [
        (A.RandFlipd(keys, prob=0.5, spatial_axis=1).set_random_state(seed_of(0)), lambda R: IR.draw_flip(R, 0.5)),
        (A.RandScaleIntensityd(keys, factors=0.25, prob=0.5).set_random_state(seed_of(1)), lambda R: IR.draw_scale(R, 0.5, 0.25)),
        (A.RandScaleIntensityd(keys, factors=(-0.1, 0.4), prob=0.5).set_random_state(seed_of(2)), lambda R: IR.draw_scale(R, 0.5, (-0.1, 0.4))),
        (A.RandShiftIntensityd(keys, offsets=0.3, prob=0.5).set_random_state(seed_of(3)), lambda R: IR.draw_shift(R, 0.5, 0.3)),
        (A.RandShiftIntensityd(keys, offsets=(0.1, 0.2), prob=0.5).set_random_state(seed_of(4)), lambda R: IR.draw_shift(R, 0.5, (0.1, 0.2))),
        (A.RandGaussianNoised(keys, prob=0.5, mean=0.1, std=0.2).set_random_state(seed_of(5)), lambda R: IR.draw_noise(R, 0.5, 0.2)),
        (A.RandGaussianNoised(keys, prob=0.5, std=0.2, sample_std=False).set_random_state(seed_of(6)), lambda R: IR.draw_noise(R, 0.5, 0.2, False)),
    ]


@pytest.mark.parametrize("seed", SEEDS)
def test_draw_order_of_each_class(seed):
    A = _A()
    for k, (t, ref) in enumerate(_classes(A, lambda i: seed + i)):
        R = np.random.RandomState(seed + k)
        got = [t.draw() for _ in range(24)]
        want = [ref(R) for _ in range(24)]
        assert got == want, (type(t).__name__, k)
        assert any(g is None for g in got) and any(g is not None for g in got)
        assert t.R.rand() == R.rand()                          # nothing drawn beyond what the restatement draws


class _Recorder:
    """stands in for utils.augment._launch: keeps what would have been uploaded"""

    def __init__(self):
        self.calls = []

    def __call__(self, entries, x_out, y_out, B, M, spatial):
        self.calls.append([(b, c, prog.flip, [list(s) for s in prog.steps]) for _, _, b, c, prog in entries])


class _FakeCuda(torch.Tensor):
    """a CPU tensor that says it lives on the device: lets the host half of the assembler run here (nothing is launched: _launch is replaced)"""
    is_cuda = True


def _fake(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype).as_subclass(_FakeCuda)


@pytest.mark.parametrize("seed", SEEDS)
def test_assembler_consumes_the_draws_of_the_sequential_compose(seed, monkeypatch):
    A = _A()
    rec = _Recorder()
    monkeypatch.setattr(A, "_launch", rec)
    keys = ["a", "b"]
    mk = lambda: [A.RandFlipd(keys + ["seg"], prob=0.5, spatial_axis=0), A.RandGaussianNoised(keys, prob=0.5, std=0.1), A.RandFlipd(keys + ["seg"], prob=0.5, spatial_axis=2),
                  A.RandScaleIntensityd(keys, 0.2, prob=0.5), A.RandShiftIntensityd(["b"], 0.1, prob=0.5)]
    asm = A.BatchAssembler(keys, "seg", mk()).set_random_state(seed)
    samples = [{"a": _fake(1, 2, 3, 4), "b": _fake(1, 2, 3, 4), "seg": _fake(1, 2, 3, 4, dtype=torch.uint8)} for _ in range(5)]
    asm(samples)
    asm(samples[:2])
    # restated: the same seeds as Compose.set_random_state hands out, then sample by sample, transform by transform
    Rs = [np.random.RandomState(s) for s in IR.compose_seeds(seed, 5)]
    want = []
    for n in (5, 2):
        images, labels = [], []
        for b in range(n):
            flip = {k: 0 for k in keys + ["seg"]}
            steps = {k: [] for k in keys}
            if IR.draw_flip(Rs[0], 0.5) is not None:
                flip = {k: v ^ 1 for k, v in flip.items()}
            p = IR.draw_noise(Rs[1], 0.5, 0.1)
            if p is not None:
                for c, k in enumerate(keys):
                    steps[k].append([3, 0.0, p[0], p[1], 0, c])
            if IR.draw_flip(Rs[2], 0.5) is not None:
                flip = {k: v ^ 4 for k, v in flip.items()}
                for k in keys:
                    for s in steps[k]:
                        s[4] ^= 4
            p = IR.draw_scale(Rs[3], 0.5, 0.2)
            if p is not None:
                for k in keys:
                    steps[k].append([1, p, 0.0, 0, 0, 0])
            p = IR.draw_shift(Rs[4], 0.5, 0.1)
            if p is not None:
                steps["b"].append([2, p, 0.0, 0, 0, 0])
            images += [(b, c, flip[k], steps[k]) for c, k in enumerate(keys)]
            labels.append((b, A.AUG_LABEL, flip["seg"], []))
        want.append(images + labels)
    assert rec.calls == want
    for t, R in zip(asm.transforms, Rs):
        assert t.R.rand() == R.rand()
    # the Compose of the same transforms, seeded the same way, draws the same on each sample in turn
    comp = A.Compose(mk()).set_random_state(seed)
    asm2 = A.BatchAssembler(keys, "seg", mk()).set_random_state(seed)
    assert [[t.draw() for t in comp.transforms] for _ in range(6)] == [[t.draw() for t in asm2.transforms] for _ in range(6)]


def test_refusals_of_the_python_surface():
    A = _A()
    for cls, arg in ((A.RandScaleIntensityd, 0.1), (A.RandShiftIntensityd, 0.1)):
        with pytest.raises(NotImplementedError, match="channel_wise"):
            cls(["a"], arg, channel_wise=True)
        for bad in ((0.1, 0.2, 0.3), (), "x", None, float("nan"), (0.1, float("inf"))):
            with pytest.raises(ValueError):
                cls(["a"], bad)
    for bad in (3, -4, (0, 3), 1.5, (0, True), "w"):
        with pytest.raises(ValueError, match="spatial_axis"):
            A.RandFlipd(["a"], spatial_axis=bad)
    assert [A.RandFlipd(["a"], spatial_axis=s).mask for s in (None, 0, 1, 2, -1, (0, 2), [1, 1])] == [7, 1, 2, 4, 4, 5, 2]
    for cls, args in ((A.RandFlipd, ()), (A.RandScaleIntensityd, (0.1,)), (A.RandShiftIntensityd, (0.1,)), (A.RandGaussianNoised, ())):
        for p in (-0.1, 1.5):
            with pytest.raises(ValueError, match="prob"):
                cls(["a"], *args, prob=p)
    for kw in (dict(std=-1.0), dict(std=float("nan")), dict(mean=float("inf"))):
        with pytest.raises(ValueError, match="RandGaussianNoised"):
            A.RandGaussianNoised(["a"], **kw)
    # a non-CUDA tensor: RuntimeError from every class that fires and from the assembler, before any GPU work
    cpu = {"a": torch.zeros(1, 2, 2, 2), "seg": torch.zeros(1, 2, 2, 2, dtype=torch.uint8)}
    for t in (A.RandFlipd(["a", "seg"], prob=1.0), A.RandScaleIntensityd(["a"], 0.1, prob=1.0), A.RandShiftIntensityd(["a"], 0.1, prob=1.0), A.RandGaussianNoised(["a"], prob=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t(cpu)
        assert t.set_random_state(0) is t
    assert A.RandFlipd(["a"], prob=0.0)(cpu)["a"] is cpu["a"]                   # a call that does not fire touches nothing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.BatchAssembler(["a"], "seg", [])([cpu])
    # dtypes and shapes, on tensors that claim to be on the device (nothing is launched: every check comes first)
    f = lambda dtype=torch.float32, shape=(1, 2, 2, 4): _fake(*shape, dtype=dtype)
    for t in (A.RandScaleIntensityd(["a"], 0.1, prob=1.0), A.RandShiftIntensityd(["a"], 0.1, prob=1.0), A.RandGaussianNoised(["a"], prob=1.0)):
        for dt in (torch.float16, torch.float64, torch.int64, torch.uint8):
            with pytest.raises(TypeError, match="not supported"):
                t({"a": f(dt)})
    for dt in (torch.float16, torch.float64, torch.int16, torch.bool):
        with pytest.raises(TypeError, match="not supported"):
            A.RandFlipd(["a"], prob=1.0)({"a": f(dt)})
    with pytest.raises(ValueError, match="spatial shapes"):
        A.RandFlipd(["a", "b"], prob=1.0)({"a": f(), "b": f(shape=(1, 2, 2, 5))})
    with pytest.raises(ValueError, match=r"expected \(C, D, H, W\)"):
        A.RandFlipd(["a"], prob=1.0)({"a": _fake(2, 2, 4)})
    asm = A.BatchAssembler(["a"], "seg", [A.RandFlipd(["a", "seg"], prob=1.0)])
    good = lambda: {"a": f(), "seg": f(torch.uint8)}
    with pytest.raises(TypeError, match="not supported"):
        asm([good(), {"a": f(torch.float64), "seg": f(torch.uint8)}])
    with pytest.raises(TypeError, match="not supported"):
        asm([{"a": f(), "seg": f(torch.int16)}])
    with pytest.raises(ValueError, match="patch shape"):
        asm([good(), {"a": f(shape=(1, 2, 3, 4)), "seg": f(torch.uint8, (1, 2, 3, 4))}])
    with pytest.raises(ValueError, match="channels per image key"):
        asm([good(), {"a": f(shape=(2, 2, 2, 4)), "seg": f(torch.uint8)}])
    with pytest.raises(ValueError, match="one channel"):
        asm([{"a": f(), "seg": f(torch.uint8, (2, 2, 2, 4))}])
    with pytest.raises(ValueError, match="no samples"):
        asm([])
    with pytest.raises(TypeError, match="is not one of"):
        A.BatchAssembler(["a"], "seg", [A.RandRotated(["a"])])
    with pytest.raises(ValueError, match="does not hold"):
        A.BatchAssembler(["a"], "seg", [A.RandFlipd(["a", "zz"])])
    with pytest.raises(ValueError, match="on the label key"):
        A.BatchAssembler(["a"], "seg", [A.RandGaussianNoised(["a", "seg"])])
    with pytest.raises(ValueError, match="no image keys"):
        A.BatchAssembler([], "seg", [])
    # more than eight pointwise steps on one key
    nine = A.BatchAssembler(["a"], "seg", [A.RandShiftIntensityd(["a"], 0.1, prob=1.0) for _ in range(9)])
    with pytest.raises(ValueError, match="pointwise steps"):
        nine([good()])


def test_from_config():
    A = _A()
    with pytest.raises(ValueError, match="unknown keys"):
        A.from_config({"flip_axes": [0], "gamma": 0.3}, ["img0"], "seg")
    with pytest.raises(ValueError, match="must be a dict"):
        A.from_config([0, 1], ["img0"], "seg")
    with pytest.raises(ValueError, match="spatial_axis"):
        A.from_config({"flip_axes": [0, 3]}, ["img0"], "seg")
    assert A.from_config({}, ["img0"], "seg").transforms == []
    asm = A.from_config({"flip_axes": [0, 1, 2], "flip_prob": 0.25, "scale": 0.1, "scale_prob": 0.15, "shift": [0.0, 0.2], "shift_prob": 0.3, "noise_std": 0.05,
                         "noise_prob": 0.4}, ["img0", "img1"], "seg")
    ts = asm.transforms
    assert [type(t).__name__ for t in ts] == ["RandFlipd"] * 3 + ["RandScaleIntensityd", "RandShiftIntensityd", "RandGaussianNoised"]
    assert [t.mask for t in ts[:3]] == [1, 2, 4] and all(t.prob == 0.25 and t.keys == ["img0", "img1", "seg"] for t in ts[:3])
    assert ts[3].factors == (-0.1, 0.1) and ts[3].prob == 0.15 and ts[4].offsets == (0.0, 0.2) and ts[4].prob == 0.3
    assert ts[5].std == 0.05 and ts[5].prob == 0.4 and ts[5].sample_std and all(t.keys == ["img0", "img1"] for t in ts[3:])
    # the loader refuses an unknown key when it is built, not at the first batch
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    cfg = {"in_ch": [1, 1], "input_size": [8, 8, 8], "n_classes": 2}
    with pytest.raises(ValueError, match="unknown keys"):
        SyntheticVolumes(cfg, 2, 1, torch.device("cpu"), augment={"flips": [0]})
    assert SyntheticVolumes(cfg, 2, 1, torch.device("cpu")).assembler is None


def test_restated_normals_mapping_and_statistics():
    """the word-to-element mapping written out once more by hand for the first two counters, and the statistics of the N normals the GPU statistics test draws:
    |mean| <= 6 / sqrt N and |var - 1| <= 6 sqrt(2 / N) are six standard errors of the sample mean / variance of N unit normals; no value exceeds
    sqrt(2 * 24 * ln 2) because u1 >= 2^-24"""
    from oracle.philox import philox4x32
    w = philox4x32(np.arange(2, dtype=np.uint64), IR.NOISE_STREAM, STAT_KEY)
    n = IR.normals(STAT_KEY, 8)
    for ctr in range(2):
        for pair in range(2):
            ra, rb = int(w[ctr, 2 * pair]), int(w[ctr, 2 * pair + 1])
            u1, u2 = ((ra >> 8) + 1) / 2.0 ** 24, (rb >> 8) / 2.0 ** 24
            assert 0.0 < u1 <= 1.0 and 0.0 <= u2 < 1.0
            rad = math.sqrt(-2.0 * math.log(u1))
            assert n[4 * ctr + 2 * pair] == pytest.approx(rad * math.cos(2 * math.pi * u2), abs=1e-14)
            assert n[4 * ctr + 2 * pair + 1] == pytest.approx(rad * math.sin(2 * math.pi * u2), abs=1e-14)
    assert np.array_equal(IR.normals(STAT_KEY, 5, 3), IR.normals(STAT_KEY, 8)[3:8])            # a pure function of (key, e)
    assert np.array_equal(IR.patch_normals(STAT_KEY, 1, (1, 3, 3)).reshape(-1), IR.normals(STAT_KEY, 18)[9:])
    V = int(np.prod(STAT_SHAPE))
    N = STAT_M * V
    x = IR.normals(STAT_KEY, N)
    mean, var = float(x.mean()), float(x.var())
    print(f"N {N}: mean {mean:.3e} (bound {6 / math.sqrt(N):.3e}), var - 1 {var - 1:.3e} (bound {6 * math.sqrt(2 / N):.3e}), max |n| {np.abs(x).max():.4f}")
    assert abs(mean) <= 6.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 6.0 * math.sqrt(2.0 / N)
    assert float(np.abs(x).max()) <= IR.MAX_ABS_NORMAL * (1 + 1e-12)
