"""CPU side of the blur / gamma / fixed-mean contrast transforms (utils/augment.py: RandGaussianSmoothd, RandScaleIntensityFixedMeand, RandAdjustContrastd,
blur_separable; csrc/augment_blur.hip, csrc/augment_stats.hip): the header constants against the Python layouts, the weight table, the draw
orders against tests/augment_stats_ref.py, from_config, every constructor refusal, the round / launch plan of a staged call, the blur restatement against scipy,
the bound of the GPU blur test on an fp32 emulation, and the seed of the mixed-firing GPU test."""
import math
import re

import numpy as np
import pytest
import torch

import augment_stats_ref as SR
import intensity_ref as IR
from test_augment_intensity_cpu import _fake

SEEDS = (0, 7, 12345)
SHAPES = [(3, 5, 7), (8, 12, 16), (17, 9, 20), (2, 40, 36)]          # shared with tests/test_augment_stats_gpu.py; (20, 24, 28): where several reduction blocks matter
BIG = (20, 24, 28)
SIGMAS = [(0.25, 0.25, 0.25), (1.5, 0.7, 1.1), (4.0, 2.0, 0.3)]
MIXED_SEED = 1                                                        # checked below: at prob 0.5 every new transform of both orders fires and stays silent within 3 samples


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def order(A, which, keys, prob):
    """the two transform orders of the fused-equals-one-at-a-time GPU test"""
    all_keys = keys + ["seg"]
    if which == 0:
        return [A.RandGaussianNoised(keys, prob=prob, std=0.1), A.RandGaussianSmoothd(keys, prob=prob), A.RandScaleIntensityFixedMeand(keys, factors=0.3, prob=prob),
                A.RandAdjustContrastd(keys, prob=prob, gamma=(0.5, 2.0), invert_image=True, retain_stats=True),
                A.RandAdjustContrastd(keys, prob=prob, gamma=(0.5, 2.0), retain_stats=True),
                A.RandFlipd(all_keys, prob=prob, spatial_axis=0), A.RandFlipd(all_keys, prob=prob, spatial_axis=2)]
    return [A.RandFlipd(all_keys, prob=prob, spatial_axis=1), A.RandAdjustContrastd(keys, prob=prob, gamma=(0.5, 2.0)), A.RandGaussianSmoothd(keys, prob=prob),
            A.RandShiftIntensityd(keys, offsets=0.1, prob=prob), A.RandScaleIntensityFixedMeand(keys, factors=0.3, preserve_range=True, prob=prob)]


def order_draws(which, prob):
    """[(restated draw of one call, is it one of the new transforms)] in the order of `order`"""
    blur = lambda R: SR.draw_blur(R, prob, (0.25, 1.5), (0.25, 1.5), (0.25, 1.5))
    con = lambda R: SR.draw_contrast(R, prob, 0.3)
    gam = lambda R: SR.draw_gamma(R, prob, (0.5, 2.0))
    flip = lambda R: IR.draw_flip(R, prob)
    if which == 0:
        return [(lambda R: IR.draw_noise(R, prob, 0.1), False), (blur, True), (con, True), (gam, True), (gam, True), (flip, False), (flip, False)]
    return [(flip, False), (gam, True), (blur, True), (lambda R: IR.draw_shift(R, prob, 0.1), False), (con, True)]


def test_header_constants_match_the_python_layouts():
    from veloxseg_amd import _hip
    A = _A()
    src = open(_hip.HEADER).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", src).group(1))
    assert "#define VX_ABI_VERSION 1" in src and val("VX_AUG_RECORD_BYTES") == 192 == A.AUG_RECORD_BYTES and val("VX_AUG_MAX_STEPS") == 8 == A.AUG_MAX_STEPS
    assert val("VX_AUG_STAT_BYTES") == A.AUG_STAT_BYTES == A._STAT.itemsize
    assert val("VX_AUG_STAT_JOB_BYTES") == A.AUG_STAT_JOB_BYTES == A._JOB.itemsize
    assert val("VX_AUG_STAT_PARTIAL_BYTES") == A.AUG_STAT_PARTIAL_BYTES and val("VX_AUG_STAT_CHUNK") == A.AUG_STAT_CHUNK
    assert val("VX_BLUR_RECORD_BYTES") == A.BLUR_RECORD_BYTES == A._BLUR.itemsize and val("VX_BLUR_MAX_TAIL") == A.BLUR_MAX_TAIL == SR.MAX_TAIL
    assert {n: A._STAT.fields[n][1] for n in A._STAT.names} == {"min": 0, "max": 4, "mean": 8, "std": 12, "s1": 16, "s2": 24}
    assert {n: A._JOB.fields[n][1] for n in A._JOB.names} == {"rec": 0, "upto": 4, "slot": 8, "frame": 12}
    assert {n: A._BLUR.fields[n][1] for n in A._BLUR.names} == {"src": 0, "dst": 8, "stride": 16, "tail": 40, "pad": 52, "w": 56, "pad2": 260}
    protos = _hip.parse_header()
    assert [n for _, n in protos["vx_blur_batch"][1]] == ["records", "n_records", "tmp", "D", "H", "W", "stream"]
    assert [n for _, n in protos["vx_augment_stats"][1]] == ["records", "n_records", "jobs", "n_jobs", "partials", "partial_bytes", "D", "H", "W", "stream"]
    assert protos["vx_augment_batch_ext"][1] == protos["vx_augment_batch"][1]                 # the same signature: another instantiation of the same pass
    assert (A._OP_CONTRAST, A._OP_GAMMA, A._OP_RETAIN) == (4, 5, 6)


def test_weight_table():
    A = _A()
    for sigma, tail in ((0.124, 1), (0.125, 1), (0.25, 1), (1.5, 6), (4.0, 16)):         # 4 sigma below 0.5 still gives one tap either side
        assert SR.tail_of(sigma) == tail
        half = A.gaussian_weights(sigma)
        full = SR.weights64(sigma)
        assert half.dtype == np.float32 and half.size == tail + 1 and full.size == 2 * tail + 1
        assert np.array_equal(full, full[::-1])                                                  # symmetric
        assert np.array_equal(half, full[tail:].astype(np.float32))                              # computed in fp64, rounded once
        # against the integral of the normal density over [k - 1/2, k + 1/2], written with erfc on the far side (another route to the same fp64 number)
        for k in range(tail + 1):
            want = 0.5 * (math.erfc((k - 0.5) / (sigma * math.sqrt(2))) - math.erfc((k + 0.5) / (sigma * math.sqrt(2))))
            assert full[tail + k] == pytest.approx(want, rel=1e-9, abs=1e-17)
        assert full.sum() <= 1.0 + 1e-15                                                         # not normalised: the truncated mass is simply missing
    for bad in (4.0001, 5.0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            A.gaussian_weights(bad)
    with pytest.raises(ValueError, match="sigma"):
        A.RandGaussianSmoothd(["a"], sigma_x=(0.25, 4.5))
    with pytest.raises(NotImplementedError, match="approx"):
        A.RandGaussianSmoothd(["a"], approx="sampled")


@pytest.mark.parametrize("seed", SEEDS)
def test_draw_order_of_each_class(seed):
    A = _A()
    keys = ["a", "b"]
    cases = [
        (A.RandScaleIntensityFixedMeand(keys, factors=0.25, prob=0.5), lambda R: SR.draw_contrast(R, 0.5, 0.25)),
        (A.RandScaleIntensityFixedMeand(keys, factors=(-1.5, 0.4), prob=0.5, preserve_range=True), lambda R: SR.draw_contrast(R, 0.5, (-1.5, 0.4))),
        (A.RandAdjustContrastd(keys, prob=0.5), lambda R: SR.draw_gamma(R, 0.5, (0.5, 4.5))),
        (A.RandAdjustContrastd(keys, prob=0.5, gamma=2.5, invert_image=True, retain_stats=True), lambda R: SR.draw_gamma(R, 0.5, 2.5)),
        (A.RandGaussianSmoothd(keys, prob=0.5), lambda R: SR.draw_blur(R, 0.5, (0.25, 1.5), (0.25, 1.5), (0.25, 1.5))),
        (A.RandGaussianSmoothd(keys, sigma_x=0.5, sigma_y=(1.0, 3.0), sigma_z=(0.3, 0.4), prob=0.5), lambda R: SR.draw_blur(R, 0.5, 0.5, (1.0, 3.0), (0.3, 0.4))),
    ]
    for k, (t, ref) in enumerate(cases):
        t.set_random_state(seed + k)
        R = np.random.RandomState(seed + k)
        got = [t.draw() for _ in range(24)]
        want = [ref(R) for _ in range(24)]
        assert got == want, (type(t).__name__, k)
        assert any(g is None for g in got) and any(g is not None for g in got)                   # firing and non-firing calls
        assert t.R.rand() == R.rand()                                                            # nothing drawn beyond what the restatement draws


def test_from_config_with_every_new_key():
    A = _A()
    with pytest.raises(ValueError, match="unknown keys"):
        A.from_config({"blur_sigma": 1.0, "gamma": 0.3}, ["img0"], "seg")
    with pytest.raises(ValueError, match="unknown keys"):
        A.from_config({"flips": [0]}, ["img0"], "seg")
    cfg = {"flip_axes": [0, 2], "noise_std": 0.05, "blur_sigma": [0.5, 1.0], "blur_prob": 0.2, "contrast_factors": 0.25, "contrast_prob": 0.15, "contrast_preserve_range": True,
           "gamma_range": [0.7, 1.5], "gamma_prob": 0.3, "gamma_invert": True, "gamma_retain_stats": True}
    ts = A.from_config(cfg, ["img0", "img1"], "seg").transforms
    assert [type(t).__name__ for t in ts] == ["RandFlipd", "RandFlipd", "RandGaussianNoised", "RandGaussianSmoothd", "RandScaleIntensityFixedMeand", "RandAdjustContrastd",
                                              "RandAdjustContrastd"]
    assert all(t.keys == ["img0", "img1"] for t in ts[2:])
    assert ts[3].sigma == [(0.5, 1.0)] * 3 and ts[3].prob == 0.2
    assert ts[4].factors == (-0.25, 0.25) and ts[4].prob == 0.15 and ts[4].preserve_range
    assert (ts[5].invert_image, ts[6].invert_image) == (True, False) and all(t.gamma == (0.7, 1.5) and t.prob == 0.3 and t.retain_stats for t in ts[5:])
    plain = A.from_config({"gamma_range": 2.0, "blur_sigma": 1.0}, ["img0"], "seg").transforms
    assert [type(t).__name__ for t in plain] == ["RandGaussianSmoothd", "RandAdjustContrastd"]
    assert plain[1].gamma == (0.5, 2.0) and not plain[1].invert_image and not plain[1].retain_stats and plain[1].prob == 0.1 and plain[0].sigma == [(1.0, 1.0)] * 3
    # the flips come first and get the first random states, whatever follows them
    a = A.from_config({"flip_axes": [0, 1, 2]}, ["img0"], "seg").set_random_state(9)
    b = A.from_config(dict(cfg, flip_axes=[0, 1, 2]), ["img0"], "seg").set_random_state(9)
    assert [t.R.rand() for t in a.transforms] == [t.R.rand() for t in b.transforms[:3]]


def test_constructor_refusals():
    A = _A()
    for g in (0.5, 0.2, -1.0):
        with pytest.raises(ValueError, match="gamma"):
            A.RandAdjustContrastd(["a"], gamma=g)
    for g in ((0.5, 1.0, 2.0), "x", (0.5, float("nan")), (-0.5, 1.0)):
        with pytest.raises(ValueError, match="gamma"):
            A.RandAdjustContrastd(["a"], gamma=g)
    for cls, args in ((A.RandAdjustContrastd, ()), (A.RandScaleIntensityFixedMeand, (0.1,)), (A.RandGaussianSmoothd, ())):
        for p in (-0.1, 1.5):
            with pytest.raises(ValueError, match="prob"):
                cls(["a"], *args, prob=p)
    with pytest.raises(NotImplementedError, match="fixed_mean"):
        A.RandScaleIntensityFixedMeand(["a"], 0.1, fixed_mean=False)
    with pytest.raises(NotImplementedError, match="channel_wise"):
        A.RandScaleIntensityFixedMeand(["a"], 0.1, channel_wise=True)
    for bad in ((0.1, 0.2, 0.3), "x", float("nan")):
        with pytest.raises(ValueError):
            A.RandScaleIntensityFixedMeand(["a"], bad)
    for bad in (0.0, (0.0, 1.0), (1.0, 5.0), "x", (1.0, 2.0, 3.0)):
        with pytest.raises(ValueError, match="sigma"):
            A.RandGaussianSmoothd(["a"], sigma_y=bad)
    with pytest.raises(ValueError, match="more than one RandGaussianSmoothd"):
        A.BatchAssembler(["a"], "seg", [A.RandGaussianSmoothd(["a"]), A.RandFlipd(["a", "seg"]), A.RandGaussianSmoothd(["a"])])
    with pytest.raises(TypeError, match="is not one of"):
        A.BatchAssembler(["a"], "seg", [A.RandRotated(["a"])])
    for t in (A.RandGaussianSmoothd(["a", "seg"]), A.RandAdjustContrastd(["seg"]), A.RandScaleIntensityFixedMeand(["seg"], 0.1)):
        with pytest.raises(ValueError, match="on the label key"):
            A.BatchAssembler(["a"], "seg", [t])
    # every check before any GPU work: CPU tensors, wrong dtypes on tensors that claim to be on the device
    cpu = {"a": torch.zeros(1, 2, 2, 2)}
    for t in (A.RandGaussianSmoothd(["a"], prob=1.0), A.RandAdjustContrastd(["a"], prob=1.0), A.RandScaleIntensityFixedMeand(["a"], 0.1, prob=1.0)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            t(cpu)
        with pytest.raises(TypeError, match="not supported"):
            t({"a": _fake(1, 2, 2, 4, dtype=torch.int32)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.blur_separable([(torch.zeros(2, 2, 2), ([1.0], [1.0], [1.0]))])
    f3 = _fake(2, 3, 4)
    for ws, msg in ((([1.0, 1.0], [1.0], [1.0]), "odd"), (([0.25, 0.5, 0.3], [1.0], [1.0]), "symmetric"), (([1.0], [1.0], [0.0] * 35), "tail"), (([1.0], [1.0]), "three weight")):
        with pytest.raises(ValueError, match=msg):
            A.blur_separable([(f3, ws)])
    with pytest.raises(ValueError, match="shape"):
        A.blur_separable([(f3, ([1.0], [1.0], [1.0])), (_fake(2, 3, 5), ([1.0], [1.0], [1.0]))])
    with pytest.raises(ValueError, match="no entries"):
        A.blur_separable([])
    # a ninth step still raises, also when a gamma's own steps would cross the limit
    nine = A.BatchAssembler(["a"], "seg", [A.RandAdjustContrastd(["a"], prob=1.0, invert_image=True, retain_stats=True) for _ in range(3)])
    with pytest.raises(ValueError, match="pointwise steps"):
        nine([{"a": _fake(1, 2, 2, 4), "seg": _fake(1, 2, 2, 4, dtype=torch.uint8)}])


def _entries(A, progs):
    """image entries (b = index, c = 0) and one label entry for _plan; nothing is read from the tensors"""
    t = _fake(2, 3, 4)
    return [(t, 0, i, 0, p) for i, p in enumerate(progs)] + [(t, 1, 0, A.AUG_LABEL, A._Program())]


def plan_calls(depth_pre, blur, depth_post, ext_pre, ext_final):
    """what a staged call makes: one statistics call per round, the materialise + blur pair when a blur fired, the final pass"""
    pre = "vx_augment_batch_ext" if ext_pre else "vx_augment_batch"
    fin = "vx_augment_batch_ext" if ext_final else "vx_augment_batch"
    return ["vx_augment_stats"] * depth_pre + ([pre, "vx_blur_batch"] if blur else []) + ["vx_augment_stats"] * depth_post + [fin]


def test_round_and_launch_plan():
    A = _A()
    w = [np.ones(1, np.float32)] * 3

    def prog(*what):
        p = A._Program()
        for x in what:
            if x == "blur":
                p.add_blur(w)
            elif x == "flip":
                p.add_flip(5)
            elif x == "con":
                p.add_step(A._OP_CONTRAST, 1.5)
            elif x == "gam":
                p.add_step(A._OP_GAMMA, 2.0)
            elif x == "gam+":
                p.add_step(A._OP_GAMMA, 2.0)
                p.add_step(A._OP_RETAIN)
            else:
                p.add_step(A._OP_ADD, 1.0)
        return p
    # no blur: the depth of the deepest chain, whatever the number of records
    st = A._plan(_entries(A, [prog("con"), prog("gam+", "con"), prog("add"), prog()]))
    assert st.calls == plan_calls(0, False, 3, False, True) and [len(r) for r in st.rounds_post] == [2, 1, 1] and st.n_slots == 4
    assert st.rounds_post[0] == [(0, 0, 0, 0), (1, 0, 1, 0)] and st.rounds_post[1] == [(1, 1, 2, 0)] and st.rounds_post[2] == [(1, 2, 3, 0)]
    assert st.records[1][5][1][0] == A._OP_RETAIN and st.records[1][5][1][3] == 2 and st.records[1][5][1][5] == 1        # retain: slot 2 in key, the gamma's slot 1 as slot 1
    # a blur alone: no statistics, the plain instantiation twice
    st = A._plan(_entries(A, [prog("add", "blur", "flip"), prog("flip")]))
    assert st.calls == plan_calls(0, True, 0, False, False) and len(st.blurs) == 1 and len(st.records) == 4
    assert st.records[3][:5] == [st.records[3][0], 0, 0, 0, 0] and st.records[0][0] is None and st.records[0][4] == 5 and st.records[1][4] == 5
    # statistics before and after the blur; a record without a blur starts in the first round
    progs = [prog("con", "flip", "blur", "gam+"), prog("con", "gam", "con"), prog("blur", "con")]
    st = A._plan(_entries(A, progs))
    assert st.calls == plan_calls(1, True, 2, True, True)
    assert [len(r) for r in st.rounds_pre] == [2] and [len(r) for r in st.rounds_post] == [3, 2]
    assert st.rounds_pre[0][0][:2] == (4, 0) and st.rounds_pre[0][0][3] == 5 and st.rounds_pre[0][1][0] == 1       # the pre record of entry 0 sits behind the 4 final records; its statistic: the frame in front of the flip
    # the same programs on four times the records: the same calls
    st4 = A._plan(_entries(A, progs * 4))
    assert st4.calls == st.calls
    # the pre record of a blurred channel with no statistics in front takes the plain instantiation
    st = A._plan(_entries(A, [prog("add", "blur", "con")]))
    assert st.calls == plan_calls(0, True, 1, False, True)


def test_blur_restatement_against_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(3)
    for shape in SHAPES:
        x = rng.standard_normal(shape)
        for sig in SIGMAS:
            ws = [SR.weights32(s) for s in sig]
            want = x.copy()
            for axis in (2, 1, 0):
                want = ndi.correlate1d(want, ws[axis].astype(np.float64), axis=axis, mode="constant", cval=0.0)
            got = SR.blur64(x.astype(np.float32), ws)
            want32 = x.astype(np.float32).astype(np.float64)
            for axis in (2, 1, 0):
                want32 = ndi.correlate1d(want32, ws[axis].astype(np.float64), axis=axis, mode="constant", cval=0.0)
            assert np.abs(got - want32).max() <= 1e-13 * max(1.0, np.abs(want32).max()), (shape, sig)


def test_blur_bound_on_the_fp32_emulation():
    """the bar of the GPU test, 4 (tail_max + 3) 2^-24 blur64(|x|): the fp32 rule of the kernel, with and without fma, stays below a quarter of it"""
    worst = 0.0
    for shape in SHAPES:
        for sig in SIGMAS:
            ws = [SR.weights32(s) for s in sig]
            for scale in (1.0, 1e3):
                x = blur_data(shape, scale)
                ref, bound = SR.blur64(x, ws), SR.blur_bound(x, ws)
                for fma in (True, False):
                    err = np.abs(SR.blur32(x, ws, fma).astype(np.float64) - ref)
                    ratio = float((err / np.maximum(bound, 1e-300)).max())
                    worst = max(worst, ratio)
                    assert ratio <= 0.25, (shape, sig, scale, fma, ratio)
    print(f"fp32 emulation: worst error / bound {worst:.3f}")


def blur_data(shape, scale):
    """N(0.3, 1) times scale, fp32: the data of the erf blur test"""
    rng = np.random.RandomState(int(np.prod(shape)) % 1000 + int(scale))
    return ((rng.standard_normal(shape) + 0.3) * scale).astype(np.float32)


def test_mirror_commutation_of_the_restated_rule():
    x = blur_data((3, 5, 7), 1.0)
    ws = [SR.weights32(s) for s in (1.5, 0.7, 1.1)]
    for fma in (True, False):
        for m in range(1, 8):
            assert np.array_equal(SR.blur32(SR.mirror(x, m), ws, fma), SR.mirror(SR.blur32(x, ws, fma), m))


def test_seed_of_the_mixed_firing_test():
    """on the draw restatement alone: with MIXED_SEED and prob 0.5, every NEW transform of both orders fires for at least one of the 3 samples and stays silent for at
    least one"""
    for which in (0, 1):
        draws = order_draws(which, 0.5)
        Rs = [np.random.RandomState(s) for s in SR.compose_seeds(MIXED_SEED, len(draws))]
        fired = [[fn(R) is not None for (fn, _), R in zip(draws, Rs)] for _ in range(3)]
        for k, (_, new) in enumerate(draws):
            col = [f[k] for f in fired]
            if new:
                assert any(col) and not all(col), (which, k, col)
    # and the product draws the same
    A = _A()
    for which in (0, 1):
        ts = order(A, which, ["a", "b"], 0.5)
        asm = A.BatchAssembler(["a", "b"], "seg", ts).set_random_state(MIXED_SEED)
        draws = order_draws(which, 0.5)
        Rs = [np.random.RandomState(s) for s in SR.compose_seeds(MIXED_SEED, len(draws))]
        for _ in range(3):
            assert [t.draw() for t in asm.transforms] == [fn(R) for (fn, _), R in zip(draws, Rs)]


def test_statistics_restatement():
    x = np.arange(-7, 8, dtype=np.float32).reshape(3, 5, 1)
    st = SR.Stats(x)
    assert st.as_tuple()[:3] == (-7.0, 7.0, 0.0) and st.s1 == 0.0 and st.s2 == 280.0 and st.std == np.float32(math.sqrt(280.0 / 14.0))
    t = torch.from_numpy(x)
    assert float(t.std()) == pytest.approx(float(st.std), rel=1e-6)                  # torch's unbiased std
    c = np.full((2, 2, 2), 3.25, dtype=np.float32)
    assert np.array_equal(SR.contrast32(c, 1.7, True), c)
    out, _ = SR.gamma64(c, 2.7, invert=True, retain=True)
    assert np.array_equal(out, c.astype(np.float64))                                 # a constant channel comes back as itself
