"""GPU: the separable blur, the device statistics and the three transforms built on them (csrc/augment_blur.hip, csrc/augment_stats.hip, the ops 4..6 of
csrc/augment_steps.h, through utils/augment.py) against tests/augment_stats_ref.py.  Shapes: every extent shorter than a tail-16 halo
(3, 5, 7), both W % 4 cases, more than one block per channel, and (20, 24, 28) / (8, 12, 140) where a channel has several reduction chunks.  Sources are crop views at
an odd W origin of a larger tensor; outputs carry guard bands that must stay untouched."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import augment_stats_ref as SR
from test_augment_stats_cpu import BIG, MIXED_SEED, SHAPES, SIGMAS, blur_data, order, plan_calls

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
GUARD = -12345.0
U = 2.0 ** -24                      # unit roundoff of fp32
POWF_ULP = 1                        # HIP's documented maximum error of device powf, in ulp (an ulp is at most 2 U relative)


def _dev():
    return torch.device("cuda", 0)


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def _crop(x):
    """numpy / CPU (..., D, H, W) -> a CUDA crop view of the same values at W origin 3 of a larger tensor (rows off a 16-byte boundary, strided)"""
    t = torch.as_tensor(np.ascontiguousarray(x))
    big = torch.full(tuple(t.shape[:-3]) + (t.shape[-3] + 2, t.shape[-2] + 3, t.shape[-1] + 8), 77.0, dtype=t.dtype, device=_dev())
    view = big[..., 1:1 + t.shape[-3], 2:2 + t.shape[-2], 3:3 + t.shape[-1]]
    view.copy_(t)
    return view


def _guarded(n, shape):
    """n contiguous (D, H, W) destinations inside one buffer with guard bands between and around them -> (buffer, destinations)"""
    V = int(np.prod(shape))
    buf = torch.full((n, V + 64), GUARD, device=_dev())
    return buf, [buf[i, 32:32 + V].view(shape) for i in range(n)]


def _guards_untouched(buf, V):
    return bool((buf[:, :32] == GUARD).all()) and bool((buf[:, 32 + V:] == GUARD).all())


def _ints(shape, seed, lo=-8, hi=8):
    return np.random.RandomState(seed).randint(lo, hi + 1, size=shape).astype(np.float32)


DYADIC = [np.array([0.25, 0.5, 0.25]), np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0, np.array([0.0, 1.0, 0.0])]


@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_blur_exact_on_dyadic_weights(shape):
    A = _A()
    triples = [(DYADIC[a], DYADIC[b], DYADIC[c]) for a, b, c in ((0, 1, 2), (1, 2, 0), (2, 0, 1), (1, 1, 1), (0, 0, 0))]          # a different triple per channel
    xs = [_ints(shape, 50 + i) for i in range(len(triples))]
    src = _crop(np.stack(xs))
    buf, outs = _guarded(len(triples), shape)
    got = A.blur_separable([(src[i], ws) for i, ws in enumerate(triples)], out=outs)
    for i, (x, ws) in enumerate(zip(xs, triples)):
        want = SR.blur64(x, ws)
        assert np.array_equal(got[i].cpu().numpy().astype(np.float64), want), (shape, i)
    assert _guards_untouched(buf, int(np.prod(shape)))
    assert bool((src.cpu() == torch.as_tensor(np.stack(xs))).all())                     # the sources are read only


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_erf_weights_against_fp64(shape):
    """bound: SR.blur_bound = 4 (tail_max + 3) 2^-24 times the fp64 blur of |x| (derived there); the fp32 emulation of the rule stays below 0.25 of it
    (tests/test_augment_stats_cpu.py::test_blur_bound_on_the_fp32_emulation)"""
    A = _A()
    cases = [(sig, scale) for sig in SIGMAS for scale in (1.0, 1e3)]
    xs = [blur_data(shape, scale) for _, scale in cases]
    wss = [[SR.weights32(s) for s in sig] for sig, _ in cases]
    src = _crop(np.stack(xs))
    buf, outs = _guarded(len(cases), shape)
    got = A.blur_separable([(src[i], ws) for i, ws in enumerate(wss)], out=outs)
    worst = 0.0
    for i, (x, ws) in enumerate(zip(xs, wss)):
        err = np.abs(got[i].cpu().numpy().astype(np.float64) - SR.blur64(x, ws))
        bound = SR.blur_bound(x, ws)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert (err <= bound).all(), (shape, cases[i], float((err / np.maximum(bound, 1e-300)).max()))
    print(f"blur {shape}: worst error / bound {worst:.3f}")
    assert _guards_untouched(buf, int(np.prod(shape)))


@pytest.mark.parametrize("shape", SHAPES)
def test_blur_commutes_with_every_mirror_on_bytes(shape):
    A = _A()
    x = blur_data(shape, 1.0)
    ws = [SR.weights32(s) for s in (1.5, 0.7, 1.1)]
    src = _crop(np.stack([SR.mirror(x, m) for m in range(8)]))
    got = A.blur_separable([(src[m], ws) for m in range(8)])
    plain = got[0].cpu().numpy()
    for m in range(1, 8):
        assert np.array_equal(got[m].cpu().numpy().view(np.int32), SR.mirror(plain, m).view(np.int32)), (shape, m)


def _slots(A, t):
    return t.cpu().numpy().view(A._STAT)


@pytest.mark.parametrize("shape", [(3, 5, 7), (8, 12, 140), BIG])
def test_statistics_exact_deterministic_and_independent_of_the_other_records(shape):
    """integer-valued data: the fp64 sums are exact in any order, so every field is held to ==; V = 105, 13 440 (twice: 8 x 12 x 140 and 20 x 24 x 28, four chunks)"""
    A = _A()
    xs = [_ints(shape, 70 + i, -20, 20) for i in range(8)]
    src = _crop(np.stack(xs))

    def prog(flip):
        p = A._Program()
        p.add_step(A._OP_MUL, 2.0)
        p.add_step(A._OP_ADD, 3.0)
        p.add_flip(flip)
        return p
    entries = [(src[i], prog((i * 3 + 5) % 8)) for i in range(8)]
    first = _slots(A, A.program_statistics(entries))
    second = _slots(A, A.program_statistics(entries))
    alone = _slots(A, A.program_statistics(entries[:1]))
    assert first.tobytes() == second.tobytes()                                          # bit-equal twice in a row
    assert first[:1].tobytes() == alone.tobytes()                                       # alone vs among seven other records
    for i, x in enumerate(xs):
        want = SR.Stats(2.0 * x + 3.0)
        got = tuple(float(first[i][n]) for n in ("min", "max", "mean", "std", "s1", "s2"))
        assert got == want.as_tuple(), (shape, i, got, want.as_tuple())
    # non-integer data: still the same bits twice and alone, and within fp64 rounding of the restatement
    y = _crop(np.stack([blur_data(shape, 1.0), blur_data(shape, 1e3)]))
    e2 = [(y[0], A._Program()), (y[1], prog(6))]
    a, b, c = _slots(A, A.program_statistics(e2)), _slots(A, A.program_statistics(e2)), _slots(A, A.program_statistics(e2[1:]))
    assert a.tobytes() == b.tobytes() and a[1:].tobytes() == c.tobytes()
    want = SR.Stats(blur_data(shape, 1.0))
    assert float(a[0]["min"]) == float(want.min) and float(a[0]["max"]) == float(want.max)
    assert float(a[0]["s1"]) == pytest.approx(want.s1, rel=1e-12, abs=1e-9) and float(a[0]["s2"]) == pytest.approx(want.s2, rel=1e-12)


def _one(A, t, x):
    """the transform t (prob 1) on the key 'a' = a crop view of x (C, D, H, W) -> CPU numpy (C, D, H, W)"""
    return t({"a": _crop(x)})["a"].cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_fixed_mean_contrast_equals_the_fp32_restatement(shape):
    A = _A()
    x = np.stack([_ints(shape, 90, -8, 8), _ints(shape, 91, 0, 30)])                     # two channels of one key: statistics are per channel
    for f, preserve in ((0.5, False), (-1.75, False), (1.0, True), (-1.75, True)):
        t = A.RandScaleIntensityFixedMeand(["a"], factors=(f, f), preserve_range=preserve, prob=1.0)
        got = _one(A, t, x)
        f32 = float(np.float32(1.0 + f))
        for c in range(2):
            want = SR.contrast32(x[c], f32, preserve)
            assert np.array_equal(got[c].view(np.int32), want.view(np.int32)), (shape, f, preserve, c)
        if preserve and f == 1.0:
            free = np.stack([SR.contrast32(x[c], f32, False) for c in range(2)])
            assert (free != got).any(), "the clamp is not visible"
            assert got[0].min() == x[0].min() and got[0].max() == x[0].max()


def gamma_bar(info):
    """absolute bar of the gamma map against fp64, from the operation count.  With u = (v - min) / (r + 1e-7): the subtraction, r, the denominator and the division
    are four roundings, (1 + 4U)^g <= 1 + 4 g U to first order (doubled below for the second order); powf adds POWF_ULP ulp = 2 POWF_ULP U relative; the product with r
    one more; all of these are relative to u^g r <= r.  The final addition of min rounds a value of magnitude at most amax = max(|min|, |max|)."""
    return ((8.0 * max(info["g"], 1.0) + 2.0 * POWF_ULP + 2.0) * info["r"] + 2.0 * info["amax"]) * U


def retain_bar(info):
    """bar of (v' - mean2) / (std2 + 1e-8) * std1 + mean1 against fp64.  e = gamma_bar is the error of every v'.  mean2 moves by at most e + U |mean2| (its rounding to
    fp32), std2 by at most 1.01 e + U std2 (the standard deviation is 1-Lipschitz in the largest deviation, V / (V - 1) <= 1.01), mean1 and std1 by their fp32
    rounding.  With z = (v' - mean2) / std2 and dev = max |v' - mean2|: the numerator is off by 2 e + U (|mean2| + 2 dev), the quotient in addition by
    |z| (1.01 e + 2 U std2) / std2 and its own rounding; the result is scaled by K = std1 / std2, and four more roundings act on values of magnitude at most
    |mean1| + |z| std1."""
    e = gamma_bar(info)
    K = info["s1"] / info["s2"]
    z = info["dev2"] / info["s2"]
    return K * (2.0 * e + U * (abs(info["m2"]) + 2.0 * info["dev2"])) + K * z * (1.01 * e + 3.0 * U * info["s2"]) + 6.0 * U * (abs(info["m1"]) + z * info["s1"])


GAMMA_MEASURED = {}


@pytest.mark.parametrize("g", [0.5, 1.0, 2.7, 4.5])
def test_gamma_against_fp64(g):
    A = _A()
    worst = {"plain": 0.0, "retain": 0.0}
    for shape in SHAPES + [BIG]:
        x = np.stack([blur_data(shape, 1.0), blur_data(shape, 50.0)])
        for invert in (False, True):
            for retain in (False, True):
                t = A.RandAdjustContrastd(["a"], prob=1.0, gamma=(g, g), invert_image=invert, retain_stats=retain)
                got = _one(A, t, x).astype(np.float64)
                for c in range(2):
                    want, info = SR.gamma64(x[c], g, invert, retain)
                    bar = retain_bar(info) if retain else gamma_bar(info)
                    err = float(np.abs(got[c] - want).max())
                    worst["retain" if retain else "plain"] = max(worst["retain" if retain else "plain"], err / bar)
                    assert err <= bar, (shape, g, invert, retain, c, err, bar)
                    if retain:                                   # the output keeps the input's mean and standard deviation
                        xin = x[c].astype(np.float64)
                        assert abs(got[c].mean() - xin.mean()) <= bar and abs(got[c].std(ddof=1) - xin.std(ddof=1)) <= bar, (shape, g, invert, c)
        # a constant channel comes back as itself
        const = np.full((1,) + shape, 3.25, dtype=np.float32)
        for invert, retain in ((False, False), (True, True), (False, True)):
            t = A.RandAdjustContrastd(["a"], prob=1.0, gamma=(g, g), invert_image=invert, retain_stats=retain)
            assert np.array_equal(_one(A, t, const), const), (shape, g, invert, retain)
    print(f"gamma {g}: measured maximum error / bar: plain {worst['plain']:.3f}, retain_stats {worst['retain']:.3f}")


def _samples(shape, B, keys, seed):
    out = []
    for b in range(B):
        d = {k: _crop(blur_data(shape, 1.0 + 3 * m)[None] + np.float32(b)) for m, k in enumerate(keys)}
        d["seg"] = _crop((np.random.RandomState(seed + b).rand(1, *shape) > 0.7).astype(np.uint8))
        out.append(d)
    return out


@pytest.mark.parametrize("prob,seed", [(1.0, 3), (0.5, MIXED_SEED)])
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_assembly_equals_the_transforms_one_at_a_time(shape, which, prob, seed):
    A = _A()
    keys, B = ["img0", "img1"], 3
    samples = _samples(shape, B, keys, 500)
    x, y = A.BatchAssembler(keys, "seg", order(A, which, keys, prob)).set_random_state(seed)(samples)
    comp = A.Compose(order(A, which, keys, prob)).set_random_state(seed)
    xs, ys = [], []
    for d in samples:
        o = d
        for t in comp.transforms:                                # the transforms called one at a time, each its own calls
            o = t(o)
        xs.append(torch.cat([o[k] for k in keys], 0))
        ys.append(o["seg"].long())
    assert x.shape == (B, 2) + shape and y.shape == (B, 1) + shape and x.dtype == torch.float32 and y.dtype == torch.int64
    assert _same(x, torch.stack(xs)) and _same(y, torch.stack(ys)), (shape, which, prob)
    assert bool(torch.isfinite(x).all())
    plain = torch.stack([torch.cat([d[k] for k in keys], 0) for d in samples])
    assert not _same(x, plain), "no transform fired: the comparison shows nothing"


def _record_calls(monkeypatch):
    from veloxseg_amd import _hip as H
    calls = []
    real = H.call
    monkeypatch.setattr(H, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


def test_calls_of_a_batch(monkeypatch):
    A = _A()
    keys, shape = ["img0", "img1"], (8, 12, 16)
    calls = _record_calls(monkeypatch)
    # nothing new firing: today's one call and today's table bytes
    packed = []
    launch = A._launch
    monkeypatch.setattr(A, "_launch", lambda entries, *a: (packed.append((entries, A._pack(entries).numpy().copy())), launch(entries, *a))[1])
    ts = [A.RandFlipd(keys + ["seg"], prob=1.0, spatial_axis=2), A.RandShiftIntensityd(keys, (0.25, 0.25), prob=1.0)] + order(A, 0, keys, 0.0)[1:5]
    samples = _samples(shape, 2, keys, 600)
    A.BatchAssembler(keys, "seg", ts).set_random_state(1)(samples)
    assert calls == ["vx_augment_batch"]
    entries, table = packed[0]
    want = np.zeros(len(entries), dtype=A._REC)
    for r, (t, code, b, c, prog) in zip(want, entries):
        r["src"], r["stride"], r["dtype"], r["b"], r["c"], r["flip"] = t.data_ptr(), t.stride(), code, b, c, 4
        if c != A.AUG_LABEL:
            r["n_steps"], r["step"][0] = 1, (2, 0.25, 0.0, 0)
    assert table.tobytes() == want.tobytes() and not table.reshape(-1, A.AUG_RECORD_BYTES)[:, 52:64].any()
    # everything firing: the plan of the CPU test, the same for B = 1 and B = 4
    for which, plan in ((0, plan_calls(0, True, 5, False, True)), (1, plan_calls(1, True, 1, True, True))):
        lists = []
        for B in (1, 4):
            calls.clear()
            A.BatchAssembler(keys, "seg", order(A, which, keys, 1.0)).set_random_state(2)(_samples(shape, B, keys, 600))
            lists.append(list(calls))
        assert lists[0] == lists[1] == plan, (which, lists)


def test_refused_calls_leave_the_outputs_untouched(monkeypatch):
    A = _A()
    from veloxseg_amd import _hip as H
    shape = (3, 5, 7)
    V = int(np.prod(shape))
    src = _crop(_ints(shape, 5))
    buf, outs = _guarded(1, shape)
    outs[0].fill_(GUARD)
    one = np.array([1.0])
    calls = _record_calls(monkeypatch)
    for ws, msg in (((np.ones(35) / 35, one, one), "tail"), ((np.array([0.5, 0.5]), one, one), "odd"), ((np.array([0.25, 0.5, 0.3]), one, one), "symmetric")):
        with pytest.raises(ValueError, match=msg):
            A.blur_separable([(src, ws)], out=outs)
    with pytest.raises(ValueError, match="overlaps"):
        A.blur_separable([(outs[0], (one, one, one))], out=outs)
    assert calls == []                                                                   # refused before any call
    tab = torch.zeros(A.BLUR_RECORD_BYTES + 8, dtype=torch.uint8, device=_dev())
    tmp = torch.empty(V, device=_dev())
    st = H.stream_ptr()
    ok = dict(records=tab.data_ptr(), n=1, tmp=tmp.data_ptr(), D=3, H=5, W=7)
    for kw, msg in ((dict(records=None), "null pointer"), (dict(tmp=None), "null pointer"), (dict(n=0), "no records"), (dict(D=0), "non-positive extent"),
                    (dict(W=-1), "non-positive extent"), (dict(records=tab.data_ptr() + 4), "misaligned")):
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=msg):
            H.call("vx_blur_batch", a["records"], a["n"], a["tmp"], a["D"], a["H"], a["W"], st)
    part = torch.empty(64, dtype=torch.uint8, device=_dev())
    ok = dict(records=tab.data_ptr(), n_records=1, jobs=tab.data_ptr() + 8, n_jobs=1, partials=part.data_ptr(), nbytes=64, D=3, H=5, W=7)
    for kw, msg in ((dict(records=None), "null pointer"), (dict(jobs=None), "null pointer"), (dict(partials=None), "null pointer"), (dict(n_jobs=0), "no records or no jobs"),
                    (dict(H=0), "non-positive extent"), (dict(jobs=tab.data_ptr() + 4), "misaligned"), (dict(nbytes=16), "partials hold")):
        a = dict(ok, **kw)
        with pytest.raises(RuntimeError, match=msg):
            H.call("vx_augment_stats", a["records"], a["n_records"], a["jobs"], a["n_jobs"], a["partials"], a["nbytes"], a["D"], a["H"], a["W"], st)
    # a table of zeros: records without pointers / a job whose record has no statistics table write nothing
    H.call("vx_blur_batch", tab.data_ptr(), 1, tmp.data_ptr(), 3, 5, 7, st)
    H.call("vx_augment_stats", tab.data_ptr(), 1, tab.data_ptr() + 8, 1, part.data_ptr(), 64, 3, 5, 7, st)
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all()) and not bool(tab.any())
    # the Python surface on real device tensors: every check before any call
    calls.clear()
    with pytest.raises(TypeError, match="not supported"):
        A.RandGaussianSmoothd(["a"], prob=1.0)({"a": src[None].double()})
    two = [A.RandGaussianSmoothd(["a"], prob=1.0), A.RandGaussianSmoothd(["a"], prob=1.0)]
    with pytest.raises(ValueError, match="more than one RandGaussianSmoothd"):
        A.BatchAssembler(["a"], "seg", two)
    assert calls == []


AUG_CFG = {"flip_axes": [0, 1, 2], "flip_prob": 0.5}
NEW_CFG = dict(AUG_CFG, noise_std=0.1, noise_prob=0.5, blur_sigma=[0.5, 1.5], blur_prob=0.5, contrast_factors=0.25, contrast_prob=0.5, contrast_preserve_range=True,
               gamma_range=[0.7, 1.5], gamma_prob=0.5, gamma_invert=True, gamma_retain_stats=True)


def test_loader_with_the_new_keys():
    from recipe import CASES
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    cfg, _ = CASES["g2_32_m2"]
    mk = lambda aug: list(SyntheticVolumes(cfg, 2, 2, _dev(), volume=(72, 64, 56), augment=aug))
    flips, new, again = mk(AUG_CFG), mk(NEW_CFG), mk(NEW_CFG)
    assert len(new) == 2
    for (x, y), (x2, y2), (fx, fy) in zip(new, again, flips):
        assert _same(x, x2) and _same(y, y2)                                             # reproducible from its seed
        assert _same(y, fy)                                                              # the flips' random states are handed out first and do not move
        assert x.shape == fx.shape and bool(torch.isfinite(x).all())
    assert any(not _same(a[0], f[0]) for a, f in zip(new, flips))


def test_two_training_steps_with_the_new_keys():
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    from veloxseg_amd.utils.train_loop import run_train
    cfg, _ = CASES["g2_32_m2"]
    args = types.SimpleNamespace(model_name="VeloxSeg", dataset_name="AutoPETII", checkpoint_path=None, synthetic_steps=2, augment=True)
    h = run_train(args, dict(TRAIN_CFG, epochs=1, augment=NEW_CFG), {"VeloxSeg": cfg})
    assert len(h["loss"]) == 1 and math.isfinite(h["loss"][0])
    with pytest.raises(ValueError, match="unknown keys"):
        run_train(args, dict(TRAIN_CFG, epochs=1, augment={"gamma": 1.0}), {"VeloxSeg": cfg})
