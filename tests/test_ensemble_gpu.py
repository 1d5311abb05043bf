"""GPU: ensemble inference -- vx_softmax_accumulate and vx_prob_finalize (csrc/ensemble.hip) against tests/ensemble_ref.py, and the Python surface
(utils/ensemble.py: ProbabilityAccumulator, softmax_mean, infer_ensemble, run_ensemble.py) end to end.  Exact columns, labels and the end-to-end runs are held
to == (int32 bytes for floats); random columns are held to bars derived from the 1 ulp of expf / logf, the rounded additions and the division."""
import csv
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import ensemble_ref as ER

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PAD = 64            # sentinel elements behind every output buffer: a kernel that runs past its extent is caught, not only suffered
SENTINEL = -7.5
U = 2.0 ** -24      # unit roundoff of fp32
INF, NAN = float("inf"), float("nan")

# (name, V, logits viewed from element 1, psum viewed from element 1): 105 = the scalar path with one partial block; 192 = the vector path with a partial block;
# 2052 = several blocks and a tail; the last two are V % 4 == 0 buffers whose base is 4 bytes past a 16-byte boundary: contiguous, misaligned, so the scalar path
LAYOUTS = [("3x5x7", 105, False, False), ("4x6x8", 192, False, False), ("2052", 2 * 1024 + 4, False, False),
           ("192_logits_off1", 192, True, False), ("192_psum_off1", 192, False, True)]
KS = [1, 2, 3, 4, 5, 9]         # 9 takes the re-read path
WEIGHT_SETS = [[1.0], None, None, None, [0.5, 0.25, 0.25], [1, 2, 3]]       # None: equal weights for N = 2, 3, 4 (float32(1 / 3) is not dyadic)
EQUAL_N = [None, 2, 3, 4, None, None]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def stream_pool_left_where_it_was():
    """torch deals torch.cuda.Stream() objects round-robin from a process-wide pool of 32, and a test of another module (the forked-stream capture of
    tests/test_tape_gpu.py) depends on which pool stream it is dealt: a side stream that happens to be torch's default capture stream is no fork.  The tape captures of
    this module draw from that pool, so the module leaves the pool's position where it found it: one full turn is recorded on the way in (32 draws: the position is
    unchanged), and on the way out streams are drawn until the last one of that turn comes up again."""
    turn = [torch.cuda.Stream().cuda_stream for _ in range(32)]
    yield
    if len(set(turn)) == 32:
        for _ in range(32):
            if torch.cuda.Stream().cuda_stream == turn[-1]:
                break


def _buffer(n, off, fill=SENTINEL, dtype=torch.float32):
    """a device buffer of n elements behind `off` leading ones and in front of PAD sentinels -> (the n-element view, the whole buffer)"""
    whole = torch.full((off + n + PAD,), fill, device=dev(), dtype=dtype)
    return whole[off:off + n], whole


def _intact(whole, n, off, fill=SENTINEL):
    return bool((whole[:off] == fill).all()) and bool((whole[off + n:] == fill).all())


def _place(x, off):
    view, _ = _buffer(x.numel(), off)
    view.copy_(x.reshape(-1))
    return view.view(x.shape)


def _accumulate(logits, psum, w, first):
    from veloxseg_amd import _hip as H
    B, K, V = logits.shape
    assert logits.is_contiguous() and psum.is_contiguous() and psum.numel() == logits.numel()
    H.call("vx_softmax_accumulate", H.P(logits), H.P(psum), B, K, V, float(w), int(first), H.stream_ptr())


def _finalize(psum, labels, entropy):
    from veloxseg_amd import _hip as H
    B, K, V = psum.shape
    H.call("vx_prob_finalize", H.P(psum), H.P(labels, torch.uint8), H.P(entropy), B, K, V, H.stream_ptr())


def _argmax_channels(psum):
    from veloxseg_amd import _hip as H
    B, K, V = psum.shape
    src = psum.clone()                                   # (an aligned copy: the reference kernel is the project's own)
    out = torch.empty((B, V), device=psum.device, dtype=torch.uint8)
    H.call("vx_argmax_channels", H.P(src), H.P(out, torch.uint8), B, K, V, H.stream_ptr())
    return out


@functools.lru_cache(maxsize=None)
def _exact(B, K, V, model):
    """(logits (B, K, V), fp32 probabilities) of exact columns for one model of an ensemble, computed once and shared"""
    cols = [ER.exact_columns(K, (V,), 1000 * model + 10 * K + b) for b in range(B)]
    return torch.stack([c[0] for c in cols]), torch.stack([c[1] for c in cols])


def _expected(B, K, V, weights, n):
    w = ER.normalise_weights(weights, n)
    want = None
    for i in range(n):
        want = ER.accumulate32(want, _exact(B, K, V, i)[1], w[i])
    return w, want


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_exact_columns_equal_the_fp32_restatement_in_bytes(layout, K, B):
    """test 1: every probability is exactly 0 or fl(1 / m), so psum must equal the chain t = w * p; psum = psum + t in bytes -- an fma, another summation order, a wrong
    first call or a wrong alignment dispatch (the off-by-one-element views, the tails) fail it"""
    _, V, loff, poff = layout
    n_el = B * K * V
    for weights, n_eq in zip(WEIGHT_SETS, EQUAL_N):
        n = n_eq if weights is None else len(weights)
        w, want = _expected(B, K, V, weights, n)
        psum, whole = _buffer(n_el, int(poff))
        psum = psum.view(B, K, V)
        for i in range(n):
            _accumulate(_place(_exact(B, K, V, i)[0].to(dev()), int(loff)), psum, w[i], i == 0)
        torch.cuda.synchronize()
        assert ER.same_bits(psum, want), (layout[0], K, B, weights, n)
        assert _intact(whole, n_el, int(poff)), "the kernel wrote outside psum"
        assert bool(torch.isnan(psum[:, :, :3]).all()) and not bool(torch.isnan(psum[:, :, 3:]).any())      # all -inf, a +inf, a NaN: all-NaN columns, nothing else


@pytest.mark.parametrize("K", [2, 5, 9])
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_first_call_writes_psum_without_reading_it(layout, K):
    """test 2: a NaN-filled psum with first = 1 gives the N = 1 result of test 1"""
    _, V, loff, poff = layout
    B = 2
    w, want = _expected(B, K, V, [1.0], 1)
    psum, whole = _buffer(B * K * V, int(poff))
    psum.fill_(NAN)
    psum = psum.view(B, K, V)
    _accumulate(_place(_exact(B, K, V, 0)[0].to(dev()), int(loff)), psum, w[0], True)
    torch.cuda.synchronize()
    assert ER.same_bits(psum, want) and _intact(whole, B * K * V, int(poff))


def _softmax_bar(x64, p64, K):
    """|p_gpu - p| allowed, from the parts of the kernel: d_c = x_c - m is one fp32 subtraction (relative error u of d, so |d_c| u relative in e_c), expf is within 1 ulp
    (2 u relative), the sum carries K - 1 rounded additions and the e_j's own errors weighted by p_j, the quotient one rounding:
    |dp_c| <= p_c * ((|d_c| + 2) + sum_j p_j (|d_j| + 2) + (K - 1) + 1) u, first order; 2^-10 of it covers the second order ((|d| u)^2 at |d| < 2^10), and 2^-148 the
    results that are subnormal (expf's ulp there is 2^-149 absolute, the quotient's rounding at most 2^-150)."""
    own = (x64 - x64.max(dim=1, keepdim=True).values).abs() + 2
    return p64 * (own + (p64 * own).sum(dim=1, keepdim=True) + K) * U * (1 + 2.0 ** -10) + 2.0 ** -148


@pytest.mark.parametrize("scale", [1.0, 10.0, 80.0])
@pytest.mark.parametrize("K", [2, 3, 4, 5, 9])
def test_random_columns_are_within_the_derived_bar_of_fp64(K, scale):
    """test 3: normal logits at three scales against the fp64 restatement, on the scalar and the vector path (observed ratios: DESIGN.md section 30)"""
    for V in (105, 192):
        x = torch.randn((2, K, V), generator=torch.Generator().manual_seed(17 * K + V)) * scale
        psum, whole = _buffer(x.numel(), 0)
        psum = psum.view(x.shape)
        _accumulate(x.to(dev()), psum, 1.0, True)               # weight 1: 0 + 1 * p = p, the soft-max itself
        torch.cuda.synchronize()
        want = ER.softmax64(x)
        ratio = float(((psum.cpu().double() - want).abs() / _softmax_bar(x.double(), want, K)).max())
        print(f"softmax K = {K}, scale {scale}, V = {V}: max |dp| / bar = {ratio:.3f}")
        assert ratio <= 1.0, (K, scale, V, ratio)
        assert _intact(whole, x.numel(), 0)


def _mean_psum(B, K, V, seed, off=0):
    """the mean of two random models' soft-max, formed by the kernel itself, in a buffer viewed from element `off`"""
    g = torch.Generator().manual_seed(seed)
    psum, _ = _buffer(B * K * V, off)
    psum = psum.view(B, K, V)
    for i in range(2):
        _accumulate((torch.randn((B, K, V), generator=g) * 3).to(dev()), psum, 0.5, i == 0)
    return psum


def _check_labels(psum):
    B, K, V = psum.shape
    off = 0
    labels, whole = _buffer(B * V, off, fill=255, dtype=torch.uint8)
    labels = labels.view(B, V)
    _finalize(psum, labels, None)
    ref = _argmax_channels(psum)
    torch.cuda.synchronize()
    assert torch.equal(labels, ref), "labels differ from vx_argmax_channels(psum)"
    assert torch.equal(labels.cpu(), ER.argmax_rule(psum.cpu(), 1)[:, 0])
    assert _intact(whole, B * V, off, fill=255)
    return labels


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_labels_are_vx_argmax_channels_of_psum(layout, K, B):
    """test 4: bytes-equal on random means, on exact ties (two models disagree at equal weight: the lower class wins) and on NaN columns"""
    _, V, loff, poff = layout
    off = int(loff or poff)
    _check_labels(_mean_psum(B, K, V, 31 * K + V + B, off))
    # exact ties and NaN columns: model A is sure of class a(v), model B of class b(v); the mean is 0.5 / 0.5 where they differ, and column 1 holds a NaN
    g = torch.Generator().manual_seed(K + V)
    ca, cb = torch.randint(0, K, (B, V), generator=g), torch.randint(0, K, (B, V), generator=g)
    psum, _ = _buffer(B * K * V, off)
    psum = psum.view(B, K, V)
    for i, cls in enumerate((ca, cb)):
        x = torch.full((B, K, V), -INF)
        x.scatter_(1, cls[:, None], 0.0)
        x[:, K - 1, 1] = NAN
        _accumulate(x.to(dev()), psum, 0.5, i == 0)
    labels = _check_labels(psum).cpu()
    want = torch.minimum(ca, cb).to(torch.uint8)
    want[:, 1] = 0                                          # an all-NaN column: its first NaN
    assert torch.equal(labels, want)
    assert bool(torch.isnan(psum[:, :, 1]).all())
    if K > 1:
        tie = (ca != cb)
        tie[:, 1] = False
        assert bool(tie.any()) and bool((psum.cpu().max(1).values[tie] == 0.5).all())


def _entropy_bar(p64, K):
    """|h_gpu - h| allowed for fp32 probabilities p: a term -(p ln p) carries logf's 1 ulp (2 u relative) and the product's rounding (u), the sum K - 1 rounded additions
    of non-negative terms (p <= 1): (3 + K - 1) u * sum_c |p_c ln p_c|, first order, with 2^-10 of it for the second order and K * 2^-149 for subnormal terms"""
    t = torch.where(p64 == 0, torch.zeros_like(p64), (p64 * torch.log(p64)).abs())
    return t.sum(dim=1) * (K + 2) * U * (1 + 2.0 ** -10) + K * 2.0 ** -149


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("layout", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_entropy_of_the_mean(layout, K):
    """test 5: one-hot columns give +0.0 by bit pattern, NaN columns NaN, columns with zeros count them as +0, random columns are within the derived bar of fp64
    (observed ratios: DESIGN.md section 30); labels and entropy from one call are those of two"""
    _, V, loff, poff = layout
    off, B = int(loff or poff), 2
    # one-hot, NaN and half / half columns, written directly
    p = torch.zeros((B, K, V))
    hot = torch.randint(0, K, (B, V), generator=torch.Generator().manual_seed(V + K))
    p.scatter_(1, hot[:, None], 1.0)
    p[:, 0, 2] = NAN
    if K > 1:
        p[:, :, 5] = 0.0
        p[:, 0, 5] = p[:, K - 1, 5] = 0.5
    psum = _place(p.to(dev()), off)
    ent, whole = _buffer(B * V, off, fill=NAN)
    ent = ent.view(B, V)
    _finalize(psum, None, ent)
    torch.cuda.synchronize()
    bits = ent.cpu().view(torch.int32)
    plain = torch.ones(V, dtype=torch.bool)
    plain[2] = False
    if K > 1:
        plain[5] = False
        assert bool(((ent[:, 5].cpu().double() - ER.entropy64(p[:, :, 5:6])[:, 0, 0]).abs() <= _entropy_bar(p[:, :, 5].double(), K)).all())
    assert bool((bits[:, plain] == 0).all()), "a one-hot column did not give +0.0"
    assert bool(torch.isnan(ent[:, 2]).all())
    assert bool(torch.isnan(whole[:off]).all()) and bool(torch.isnan(whole[off + B * V:]).all())
    # random means
    psum = _mean_psum(B, K, V, 7 * K + V, off)
    ent2, _ = _buffer(B * V, off)
    ent2 = ent2.view(B, V)
    _finalize(psum, None, ent2)
    p64 = psum.cpu().double()
    ratio = float(((ent2.cpu().double() - ER.entropy64(p64)[:, 0]).abs() / _entropy_bar(p64, K)).max()) if K > 1 else 0.0
    print(f"entropy K = {K}, {layout[0]}: max |dh| / bar = {ratio:.3f}")
    assert ratio <= 1.0, (K, layout[0], ratio)
    # both outputs in one call
    lab, _ = _buffer(B * V, off, fill=255, dtype=torch.uint8)
    ent3, _ = _buffer(B * V, off)
    _finalize(psum, lab.view(B, V), ent3.view(B, V))
    assert ER.same_bits(ent3.view(B, V), ent2) and torch.equal(lab.view(B, V), _check_labels(psum))


def test_accumulator_object_and_softmax_mean():
    from veloxseg_amd.utils import ensemble as E
    B, K, sp = 2, 3, (4, 6, 8)
    g = torch.Generator().manual_seed(4)
    xs = [(torch.randn((B, K) + sp, generator=g) * 4).to(dev()) for _ in range(3)]
    w = E.normalise_weights([1, 2, 3], 3)
    acc = E.ProbabilityAccumulator(K, sp, dev(), batch=B)
    with pytest.raises(RuntimeError, match="nothing was added"):
        acc.probabilities()
    acc.psum.fill_(NAN)
    want = torch.empty((B, K, 192), device=dev())
    for i, x in enumerate(xs):
        acc.add(x, w[i])
        _accumulate(x.view(B, K, -1), want, w[i], i == 0)
    assert acc.probabilities() is acc.psum and ER.same_bits(acc.psum.view(B, K, -1), want)
    p, lab, ent = E.softmax_mean(xs, weights=[1, 2, 3], entropy=True)
    assert ER.same_bits(p, acc.psum) and torch.equal(lab, acc.labels()) and ER.same_bits(ent, acc.entropy())
    assert lab.shape == (B, 1) + sp and lab.dtype == torch.uint8 and ent.shape == (B, 1) + sp
    assert torch.equal(lab.view(B, -1), _argmax_channels(p.view(B, K, -1)))
    assert float((p.cpu().double() - ER.mean64([x.cpu() for x in xs], [1, 2, 3])).abs().max()) <= 64 * U
    assert len(E.softmax_mean(xs)) == 2
    with pytest.raises(ValueError, match="classes"):
        acc.add(xs[0][:, :2], 0.5)
    with pytest.raises(ValueError, match="do not fit"):
        acc.add(xs[0][:, :, :2], 0.5)
    with pytest.raises(ValueError, match="weight"):
        acc.add(xs[0], 0.0)


class Stub(torch.nn.Module):
    """voxel-wise predictor: logit of class c = 0 where channel 0 exceeds t[c], -inf elsewhere.  Overlapping windows and mirrored windows agree, so the blended logits
    are exactly 0 or -inf whatever the window weights"""

    def __init__(self, thresholds, fail=False):
        super().__init__()
        self.t, self.fail, self.calls = [float(t) for t in thresholds], fail, 0

    def logits(self, x):
        return torch.cat([torch.where(x[:, :1] > t, 0.0, -INF) for t in self.t], dim=1)

    def forward(self, x):
        self.calls += 1
        if self.fail:
            raise RuntimeError("stub failure")
        return self.logits(x)


STUBS = [[-2.0, 0.0, 0.7], [-1.5, -1.0, 0.1], [-2.5, 0.5, -0.3]]


@pytest.mark.parametrize("kw", [dict(), dict(blend="gaussian", mirror_axes=(2,))], ids=["plain", "gaussian_mirror2"])
@pytest.mark.parametrize("n", [2, 3])
def test_end_to_end_on_stub_predictors_equals_the_cpu_restatement(n, kw):
    """test 6: volume 1 x 2 x 40^3, roi 32^3, overlap 0.5: probabilities in bytes, labels, and the positions where the entropy is +0 / NaN"""
    from veloxseg_amd.utils import ensemble as E
    vol = torch.randn((1, 2, 40, 40, 40), generator=torch.Generator().manual_seed(6))
    stubs = [Stub(t).eval() for t in STUBS[:n]]
    stubs[0].train()
    weights = None if n == 3 else [1, 3]
    p, lab, ent = E.infer_ensemble(stubs, vol.to(dev()), (32, 32, 32), 2, 0.5, weights=weights, taped=False, entropy=True, **kw)
    assert all(s.calls > 0 for s in stubs) and stubs[0].training and not stubs[1].training
    w = ER.normalise_weights(weights, n)
    want = None
    for s, wi in zip(stubs, w):
        want = ER.accumulate32(want, ER.softmax64(s.logits(vol)).float(), wi)
    assert p.shape == (1, 3, 40, 40, 40) and lab.shape == ent.shape == (1, 1, 40, 40, 40)
    assert ER.same_bits(p, want)
    assert torch.equal(lab.cpu(), ER.argmax_rule(want, 1))
    nan = torch.isnan(want).any(1, keepdim=True)
    one_hot = (want == 1).any(1, keepdim=True)
    assert bool(nan.any()) and bool(one_hot.any()) and not bool((nan | one_hot).all())
    assert torch.equal(torch.isnan(ent).cpu(), nan)
    assert torch.equal(ent.cpu().view(torch.int32) == 0, one_hot)
    assert bool((ent.cpu()[~nan & ~one_hot] > 0).all())


def test_training_flags_are_restored_when_a_later_model_raises_and_class_counts_must_agree():
    from veloxseg_amd.utils import ensemble as E
    vol = torch.randn((1, 2, 40, 40, 40), generator=torch.Generator().manual_seed(6)).to(dev())
    a, b = Stub(STUBS[0]).train(), Stub(STUBS[1], fail=True).train()
    with pytest.raises(RuntimeError, match="stub failure"):
        E.infer_ensemble([a, b], vol, (32, 32, 32), 2, 0.5, taped=False)
    assert a.training and b.training and a.calls > 0
    c = Stub(STUBS[0][:2]).eval()                             # declares nothing: found out when its logits arrive
    with pytest.raises(ValueError, match="classes"):
        E.infer_ensemble([a, c], vol, (32, 32, 32), 2, 0.5, taped=False)
    assert a.training and not c.training


@pytest.fixture(scope="module")
def two_models(golden_dir):
    sys.path.insert(0, golden_dir)
    from recipe import CASES, fill_state_dict
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    cfg, _ = CASES["g2_32_m2"]
    out = []
    for seed in (7, 8):
        model = VeloxSeg(**cfg)
        model.load_state_dict(fill_state_dict(model.state_dict(), seed=seed))
        out.append(model.to(dev()).eval())
    return out


@pytest.fixture(scope="module")
def model_logits(two_models):
    """the two models' own infer_volume results on the shared volume, computed once (this also captures every tape and replica the later calls replay)"""
    from veloxseg_amd.utils import inference_runtime as IR
    x = torch.randn((1, 2, 48, 40, 36), generator=torch.Generator().manual_seed(5)).to(dev())
    with torch.inference_mode():
        outs = [IR.infer_volume(m, x, (32, 32, 32), 2, 0.5) for m in two_models]
    return x, [o[0].clone() for o in outs], [o[1].clone() for o in outs]


def test_end_to_end_on_real_models_equals_softmax_mean_of_their_logits(two_models, model_logits):
    """test 7: infer_ensemble through the tapes == softmax_mean of the two infer_volume logits, byte for byte; unequal weights; native=; postprocess=; training flags;
    no recapture on the second call"""
    from veloxseg_amd.utils import ensemble as E
    from veloxseg_amd.utils.components import Postprocess
    from veloxseg_amd.utils.preprocess import labels_on_native_grid
    x, logits, _ = model_logits
    roi = (32, 32, 32)
    tps = [m.__dict__["_vx_taped_predictor"] for m in two_models]
    tapes = [dict(tp._tapes) for tp in tps]
    replicas = [dict(tp.__dict__.get("_replicas", {})) for tp in tps]
    assert all(len(t) > 0 for t in tapes)
    two_models[0].train()
    try:
        for weights in (None, [1, 3]):
            p, lab, ent = E.infer_ensemble(two_models, x, roi, 2, 0.5, weights=weights, entropy=True)
            wp, wlab, went = E.softmax_mean(logits, weights=weights, entropy=True)
            assert ER.same_bits(p, wp) and torch.equal(lab, wlab) and ER.same_bits(ent, went), weights
            assert p.shape == (1, 2, 48, 40, 36) and lab.shape == (1, 1, 48, 40, 36) and lab.dtype == torch.uint8
            assert float((p.cpu().double() - ER.mean64([l.cpu() for l in logits], weights)).abs().max()) <= 64 * U
        assert two_models[0].training and not two_models[1].training
        # no capture beyond those of the models' own runs: the predictors hang on the models and are reused
        for m, tp, t, r in zip(two_models, tps, tapes, replicas):
            assert m.__dict__["_vx_taped_predictor"] is tp
            assert set(tp._tapes) == set(t) and all(tp._tapes[k] is t[k] for k in t)
            now = tp.__dict__.get("_replicas", {})
            assert set(now) == set(r) and all(now[k] is r[k] for k in r)
        native = {"native_shape": (60, 50, 45), "native_spacing": (0.8, 0.8, 0.8), "net_spacing": (1.0, 1.0, 1.0)}
        pn, labn = E.infer_ensemble(two_models, x, roi, 2, 0.5, native=native)
        assert ER.same_bits(pn, E.softmax_mean(logits)[0])
        assert labn.shape == (1, 1, 60, 50, 45)
        assert torch.equal(labn[0, 0], labels_on_native_grid(pn[0], native["native_shape"], native["net_spacing"], native["native_spacing"]))
        post = {"keep_largest": 1, "connectivity": 6}
        plain = E.softmax_mean(logits)[1]
        pp, labp = E.infer_ensemble(two_models, x, roi, 2, 0.5, postprocess=post)
        assert torch.equal(labp, Postprocess.from_config(post)(plain)) and ER.same_bits(pp, pn)
        seen = []

        class Spy(Postprocess):
            def __call__(self, labels):
                seen.append(labels.clone())
                return super().__call__(labels)
        _, labs = E.infer_ensemble(two_models, x, roi, 2, 0.5, postprocess=Spy(keep_largest=1, connectivity=6))
        assert len(seen) == 1 and torch.equal(seen[0], plain) and torch.equal(labs, labp)       # it ran once, on the final labels only
    finally:
        two_models[0].eval()


def test_one_model_ensemble_agrees_with_infer_volume_where_the_logit_gap_is_clear(two_models, model_logits):
    """the labels of a one-model ensemble are NOT guaranteed to be infer_volume's (soft-max is monotone in exact arithmetic only), so equality is asserted on voxels
    whose top-two logit gap is at least 1e-3, and those must be at least 99 % of the volume (the oracle's own gap statistic for these seeded weights is 0.02 %)"""
    from veloxseg_amd.utils import ensemble as E
    x, logits, labels = model_logits
    for m, l, lab in zip(two_models, logits, labels):
        p, got = E.infer_ensemble([m], x, (32, 32, 32), 2, 0.5)
        assert ER.same_bits(p, E.softmax_mean([l])[0])
        top = l.topk(2, dim=1).values
        clear = (top[:, :1] - top[:, 1:]) >= 1e-3
        left_out = 1.0 - float(clear.float().mean())
        print(f"share of voxels with a top-two logit gap below 1e-3: {left_out:.5f}")
        assert left_out <= 0.01
        assert torch.equal(got[clear], lab[clear])


@pytest.mark.parametrize("source", ["seeds", "checkpoints"])
def test_run_ensemble_end_to_end(tmp_path, source):
    """test 8: run_ensemble.py in a child process on two models writes one CSV row whose Dice is that of infer_ensemble's labels for the same models: built
    from the seeds 12345 + i, or (other weights) read from <checkpoint_dir>/a.pth and b.pth"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    from veloxseg_amd.utils import ensemble as E
    from veloxseg_amd.utils.load_model import load_model
    from veloxseg_amd.utils.metric.metrics import metrics_tensor
    cfg, _ = CASES["g2_32_m2"]
    mc, tc, te = tmp_path / "models.json", tmp_path / "train.json", tmp_path / "test.json"
    mc.write_text(json.dumps({"VeloxSeg": cfg}))
    tc.write_text(json.dumps(dict(TRAIN_CFG, patch_size={"AutoPETII": [32, 32, 32]})))
    te.write_text(json.dumps({"sliding_window": {"overlap": 0.5}, "ensemble": {"weights": [1, 3]}}))
    out = tmp_path / "ens.csv"
    models, extra = [], []
    for i, name in enumerate("ab"):
        torch.manual_seed((12345 if source == "seeds" else 777) + i)
        models.append(load_model("VeloxSeg", {"VeloxSeg": cfg}))
        if source == "checkpoints":
            torch.save({"model": models[-1].state_dict()}, tmp_path / f"{name}.pth")
            extra = ["--checkpoint_dir", str(tmp_path)]
        models[-1] = models[-1].to(dev()).eval()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_ensemble.py"), "--dataset_name", "AutoPETII", "--model_name", "VeloxSeg", "--train_config", str(tc),
                        "--model_config", str(mc), "--test_config", str(te), "--checkpoint_index", "a,b", "--synthetic", "1",
                        "--volume_shape", "40", "40", "40", "--out_csv", str(out), *extra], capture_output=True, text=True, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = list(csv.DictReader(open(out)))
    assert len(rows) == 1 and rows[0]["name"] == "synthetic_0"
    g = torch.Generator().manual_seed(12345)
    x = torch.randn((1, sum(cfg["in_ch"]), 40, 40, 40), generator=g)
    y = torch.randint(0, cfg["n_classes"], (1, 1, 40, 40, 40), generator=g)
    with torch.inference_mode():
        _, lab = E.infer_ensemble(models, x.to(dev()).float(), [32, 32, 32], TRAIN_CFG["batch_size"], 0.5, weights=[1, 3])
        dice = metrics_tensor(y.to(dev()), lab.long())[6]
    assert float(rows[0]["Dice"]) == float(dice)
    assert float(rows[0]["Prediction"]) == float((lab > 0).sum())
