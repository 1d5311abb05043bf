"""GPU: the fused optimizer step with global-norm gradient clipping, EMA weights and param groups -- vx_grad_sqnorm_partials and
vx_adamw_step_ex against torch (clip_grad_norm_ + torch.optim.AdamW) and fp64 restatements, then TrainEngine with all three on: eager, taped, pipelined, data
parallel, and through run_train / run_test.py."""
import copy
import functools
import json
import math
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from recipe import CASES, LOSS_CFG, make_inputs  # noqa: E402

ATOL, RTOL = 1e-7, 1e-6          # the bars of tests/test_hip_ops_gpu.py::test_adamw_matches_torch (parameters)
# Moments against TORCH's: the kernels form 1 - beta in fp32 from the fp32 beta (vx_adamw_step's arithmetic, unchanged), torch rounds the fp64 difference.
# 1 - fp32(0.999) = 0.99998713e-3 against 1e-3: a relative 1.3e-5 on every term of exp_avg_sq (2e-7 on exp_avg), which the parameters see through sqrt(v) as ~1e-9 absolute.
RTOL_MOMENTS = 2e-5
OMB1, OMB2 = float(np.float32(1.0) - np.float32(0.9)), float(np.float32(1.0) - np.float32(0.999))          # what the kernels multiply the gradient terms by
B1, B2, EPS = 0.9, 0.999, 1e-8


def _H():
    from veloxseg_amd import _hip as H
    return H


def dev():
    return torch.device("cuda", 0)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def close(a, b, what, atol=ATOL, rtol=RTOL):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaNs differ"
    ok = ~torch.isnan(b)
    err = (a[ok] - b[ok]).abs()
    bad = err > atol + rtol * b[ok].abs()
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} outside {atol}+{rtol}*|ref|, max err {float(err.max()):.3e}"


def partials(g):
    H = _H()
    ws = torch.full((H.query("vx_grad_sqnorm_blocks"),), float("nan"), device=g.device, dtype=torch.float64)      # (every slot must be written)
    H.call("vx_grad_sqnorm_partials", g.data_ptr(), g.numel(), H.P(ws, torch.float64), H.stream_ptr())
    return ws


def step_ex(p, g, m, v, step, lr=2.5e-4, wd=0.01, gscale=1.0, ws=None, max_norm=0.0, stats=None, write_stats=1, ema=None, omd=0.0, table=None, glr=None, gwd=None, n=None):
    import ctypes
    H = _H()
    ng = 0 if glr is None else len(glr)
    hl, hw = (ctypes.c_float * 8)(*(glr or [])), (ctypes.c_float * 8)(*(gwd or []))
    H.call("vx_adamw_step_ex", p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), int(n if n is not None else p.numel()), lr, B1, B2, EPS, wd, step, gscale,
           None if ws is None else H.P(ws, torch.float64), 0 if ws is None else ws.numel(), float(max_norm), None if stats is None else H.P(stats), write_stats,
           None if ema is None else ema.data_ptr(), float(omd), None if table is None else table.data_ptr(), ctypes.addressof(hl) if ng else None,
           ctypes.addressof(hw) if ng else None, ng, H.stream_ptr())


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


# ====================================================================================================================== the norm
def _mixed(n, seed):
    """magnitudes from 1e-20 to 1e18: the squares of either end are outside fp32's range"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.pow(10.0, torch.rand(n, generator=g) * 38.0 - 20.0)


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 4 * 255 + 3, (1 << 20) + 5])
def test_sqnorm_partials_sum_in_fp64_and_repeat_bit_for_bit(n):
    """Bound: every term g_i^2 is positive, so whatever the order, the computed sum is sum g_i^2 (1 + d_i) with |d_i| <= (k_i + 1) u, u = 2^-53, k_i = the additions
    term i passes through (+ 1 for its square).  In the kernel k_i <= 4 * ceil(n / (4 * 65536)) + 1 (a thread's chain: <= 21 at n = 2^20 + 5) + 6 (wave butterfly) + 3 (waves)
    = 30; the partials are added here with math.fsum (one rounding).  So the kernel is within 32 u = 3.6e-15 of the exact sum, torch's own cascaded fp64 sum within a few
    hundred u at worst: 1e-13 is the fp64 summation bound for these n with slack, and 7 orders of magnitude below what fp32 accumulation could give."""
    g = _mixed(n, seed=n)
    gd = g.to(dev())
    ws = partials(gd)
    assert bool(torch.isfinite(ws).all()) and bool((ws >= 0).all())
    got = math.fsum(ws.cpu().tolist())
    ref = float(torch.sum(g.double() ** 2))
    print(f"n={n}: sum g^2 kernel {got:.17e} torch {ref:.17e} rel {abs(got - ref) / ref:.3e}")
    assert abs(got - ref) <= 1e-13 * ref
    assert torch.equal(partials(gd), ws), "two runs differ"
    assert torch.equal(partials(gd.clone()), ws), "the same gradient in another buffer gives other bits"
    if n > 4:          # a buffer that is not 16-byte aligned takes the scalar path: same bound
        ws1 = partials(torch.cat([gd[:1], gd])[1:])
        assert abs(math.fsum(ws1.cpu().tolist()) - ref) <= 1e-13 * ref


@pytest.mark.parametrize("bad", [float("inf"), float("nan")], ids=["inf", "nan"])
def test_nonfinite_gradient_follows_torch_and_is_counted(bad):
    """error_if_nonfinite=False: nothing is skipped -- an infinite norm gives coef 0 (inf * 0 = NaN at the infinite element, 0 elsewhere), a NaN norm NaN everywhere"""
    n = 1000
    p0, g0 = rnd(n), rnd(n, seed=1)
    g0[137] = bad
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=2.5e-4, weight_decay=0.01)
    pt.grad = g0.clone()
    torch.nn.utils.clip_grad_norm_([pt], 1.0)
    opt.step()
    d = dev()
    p, g, m, v = p0.to(d), g0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    stats = torch.zeros(4, device=d)
    stats[2] = 3.0
    step_ex(p, g, m, v, 1, ws=partials(g), max_norm=1.0, stats=stats)
    assert float(stats[2]) == 4.0, "the non-finite counter must go up by one"
    assert not math.isfinite(float(stats[0]))
    close(p, pt.data, "p")
    close(m, opt.state[pt]["exp_avg"], "m", rtol=RTOL_MOMENTS)
    close(v, opt.state[pt]["exp_avg_sq"], "v", rtol=RTOL_MOMENTS)
    assert int(torch.isnan(p).sum()) == (1 if bad == float("inf") else n)
    # a finite step leaves the counter alone
    g2 = rnd(n, seed=2).to(d)
    step_ex(torch.zeros(n, device=d), g2, torch.zeros(n, device=d), torch.zeros(n, device=d), 1, ws=partials(g2), max_norm=1.0, stats=stats)
    assert float(stats[2]) == 4.0 and math.isfinite(float(stats[0]))


# ====================================================================================================================== the update
@pytest.mark.parametrize("n", [10007, 4096])
def test_everything_off_is_bit_identical_to_vx_adamw_step(n):
    H = _H()
    d = dev()
    p0 = rnd(n)
    pa, ma, va = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    pb, mb, vb = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    for step in range(1, 4):
        g = (rnd(n, seed=step) * step).to(d)
        H.call("vx_adamw_step", H.P(pa), H.P(g), H.P(ma), H.P(va), n, 2.5e-4, B1, B2, EPS, 0.01, step, 0.5, H.stream_ptr())
        step_ex(pb, g, mb, vb, step, gscale=0.5)
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb)
    assert not torch.equal(pa.cpu(), p0)


def test_clip_matches_clip_grad_norm_and_torch_adamw():
    d = dev()
    n, max_norm = 10007, 10.0
    p0, g0 = rnd(n), rnd(n, seed=1)                    # ||g0|| ~ 100
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=2.5e-4, weight_decay=0.01)
    p, m, v = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    stats = torch.zeros(4, device=d)
    # step 1: far above max_norm; step 2: below it (coef must be exactly 1); step 3: grad_scale = 0.5 (the norm is of the averaged gradient)
    for step, (mult, gscale) in enumerate([(1.0, 1.0), (0.05, 1.0), (2.0, 0.5)], start=1):
        gi = g0 * mult
        pt.grad = gi * gscale
        torch.nn.utils.clip_grad_norm_([pt], max_norm)
        opt.step()
        gd = gi.to(d)
        step_ex(p, gd, m, v, step, gscale=gscale, ws=partials(gd), max_norm=max_norm, stats=stats)
        total64 = math.sqrt(float(torch.sum(gi.double() ** 2))) * gscale
        coef64 = min(1.0, max_norm / (total64 + 1e-6))
        total, coef = float(stats[0]), float(stats[1])
        print(f"step {step}: total {total!r} (fp64 {total64!r}) coef {coef!r} (fp64 {coef64!r})")
        assert abs(total - float(np.float32(total64))) <= ulp32(total64)
        assert abs(coef - float(np.float32(coef64))) <= ulp32(coef64)
        assert (coef == 1.0) == (step == 2) and (step == 2 or coef < 0.2)
    assert float(stats[2]) == 0.0
    close(p, pt.data, "p")
    close(m, opt.state[pt]["exp_avg"], "m", rtol=RTOL_MOMENTS)
    close(v, opt.state[pt]["exp_avg_sq"], "v", rtol=RTOL_MOMENTS)


@pytest.mark.parametrize("ngroups", [2, 3])
def test_param_groups_match_torch_adamw_groups(ngroups):
    """a flat buffer of 64-aligned slices of unequal size, each slice in one group; the update issued as two range calls, the second from a non-zero chunk offset"""
    d = dev()
    sizes = [100, 64, 333, 7, 1000, 129]
    group_of = [0, 1, 0, ngroups - 1, 1, 0]
    glr, gwd = [2.5e-4, 1e-3, 5e-5][:ngroups], [0.01, 0.0, 0.1][:ngroups]
    offs, off = [], 0
    for k in sizes:
        offs.append(off)
        off = (off + k + 63) // 64 * 64
    n = off
    table = torch.zeros(n // 64, dtype=torch.uint8)
    P0, G0 = torch.zeros(n), torch.zeros(n)
    tps = []
    for i, (o, k) in enumerate(zip(offs, sizes)):
        table[o // 64:(o + k + 63) // 64] = group_of[i]
        P0[o:o + k] = rnd(k, seed=10 + i)
        G0[o:o + k] = rnd(k, seed=20 + i)                # (the alignment gaps stay zero, as in FlatParams)
        tps.append(torch.nn.Parameter(P0[o:o + k].clone()))
    opt = torch.optim.AdamW([{"params": [tp for tp, gi in zip(tps, group_of) if gi == g_], "lr": glr[g_], "weight_decay": gwd[g_]} for g_ in range(ngroups)])
    p, m, v, tab = P0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d), table.to(d)
    lo = offs[2]
    assert lo % 64 == 0 and lo > 0
    for step in range(1, 4):
        for tp, o, k in zip(tps, offs, sizes):
            tp.grad = G0[o:o + k] * step
        opt.step()
        g = (G0 * step).to(d)
        step_ex(p[:lo], g[:lo], m[:lo], v[:lo], step, lr=7.0, wd=7.0, table=tab, glr=glr, gwd=gwd)                       # (the scalar lr / wd must not be read)
        step_ex(p[lo:], g[lo:], m[lo:], v[lo:], step, lr=7.0, wd=7.0, table=tab[lo // 64:], glr=glr, gwd=gwd)
    for i, (tp, o, k) in enumerate(zip(tps, offs, sizes)):
        close(p[o:o + k], tp.data, f"p[{i}]")
        close(m[o:o + k], opt.state[tp]["exp_avg"], f"m[{i}]", rtol=RTOL_MOMENTS)
        close(v[o:o + k], opt.state[tp]["exp_avg_sq"], f"v[{i}]", rtol=RTOL_MOMENTS)


@pytest.mark.parametrize("n", [10007, 4096])
def test_ema_follows_the_parameters(n):
    """Per step e' = fma(w, p' - e, e): one subtraction and one fused multiply-add = two roundings, each of relative size u = 2^-24.  The subtraction errs by at most
    u |p' - e| <= 2 u M (M = max(|e|, |p'|)) and enters scaled by w; the fma errs by at most u |e'| <= u M.  With w <= 1/2 a step adds at most 2 u M, and the error carried
    over from earlier steps is multiplied by (1 - w) < 1: after k steps |e - e_fp64| <= 2 k 2^-24 max(|e|, |p|), against an fp64 restatement that uses the same fp32 w."""
    d = dev()
    decay, k = 0.9, 5
    w32 = float(np.float32(1.0 - decay))
    p0 = rnd(n)
    p, m, v = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    e = (p0 + rnd(n, seed=3) * 0.1).to(d)
    e64 = e.double().clone()
    for step in range(1, k + 1):
        g = rnd(n, seed=30 + step).to(d)
        step_ex(p, g, m, v, step, lr=1e-2, ema=e, omd=1.0 - decay)
        e64 = e64 + w32 * (p.double() - e64)
    bound = 2 * k * 2.0 ** -24 * torch.maximum(e64.abs(), p.double().abs())
    err = (e.double() - e64).abs()
    print(f"n={n}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all())
    assert float((e.double() - p.double()).abs().max()) > 1e-3          # (it is an average, not a copy)


# ====================================================================================================================== the engine
def _crit():
    from veloxseg_amd.utils.loss import Loss
    return Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=2)


def _model():
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    cfg, _ = CASES["g2_32_m2"]                      # all dropout p = 0: deterministic
    torch.manual_seed(5)
    return VeloxSeg(**cfg).cuda()


OPT_ARGS = {"lr": 1e-3, "weight_decay": 0.05, "no_weight_decay": "1d"}
DECAY = 0.9


@functools.lru_cache(maxsize=None)
def _unclipped_norm():
    """the gradient norm of the first step (no clipping): max_grad_norm is half of it, so that clipping is active"""
    from veloxseg_amd.engine import TrainEngine
    cfg, _ = CASES["g2_32_m2"]
    x, lab = make_inputs(cfg, 2)
    eng = TrainEngine(_model(), _crit(), (2, 2, 32, 32, 32), lr=0.0, weight_decay=0.0)
    eng.step(x.cuda(), lab.cuda())
    return float(eng.flat.grad.double().pow(2).sum().sqrt())


def _expected(eng, before, g, t):
    """the update restated with plain torch ops in fp32 from the pre-step state and the step's own flat.grad"""
    p0, m0, v0, e0 = before
    norm64 = float(g.double().pow(2).sum().sqrt())
    coef = 1.0 if eng.max_grad_norm is None else float(np.float32(min(1.0, eng.max_grad_norm / (norm64 + 1e-6))))
    groups = eng.optimizer.param_groups
    tab = eng._chunk_group.long()
    lr = torch.tensor([g_["lr"] for g_ in groups], device=g.device, dtype=torch.float32)[tab].repeat_interleave(64)
    wd = torch.tensor([g_["weight_decay"] for g_ in groups], device=g.device, dtype=torch.float32)[tab].repeat_interleave(64)
    bc1, bc2s = np.float32(1.0 - B1 ** t), np.float32(math.sqrt(1.0 - B2 ** t))
    gi = (g * 1.0) * coef
    p = p0 * (1.0 - lr * wd)
    m = B1 * m0 + OMB1 * gi
    v = B2 * v0 + (OMB2 * gi) * gi
    p = p - (lr / float(bc1)) * (m / (v.sqrt() / float(bc2s) + EPS))
    e = e0 + float(np.float32(1.0 - DECAY)) * (p - e0)
    return norm64, coef, p, m, v, e


@functools.lru_cache(maxsize=None)
def _run(use_graph, pipe, clip=True):
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.utils.optimizers.optimizers import build_optimizer
    cfg, _ = CASES["g2_32_m2"]
    x, lab = make_inputs(cfg, 2)
    x, lab = x.cuda(), lab.cuda()
    model = _model()
    opt = build_optimizer(model, "adamw", OPT_ARGS)
    eng = TrainEngine(model, _crit(), (2, 2, 32, 32, 32), optimizer=opt, use_graph=use_graph, pipeline_tail=pipe,
                      max_grad_norm=0.5 * _unclipped_norm() if clip else None, ema_decay=DECAY)
    assert len(opt.param_groups) == 2 and eng.ema is not None
    losses, checks = [], []
    for t in range(1, 4):
        before = tuple(b.clone() for b in (eng.flat.param, eng.m, eng.v, eng.ema))
        losses.append(float(eng.step(x, lab)))
        eng.flush()
        torch.cuda.synchronize()
        checks.append((_expected(eng, before, eng.flat.grad.clone(), t), float(eng.grad_norm) if clip else None, float(eng.clip_coef) if clip else None,
                       tuple(b.clone() for b in (eng.flat.param, eng.m, eng.v, eng.ema))))
    assert eng.use_graph == use_graph, "the capture fell back to eager launches"
    return eng, losses, checks


@pytest.mark.parametrize("use_graph,pipe", [(False, False), (False, True), (True, False), (True, True)], ids=["eager", "eager_pipe", "tape", "tape_pipe"])
def test_engine_step_with_clip_ema_and_groups(use_graph, pipe):
    eng, losses, checks = _run(use_graph, pipe)
    assert not eng._pipe_active(), "clipping needs every range's partials: the step must not be pipelined"
    for t, ((norm64, coef, p, m, v, e), gn, cc, (gp, gm, gv, ge)) in enumerate(checks, start=1):
        print(f"step {t}: grad_norm {gn!r} (fp64 {norm64!r}) coef {cc!r}")
        assert abs(gn - float(np.float32(norm64))) <= ulp32(norm64)
        assert abs(cc - coef) <= ulp32(coef) and cc < 1.0, "clipping must be active"
        close(gp, p, f"param after step {t}")
        close(gm, m, f"exp_avg after step {t}")
        close(gv, v, f"exp_avg_sq after step {t}")
        close(ge, e, f"ema after step {t}")
    assert eng.nonfinite_steps() == 0 and eng.t == 3
    if use_graph:          # taped and eager runs: the bars tests/test_train_harness_gpu.py uses for that comparison
        for a, b in zip(losses, _run(False, False)[1]):
            assert abs(a - b) <= 2e-3 * max(abs(b), 1e-3), (losses, _run(False, False)[1])


def test_ema_and_groups_alone_keep_the_pipelined_split():
    """without clipping the pipelined tail stays: the decoder half of the update (its EMA and its slice of the chunk table included) runs on the fourth lane"""
    eng, losses, checks = _run(True, True, clip=False)
    assert eng._pipe_active() and eng._tail_pending and eng._norm_ws is None and eng.grad_norm is None
    for t, ((_, _, p, m, v, e), _, _, (gp, gm, gv, ge)) in enumerate(checks, start=1):
        close(gp, p, f"param after step {t}")
        close(gm, m, f"exp_avg after step {t}")
        close(gv, v, f"exp_avg_sq after step {t}")
        close(ge, e, f"ema after step {t}")
    for a, b in zip(losses, _run(False, False)[1][:1]):          # (the first step: same parameters, clipping does not touch the loss)
        assert abs(a - b) <= 2e-3 * max(abs(b), 1e-3), (losses, _run(False, False)[1])


def test_ema_weights_swap_in_place_and_a_taped_predictor_follows():
    from veloxseg_amd.engine import TapedPredictor
    eng = _run(False, False)[0]
    model = eng.model
    x = torch.randn((2, 2, 32, 32, 32), generator=torch.Generator().manual_seed(7)).cuda()
    model.eval()
    tp = TapedPredictor(model)

    def both():
        with torch.inference_mode():
            a = tp(x).float().clone()
            b = model(x)
            b = (b[0] if isinstance(b, (list, tuple)) else b).float().clone()
        return a, b
    a0, b0 = both()
    assert torch.equal(a0, b0)
    before = eng.flat.param.clone()
    ptrs = [p.data_ptr() for p in model.parameters()]
    ema_sd = eng.ema_state_dict()
    with eng.ema_weights():
        sd = model.state_dict()
        assert list(sd) == list(ema_sd) and all(torch.equal(sd[k], ema_sd[k]) for k in sd)
        a1, b1 = both()
        assert torch.equal(a1, b1) and not torch.equal(a1, a0), "the predictor did not pick the EMA weights up"
    assert torch.equal(eng.flat.param, before) and ptrs == [p.data_ptr() for p in model.parameters()]
    assert all(torch.equal(v, ema_sd[k]) for k, v in eng.ema_state_dict().items())
    a2, b2 = both()
    assert torch.equal(a2, b2) and torch.equal(a2, a0), "the predictor kept the EMA weights after the context"
    # a step inside the context would train the EMA as if it were the parameters: it raises, and the weights are still swapped back
    with pytest.raises(RuntimeError, match="inside ema_weights"):
        with eng.ema_weights():
            eng.step()
    assert torch.equal(eng.flat.param, before) and all(torch.equal(v, ema_sd[k]) for k, v in eng.ema_state_dict().items())
    # round trip of the EMA state
    other = {k: (v + 1.0 if v.is_floating_point() else v) for k, v in ema_sd.items()}
    eng.load_ema_state_dict(other)
    assert all(torch.equal(v, other[k]) for k, v in eng.ema_state_dict().items())
    eng.load_ema_state_dict(ema_sd)
    model.train()


def test_default_engine_allocates_nothing_and_equals_the_explicit_none_engine():
    """A default-constructed engine and one given max_grad_norm=None, ema_decay=None: nothing allocated, the launches of a step are the same list (vx_adamw_step, none
    of the new entries), and three steps are bit-equal.  Two eager passes over the same batch do NOT give the same gradient to the bit -- the weight-gradient kernels add
    with float atomics (measured here: parameters of two identical default engines differ by up to 2.0e-4 = one sign-like Adam step after three steps) -- so the second
    engine is fed the gradients the first one computed and its three updates must reproduce the first engine's parameters and moments exactly."""
    from veloxseg_amd.engine import TrainEngine
    cfg, _ = CASES["g2_32_m2"]
    x, lab = make_inputs(cfg, 2)
    x, lab = x.cuda(), lab.cuda()
    H = _H()
    orig = H.call
    engines, calls = [], []
    for kw in ({}, {"max_grad_norm": None, "ema_decay": None}):
        eng = TrainEngine(_model(), _crit(), (2, 2, 32, 32, 32), **kw)
        assert eng.ema is None and eng._norm_ws is None and eng._stats is None and eng._chunk_group is None and eng.grad_norm is None and eng.clip_coef is None
        engines.append(eng)
        calls.append([])
    a, b = engines
    assert torch.equal(a.flat.param, b.flat.param)
    for t in range(3):
        H.call = lambda name, *args: (calls[0].append(name), orig(name, *args))[1]
        try:
            a.step(x, lab)
        finally:
            H.call = orig
        if t == 0:          # one whole step of the second engine, on a copy of its state: the same launches in the same order
            keep = tuple(buf.clone() for buf in (b.flat.param, b.m, b.v))
            H.call = lambda name, *args: (calls[1].append(name), orig(name, *args))[1]
            try:
                b.step(x, lab)
            finally:
                H.call = orig
            for buf, k in zip((b.flat.param, b.m, b.v), keep):
                buf.copy_(k)
            b.t -= 1
            assert calls[1] == calls[0] and calls[0].count("vx_adamw_step") == 1
        b.flat.grad.copy_(a.flat.grad)
        b._adamw()
        torch.cuda.synchronize()
        assert torch.equal(a.flat.param, b.flat.param) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v), t
    assert calls[0].count("vx_adamw_step") == 3 and "vx_adamw_step_ex" not in calls[0] and "vx_grad_sqnorm_partials" not in calls[0]
    assert a.t == b.t == 3
    # and the explicit-None engine's own three whole steps (its forward and backward included) track the default engine's at the bars of the eager / tape comparison
    c = TrainEngine(_model(), _crit(), (2, 2, 32, 32, 32), max_grad_norm=None, ema_decay=None)
    la, lc = [], []
    a2 = TrainEngine(_model(), _crit(), (2, 2, 32, 32, 32))
    for _ in range(3):
        la.append(float(a2.step(x, lab)))
        lc.append(float(c.step(x, lab)))
    for u, w in zip(lc, la):
        assert abs(u - w) <= 2e-3 * max(abs(w), 1e-3), (lc, la)
    assert la[-1] != la[0]


# ====================================================================================================================== data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, out_dir, backend, use_graph, max_norm):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from veloxseg_amd.engine import TrainEngine
    cfg, _ = CASES["g2_32_m2"]
    x, lab = make_inputs(cfg, 2)
    per = 2 // world
    eng = TrainEngine(_model(), _crit(), (per, 2, 32, 32, 32), use_graph=use_graph, overlap=True, bucket_min_bytes=1 << 14, force_comm=True, pipeline_tail=use_graph,
                      max_grad_norm=max_norm, ema_decay=DECAY)
    assert eng.dp and eng.world == world
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        eng.step(x[per * rank:per * (rank + 1)].cuda(), lab[per * rank:per * (rank + 1)].cuda())
    eng.flush()
    torch.cuda.synchronize()
    assert eng.use_graph == use_graph
    torch.save({"param": eng.flat.param.cpu(), "ema": eng.ema.cpu(), "coef": eng.clip_coef.cpu(), "norm": eng.grad_norm.cpu(), "grad": (eng.flat.grad / world).cpu()},
               os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("backend,world,use_graph", [("gloo", 2, False), ("gloo", 2, True), ("nccl", 1, True)], ids=["two_ranks_eager", "two_ranks_tape", "one_rank_rccl_tape"])
def test_data_parallel_replicas_clip_alike(tmp_path, backend, world, use_graph):
    """two ranks sharing the GPU over gloo (and the one-rank RCCL group with force_comm): the norm is of the AVERAGED gradient, every rank derives the same coefficient to
    the bit -- otherwise the replicas would drift apart -- and the step equals the single-process step on the concatenated batch"""
    import torch.multiprocessing as mp
    from veloxseg_amd.engine import TrainEngine
    max_norm = 0.5 * _unclipped_norm()
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, str(tmp_path), backend, use_graph, max_norm)) for r in range(world)]
    for p_ in procs:
        p_.start()
    for p_ in procs:
        p_.join(400)
    alive = [p_ for p_ in procs if p_.is_alive()]
    for p_ in alive:
        p_.kill()
    assert not alive and all(p_.exitcode == 0 for p_ in procs), [p_.exitcode for p_ in procs]
    res = [torch.load(os.path.join(str(tmp_path), f"r{r}.pt")) for r in range(world)]
    for r in res[1:]:
        assert torch.equal(r["coef"], res[0]["coef"]) and torch.equal(r["norm"], res[0]["norm"]) and torch.equal(r["param"], res[0]["param"]) and torch.equal(r["ema"], res[0]["ema"])
    assert float(res[0]["coef"]) < 1.0
    cfg, _ = CASES["g2_32_m2"]
    x, lab = make_inputs(cfg, 2)
    eng = TrainEngine(_model(), _crit(), (2, 2, 32, 32, 32), max_grad_norm=max_norm, ema_decay=DECAY)
    eng.step(x.cuda(), lab.cuda())
    torch.cuda.synchronize()
    g_ref = eng.flat.grad.cpu()
    rel = float((res[0]["grad"] - g_ref).norm() / g_ref.norm())
    assert rel < 1e-5, rel                                                     # (the bars of tests/test_dp_gpu.py)
    assert abs(float(res[0]["norm"]) - float(eng.grad_norm)) <= 1e-5 * float(eng.grad_norm)
    assert abs(float(res[0]["coef"]) - float(eng.clip_coef)) <= 1e-5 * float(eng.clip_coef)
    mask = g_ref.abs() > 1e-6
    assert float((res[0]["param"] - eng.flat.param.cpu())[mask].abs().max()) < 1e-6
    assert float((res[0]["ema"] - eng.ema.cpu())[mask].abs().max()) < 1e-6


# ====================================================================================================================== run_train / run_test.py
@pytest.mark.timeout(600)
def test_run_train_with_the_three_config_keys_and_run_test_on_the_ema_checkpoint(tmp_path):
    from test_train_harness_cpu import TRAIN_CFG
    from veloxseg_amd.utils.load_model import load_ema
    from veloxseg_amd.utils.train_loop import SyntheticPatches, run_train
    cfg, _ = CASES["g2_32_m2"]
    tc = copy.deepcopy(dict(TRAIN_CFG, epochs=2, val_interval=1, patch_size={"AutoPETII": [32, 32, 32]}))
    tc["optimizer"]["optimizer_args"]["no_weight_decay"] = "1d"
    tc["optimizer"]["max_grad_norm"] = 12.0
    tc["ema"] = {"decay": 0.5, "validate": True}
    args = types.SimpleNamespace(model_name="VeloxSeg", dataset_name="AutoPETII", checkpoint_path=None, synthetic_steps=2)
    torch.manual_seed(12345)
    val = list(SyntheticPatches(cfg, 2, 1, torch.device("cuda", 0), seed=99))
    h = run_train(args, tc, {"VeloxSeg": cfg}, val_loader=val, save_path=str(tmp_path / "run"))
    eng = h["engine"]
    assert len(h["loss"]) == 2 and h["loss"][-1] < h["loss"][0], h["loss"]
    assert len(h["grad_norm"]) == 2 and all(g > 0 and math.isfinite(g) for g in h["grad_norm"]) and len(h["val_dice"]) == 2
    assert len(eng.optimizer.param_groups) == 2 and eng.max_grad_norm == 12.0 and eng.ema_decay == 0.5 and eng.t == 4
    f = os.path.join(str(tmp_path / "run"), "1.pth")
    ck = torch.load(f)
    assert "ema" in ck and list(ck["ema"]) == list(ck["model"])
    assert any(not torch.equal(ck["ema"][k], ck["model"][k]) for k in ck["model"])
    ema = load_ema(f, torch.device("cuda", 0))
    assert all(torch.equal(v, ema[k]) for k, v in eng.ema_state_dict().items())
    # resume from the epoch-0 checkpoint: the EMA comes back with it, epoch 1 is replayed on the same data
    a2 = types.SimpleNamespace(model_name="VeloxSeg", dataset_name="AutoPETII", checkpoint_path=os.path.join(str(tmp_path / "run"), "0.pth"), synthetic_steps=2)
    h2 = run_train(a2, tc, {"VeloxSeg": cfg}, val_loader=val)
    assert len(h2["loss"]) == 1
    assert abs(h2["loss"][0] - h["loss"][1]) <= 2e-4 * abs(h["loss"][1]), (h2["loss"], h["loss"])
    for k, v in h2["engine"].ema_state_dict().items():
        # (an EMA restarted from the parameters instead of the checkpoint would be off by about decay^2 |p - e| ~ the size of two updates; 1e-4 is a tenth of one lr)
        assert float((v.float() - ck["ema"][k].cuda().float()).abs().max()) <= 1e-4, k
    # run_test.py (unchanged) as a fresh child process on the checkpoint whose "model" entry is the EMA
    from veloxseg_amd.utils.load_model import ema_checkpoint
    fe = ema_checkpoint(f, os.path.join(str(tmp_path / "run"), "1_ema.pth"))
    cke = torch.load(fe)
    assert "ema" not in cke and set(cke) == set(ck) - {"ema"} and all(torch.equal(cke["model"][k].cpu(), ck["ema"][k].cpu()) for k in ck["ema"])
    with pytest.raises(KeyError, match="no \"ema\" entry"):
        ema_checkpoint(fe, os.path.join(str(tmp_path / "run"), "x.pth"))
    # a reader in this package: load_checkpoint(..., weights="ema")
    from veloxseg_amd.utils.load_model import load_checkpoint, load_model
    m_ema = load_checkpoint(load_model("VeloxSeg", {"VeloxSeg": cfg}), f, weights="ema")
    assert all(torch.equal(v.cpu(), ck["ema"][k].cpu()) for k, v in m_ema.state_dict().items())
    with pytest.raises(KeyError, match="no \"ema\" entry"):
        load_checkpoint(load_model("VeloxSeg", {"VeloxSeg": cfg}), fe, weights="ema")
    mc, tcf, te = tmp_path / "models.json", tmp_path / "train.json", tmp_path / "test.json"
    mc.write_text(json.dumps({"VeloxSeg": cfg}))
    tcf.write_text(json.dumps(tc))
    te.write_text(json.dumps({"sliding_window": {"overlap": 0.25}}))
    env = dict(os.environ, PYTHONPATH=ROOT)
    cmd = [sys.executable, os.path.join(ROOT, "run_test.py"), "--dataset_name", "AutoPETII", "--model_name", "VeloxSeg", "--train_config", str(tcf), "--model_config", str(mc),
           "--test_config", str(te), "--checkpoint_dir", str(tmp_path / "run"), "--checkpoint_index", "1_ema", "--synthetic", "1", "--volume_shape", "48", "40", "36"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "synthetic_0" in r.stdout
