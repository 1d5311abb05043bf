"""Dropout ON: the HIP kernels against the CPU oracle applying the SAME masks.

The product's dropout masks are a pure function of ({seed, step}, site id, element index) (veloxseg_amd/csrc/vx_common.h), restated in
numpy by oracle/philox.py (pinned by tests/test_dropout_cpu.py); the oracle applies them through forward(masks=) at the places the reference
drops (pinned against the reference itself by tests/test_oracle_golden.py::test_train_dropout_masks_vs_reference).  So a training step with
dropout on is held to the same bars as at p = 0: a mask index that leaves out the batch or modality offset, two sites on one stream, a mask
applied before instead of after a residual add, a wrong keep scale or a step counter that does not advance fail here even when every kernel
shares the mistake.

Attention sites draw 16 random bits per decision: p is represented as thr16 / 65536 (6554 / 65536 = 0.100006 at p = 0.1) and kept weights
are scaled by 65536 / (65536 - thr16); the restatement does the same, so the comparisons below are exact in the masks.
"""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import philox as P  # noqa: E402
from oracle import veloxseg_oracle as O  # noqa: E402
from recipe import CASES, DROP_CASES, DROP_SEED, DROP_STEP, LOSS_CFG, dropout_sites, fill_state_dict, make_inputs  # noqa: E402

SEED = 0x2_0000_0011          # >= 2^32: the high key word matters


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


def _set_rng(seed, step):
    import veloxseg_amd.functional as VF
    VF.rng_state(_dev()).copy_(torch.tensor([seed, step], dtype=torch.int64))


def _rng():
    import veloxseg_amd.functional as VF
    return [int(v) for v in VF.rng_state(_dev()).cpu()]


# ---------------------------------------------------------------------------------------------------------------------------------
# a. device masks equal the restatement bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 5, 4099, 1 << 20])
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_residual_dropout_masks_bit_exact(n, p):
    """VF.residual_dropout(None, ones, 0, p, site) returns the mask itself (0 or the fp32 keep scale 1 / (1 - p)); its backward multiplies
    by the same mask"""
    import veloxseg_amd.functional as VF
    for seed, step, site in ((SEED, 1, 7), (0x7FFF_FFFF_0000_0003, 12345, 301)):
        _set_rng(seed, step)
        z = torch.ones(n, device="cuda", requires_grad=True)
        out = VF.residual_dropout(None, z, 0.0, p, site)
        g = torch.randn(n, device="cuda")
        out.backward(g)
        torch.cuda.synchronize()
        ref = P.site_scales(seed, step, site, n, p)
        assert torch.equal(out.detach().cpu(), ref), (n, p, int((out.detach().cpu() != ref).sum()))
        assert torch.equal(z.grad.cpu(), g.cpu() * ref)
        assert _rng() == [seed, step], "a dropout op must not move the step counter"


@pytest.mark.parametrize("shape", [(1, 1, 3, 5, 7), (2, 12, 3, 3, 3), (3, 20, 5, 6, 7)])
@pytest.mark.parametrize("p", [0.1, 0.3])
def test_gelu_and_axpy_dropout_vs_fp64(shape, p):
    """GELU-drop (forward and backward) and the residual axpy with dropout (out = alpha * x + Drop(z)) at lengths that are not multiples of 4,
    against fp64 references that apply the restated masks"""
    import veloxseg_amd.functional as VF
    g = torch.Generator().manual_seed(11)
    a = torch.randn(shape, generator=g)
    dh = torch.randn(shape, generator=g)
    site, step = 23, 4
    _set_rng(SEED, step)
    ad = a.cuda().requires_grad_(True)
    h = VF.gelu_dropout(ad, p, site)
    h.backward(dh.cuda())
    torch.cuda.synchronize()
    m = P.site_scales(SEED, step, site, a.numel(), p).view(shape).double()
    a64 = a.double().requires_grad_(True)
    ref = 0.5 * a64 * (1 + torch.erf(a64 / 2 ** 0.5)) * m
    ref.backward(dh.double())
    torch.testing.assert_close(h.detach().cpu().double(), ref.detach(), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(ad.grad.cpu().double(), a64.grad, atol=1e-5, rtol=1e-5)
    x = torch.randn(shape, generator=g)
    xd, zd = x.cuda().requires_grad_(True), a.cuda().requires_grad_(True)
    out = VF.residual_dropout(xd, zd, 2.0, p, site + 1)
    out.backward(dh.cuda())
    torch.cuda.synchronize()
    m2 = P.site_scales(SEED, step, site + 1, a.numel(), p).view(shape).double()
    torch.testing.assert_close(out.detach().cpu().double(), 2.0 * x.double() + a.double() * m2, atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(xd.grad.cpu().double(), 2.0 * dh.double(), atol=1e-6, rtol=1e-6)
    torch.testing.assert_close(zd.grad.cpu().double(), dh.double() * m2, atol=1e-6, rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. the kernels that draw masks inside fused blocks, at shapes where index code breaks
# ---------------------------------------------------------------------------------------------------------------------------------
BLOCKS = [
    # (grid, window, M, C, heads, min_dim_head, ffn ratio, B): ML = M * l
    ([6, 6, 6], [3, 3, 3], 1, 12, 1, 4, 3, 2),       # l = 27 (ML % 4 != 0), C % 16 != 0, V = 216
    ([6, 6, 6], [3, 3, 3], 2, 16, 1, 4, 3, 2),       # ML = 54
    ([6, 6, 6], [3, 3, 3], 3, 16, 1, 4, 2, 2),       # ML = 81, M = 3
    ([6, 6, 4], [3, 3, 2], 2, 16, 2, 4, 3, 2),       # ML = 36 (% 8 != 0), two heads
    ([8, 8, 8], [2, 2, 2], 2, 16, 1, 4, 3, 3),       # ML = 16, three scales, B = 3
    ([12, 12, 12], [3, 3, 3], 2, 32, 2, 8, 3, 2),    # the g1 level-1 geometry: scales 3, 6, 12
    ([32, 32, 32], [4, 4, 4], 2, 16, 1, 4, 3, 1),    # V = 32768 > 16384 (vx_mlp_tpw switch), ML = 128: the headline level-1 geometry
    ([3, 3, 3], [3, 3, 3], 2, 16, 1, 4, 3, 2),       # V = 27 (% 4 != 0), one window, ML = 54
]


@pytest.mark.parametrize("geom", BLOCKS, ids=lambda g: f"g{'x'.join(map(str, g[0]))}_w{'x'.join(map(str, g[1]))}_M{g[2]}_C{g[3]}_h{g[4]}_B{g[7]}")
def test_transformer_block_dropout_vs_oracle(geom):
    """one Paired_Windows_TransformerBlock (attention forward / backward, mix conv + residual + dropout, the fused FFN tail with GELU-drop and
    both MLP dropout sites) with every rate 0.1, forward and backward, against oracle.pwa_block with the restated masks"""
    from veloxseg_amd.model.components.PWA import Paired_Windows_TransformerBlock
    grid, win, M, C, heads, mdh, r, B = geom
    torch.manual_seed(5)
    blk = Paired_Windows_TransformerBlock(input_size=grid, in_channels=[C] * M, min_big_window_size=win, num_heads=heads, min_dim_head=mdh,
                                          attn_drop=0.1, proj_drop=0.1, drop_path=0.0, ffn_expansion_ratio=r, dim=3)
    sd = {k: v.clone() for k, v in blk.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    for k, v in sd.items():
        if torch.is_floating_point(v):
            v.add_(0.1 * torch.randn(v.shape, generator=g))
    blk.load_state_dict(sd)
    blk = blk.cuda().train()
    sites = dropout_sites(blk)
    assert len(sites) == 1 + M + 2 * M
    xs = [torch.randn(B, C, *grid, generator=g) for _ in range(M)]
    gys = [torch.randn(B, C, *grid, generator=g) for _ in range(M)]
    step = 6
    _set_rng(SEED, step)
    xd = [x.cuda().requires_grad_(True) for x in xs]
    ys = blk(xd)
    torch.autograd.backward(ys, [gy.cuda() for gy in gys])
    torch.cuda.synchronize()
    plan = O.plan_pwa(grid, win, [1, 1, 1], 2, heads, mdh, C)
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if torch.is_floating_point(v)}
    full = dict(sd)
    full.update(params)
    xr = [x.clone().requires_grad_(True) for x in xs]
    masks = dict(seed=SEED, step=step, sites=sites)
    refs = O.pwa_block(xr, full, "", plan, dict(attn=0.1, proj=0.1), True, masks)
    torch.autograd.backward(refs, gys)
    for m in range(M):
        a, b = ys[m].detach().cpu(), refs[m].detach()
        err = (a - b).abs()
        assert bool((err <= 1e-4 * b.abs().clamp(min=1.0)).all()), (m, float(err.max()))
        gx, gr = xd[m].grad.cpu().double(), xr[m].grad.double()
        assert float((gx - gr).norm() / gr.norm()) <= 2e-4, (m, float((gx - gr).norm() / gr.norm()))
    bad = []
    for k, p in blk.named_parameters():
        gp, gr = p.grad.detach().cpu().double(), params[k].grad.double()
        wn = float(params[k[:-len("bias")] + "weight"].grad.norm()) if (".qkv_proj." in k and k.endswith(".1.bias")) else 0.0
        if float(gr.norm()) <= 1e-4 * wn:
            # a key bias of a one-modality block: it shifts a query's scores by a constant, the soft-max ignores it (with or without dropout
            # after it) and its gradient is round-off on both sides; held to that level against the key weights' gradient
            assert float(gp.norm()) <= 1e-4 * wn, (k, float(gp.norm()), float(gr.norm()), wn)
            continue
        rel = float((gp - gr).norm() / (gr.norm() + 1e-4))
        if rel > 2e-3:
            bad.append((k, rel))
    assert not bad, bad
    # the masks are what makes the two agree: the oracle at another step is far away
    far = O.pwa_block(xs, sd, "", plan, dict(attn=0.1, proj=0.1), True, dict(masks, step=step + 1))
    assert max(float((ys[m].detach().cpu() - far[m]).abs().max()) for m in range(M)) > 1e-2


# ---------------------------------------------------------------------------------------------------------------------------------
# c. the whole network at the configured p = 0.1 at every site
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(cfg_d):
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    model = VeloxSeg(**cfg_d)
    sd = fill_state_dict(model.state_dict(), seed=7)
    model.load_state_dict(sd)
    return model.cuda().train(), sd, dropout_sites(model)


def _oracle_step(x, labels, sd, cfg, masks):
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if torch.is_floating_point(v)}
    full = dict(sd)
    full.update(params)
    ro = O.forward(x, full, cfg, training=True, masks=masks)
    rl = O.loss(ro, labels, x, cfg.M, LOSS_CFG)
    rl.backward()
    return [t.detach() for t in ro], float(rl.detach()), {k: p.grad.double() for k, p in params.items()}


def _check(outs, loss, grads, ref, what, which=None):
    ro, rl, rg = ref
    if outs is not None:
        assert len(outs) == len(ro)
        for i, (a, b) in enumerate(zip(outs, ro)):
            if which is not None and i not in which:
                continue
            err = (a.detach().float().cpu() - b).abs()
            tol = 1e-4 * b.abs().clamp(min=1.0)
            assert bool((err <= tol).all()), f"{what}: train output {i}: max err {float(err.max()):.3e}"
    assert abs(loss - rl) <= 1e-4 * abs(rl), (what, loss, rl)
    bad = []
    for k, r in rg.items():
        rel = float((grads[k] - r).norm() / (r.norm() + 1e-4))
        if rel > 2e-3:
            bad.append((k, rel, float(r.norm())))
    assert not bad, (what, sorted(bad, key=lambda t: -t[1])[:8])


def _engine_grads(eng):
    out = {}
    for n, p in zip(eng.flat.names, eng.flat.params):
        o, k = eng.flat.slices[n]
        out[n] = eng.flat.grad[o:o + k].view(p.shape).detach().cpu().double()
    return out


def _check_fixture(golden_dir, loss, grads):
    import os
    fix = torch.load(os.path.join(golden_dir, "g1_48_m2_drop.pt"), weights_only=False)
    assert abs(loss - fix["loss"]) <= 1e-4 * abs(fix["loss"]), (loss, fix["loss"])
    for k, g in grads.items():
        gn = float(g.norm())
        assert abs(gn - fix["grad_norms"][k]) <= 3e-3 * max(fix["grad_norms"][k], 1e-3), (k, gn, fix["grad_norms"][k])


def test_g1_drop_module_path_vs_oracle_and_reference(golden_dir):
    """g1_48_m2 at B = 2 with p = 0.1 at every site through the plain nn.Module + Loss + backward: a training forward advances the step
    counter first (VeloxSeg.forward -> VF.advance_rng) and draws {seed, step + 1}; outputs, loss and every parameter gradient against the
    oracle at that step, loss and gradient norms against the reference's own dropout-on step (g1_48_m2_drop.pt)"""
    from veloxseg_amd.utils.loss import Loss
    cfg_d, B = DROP_CASES["g1_48_m2_drop"]
    model, sd, sites = _model(cfg_d)
    cfg = O.OracleConfig(**cfg_d)
    x, labels = make_inputs(cfg_d, B)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, torch.device("cuda"), num_modal=cfg.M)
    _set_rng(DROP_SEED, DROP_STEP - 1)
    outs = model(x.cuda())
    assert _rng() == [DROP_SEED, DROP_STEP]
    loss = crit(outs, labels.cuda(), sr_labels=x.cuda())
    loss.backward()
    torch.cuda.synchronize()
    grads = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters()}
    ref = _oracle_step(x, labels, sd, cfg, dict(seed=DROP_SEED, step=DROP_STEP, sites=sites))
    _check(outs, float(loss), grads, ref, "module")
    _check_fixture(golden_dir, float(loss), grads)


def test_g1_drop_taped_steps_vs_oracle(golden_dir):
    """the same case through TrainEngine's launch tapes (lr = 0): the capture's warm-up and self-check restore {seed, step}, and every replayed
    step bumps the step word in place at the head of its encoder forward (engine._s_enc_fwd, RNG_INPLACE) -- so from {seed, s} the k-th
    step draws {seed, s + k}.  Three consecutive steps, each against the oracle at its own step number; the first also against the
    reference's fixture"""
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.utils.loss import Loss
    cfg_d, B = DROP_CASES["g1_48_m2_drop"]
    model, sd, sites = _model(cfg_d)
    cfg = O.OracleConfig(**cfg_d)
    x, labels = make_inputs(cfg_d, B)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, torch.device("cuda"), num_modal=cfg.M)
    eng = TrainEngine(model, crit, (B, sum(cfg_d["in_ch"]), *cfg_d["input_size"]), lr=0.0, weight_decay=0.0, use_graph=True, overlap=False)
    _set_rng(DROP_SEED, DROP_STEP - 1)
    seen = []
    for k in range(3):
        loss = float(eng.step(x.cuda(), labels.cuda()) if k == 0 else eng.step())
        torch.cuda.synchronize()
        assert eng.use_graph and eng.graphs is not None, "the capture's self-check failed: the step did not run as launch tapes"
        step = DROP_STEP + k
        assert _rng() == [DROP_SEED, step], (k, _rng())
        grads = _engine_grads(eng)
        ref = _oracle_step(x, labels, sd, cfg, dict(seed=DROP_SEED, step=step, sites=sites))
        _check(eng.last_outputs, loss, grads, ref, f"taped step {k + 1}", which=(0, 4))      # full-resolution logits, reconstructions
        if k == 0:
            _check_fixture(golden_dir, loss, grads)
        seen.append(loss)
    assert len(set(seen)) == 3, seen          # new masks every step


def test_g5_b4_drop_taped_step_vs_oracle():
    """the benchmarked path: g5_128_m2 (autopet128's model) at B = 4 with p = 0.1 at every site, one replayed taped step against the oracle"""
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.utils.loss import Loss
    cfg_d = dict(CASES["g5_128_m2"][0], proj_drop=0.1, conv_drop=0.1, attn_drop=0.1)
    B = 4
    model, sd, sites = _model(cfg_d)
    cfg = O.OracleConfig(**cfg_d)
    x, labels = make_inputs(cfg_d, B)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, torch.device("cuda"), num_modal=cfg.M)
    eng = TrainEngine(model, crit, (B, sum(cfg_d["in_ch"]), *cfg_d["input_size"]), lr=0.0, weight_decay=0.0, use_graph=True, overlap=False)
    _set_rng(SEED, 40)
    eng.step(x.cuda(), labels.cuda())
    loss = float(eng.step())
    torch.cuda.synchronize()
    assert eng.use_graph and eng.graphs is not None
    assert _rng() == [SEED, 42]
    ref = _oracle_step(x, labels, sd, cfg, dict(seed=SEED, step=42, sites=sites))
    _check(None, loss, _engine_grads(eng), ref, "g5 B=4 tape")


# ---------------------------------------------------------------------------------------------------------------------------------
# d. bf16 storage mode with dropout on
# ---------------------------------------------------------------------------------------------------------------------------------
def test_bf16_storage_taped_step_with_dropout_vs_oracle():
    """g5_128_m2 at B = 2 in the bf16 storage mode (16-bit block-internal tensors and heads) through the tapes, p = 0.1 at every site, against
    the fp32 oracle with the same masks, at the gates of test_bf16_gpu.test_bf16_storage_mode_taped_step_vs_oracle: loss within 1 %, logits and
    reconstructions within 1e-2 relative RMS, flat gradient within 3e-2 relative RMS"""
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.utils.loss import Loss
    cfg_d = dict(CASES["g5_128_m2"][0], proj_drop=0.1, conv_drop=0.1, attn_drop=0.1)
    B = 2
    model, sd, sites = _model(cfg_d)
    cfg = O.OracleConfig(**cfg_d)
    x, labels = make_inputs(cfg_d, B)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, torch.device("cuda"), num_modal=cfg.M)
    eng = TrainEngine(model, crit, (B, sum(cfg_d["in_ch"]), *cfg_d["input_size"]), lr=0.0, weight_decay=0.0, use_graph=True, overlap=False, precision="bf16")
    _set_rng(SEED, 7)
    eng.step(x.cuda(), labels.cuda())
    loss = float(eng.step())
    torch.cuda.synchronize()
    assert eng.use_graph and eng.graphs is not None
    assert _rng() == [SEED, 9]
    outs = eng.last_outputs
    assert outs[0].dtype == torch.bfloat16
    ro, rl, rg = _oracle_step(x, labels, sd, cfg, dict(seed=SEED, step=9, sites=sites))
    assert abs(loss - rl) <= 1e-2 * abs(rl), (loss, rl)
    for i in (0, 4):
        a, r = outs[i].float().cpu(), ro[i]
        assert float((a - r).norm() / r.norm()) <= 1e-2, (i, float((a - r).norm() / r.norm()))
    grads = _engine_grads(eng)
    num = sum(float((grads[k] - rg[k]).pow(2).sum()) for k in rg)
    den = sum(float(rg[k].pow(2).sum()) for k in rg)
    assert (num / den) ** 0.5 <= 3e-2, (num / den) ** 0.5
