"""GPU parity of the whole path: veloxseg_amd.VeloxSeg (+ Loss) vs the CPU oracle and vs the reference-generated goldens.
Bar (fp32): |dlogit| <= 1e-4*max(1,|logit|); argmax bit-exact wherever the oracle's top-2 margin exceeds 1e-4;
loss within 1e-4 relative; parameter gradients within 2e-3 of the oracle's norm."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import veloxseg_oracle as O  # noqa: E402
from recipe import CASES, LOSS_CFG, check_compact, fill_state_dict, make_inputs, unpack_mask  # noqa: E402


def _build(name):
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    cfg_d, B = CASES[name]
    model = VeloxSeg(**cfg_d)
    sd = fill_state_dict(model.state_dict(), seed=7)
    model.load_state_dict(sd)
    x, labels = make_inputs(cfg_d, B)
    return cfg_d, B, model.cuda(), sd, x, labels


@pytest.mark.parametrize("name", list(CASES))
def test_eval_logits_vs_oracle_and_golden(golden_dir, name):
    cfg_d, B, model, sd, x, labels = _build(name)
    model.eval()
    with torch.no_grad():
        logits = model(x.cuda()).cpu()
        ref = O.forward(x, sd, O.OracleConfig(**cfg_d), training=False)
    err = (logits - ref).abs()
    tol = 1e-4 * ref.abs().clamp(min=1.0)
    assert bool((err <= tol).all()), f"max err {float(err.max()):.3e}, bad frac {float((err > tol).float().mean()):.3e}"
    top2 = ref.topk(2, dim=1).values
    confident = (top2[:, 0] - top2[:, 1]) > 1e-4
    am, amr = logits.argmax(1), ref.argmax(1)
    assert bool((am == amr)[confident].all()), "argmax differs on a voxel whose margin exceeds the tolerance"
    fix = torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)
    check_compact(logits, fix["eval_logits"], 2e-4, 2e-4, "eval logits vs reference golden")
    fix["argmax"] = unpack_mask(fix["argmax"])
    mism = float((am.to(torch.uint8) != fix["argmax"]).float().mean())
    assert mism <= 1e-5, f"argmax vs reference golden differs on {mism:.2e} of voxels"
    # Dice delta vs the reference (north-star bar: < 1e-3): Dice of our mask and of the reference's golden mask against the same labels,
    # computed by the on-device metrics (utils/metric): the masks are equal, so the delta is 0 up to the <= 1e-5 voxel allowance above
    from veloxseg_amd.utils.metric import metrics as M, metrics_brats as MB
    lab = labels.cuda()
    ours, theirs = am.to(torch.uint8).unsqueeze(1).cuda(), fix["argmax"].unsqueeze(1).cuda()
    if cfg_d["n_classes"] == 2:
        d_ours, d_ref = M.metrics_tensor(lab, ours)[-1], M.metrics_tensor(lab, theirs)[-1]
    else:
        d_ours, d_ref = MB.cal_dice(ours, lab)[0], MB.cal_dice(theirs, lab)[0]
    assert abs(d_ours - d_ref) < 1e-3, (d_ours, d_ref)


@pytest.mark.parametrize("name", ["g2_32_m2", "g1_48_m2", "g3_64_brats", "g4_aniso_m2", "g5_128_m2", "g6_128_brats", "g7_96_m2"])
def test_train_step_vs_oracle(golden_dir, name):
    from veloxseg_amd.utils.loss import Loss
    import types
    cfg_d, B, model, sd, x, labels = _build(name)
    cfg = O.OracleConfig(**cfg_d)
    model.train()
    outs = model(x.cuda())
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, torch.device("cuda"), num_modal=cfg.M)
    loss = crit(outs, labels.cuda(), sr_labels=x.cuda())
    loss.backward()
    torch.cuda.synchronize()
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if torch.is_floating_point(v)}
    full = dict(sd)
    full.update(params)
    ro = O.forward(x, full, cfg, training=True)
    rl = O.loss(ro, labels, x, cfg.M, LOSS_CFG)
    rl.backward()
    assert len(outs) == len(ro)
    for i, (a, b) in enumerate(zip(outs, ro)):
        err = (a.detach().cpu() - b.detach()).abs()
        tol = 1e-4 * b.detach().abs().clamp(min=1.0)
        assert bool((err <= tol).all()), f"train output {i}: max err {float(err.max()):.3e}"
    assert abs(float(loss) - float(rl)) <= 1e-4 * abs(float(rl)), (float(loss), float(rl))
    bad = []
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        g, r = p.grad.detach().cpu().double(), params[k].grad.double()
        rel = float((g - r).norm() / (r.norm() + 1e-4))      # biases in front of an InstanceNorm / key biases have ~0 gradient
        if rel > 2e-3:
            bad.append((k, rel, float(r.norm())))
    assert not bad, sorted(bad, key=lambda t: -t[1])[:8]
    fix = torch.load(os.path.join(golden_dir, name + ".pt"), weights_only=False)
    if name != "g2_32_m2":
        assert abs(float(loss) - fix["loss"]) <= 1e-4 * abs(fix["loss"])
        for k, p in model.named_parameters():
            gn = float(p.grad.double().norm())
            assert abs(gn - fix["grad_norms"][k]) <= 3e-3 * max(fix["grad_norms"][k], 1e-3), (k, gn, fix["grad_norms"][k])


@pytest.mark.parametrize("name,mode", [("g5_128_m2", "tape"), ("g6_128_brats", "tape"), ("g5_128_m2", "module")])
def test_benchmarked_batch_b4_vs_oracle(name, mode):
    """The BENCHMARKED shapes at the BENCHMARKED batch: bench.py's headline is autopet128 (= g5's model kwargs) at B = 4 per GPU and BASELINE configs[3] is
    brats128 at B = 4 per GPU; the golden cases run B = 1.  One training step at B = 4 (dropout 0, as every oracle comparison) against oracle.forward / loss /
    autograd: loss 1e-4 relative, every parameter gradient 2e-3 of the oracle's norm.  mode "tape": through TrainEngine with launch tapes, staged loss and the fused
    deep-supervision loss -- the path the bench line times (gradients read from the engine's flat buffer); mode "module": the plain nn.Module + Loss + backward."""
    import types
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg_d, _ = CASES[name]
    B = 4
    model = VeloxSeg(**cfg_d)
    sd = fill_state_dict(model.state_dict(), seed=7)
    model.load_state_dict(sd)
    model = model.cuda().train()
    x, labels = make_inputs(cfg_d, B)
    cfg = O.OracleConfig(**cfg_d)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, torch.device("cuda"), num_modal=cfg.M)
    if mode == "tape":
        eng = TrainEngine(model, crit, (B, sum(cfg_d["in_ch"]), *cfg_d["input_size"]), lr=0.0, weight_decay=0.0, use_graph=True, overlap=False)
        loss = float(eng.step(x.cuda(), labels.cuda()))
        torch.cuda.synchronize()
        assert eng.use_graph and eng.graphs is not None, "the capture's self-check failed: the step did not run as launch tapes"
        loss = float(eng.step())                 # a REPLAYED step (lr = 0: same parameters), the thing the bench times
        torch.cuda.synchronize()
        grads = {}
        for n, p in zip(eng.flat.names, eng.flat.params):
            o, k = eng.flat.slices[n]
            grads[n] = eng.flat.grad[o:o + k].view(p.shape).detach().cpu().double()
    else:
        outs = model(x.cuda())
        lt = crit(outs, labels.cuda(), sr_labels=x.cuda())
        lt.backward()
        torch.cuda.synchronize()
        loss = float(lt)
        grads = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters()}
    params = {k: v.clone().requires_grad_(True) for k, v in sd.items() if torch.is_floating_point(v)}
    full = dict(sd)
    full.update(params)
    ro = O.forward(x, full, cfg, training=True)
    rl = O.loss(ro, labels, x, cfg.M, LOSS_CFG)
    rl.backward()
    assert abs(loss - float(rl)) <= 1e-4 * abs(float(rl)), (loss, float(rl))
    bad = []
    for k in grads:
        r = params[k].grad.double()
        rel = float((grads[k] - r).norm() / (r.norm() + 1e-4))
        if rel > 2e-3:
            bad.append((k, rel, float(r.norm())))
    assert len(grads) == len([k for k, _ in model.named_parameters()])
    assert not bad, sorted(bad, key=lambda t: -t[1])[:8]


def test_cpu_input_fails_loudly():
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    cfg_d, B = CASES["g2_32_m2"]
    model = VeloxSeg(**cfg_d)
    with pytest.raises(RuntimeError, match="MI355X"):
        model(torch.zeros(1, 2, 32, 32, 32))


def test_full_size_properties_128():
    """BASELINE-size (128^3, M=2, windows [4,8,4,4]) size-independent checks: per-sample independence of the batch
    (every op is per-sample), finite loss, gradient of every parameter present and finite."""
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    import types
    cfg = dict(CASES["g1_48_m2"][0], input_size=[128, 128, 128], patch_size=4, min_big_window_sizes=[[4] * 3, [8] * 3, [4] * 3, [4] * 3])
    torch.manual_seed(1)
    model = VeloxSeg(**cfg).cuda()
    x = torch.randn(2, 2, 128, 128, 128, device="cuda")
    lab = (torch.rand(2, 1, 128, 128, 128, device="cuda") > 0.97).long()
    model.eval()
    with torch.no_grad():
        both = model(x)
        one = model(x[1:2].contiguous())
    assert torch.equal(both[1:2], one), "batch samples must not interact"
    model.train()
    outs = model(x)
    loss = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=2)(outs, lab, sr_labels=x)
    loss.backward()
    assert torch.isfinite(loss)
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k


def test_engine_graph_and_two_phase_backward_match_plain_step(golden_dir):
    """TrainEngine: (a) the staged pass (enc_fwd, dec_fwd[k], loss, dec_bwd[k], enc_bwd with detached leaves in between) that
    the per-stage hipGraphs are captured from gives the same gradients as one plain backward; (b) the hipGraph-captured step reproduces the eager step; (c) the fused AdamW moves the flat parameters."""
    import types
    from veloxseg_amd import functional as VF
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg_d, B = CASES["g2_32_m2"]
    x, labels = make_inputs(cfg_d, 2)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=2)

    def make(use_graph):
        torch.manual_seed(3)
        model = VeloxSeg(**cfg_d).cuda()
        VF.manual_seed(99, "cuda")
        return TrainEngine(model, crit, (2, 2, 32, 32, 32), use_graph=use_graph, overlap=False)

    e1 = make(False)
    e1.x.copy_(x.cuda()); e1.labels.copy_(labels.cuda())
    e1.model.train()
    e1.flat.reattach()
    e1._fwd_bwd_single()
    g_single = e1.flat.grad.clone()
    VF.manual_seed(99, "cuda")
    e1._eager_pass()                       # the staged pass (detached leaves at the encoder and decoder outputs)
    torch.cuda.synchronize()
    assert float((e1.flat.grad - g_single).abs().max()) <= 1e-5 * float(g_single.abs().max()), "staged backward differs"
    assert e1.flat.split > 0 and e1.flat.split < e1.flat.numel
    # graph vs eager, 3 optimisation steps each (dropout p=0 in this config => deterministic)
    ea, eb = make(False), make(True)
    la = [float(ea.step(x.cuda(), labels.cuda())) for _ in range(3)]
    lb = [float(eb.step(x.cuda(), labels.cuda())) for _ in range(3)]
    assert all(abs(a - b) <= 2e-4 * abs(a) for a, b in zip(la, lb)), (la, lb)
    assert la[2] < la[0], "three AdamW steps on a fixed batch must reduce the loss"
    assert float((ea.flat.param - eb.flat.param).abs().max()) < 5e-4


def test_graph_replay_after_device_sync_matches_eager():
    """Regression for the ROCm 7.2 single-chain graph replay fault (veloxseg_amd/__init__.py): replays separated by
    hipDeviceSynchronize used to return garbage (loss 1e6 .. inf) from the second replay on at 128^3.  The engine's multi-branch
    capture must survive its own self-check (use_graph stays True) and track the eager step, dropout streams included."""
    import types
    from bench import LOSS_CFG as BL, WORKLOADS, synth
    from veloxseg_amd import functional as VF
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg, _ = WORKLOADS["autopet128"]
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), BL, None, num_modal=2)
    x, lab = synth(cfg, 1, "cuda", 12345)
    losses = {}
    for use_graph in (False, True):
        torch.manual_seed(12345)
        model = VeloxSeg(**cfg).cuda()
        VF.manual_seed(5, "cuda")
        eng = TrainEngine(model, crit, (1, 2, 128, 128, 128), use_graph=use_graph, overlap=False)
        assert eng.use_graph == use_graph
        out = []
        for it in range(5):
            l = eng.step(x, lab) if it == 0 else eng.step()
            torch.cuda.synchronize()
            out.append(float(l))
        assert eng.use_graph == use_graph, "graph self-check failed: engine fell back to eager launches"
        losses[use_graph] = out
        del eng, model
    for a, b in zip(losses[False], losses[True]):
        assert abs(a - b) <= 2e-3 * abs(a), losses
    assert losses[True][-1] < losses[True][0]


def test_composite_blocks_equal_the_fine_grained_operators():
    """functional.USE_COMPOSITE (one autograd node per JLC block / FFN tail) runs the same kernels in the same order as the per-operator
    graph: outputs, loss and every gradient agree to summation-order noise, with dropout active (same Philox streams)."""
    import types
    from veloxseg_amd import functional as VF
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg_d, _ = CASES["g2_32_m2"]
    cfg_d = dict(cfg_d, proj_drop=0.1, conv_drop=0.1, attn_drop=0.1)
    x, labels = make_inputs(cfg_d, 2)
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=2)
    res = {}
    try:
        for flag in (True, False):
            VF.USE_COMPOSITE = flag
            torch.manual_seed(11)
            model = VeloxSeg(**cfg_d).cuda().train()
            VF.manual_seed(123, "cuda")
            out = model(x.cuda())
            loss = crit(out, labels.cuda(), sr_labels=x.cuda())
            loss.backward()
            torch.cuda.synchronize()
            res[flag] = (float(loss), [o.detach().clone() for o in out], {n: p.grad.clone() for n, p in model.named_parameters()})
            with torch.no_grad():
                model.eval()
                res[flag] += (model(x.cuda()).clone(),)
    finally:
        VF.USE_COMPOSITE = True
    assert abs(res[True][0] - res[False][0]) <= 1e-6 * abs(res[False][0])
    for a, b in zip(res[True][1], res[False][1]):        # (the Gram outputs are float-atomic sums: equal to round-off, not bit for bit; the fused
        # epilogues -- GELU, residual + dropout inside the 1x1 convs -- round alpha*res + mask*conv in a different order than the separate kernels: 1-2 ulp)
        assert float((a - b).abs().max()) <= 2e-5 * max(1.0, float(b.abs().max()))
    # eval logits: the composite path runs the fused block kernels (csrc/jlc.hip, csrc/mlp.hip: other summation order, GELU through the
    # A&S 7.1.26 erf with <= 3e-7 absolute error), the per-operator path erff and separate kernels: equal to fp32 noise, not bit for bit
    assert float((res[True][3] - res[False][3]).abs().max()) <= 2e-5 * max(1.0, float(res[False][3].abs().max()))
    for n, g in res[False][2].items():
        d_ = float((res[True][2][n] - g).abs().max())
        # floor 1e-6: biases in front of an InstanceNorm have a mathematically zero gradient; what both paths compute for them is ~1e-8 of
        # summation-order noise (float atomics), which differs from run to run
        assert d_ <= 2e-4 * max(0.1, float(g.abs().max())), (n, d_)          # fused blocks: fp32-noise differences in the forward, amplified at the 4^3 level


@pytest.mark.timeout(600)
def test_first_step_of_a_fresh_process_matches_serialised_kernels(tmp_path):
    """Multi-stream safety: the very first training step of a fresh process (cold caching allocator, streams just created) must give the
    same loss and gradients as the same step with AMD_SERIALIZE_KERNEL=3.  A tensor read on a forked stream without record_stream used to
    be recycled by the allocator while its reader was still queued: one weight gradient came out ~0 in the first step only."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "dbg_first_iter.py")
    ref = str(tmp_path / "ref.pt")
    env = dict(os.environ, PYTHONPATH=root)
    r = subprocess.run([sys.executable, tool, "save", ref], env=dict(env, AMD_SERIALIZE_KERNEL="3"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-1500:]
    for _ in range(3):
        r = subprocess.run([sys.executable, tool, "cmp", ref], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-1500:]
        assert "\n0 bad params" in r.stdout, r.stdout[-800:]


def test_two_forwards_before_their_backwards_keep_their_dropout_masks():
    """Every training forward snapshots its own {seed, step} dropout state (functional.advance_rng): forward(x1), forward(x2), backward(1),
    backward(2) must give the gradients of the two separate forward/backward pairs -- the masks a backward regenerates are those of ITS forward."""
    import types
    from veloxseg_amd import functional as VF
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    VF.RNG_INPLACE = False
    cfg_d = dict(CASES["g2_32_m2"][0], proj_drop=0.1, conv_drop=0.1, attn_drop=0.1)
    torch.manual_seed(4)
    model = VeloxSeg(**cfg_d).cuda().train()
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=2)
    xs = [make_inputs(cfg_d, 1, seed=31 + k) for k in range(2)]

    def grads():
        g = {n: p.grad.clone() for n, p in model.named_parameters()}
        for p in model.parameters():
            p.grad.zero_()
        return g

    def loss_of(k, outs):
        return crit(outs, xs[k][1].cuda(), sr_labels=xs[k][0].cuda())

    VF.manual_seed(5, "cuda")
    ref = []
    for k in range(2):
        loss_of(k, model(xs[k][0].cuda())).backward()
        torch.cuda.synchronize()
        ref.append(grads())
    VF.manual_seed(5, "cuda")
    outs = [model(xs[k][0].cuda()) for k in range(2)]          # two forwards in flight
    got = []
    for k in range(2):
        loss_of(k, outs[k]).backward()
        torch.cuda.synchronize()
        got.append(grads())
    for k in range(2):
        for n, g in ref[k].items():
            d_ = float((got[k][n] - g).abs().max())
            assert d_ <= 2e-4 * max(0.1, float(g.abs().max())), (k, n, d_)
