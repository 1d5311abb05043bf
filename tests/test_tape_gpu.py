"""Launch tape (csrc/tape.hip): a captured hipGraph read back and replayed as plain launches on several streams must compute what the
eager launches compute -- kernels from host stubs (aten, this library), module kernels (rocBLAS), memset and memcpy nodes, forked
streams -- and TrainEngine(use_graph=True, replay="tape") must track the eager engine step for step (dropout streams included)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _capture(fn):
    from veloxseg_amd.engine import LaunchTape
    g = torch.cuda.CUDAGraph(keep_graph=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()                                   # warm-up: lazy initialisation outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        out = fn()
    return LaunchTape(g, 6), out


def test_tape_replays_kernels_memsets_and_forked_streams():
    import veloxseg_amd.functional as VF
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x = torch.randn(2, 8, 16, 16, 16, device=dev)
    w = torch.randn(8, 8, 1, 1, 1, device=dev)
    a = torch.randn(64, 64, device=dev)
    side = torch.cuda.Stream()

    def fn():
        cur = torch.cuda.current_stream()
        z = torch.zeros(1000, device=dev)                      # memset node
        y = VF.conv3d(x, w, None)                              # this library's kernel (host stub)
        side.wait_stream(cur)
        with torch.cuda.stream(side):                          # forked branch
            m = a @ a                                          # rocBLAS kernel
            m2 = m * 1.0
            m2.record_stream(cur)
        y2 = torch.nn.functional.gelu(y) + 1.0                 # aten elementwise
        cur.wait_stream(side)
        return y2.sum() + m2.sum() + z.sum(), y2, m2

    tape, (tot, y2, m2) = _capture(fn)
    assert tape.n_kernels >= 4 and tape.n_lanes >= 2, (tape.n_nodes, tape.n_kernels, tape.n_lanes)
    with torch.no_grad():
        for trial in range(3):
            x.normal_()
            a.normal_()
            torch.cuda.synchronize()
            tape.replay()
            torch.cuda.synchronize()
            ref_y2 = torch.nn.functional.gelu(torch.nn.functional.conv3d(x, w)) + 1.0
            ref_m = a @ a
            assert torch.allclose(y2, ref_y2, atol=1e-4, rtol=1e-4)
            assert torch.allclose(m2, ref_m, atol=1e-3, rtol=1e-4)
            assert torch.allclose(tot, ref_y2.sum() + ref_m.sum(), rtol=1e-4, atol=1e-1)


def test_tape_replays_memcpy_nodes():
    """aten copies contiguous tensors with hipMemcpyAsync (clone(), torch.cat over dim 1 at batch 1): those nodes cannot be read back on ROCm 7.2
    and are replayed as one-node graphs"""
    dev = torch.device("cuda:0")
    a = torch.randn(1, 3, 1000, device=dev)
    b = torch.randn(1, 2, 1000, device=dev)
    tape, out = _capture(lambda: torch.cat([a, b], dim=1).clone() * 2.0)
    for _ in range(2):
        a.normal_()
        b.normal_()
        tape.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, torch.cat([a, b], dim=1) * 2.0)


def test_engine_tape_replay_tracks_the_eager_engine():
    import os, sys, types
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from recipe import CASES, LOSS_CFG, make_inputs
    import veloxseg_amd.functional as VF
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg_d = dict(CASES["g2_32_m2"][0], proj_drop=0.1, conv_drop=0.1, attn_drop=0.1)
    x, lab = make_inputs(cfg_d, 2)
    x, lab = x.cuda(), lab.cuda()
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=2)
    res = {}
    import veloxseg_amd.engine as E
    for mode in ("eager", "tape", "tape_pgo", "graph"):      # tape_pgo: the encoder tapes laid out again from measured node durations (vx_tape_build_pgo)
        VF.reset_dropout_sites()
        torch.manual_seed(11)
        model = VeloxSeg(**cfg_d).cuda()
        VF.manual_seed(77, "cuda")
        E.TAPE_PGO = mode == "tape_pgo"                  # (read when the first step captures)
        eng = TrainEngine(model, crit, (2, 2, 32, 32, 32), use_graph=mode != "eager", replay="graph" if mode == "graph" else "tape", overlap=False)
        losses = []
        for it in range(4):
            losses.append(float(eng.step(x, lab)))
            torch.cuda.synchronize()
        E.TAPE_PGO = False
        assert eng.use_graph == (mode != "eager"), "self-check of the captured stages failed: the engine fell back to eager launches"
        if mode in ("tape", "tape_pgo"):
            tapes = [eng.graphs["enc_fwd"], eng.graphs["enc_bwd"]] + eng.graphs["dec_fwd"] + eng.graphs["dec_bwd"]
            assert all(t.n_kernels > 0 for t in tapes) and eng.graphs["enc_fwd"].n_lanes >= 2      # modality / conv-chain branches on their own lanes
        res[mode] = (losses, eng.flat.param.detach().clone())
        del eng, model
    for mode in ("tape", "tape_pgo", "graph"):
        for a, b in zip(res[mode][0], res["eager"][0]):
            assert abs(a - b) <= 2e-3 * abs(b), (mode, res[mode][0], res["eager"][0])
        assert float((res[mode][1] - res["eager"][1]).abs().max()) < 2e-3, mode


def test_eager_stages_are_reproducible_at_full_size_brats128_b4():
    """Regression (round 2): the deferred weight-gradient closures allocate their temporaries when they are launched.  Taken from the CALLING stream's
    pool and used on the launch stream, a recycled block was still being read by the level-1 attention backward queued on the calling stream:
    from the third pass on (allocator cache warm) the eager passes of TrainEngine(use_graph=True) disagreed with each other by 5e-2 and the
    capture's self-check fell back to eager launches.  Same weights, same dropout streams => every pass and the tape replay agree."""
    import types
    from bench import LOSS_CFG, WORKLOADS, synth
    from veloxseg_amd import functional as VF
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg, _ = WORKLOADS["brats128"]
    B = 4
    torch.manual_seed(12345)
    model = VeloxSeg(**cfg).cuda()
    crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=len(cfg["in_ch"]))
    x, lab = synth(cfg, B, "cuda", 12345)
    eng = TrainEngine(model, crit, (B, sum(cfg["in_ch"]), *cfg["input_size"]), use_graph=True, overlap=False)
    eng.step(x, lab)
    torch.cuda.synchronize()
    assert eng.use_graph and eng.graphs is not None, "the capture's self-check (replay == eager pass) failed"
    rng = VF.rng_state(eng.dev)
    rng0 = rng.clone()
    ref = None
    for i in range(6):                       # on the default stream, as a training loop would
        rng.copy_(rng0)
        torch.cuda.synchronize()
        with eng._settings(capture=True):    # (the engine's switches -- in-place RNG step, per-modality forks -- are scoped to its own passes since round 3)
            eng._eager_pass()
        torch.cuda.synchronize()
        g = eng.flat.grad.clone()
        ref = g if ref is None else ref
        assert float((g - ref).abs().max()) < 1e-5, (i, float((g - ref).abs().max()))
    rng.copy_(rng0)
    torch.cuda.synchronize()
    eng._replay(comm=False)
    torch.cuda.synchronize()
    assert float((eng.flat.grad - ref).abs().max()) < 1e-5


def test_taped_engine_on_96_cube_patches_takes_the_fused_loss_and_tracks_eager():
    """96^3 patches (the reference's SHIPPED configurations: 3^3 / 6^3 windows, 24-wide coarse rows): since round 3 the fused deep-supervision loss, the
    patch-expand MFMA kernels and the stem weight-gradient MFMA kernel accept these rows (a partly idle last tile), and the 27- / 216-token windows take the
    one-pass MFMA attention backward.  The capture must succeed (no silent fall-back to eager launches) and track the eager engine."""
    import types
    from bench import LOSS_CFG, WORKLOADS, synth
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    cfg, _ = WORKLOADS["autopet96"]
    B = 1
    losses = {}
    import veloxseg_amd.functional as VF
    for mode in ("eager", "tape"):
        VF.reset_dropout_sites()
        torch.manual_seed(7)
        model = VeloxSeg(**cfg).cuda()
        VF.manual_seed(77, "cuda")
        crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=len(cfg["in_ch"]))
        x, lab = synth(cfg, B, "cuda", 7)
        eng = TrainEngine(model, crit, (B, sum(cfg["in_ch"]), *cfg["input_size"]), use_graph=(mode == "tape"), overlap=False)
        assert eng._ds_fused is True and model.ds_fused is False     # the library's own Loss + a width the loss kernels tile (W % 4 == 0, W <= 256); the
        # engine applies its choice inside its own passes only (TrainEngine._settings) and leaves the model's attribute as it found it
        losses[mode] = [float(eng.step(x, lab)) for _ in range(3)]
        if mode == "tape":
            assert eng.use_graph and eng.graphs is not None
    for a, b in zip(losses["eager"], losses["tape"]):
        assert abs(a - b) <= 2e-3 * abs(a), losses


def test_tape_cross_lane_dependencies_through_flag_kernels_and_through_events_agree():
    """The lanes of a tape are ordered by flag kernels (a store on the producing lane, a poll on the waiting lane: csrc/tape.hip) or -- vx_tape_set_flags(0)
    -- by events.  A diamond of forked branches whose kernels are long enough to expose a missing dependency must give the eager result in both modes,
    also when the host replays many times without synchronising in between (sequence numbers instead of resets)."""
    from veloxseg_amd import _hip as H
    dev = torch.device("cuda:0")
    torch.manual_seed(1)
    a = torch.randn(1024, 1024, device=dev)
    x0 = torch.randn(1024, 1024, device=dev)
    x = x0.clone()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def fn():
        cur = torch.cuda.current_stream()
        y = x @ a                                   # producer
        s1.wait_stream(cur); s2.wait_stream(cur)
        with torch.cuda.stream(s1):
            p = (y @ a) * 0.01                      # branch 1
            p.record_stream(cur)
        with torch.cuda.stream(s2):
            q = torch.tanh(y) @ a                   # branch 2
            q.record_stream(cur)
        cur.wait_stream(s1); cur.wait_stream(s2)
        r = p + q                                   # join
        x.copy_(torch.tanh(r * 0.01))               # the next replay reads what this one wrote
        return r

    tape, r = _capture(fn)
    assert tape.n_lanes >= 2
    def eager(n):
        xe = x0.clone()
        for _ in range(n):
            y = xe @ a
            re = (y @ a) * 0.01 + torch.tanh(y) @ a
            xe = torch.tanh(re * 0.01)
        return re
    try:
        for flags in (1, 0):
            H.call("vx_tape_set_flags", flags)
            for n in (1, 25):
                x.copy_(x0)
                torch.cuda.synchronize()
                for _ in range(n):
                    tape.replay()                   # no synchronisation between replays
                torch.cuda.synchronize()
                ref = eager(n)
                assert torch.allclose(r, ref, rtol=2e-3, atol=2e-2 * float(ref.abs().max())), (flags, n, float((r - ref).abs().max()), float(ref.abs().max()))
    finally:
        H.call("vx_tape_set_flags", 1)


def test_taped_step_soak_full_size():
    """60 replays of the full-size taped step from the same weights and dropout streams, the host running ahead of the GPU (a synchronisation every 15
    replays): every checked replay reproduces loss and gradient of the first (float-atomic noise only).  A cross-lane dependency missed once would be an
    outlier (tools/tape_soak.py is the long form)."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "tape_soak.py"), "autopet128", "2", "60"], env=dict(os.environ, VX_SYNC_EVERY="15"),
                       cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "0 outliers" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_a_poll_that_gives_up_is_reported_not_trapped():
    """a cross-lane poll whose flag never arrives (a lost dependency) gives up after the timeout: it does NOT trap the queue -- its successors run, the
    give-up is counted in a pinned host word, and the next hop / replay of the process reports it (csrc/tape.hip vx_flag_wait_k, vx_tape_flag_timeouts)"""
    from veloxseg_amd import _hip as H
    flag = torch.zeros(4, dtype=torch.int32, device="cuda")
    marker = torch.zeros(1, device="cuda")
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    H.query("vx_tape_flag_timeouts")                       # clear
    H.call("vx_tape_set_flag_timeout_ms", 20)
    try:
        H.call("vx_tape_flag_wait", flag.data_ptr(), 7, s.cuda_stream)          # nobody sets the flag to 7
        with torch.cuda.stream(s):
            marker.add_(1.0)                               # the successor of the poll
        s.synchronize()
        assert float(marker) == 1.0
        assert H.query("vx_tape_flag_timeouts") == 1
        assert H.query("vx_tape_flag_timeouts") == 0       # reading clears the count
        H.call("vx_tape_flag_wait", flag.data_ptr(), 7, s.cuda_stream)
        s.synchronize()
        with pytest.raises(RuntimeError, match="gave up"):
            H.call("vx_tape_hop", 250, s.cuda_stream, s2.cuda_stream)
        # a flag that does arrive is not a timeout
        H.call("vx_tape_flag_set", flag.data_ptr(), 9, s2.cuda_stream)
        H.call("vx_tape_flag_wait", flag.data_ptr(), 9, s.cuda_stream)
        torch.cuda.synchronize()
        assert H.query("vx_tape_flag_timeouts") == 0
        H.call("vx_tape_hop", 250, s.cuda_stream, s2.cuda_stream)
        torch.cuda.synchronize()
    finally:
        H.call("vx_tape_set_flag_timeout_ms", 5000)
        H.query("vx_tape_flag_timeouts")


def test_pipelined_decoder_tail_trains_like_the_joined_step():
    """TrainEngine(pipeline_tail=True): the decoders' weight gradients and the decoder half of AdamW of step N run beside the encoder forward of step N + 1 (joined before
    the next decoder forward; the branches work on private copies of the boundary tensors).  Same arithmetic as the joined step: losses of 5 consecutive steps and the
    parameters after them agree to float-atomics noise; flush() orders the caller's stream behind the tail."""
    import types
    from bench import LOSS_CFG, WORKLOADS, synth
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    import veloxseg_amd.functional as VF
    cfg, _ = WORKLOADS["autopet96"]
    cfg = dict(cfg, proj_drop=0.0, conv_drop=0.0, attn_drop=0.0)
    B = 2
    res = {}
    for pipe in (False, True):
        VF.reset_dropout_sites()
        torch.manual_seed(3)
        model = VeloxSeg(**cfg).cuda()
        crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=len(cfg["in_ch"]))
        eng = TrainEngine(model, crit, (B, sum(cfg["in_ch"]), *cfg["input_size"]), lr=1e-3, use_graph=True, overlap=False, pipeline_tail=pipe)
        losses = []
        for i in range(5):
            x, lab = synth(cfg, B, "cuda", 100 + i)
            losses.append(eng.step(x, lab).clone())
        assert eng.use_graph and eng.graphs is not None
        assert eng._tail_pending == pipe
        eng.flush()
        p_now = eng.flat.param.clone()             # on the caller's stream, behind flush(): the decoder half is up to date
        torch.cuda.synchronize()
        assert torch.equal(p_now, eng.flat.param)
        res[pipe] = ([float(l) for l in losses], p_now.cpu())
    for a, b in zip(res[False][0], res[True][0]):
        assert abs(a - b) <= 2e-4 * abs(a), res
    # (element-wise equality is not the bar: Adam's first steps are sign-like, so parameters whose gradient is round-off noise -- biases in front of an InstanceNorm --
    # walk by +-lr per step in either run; the two runs must agree in norm)
    rel = float((res[False][1] - res[True][1]).norm() / res[False][1].norm())
    assert rel < 2e-3, rel


def test_pipelined_decoder_tail_with_dropout_tracks_the_joined_step():
    """The same A/B as test_pipelined_decoder_tail_trains_like_the_joined_step at the configured dropout rates (0.1 at every site): the pipelined tail
    bumps the {seed, step} word in place at the head of step N + 1 while the decoder tail of step N may still run, so a tail that re-reads the step
    word would draw the next step's masks.  Losses of 5 consecutive steps and the parameters after them agree with the joined step at the same bars,
    and both runs leave the step word at start + 5."""
    import types
    from bench import LOSS_CFG, WORKLOADS, synth
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils.loss import Loss
    import veloxseg_amd.functional as VF
    cfg, _ = WORKLOADS["autopet96"]
    cfg = dict(cfg, proj_drop=0.1, conv_drop=0.1, attn_drop=0.1)
    B = 2
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {}
    for pipe in (False, True):
        VF.reset_dropout_sites()
        torch.manual_seed(3)
        model = VeloxSeg(**cfg).cuda()
        crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, None, num_modal=len(cfg["in_ch"]))
        eng = TrainEngine(model, crit, (B, sum(cfg["in_ch"]), *cfg["input_size"]), lr=1e-3, use_graph=True, overlap=False, pipeline_tail=pipe)
        VF.rng_state(dev).copy_(torch.tensor([0x3_0000_0005, 10], dtype=torch.int64))
        losses = []
        for i in range(5):
            x, lab = synth(cfg, B, "cuda", 100 + i)
            losses.append(eng.step(x, lab).clone())
        assert eng.use_graph and eng.graphs is not None
        assert eng._tail_pending == pipe
        eng.flush()
        p_now = eng.flat.param.clone()
        torch.cuda.synchronize()
        assert [int(v) for v in VF.rng_state(dev).cpu()] == [0x3_0000_0005, 15]
        res[pipe] = ([float(l) for l in losses], p_now.cpu())
    for a, b in zip(res[False][0], res[True][0]):
        assert abs(a - b) <= 2e-4 * abs(a), res
    rel = float((res[False][1] - res[True][1]).norm() / res[False][1].norm())
    assert rel < 2e-3, rel
