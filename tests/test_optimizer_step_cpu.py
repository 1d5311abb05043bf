"""CPU: host side of the fused optimizer step with gradient clipping, EMA weights and param groups: the C ABI refuses bad arguments before any
launch, the optimizer registry builds the no-weight-decay group, TrainEngine maps param groups to 64-element chunks, checkpoints carry the EMA.  No kernels are launched."""
import ctypes
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
from recipe import CASES  # noqa: E402

OPT_ARGS = {"lr": 2.5e-4, "weight_decay": 0.01}
TRAIN_CFG = {"warmup_scheduler": {"enabled": True, "warmup_epochs": 3}, "train_scheduler": {"scheduler_type": "cosine_annealing", "scheduler_args": {"epochs": 5, "min_lr": 1e-6}}}


def _model(seed=0):
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    cfg, _ = CASES["g2_32_m2"]
    torch.manual_seed(seed)
    return VeloxSeg(**cfg)


def test_new_entries_are_exported():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    protos = _hip.parse_header()
    dll = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("vx_grad_sqnorm_blocks", "vx_grad_sqnorm_partials", "vx_adamw_step_ex"):
        assert name in protos and hasattr(dll, name), name
    assert [t for t, _ in protos["vx_grad_sqnorm_partials"][1]] == ["const float*", "long", "double*", "void*"]
    assert len(protos["vx_adamw_step_ex"][1]) == 24
    nb = _hip.query("vx_grad_sqnorm_blocks")
    assert 64 <= nb <= 1024                      # "a few hundred doubles": every workgroup of the update adds them all
    assert [t for t, _ in protos["vx_adamw_step"][1]] == ["float*", "const float*", "float*", "float*", "long", "float", "float", "float", "float", "float", "long", "float", "void*"]


def test_bad_arguments_return_error_codes_without_gpu():
    from veloxseg_amd import _hip
    lr8, wd8 = (ctypes.c_float * 8)(), (ctypes.c_float * 8)()
    hl, hw = ctypes.addressof(lr8), ctypes.addressof(wd8)

    def ex(p=1, g=1, m=1, v=1, n=64, step=1, ws=None, nws=0, stats=None, write_stats=0, ema=None, table=None, glr=None, gwd=None, ngroups=0):
        _hip.call("vx_adamw_step_ex", p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 0.01, step, 1.0, ws, nws, 1.0, stats, write_stats, ema, 0.01, table, glr, gwd, ngroups, None)

    with pytest.raises(RuntimeError, match="bad args"):
        _hip.call("vx_grad_sqnorm_partials", 1, 0, 1, None)                  # n <= 0
    with pytest.raises(RuntimeError, match="bad args"):
        _hip.call("vx_grad_sqnorm_partials", None, 8, 1, None)               # null gradient
    with pytest.raises(RuntimeError, match="bad args"):
        _hip.call("vx_grad_sqnorm_partials", 1, 8, None, None)               # null workspace
    with pytest.raises(RuntimeError, match="bad args"):
        ex(n=0)
    with pytest.raises(RuntimeError, match="bad args"):
        ex(p=None)
    with pytest.raises(RuntimeError, match="bad args"):
        ex(v=None)
    with pytest.raises(RuntimeError, match="bad args"):
        ex(step=0)
    with pytest.raises(RuntimeError, match="nws"):
        ex(ws=1, nws=0)
    with pytest.raises(RuntimeError, match="nws"):
        ex(ws=1, nws=-3)
    with pytest.raises(RuntimeError, match="stats"):
        ex(ws=1, nws=4, stats=None, write_stats=1)
    with pytest.raises(RuntimeError, match="at most 8"):
        ex(table=1, glr=hl, gwd=hw, ngroups=9)
    with pytest.raises(RuntimeError, match="chunk table"):
        ex(table=1, glr=None, gwd=hw, ngroups=2)
    with pytest.raises(RuntimeError, match="chunk table"):
        ex(table=1, glr=hl, gwd=hw, ngroups=0)


def test_no_weight_decay_builds_a_second_group():
    from veloxseg_amd.utils.optimizers.optimizers import build_optimizer
    model = _model()
    params = list(model.parameters())
    opt = build_optimizer(model, "adamw", dict(OPT_ARGS, no_weight_decay="1d"))
    assert isinstance(opt, torch.optim.AdamW) and len(opt.param_groups) == 2
    decay, no_decay = opt.param_groups
    assert decay["weight_decay"] == 0.01 and no_decay["weight_decay"] == 0.0 and decay["lr"] == no_decay["lr"] == 2.5e-4
    assert {id(p) for p in no_decay["params"]} == {id(p) for p in params if p.ndim <= 1}
    assert all(p.ndim > 1 for p in decay["params"])
    assert sorted(id(p) for g in opt.param_groups for p in g["params"]) == sorted(id(p) for p in params)          # a partition of model.parameters()
    # name substrings
    opt = build_optimizer(model, "adamw", dict(OPT_ARGS, no_weight_decay=["bias"]))
    names = {id(p): n for n, p in model.named_parameters()}
    assert len(opt.param_groups) == 2 and all("bias" in names[id(p)] for p in opt.param_groups[1]["params"])
    assert not any("bias" in names[id(p)] for p in opt.param_groups[0]["params"])
    with pytest.raises(ValueError):
        build_optimizer(model, "adamw", dict(OPT_ARGS, no_weight_decay="2d"))
    # without the key: exactly the object of before -- one group over model.parameters()
    opt = build_optimizer(model, "adamw", OPT_ARGS)
    assert len(opt.param_groups) == 1 and [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in params]


def test_engine_maps_param_groups_to_chunks():
    from veloxseg_amd.engine import TrainEngine
    from veloxseg_amd.utils.optimizers.optimizers import build_optimizer
    model = _model()
    opt = build_optimizer(model, "adamw", dict(OPT_ARGS, no_weight_decay="1d"))
    eng = TrainEngine(model, None, (1, 2, 32, 32, 32), optimizer=opt)
    table = eng._chunk_group
    assert table.dtype == torch.uint8 and table.numel() == eng.flat.numel // 64
    gid = {id(p): gi for gi, g in enumerate(opt.param_groups) for p in g["params"]}
    seen = torch.zeros(table.numel(), dtype=torch.bool)
    for n, p in zip(eng.flat.names, eng.flat.params):
        o, k = eng.flat.slices[n]
        assert o % 64 == 0
        chunks = table[o // 64:(o + k + 63) // 64]
        assert bool((chunks == gid[id(p)]).all()), n
        assert not bool(seen[o // 64:(o + k + 63) // 64].any()), n          # a chunk never holds two parameters
        seen[o // 64:(o + k + 63) // 64] = True
    assert bool(seen.all())
    # lr / weight_decay are read per group at every step: what a scheduler wrote is what the launch gets
    opt.param_groups[0]["lr"], opt.param_groups[1]["lr"] = 1e-3, 5e-4
    eng._adamw_begin()
    assert list(eng._group_lr)[:2] == [ctypes.c_float(1e-3).value, ctypes.c_float(5e-4).value] and list(eng._group_wd)[:2] == [ctypes.c_float(0.01).value, 0.0]
    # the state still aliases the flat moments, per parameter
    for n, p in zip(eng.flat.names, eng.flat.params):
        o, k = eng.flat.slices[n]
        assert opt.state[p]["exp_avg"].data_ptr() == eng.m.data_ptr() + 4 * o
    # a one-group engine keeps no table; nothing is allocated for clipping / EMA by default
    eng1 = TrainEngine(_model(), None, (1, 2, 32, 32, 32), optimizer=None)
    assert eng1._chunk_group is None and eng1.ema is None and eng1._norm_ws is None and eng1._stats is None and eng1.grad_norm is None


def test_engine_refuses_groups_it_cannot_fuse():
    from veloxseg_amd.engine import TrainEngine
    model = _model()
    params = list(model.parameters())
    a, b = [p for p in params if p.ndim > 1], [p for p in params if p.ndim <= 1]
    mk = lambda **kw: torch.optim.AdamW([{"params": a}, dict({"params": b}, **kw)], lr=1e-3, weight_decay=0.01)
    with pytest.raises(NotImplementedError, match="betas"):
        TrainEngine(model, None, (1, 2, 32, 32, 32), optimizer=mk(betas=(0.8, 0.999)))
    with pytest.raises(NotImplementedError, match="betas and eps"):
        TrainEngine(model, None, (1, 2, 32, 32, 32), optimizer=mk(eps=1e-6))
    with pytest.raises(NotImplementedError, match="amsgrad"):
        TrainEngine(model, None, (1, 2, 32, 32, 32), optimizer=mk(amsgrad=True))
    with pytest.raises(ValueError, match="at most 8"):
        TrainEngine(model, None, (1, 2, 32, 32, 32), optimizer=torch.optim.AdamW([{"params": [p]} for p in params[:8]] + [{"params": params[8:]}], lr=1e-3))
    with pytest.raises(ValueError, match="partition"):
        TrainEngine(model, None, (1, 2, 32, 32, 32), optimizer=torch.optim.AdamW([{"params": a}], lr=1e-3))


def test_checkpoint_carries_the_ema_only_when_given(tmp_path):
    from veloxseg_amd.utils.load_model import ema_checkpoint, load_checkpoint, load_ema, save_checkpoint
    from veloxseg_amd.utils.optimizers.optimizers import build_optimizer
    from veloxseg_amd.utils.optimizers.schedulers import build_scheduler
    model = _model()
    opt = build_optimizer(model, "adamw", OPT_ARGS)
    warm, train = build_scheduler(opt, "warmup_scheduler", TRAIN_CFG), build_scheduler(opt, "training_scheduler", TRAIN_CFG)
    base = {"model", "optimizer", "warmup_scheduler", "training_scheduler", "epoch", "best_train_dice", "best_val_dice"}
    f0, f1 = str(tmp_path / "plain.pth"), str(tmp_path / "ema.pth")
    save_checkpoint(model, opt, warm, train, 4, 0.5, 0.25, f0)
    assert set(torch.load(f0)) == base and load_ema(f0) is None
    ema = {k: v.clone() + 1.0 if v.is_floating_point() else v.clone() for k, v in model.state_dict().items()}
    save_checkpoint(model, opt, warm, train, 4, 0.5, 0.25, f1, ema=ema)
    assert set(torch.load(f1)) == base | {"ema"}
    got = load_ema(f1, torch.device("cpu"))
    assert list(got) == list(ema) and all(torch.equal(got[k], ema[k]) for k in ema)
    model2 = _model(1)
    opt2 = build_optimizer(model2, "adamw", OPT_ARGS)
    out = load_checkpoint(model2, f1, opt2, build_scheduler(opt2, "warmup_scheduler", TRAIN_CFG), build_scheduler(opt2, "training_scheduler", TRAIN_CFG))
    assert len(out) == 7 and out[4:] == (5, 0.5, 0.25)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), model2.state_dict().values()))          # the "model" entry, not the EMA
    # the EMA as the "model" entry of a copy: what run_test.py --checkpoint_index (unchanged) and the reference's own readers load
    f2 = ema_checkpoint(f1, str(tmp_path / "ema_as_model.pth"))
    ck2 = torch.load(f2)
    assert set(ck2) == base and all(torch.equal(ck2["model"][k], ema[k]) for k in ema)
    model3 = load_checkpoint(_model(2), f2)
    assert all(torch.equal(v, ema[k]) for k, v in model3.state_dict().items())
    with pytest.raises(KeyError, match="no \"ema\" entry"):
        ema_checkpoint(f0, str(tmp_path / "x.pth"))
    # load_checkpoint(..., weights="ema"): the EMA into the model, a clear error without one; `extras` hands the EMA over from the same read
    model4 = load_checkpoint(_model(3), f1, weights="ema")
    assert all(torch.equal(v, ema[k]) for k, v in model4.state_dict().items())
    with pytest.raises(KeyError, match="no \"ema\" entry"):
        load_checkpoint(_model(3), f0, weights="ema")
    with pytest.raises(ValueError):
        load_checkpoint(_model(3), f1, weights="best")
    ex1, ex0 = {}, {}
    load_checkpoint(_model(3), f1, extras=ex1)
    load_checkpoint(_model(3), f0, extras=ex0)
    assert ex0 == {"ema": None} and list(ex1["ema"]) == list(ema) and all(torch.equal(ex1["ema"][k], ema[k]) for k in ema)
