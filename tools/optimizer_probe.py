#!/usr/bin/env python3
"""What gradient clipping, EMA weights and param groups cost the taped training step: one process, autopet128, B = 4, fp32.

1. Median step time over REPLAYS replays of the taped step for {off, clip, ema, groups, all} x pipeline_tail {off, on}.  One engine per configuration (its own model,
   seeded alike), all built and warmed up first; then the configurations are timed alternately, ROUNDS times, REPLAYS / ROUNDS steps per window, every window between
   device synchronises (steps are enqueued back to back, as the step loop does); all window means are printed, the table uses their median.
2. The two kernels alone on flat buffers of the model's size, REPS back-to-back launches between HIP events: vx_grad_sqnorm_partials, vx_adamw_step (the default
   update) and vx_adamw_step_ex with clip / EMA / groups / all, beside a device-to-device copy_ of 9 MB.
Prints one JSON object; `--json FILE` also writes it.  Needs the GPU: there is nothing to time without one."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import torch

from bench import LOSS_CFG, WORKLOADS, synth
from veloxseg_amd import _hip as H
from veloxseg_amd.engine import TrainEngine
from veloxseg_amd.model.VeloxSeg import VeloxSeg
from veloxseg_amd.utils.loss import Loss
from veloxseg_amd.utils.optimizers.optimizers import build_optimizer

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--workload", default="autopet128")
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--replays", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--only-kernels", action="store_true")
args = ap.parse_args()
if not torch.cuda.is_available():
    raise SystemExit("optimizer_probe: no GPU -- nothing is timed on the host")
dev = torch.device("cuda")
REPS = 50
MODES = {"off": {}, "clip": {"clip": True}, "ema": {"ema": True}, "groups": {"groups": True}, "all": {"clip": True, "ema": True, "groups": True}}


def steps():
    cfg, _ = WORKLOADS[args.workload]
    B = args.batch
    x, lab = synth(cfg, B, dev, 12345)
    engines = {}
    for pipe in (False, True):
        for name, m in MODES.items():
            torch.manual_seed(12345)
            model = VeloxSeg(**cfg).to(dev)
            crit = Loss(types.SimpleNamespace(model_name="VeloxSeg"), LOSS_CFG, dev, num_modal=len(cfg["in_ch"]))
            oargs = {"lr": 2.5e-4, "weight_decay": 0.01}
            if m.get("groups"):
                oargs["no_weight_decay"] = "1d"
            eng = TrainEngine(model, crit, (B, sum(cfg["in_ch"]), *cfg["input_size"]), use_graph=True, pipeline_tail=pipe, optimizer=build_optimizer(model, "adamw", oargs),
                              max_grad_norm=1.0 if m.get("clip") else None, ema_decay=0.999 if m.get("ema") else None)
            for _ in range(4):                                   # capture + warm-up
                eng.step(x, lab)
            eng.flush()
            torch.cuda.synchronize()
            if not eng.use_graph:
                raise SystemExit(f"optimizer_probe: the capture of {name} fell back to eager launches")
            engines[(name, pipe)] = eng
    per = max(1, args.replays // args.rounds)
    ms = {k: [] for k in engines}
    for _ in range(args.rounds):
        for k, eng in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                eng.step()
            eng.flush()
            torch.cuda.synchronize()
            ms[k].append(round((time.perf_counter() - t0) * 1e3 / per, 4))
    out = {}
    for (name, pipe), v in ms.items():
        base = statistics.median(ms[("off", pipe)])
        med = statistics.median(v)
        eng = engines[(name, pipe)]
        out[f"{name}, pipeline_tail={'on' if pipe else 'off'}"] = {"ms_per_step_windows": v, "ms_per_step_median": round(med, 4), "delta_us_to_off": round((med - base) * 1e3, 1),
                                                                  "pipelined": bool(eng._pipe_active()), "replays": per * args.rounds}
    out["_note"] = {"flat_elements": int(eng.flat.numel), "param_groups_with_groups_on": 2, "steps_per_window": per, "windows": args.rounds}
    return out


def timed(fn):
    for _ in range(5):
        fn()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        runs.append(round(e0.elapsed_time(e1) * 1000 / REPS, 2))
    return runs


def kernels():
    cfg, _ = WORKLOADS[args.workload]
    from veloxseg_amd.engine import FlatParams
    n = FlatParams(VeloxSeg(**cfg)).numel
    p, g, m, v, e = (torch.randn(n, device=dev) * s for s in (1.0, 1e-3, 1e-3, 0.0, 1.0))
    v = v.abs() + 1e-6
    nb = H.query("vx_grad_sqnorm_blocks")
    ws, stats = torch.zeros(nb, device=dev, dtype=torch.float64), torch.zeros(4, device=dev)
    table = (torch.arange(n // 64, device=dev) % 2).to(torch.uint8)
    glr, gwd = (ctypes.c_float * 8)(2.5e-4, 2.5e-4), (ctypes.c_float * 8)(0.01, 0.0)
    st = H.stream_ptr()
    common = (H.P(p), H.P(g), H.P(m), H.P(v), n, 0.0, 0.9, 0.999, 1e-8, 0.0, 10, 1.0)          # lr = 0: the buffers keep their values

    def ex(clip, ema, groups):
        H.call("vx_adamw_step_ex", *common, H.P(ws, torch.float64) if clip else None, nb if clip else 0, 1.0, H.P(stats) if clip else None, 1, H.P(e) if ema else None, 0.001,
               H.P(table, torch.uint8) if groups else None, ctypes.addressof(glr) if groups else None, ctypes.addressof(gwd) if groups else None, 2 if groups else 0, st)
    a, b = torch.randn(n, device=dev), torch.empty(n, device=dev)
    calls = {"vx_grad_sqnorm_partials": (lambda: H.call("vx_grad_sqnorm_partials", H.P(g), n, H.P(ws, torch.float64), st), 4 * n),
             "vx_adamw_step": (lambda: H.call("vx_adamw_step", *common, st), 28 * n),
             "vx_adamw_step_ex off": (lambda: ex(False, False, False), 28 * n),
             "vx_adamw_step_ex clip": (lambda: ex(True, False, False), 28 * n),
             "vx_adamw_step_ex ema": (lambda: ex(False, True, False), 36 * n),
             "vx_adamw_step_ex groups": (lambda: ex(False, False, True), 28 * n),
             "vx_adamw_step_ex all": (lambda: ex(True, True, True), 36 * n),
             "copy_ of the flat buffer": (lambda: b.copy_(a), 8 * n)}
    out = {"flat_elements": int(n), "partials_per_call": int(nb)}
    for name, (fn, nbytes) in calls.items():
        us = timed(fn)
        out[name] = {"us_per_call": us, "us_median": statistics.median(us), "bytes_read_and_written": nbytes}
    return out


res = {"workload": f"{args.workload}, B = {args.batch}, fp32, taped step (TrainEngine(use_graph=True)), one process"}
if not args.only_kernels:
    res["step"] = steps()
res["kernels"] = kernels()
print(json.dumps(res, indent=1))
if args.json:
    os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
    json.dump(res, open(args.json, "w"), indent=1)
