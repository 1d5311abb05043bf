#!/usr/bin/env python3
"""Ensemble inference entrypoint: run_test.py's command line with SEVERAL models -- sliding-window segmentation by the weighted mean of the models' soft-max
probabilities (veloxseg_amd.utils.ensemble.infer_ensemble) + Dice.  run_test.py itself is unchanged and stays the one-model entrypoint.

--checkpoint_index a,b,c names one model each: <checkpoint_dir>/<name>.pth, or, without --checkpoint_dir, seeded random weights, model i from seed 12345 + i (so the
synthetic path works; model 0 is run_test.py's model).  test_config["ensemble"]["weights"] (optional): one finite positive number per model, normalised on the host;
mirror_axes, blend and sigma_scale are read from test_config["sliding_window"] as run_test.py's driver reads them.  Volumes as in run_test.py: synthetic, or
--data_module.  Metrics are computed on the ensemble's labels; the CSV has run_test.py's columns.
"""
import argparse
import csv
import importlib
import json
import os
import time

SUPPORTED_DATASETS = ("AutoPETII", "Hecktor2022", "BraTS2021")

if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--dataset_name", type=str, required=True, choices=SUPPORTED_DATASETS)
    parser.add_argument("--model_name", type=str, required=True)
    parser.add_argument("--train_date", type=str, default=None)
    parser.add_argument("--model_index", type=str, default=None)
    parser.add_argument("--checkpoint_dir", type=str, default=None, help="directory holding <name>.pth for every name of --checkpoint_index")
    parser.add_argument("--checkpoint_index", type=str, required=True, help="comma-separated names, one model each")
    parser.add_argument("--model_config", type=str, required=True)
    parser.add_argument("--train_config", type=str, required=True)
    parser.add_argument("--test_config", type=str, required=True)
    parser.add_argument("--gpu_id", type=str, default="0")
    parser.add_argument("--num_workers", type=int, default=8)
    parser.add_argument("--specific_sample", type=int, default=None)
    parser.add_argument("--select_modal", type=int, default=None)
    parser.add_argument("--use_hd95", type=int, default=None, help="HD95 needs medpy (not available): must stay 0 / unset")
    parser.add_argument("--synthetic", type=int, default=2, help="number of synthetic volumes")
    parser.add_argument("--volume_shape", type=int, nargs=3, default=[240, 240, 155])
    parser.add_argument("--data_module", type=str, default=None)
    parser.add_argument("--out_csv", type=str, default=None)
    args = parser.parse_args()
    if args.use_hd95:
        raise SystemExit("HD95 (medpy) is out of scope of veloxseg_amd")
    names = [n for n in args.checkpoint_index.split(",") if n]
    if not names:
        raise SystemExit("--checkpoint_index needs at least one name")
    cfgs = {}
    for k in ("model_config", "train_config", "test_config"):
        with open(getattr(args, k), "r", encoding="utf-8") as f:
            cfgs[k] = json.load(f)
    import veloxseg_amd  # noqa: F401
    import torch
    from veloxseg_amd.utils.ensemble import infer_ensemble
    from veloxseg_amd.utils.load_model import load_checkpoint, load_model
    torch.cuda.set_device(int(args.gpu_id.split(",")[0]))
    models = []
    for i, n in enumerate(names):
        torch.manual_seed(12345 + i)
        m = load_model(args.model_name, cfgs["model_config"])
        if args.checkpoint_dir:
            m = load_checkpoint(m, os.path.join(args.checkpoint_dir, n + ".pth"))
        models.append(m.cuda().eval())
    sw = cfgs["test_config"]["sliding_window"]
    kw = {k: (tuple(sw[k]) if k == "mirror_axes" else sw[k]) for k in ("mirror_axes", "blend", "sigma_scale") if sw.get(k) is not None}
    kw["weights"] = (cfgs["test_config"].get("ensemble") or {}).get("weights")
    mcfg = cfgs["model_config"][args.model_name]
    brats = args.dataset_name == "BraTS2021"
    if brats:
        from veloxseg_amd.utils.metric.metrics_brats import cal_dice
    else:
        from veloxseg_amd.utils.metric.metrics import metrics_tensor
    if args.data_module:
        volumes = importlib.import_module(args.data_module).iter_volumes(args, cfgs["train_config"], cfgs["test_config"])
    else:
        def volumes():
            g = torch.Generator().manual_seed(12345)
            for i in range(args.synthetic):
                x = torch.randn((1, sum(mcfg["in_ch"]), *args.volume_shape), generator=g)
                y = torch.randint(0, mcfg["n_classes"], (1, 1, *args.volume_shape), generator=g)
                yield f"synthetic_{i}", x, y
        volumes = volumes()
    patch = cfgs["train_config"]["patch_size"][args.dataset_name] if isinstance(cfgs["train_config"].get("patch_size"), dict) else mcfg["input_size"]
    rows = []
    with torch.inference_mode():
        for name, x, y in volumes:
            t0 = time.perf_counter()
            out = infer_ensemble(models, x.cuda().float(), patch, cfgs["train_config"]["batch_size"], sw["overlap"], **kw)[1].long()
            if brats:
                avg, et, tc, wt = cal_dice(out, y.cuda())
                rows.append([name, avg, et, tc, wt, float((out > 0).sum()), float((y > 0).sum())])
            else:
                fp, fn, _, _, _, iou, dice = metrics_tensor(y.cuda(), out)
                rows.append([name, dice, iou, fp, fn, float((out > 0).sum()), float((y > 0).sum())])
            torch.cuda.synchronize()
            print(name, [round(v, 4) if isinstance(v, float) else v for v in rows[-1][1:]], f"{(time.perf_counter() - t0) * 1e3:.1f} ms")
    if args.out_csv:
        with open(args.out_csv, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["name", "Avg_Dice", "ET_Dice", "TC_Dice", "WT_Dice", "Prediction", "Label"] if brats else ["name", "Dice", "IoU", "FP", "FN", "Prediction", "Label"])
            w.writerows(rows)
