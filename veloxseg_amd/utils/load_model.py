"""Model registry / checkpoint helpers (reference: utils/load_model.py:83-148), VeloxSeg entry only."""
from collections import OrderedDict

import torch


def load_model(model_name, config):
    if model_name != "VeloxSeg":
        raise ValueError("Invalid model name, now {} (veloxseg_amd provides VeloxSeg only)".format(model_name))
    from ..model.VeloxSeg import VeloxSeg
    return VeloxSeg(**config[model_name])


def checkpoint_DDP_to_SingleGPU(checkpoint):
    out = OrderedDict()
    for k, v in checkpoint.items():
        out[k[len("module."):] if k.startswith("module.") else k] = v
    return out


def save_checkpoint(model, optimizer, warmup_scheduler, training_scheduler, epoch, best_train_dice, best_val_dice, filename="checkpoint.pth", ema=None):
    """the reference's checkpoint; `ema` (TrainEngine.ema_state_dict()) adds an "ema" entry -- without it the key set is the reference's"""
    ckpt = {"model": model.state_dict(), "optimizer": optimizer.state_dict(), "warmup_scheduler": warmup_scheduler.state_dict(),
            "training_scheduler": training_scheduler.state_dict(), "epoch": epoch + 1, "best_train_dice": best_train_dice,
            "best_val_dice": best_val_dice}
    if ema is not None:
        ckpt["ema"] = ema
    torch.save(ckpt, filename)


def load_ema(filename, device=torch.device("cpu")):
    """the "ema" state dict of a checkpoint written with save_checkpoint(..., ema=...), or None when it has none"""
    ema = torch.load(filename, map_location=device).get("ema")
    return None if ema is None else checkpoint_DDP_to_SingleGPU(ema)


def ema_checkpoint(filename, out):
    """write a copy of checkpoint `filename` whose "model" entry is its EMA (the "ema" entry is dropped), for readers that know the reference's checkpoint format
    only: run_test.py --checkpoint_index and the reference's own scripts then predict with the EMA weights (a reader in this package passes
    load_checkpoint(..., weights="ema") instead).  Raises when the checkpoint has no EMA"""
    ckpt = torch.load(filename, map_location="cpu")
    if ckpt.get("ema") is None:
        raise KeyError(f'{filename} holds no "ema" entry (train with train_config["ema"] = {{"decay": ...}})')
    ckpt["model"] = ckpt.pop("ema")
    torch.save(ckpt, out)
    return out


def load_checkpoint(model, filename, optimizer=None, warmup_scheduler=None, training_scheduler=None, device=torch.device("cpu"), weights="model", extras=None):
    """the reference's reader.  Beyond it: weights="ema" loads the checkpoint's "ema" entry into the model instead of "model" (KeyError with a clear message when the
    checkpoint has none); `extras`, a dict, receives the entries beyond the reference's key set (extras["ema"] = the EMA state dict or None) from the same read"""
    if weights not in ("model", "ema"):
        raise ValueError('weights must be "model" or "ema"')
    ckpt = torch.load(filename, map_location=device)
    if weights == "ema" and ckpt.get("ema") is None:
        raise KeyError(f'{filename} holds no "ema" entry (train with train_config["ema"] = {{"decay": ...}})')
    model.load_state_dict(checkpoint_DDP_to_SingleGPU(ckpt[weights]))
    if extras is not None:
        extras["ema"] = None if ckpt.get("ema") is None else checkpoint_DDP_to_SingleGPU(ckpt["ema"])
    if optimizer is None:
        return model
    optimizer.load_state_dict(ckpt["optimizer"])
    for state in optimizer.state.values():
        for k, v in state.items():
            if isinstance(v, torch.Tensor):
                state[k] = v.to(device)
    warmup_scheduler.load_state_dict(ckpt["warmup_scheduler"])
    training_scheduler.load_state_dict(ckpt["training_scheduler"])
    return model, optimizer, warmup_scheduler, training_scheduler, ckpt["epoch"], ckpt["best_train_dice"], ckpt["best_val_dice"]
