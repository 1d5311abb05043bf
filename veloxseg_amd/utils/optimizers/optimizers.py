"""Optimizer registry -- mirrors utils/optimizers/optimizers.py of the reference (same names, same torch.optim objects).
With TrainEngine the AdamW object is the STATE CARRIER (param_groups drive the LR schedulers, .state aliases the engine's flat
moment buffers so optimizer.state_dict() is the reference checkpoint format); the update itself is the fused HIP vx_adamw_step.
Beyond the reference: optimizer_args["no_weight_decay"] ("1d" or a list of name substrings) puts the matched parameters into a second group with weight_decay 0."""
from typing import Dict

import torch.optim as optim


def optim_adam(model, optimizer_args):
    return optim.Adam(model.parameters(), lr=optimizer_args["lr"], weight_decay=optimizer_args.get("weight_decay"))


def optim_sgd(model, optimizer_args):
    return optim.SGD(model.parameters(), lr=optimizer_args["lr"], weight_decay=optimizer_args.get("weight_decay"), momentum=optimizer_args.get("momentum"))


def split_no_weight_decay(model, rule):
    """-> (decayed, not decayed) parameters of `model` in registration order.  rule = "1d": every parameter with ndim <= 1 (biases, norm scales and shifts);
    or a list of name substrings (e.g. ["bias", "norm", "relative_position"])"""
    if isinstance(rule, str):
        if rule != "1d":
            raise ValueError('no_weight_decay must be "1d" or a list of name substrings')
        hit = lambda n, p: p.ndim <= 1
    else:
        subs = [str(s) for s in rule]
        hit = lambda n, p: any(s in n for s in subs)
    decay, no_decay = [], []
    for n, p in model.named_parameters():
        (no_decay if hit(n, p) else decay).append(p)
    return decay, no_decay


def optim_adamw(model, optimizer_args):
    rule = optimizer_args.get("no_weight_decay")
    if rule is None:
        return optim.AdamW(model.parameters(), lr=optimizer_args["lr"], weight_decay=optimizer_args["weight_decay"])
    # two param groups (TrainEngine's fused update reads lr / weight_decay per group: engine.bind_optimizer); an empty group is left out
    decay, no_decay = split_no_weight_decay(model, rule)
    groups = [{"params": ps, "weight_decay": wd} for ps, wd in ((decay, optimizer_args["weight_decay"]), (no_decay, 0.0)) if ps]
    return optim.AdamW(groups, lr=optimizer_args["lr"], weight_decay=optimizer_args["weight_decay"])


def build_optimizer(model, optimizer_type: str, optimizer_args: Dict):
    if optimizer_type == "adam":
        return optim_adam(model, optimizer_args)
    elif optimizer_type == "adamw":
        return optim_adamw(model, optimizer_args)
    elif optimizer_type == "sgd":
        return optim_sgd(model, optimizer_args)
    raise ValueError("must be adam or adamw for now")
