#!/usr/bin/env python3
"""Make the EMA weights of a training checkpoint the ones inference loads: writes a copy of SRC whose "model" entry is SRC's "ema" entry
(veloxseg_amd.utils.load_model.ema_checkpoint), e.g.

    python tools/ema_checkpoint.py ck/val_best.pth ck/val_best_ema.pth
    python run_test.py ... --checkpoint_dir ck --checkpoint_index val_best_ema

Needs no GPU."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from veloxseg_amd.utils.load_model import ema_checkpoint

if __name__ == "__main__":
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    try:
        print(ema_checkpoint(sys.argv[1], sys.argv[2]))
    except KeyError as e:
        raise SystemExit(str(e.args[0]))
