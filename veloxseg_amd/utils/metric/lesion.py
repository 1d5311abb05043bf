"""Lesion-level evaluation on the GPU: the autoPET challenge's false-positive and false-negative volumes, defined on connected components, next to Dice.

  false_pos_vol   volume of the PREDICTED components that share no voxel with the ground truth
  false_neg_vol   volume of the GROUND-TRUTH components that share no voxel with the prediction

Both maps are binarised with `!= 0` and labelled with 18-connectivity by default (the connectivity the challenge defines its components with); one shared voxel
counts as overlap.  This restates the definition of the challenge's published script; it is NOT pinned against that script: the oracle is the numpy restatement in
tests/components_ref.py.  `metrics_tensor`'s FP / FN (utils/metric/metrics.py) are per-voxel rates and cannot express these.

The labelling and the tallies are HIP kernels (csrc/components.hip); per sample seven integers come back to the host, in one copy for the whole batch."""
import torch

from ..components import _samples, _sizes, connected_components


def lesion_metrics(gt: torch.Tensor, pred: torch.Tensor, voxel_volume: float = 1.0, connectivity: int = 18):
    """gt, pred: (B, 1, D, H, W) or (D, H, W) device label maps (bool / uint8 / int32 / int64) -> one dict per sample (a list; a single dict for (D, H, W)):
    false_pos_vol, false_neg_vol (int64 voxel counts times voxel_volume, formed in float64 on the host), n_gt, n_pred (component counts), n_gt_detected (ground-truth
    components that touch the prediction), n_pred_matched (predicted components that touch the ground truth) and dice = 2 |gt & pred| / (|gt| + |pred|), 1.0 when
    both maps are empty."""
    g, batched = _samples(gt, "lesion_metrics")
    p, _ = _samples(pred, "lesion_metrics")
    if g.shape != p.shape:
        raise ValueError(f"lesion_metrics: ground truth {tuple(gt.shape)} and prediction {tuple(pred.shape)} differ in shape")
    shape = (g.shape[0], 1) + tuple(g.shape[1:])
    gb, pb = (g != 0).view(torch.uint8).reshape(shape), (p != 0).view(torch.uint8).reshape(shape)
    cg, ng = connected_components(gb, connectivity)
    cp, np_ = connected_components(pb, connectivity)
    sg, hg, _ = _sizes(cg, ng, pb, "lesion_metrics")
    sp, hp, _ = _sizes(cp, np_, gb, "lesion_metrics")
    rows = []
    for b in range(g.shape[0]):
        s_g, h_g, s_p, h_p = sg[b][1:], hg[b][1:], sp[b][1:], hp[b][1:]
        rows.append(torch.stack([(s_p * (h_p == 0)).sum(), (s_g * (h_g == 0)).sum(), (h_g > 0).sum(), (h_p > 0).sum(), h_g.sum(), s_g.sum(), s_p.sum()]))
    host = torch.stack(rows).cpu().tolist()          # the one device -> host copy
    out = []
    for b, (fp, fn, det, mat, inter, vg, vp) in enumerate(host):
        out.append({"false_pos_vol": float(fp) * float(voxel_volume), "false_neg_vol": float(fn) * float(voxel_volume), "n_gt": ng[b], "n_pred": np_[b],
                    "n_gt_detected": int(det), "n_pred_matched": int(mat), "dice": 1.0 if vg + vp == 0 else 2.0 * inter / (vg + vp)})
    return out if batched else out[0]
