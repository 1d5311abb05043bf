"""Ensemble inference: the weighted mean of the soft-max probabilities of several models (cross-validation folds, or logits of other networks), its arg-max labels
and its per-voxel entropy, on the GPU (csrc/ensemble.hip).

One kernel call per model adds weight * softmax(logits) into ONE probability volume (vx_softmax_accumulate), one call at the end forms labels and entropy
(vx_prob_finalize): at most one logits volume and one probability volume are alive, however many models take part.  The weights are normalised on the host, so the
volume is the weighted mean itself and nothing divides at the end.

Caveat: the labels of a ONE-model ensemble are not guaranteed to equal infer_volume's.  Soft-max is monotone in exact arithmetic only: two logits closer than about
one ulp of their exp can round to equal probabilities, and the tie then goes to the lower class."""
from __future__ import annotations

import math
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _hip as H


def normalise_weights(weights, n: int) -> List[float]:
    """the n ensemble weights as the kernels take them: w_i / sum(w) formed in fp64 and rounded to fp32 (None: float32(1 / n) each).  Weights must be finite and
    positive, one per model; anything else raises ValueError"""
    if n < 1:
        raise ValueError("ensemble: at least one model is needed")
    if weights is None:
        return [float(np.float32(1.0 / n))] * n
    try:
        weights = list(weights)
        w = [float(x) for x in weights]
    except (TypeError, ValueError):
        raise ValueError(f"ensemble: weights must be {n} finite positive numbers, got {weights!r}") from None
    if len(w) != n:
        raise ValueError(f"ensemble: {len(w)} weights for {n} models")
    if any(isinstance(x, (bool, str)) for x in weights) or not all(math.isfinite(x) and x > 0 for x in w):
        raise ValueError(f"ensemble: weights must be finite and positive, got {weights!r}")
    total = math.fsum(w)
    out = [float(np.float32(x / total)) for x in w]
    if not all(math.isfinite(x) and x > 0 for x in out):
        raise ValueError(f"ensemble: weights {weights!r} do not normalise to positive fp32 numbers")
    return out


class ProbabilityAccumulator:
    """owns psum (B, K, D, H, W) fp32: after add(logits_i, w_i) for every model, with the w_i of normalise_weights, it holds the weighted mean of the models' soft-max
    probabilities.  The first add writes psum (it is never zeroed), the others add to it; finalize / labels / entropy read it."""

    def __init__(self, K: int, spatial: Sequence[int], device, batch: int = 1):
        K, batch, spatial = int(K), int(batch), tuple(int(s) for s in spatial)
        if not 1 <= K <= 256:
            raise ValueError(f"ProbabilityAccumulator: {K} classes outside 1..256 (labels are uint8)")
        if batch < 1 or len(spatial) != 3 or min(spatial) < 1:
            raise ValueError(f"ProbabilityAccumulator: bad extent, batch {batch}, spatial {spatial}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("veloxseg_amd ensemble runs on MI355X only (no CPU path); give a cuda device")
        self.K, self.batch, self.spatial = K, batch, spatial
        self.V = spatial[0] * spatial[1] * spatial[2]
        self.count = 0
        self.psum = torch.empty((batch, K) + spatial, device=device, dtype=torch.float32)

    def add(self, logits: torch.Tensor, weight: float) -> None:
        """psum (= for the first call, += after it) weight * softmax(logits, dim=1): one vx_softmax_accumulate call.  logits: (B, K, D, H, W) float32 on psum's device"""
        if logits.dim() != 5 or tuple(logits.shape[2:]) != self.spatial or logits.shape[0] != self.batch:
            raise ValueError(f"ensemble: logits of shape {tuple(logits.shape)} do not fit the accumulator's {tuple(self.psum.shape)}")
        if logits.shape[1] != self.K:
            raise ValueError(f"ensemble: a model with {logits.shape[1]} classes in an ensemble of {self.K}")
        weight = float(weight)
        if not (math.isfinite(weight) and weight > 0):
            raise ValueError(f"ensemble: weight {weight!r} is not finite and positive")
        if logits.device != self.psum.device:
            raise RuntimeError(f"veloxseg_amd ensemble: logits live on {logits.device}, the accumulator on {self.psum.device} (there is no CPU path)")
        H.call("vx_softmax_accumulate", H.P(logits.contiguous()), H.P(self.psum), self.batch, self.K, self.V, weight, int(self.count == 0), H.stream_ptr())
        self.count += 1

    def probabilities(self) -> torch.Tensor:
        """psum itself, no copy"""
        if self.count == 0:
            raise RuntimeError("ProbabilityAccumulator: nothing was added yet")
        return self.psum

    def finalize(self, labels: bool = True, entropy: bool = False):
        """-> (uint8 labels (B, 1, D, H, W) or None, fp32 entropy (B, 1, D, H, W) or None) from ONE vx_prob_finalize call.  Labels: first NaN, else first maximum,
        byte for byte vx_argmax_channels(psum); entropy: -sum p ln p in nats"""
        if not (labels or entropy):
            raise ValueError("ProbabilityAccumulator.finalize: ask for labels, entropy or both")
        p = self.probabilities()
        shape = (self.batch, 1) + self.spatial
        lab = torch.empty(shape, device=p.device, dtype=torch.uint8) if labels else None
        ent = torch.empty(shape, device=p.device, dtype=torch.float32) if entropy else None
        H.call("vx_prob_finalize", H.P(p), H.P(lab, torch.uint8), H.P(ent), self.batch, self.K, self.V, H.stream_ptr())
        return lab, ent

    def labels(self) -> torch.Tensor:
        return self.finalize(labels=True, entropy=False)[0]

    def entropy(self) -> torch.Tensor:
        return self.finalize(labels=False, entropy=True)[1]


def _check_logits_list(logits_list):
    if len(logits_list) == 0:
        raise ValueError("ensemble: at least one model is needed")
    first = logits_list[0]
    for x in logits_list:
        if not isinstance(x, torch.Tensor) or x.dim() != 5 or x.dtype != torch.float32:
            raise ValueError("ensemble: every entry must be a (B, K, D, H, W) float32 tensor")
        if x.shape[1] != first.shape[1]:
            raise ValueError(f"ensemble: models with {first.shape[1]} and {x.shape[1]} classes cannot be averaged")
        if x.shape != first.shape:
            raise ValueError(f"ensemble: logits of shapes {tuple(first.shape)} and {tuple(x.shape)} cannot be averaged")


def softmax_mean(logits_list: Sequence[torch.Tensor], weights=None, entropy: bool = False):
    """the functional form for logits the caller already has (they may come from other networks: only K and the spatial shape must agree):
    -> (mean probabilities (B, K, D, H, W), uint8 labels (B, 1, D, H, W)), and the entropy (B, 1, D, H, W) of the mean as a third value with entropy=True.
    One kernel call per entry and one at the end.  See the module's caveat on one-model ensembles."""
    logits_list = list(logits_list)
    _check_logits_list(logits_list)
    w = normalise_weights(weights, len(logits_list))
    x0 = logits_list[0]
    if not x0.is_cuda:
        raise RuntimeError("veloxseg_amd ensemble runs on MI355X only (no CPU path); move the logits to a cuda device")
    acc = ProbabilityAccumulator(x0.shape[1], x0.shape[2:], x0.device, batch=x0.shape[0])
    for x, wi in zip(logits_list, w):
        acc.add(x, wi)
    lab, ent = acc.finalize(labels=True, entropy=entropy)
    return (acc.probabilities(), lab, ent) if entropy else (acc.probabilities(), lab)


def _declared_classes(model) -> Optional[int]:
    inner = getattr(model, "_model", model)          # (inference_runtime.Net wraps the model)
    k = getattr(inner, "n_classes", None)
    return int(k) if isinstance(k, int) and not isinstance(k, bool) else None


@torch.inference_mode()
def infer_ensemble(models: Sequence[torch.nn.Module], volume: torch.Tensor, roi_size: Sequence[int], sw_batch_size: int, overlap: float, weights=None,
                   taped: bool = True, postprocess=None, mirror_axes: Sequence[int] = (), blend: str = "constant", sigma_scale=0.125, native=None,
                   entropy: bool = False):
    """eval-mode sliding-window segmentation of one (B, C, D, H, W) volume by an ensemble -> (mean soft-max probabilities (B, K, D, H, W), uint8 labels (B, 1, ...)),
    and the entropy of the mean (B, 1, D, H, W) as a third value with entropy=True.
    The models run one after another through inference_runtime.infer_volume (each with its own TapedPredictor, tapes and replicas; taped, mirror_axes, blend and
    sigma_scale are handed on: windows and mirrors are blended in LOGIT space, per model, as before); each model's logits are added into the one probability volume and
    released before the next model runs.  weights: None (equal) or one finite positive number per model, normalised on the host (normalise_weights).
    native: infer_volume's dict; the labels then come from labels_on_native_grid(probabilities[b], ...) -- the mean probabilities are interpolated and then arg-maxed,
    nnU-Net's order -- and live on the image's own grid; probabilities and entropy stay on the network grid.  postprocess: runs on the final labels only.
    Every model's training flag is restored, also when a later model raises.  An empty list, bad weights, models that declare different n_classes: ValueError before
    any GPU work (models that declare nothing are checked when their logits arrive); a non-CUDA volume: RuntimeError, as from sliding_window_inference.
    Caveat: the labels of a ONE-model ensemble are not guaranteed to equal infer_volume's -- soft-max is monotone in exact arithmetic only; two logits closer than about
    one ulp of their exp can round to equal probabilities, and the tie then goes to the lower class."""
    from .inference_runtime import infer_volume
    models = list(models)
    w = normalise_weights(weights, len(models))
    declared = [k for k in map(_declared_classes, models) if k is not None]
    if len(set(declared)) > 1:
        raise ValueError(f"ensemble: models with different numbers of classes {sorted(set(declared))} cannot be averaged")
    if native is not None:
        from .preprocess import check_native_geometry
        native = check_native_geometry(native)
    if postprocess is not None:
        from .components import Postprocess
        postprocess = postprocess if isinstance(postprocess, Postprocess) else Postprocess.from_config(postprocess)
    if not volume.is_cuda:
        raise RuntimeError("veloxseg_amd sliding window runs on MI355X only (no CPU path); move the volume to a cuda device")
    acc = None
    for model, wi in zip(models, w):
        logits, _ = infer_volume(model, volume, roi_size, sw_batch_size, overlap, taped=taped, postprocess=None, mirror_axes=mirror_axes, blend=blend,
                                 sigma_scale=sigma_scale, native=None)
        if acc is None:
            acc = ProbabilityAccumulator(logits.shape[1], logits.shape[2:], logits.device, batch=logits.shape[0])
        acc.add(logits, wi)
        del logits
    labels, ent = acc.finalize(labels=native is None, entropy=entropy) if (native is None or entropy) else (None, None)
    psum = acc.probabilities()
    if native is not None:
        from .preprocess import labels_on_native_grid
        labels = torch.stack([labels_on_native_grid(psum[b], native["native_shape"], native["net_spacing"], native["native_spacing"])
                              for b in range(psum.shape[0])])[:, None]
    if postprocess is not None:
        labels = postprocess(labels)
    return (psum, labels, ent) if entropy else (psum, labels)
