"""Autograd operators of the VeloxSeg hot path, each backed by hand-written HIP kernels (libveloxseg_hip.so).

Every operator takes / returns contiguous fp32 NCDHW CUDA tensors and launches on the current PyTorch
HIP stream, so a whole training step can be captured into one hipGraph.  Parameter gradients are
ACCUMULATED IN PLACE into `param.grad` by the weight-gradient kernels (float atomics), and `None` is
returned to autograd for them: no per-parameter AccumulateGrad kernels, one flat gradient buffer for
the RCCL all-reduce and the fused AdamW (see veloxseg_amd/engine.py).

The host side of the convolutions, norms, element-wise operators and composite blocks -- kernel selection, workspaces, autograd nodes -- is C++
(csrc/_vxops.cpp); the functions here call those nodes directly or through torch.ops.veloxseg.*, the fused loss among them (torch.ops.veloxseg.seg_loss).
The fused PWA chains and the fan-out are Python autograd functions over the same C ABI; StagedLoss, the loss taken apart for the taped step, calls it without autograd.

There is no CPU implementation here on purpose (tier rule: the product path has no fallback).
"""
from __future__ import annotations

import itertools
import os
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _hip as H

# host-side kernel choices of the C++ operator bodies (csrc/_vxops.cpp `Flags`); change them with set_host_flags(), which forwards them
WGRAD_UNTILED = False                         # generic weight gradient on the untiled reference kernel vx_conv3d_bwd_weight (A/B tests) instead of the tiled one
USE_EXPAND_MFMA = True                        # patch-expand input gradient on fp32 MFMA (False = conv_s1 VALU kernel)
# fp32 mode of the patch-expand layers (forward + input gradient, 49 % of the training FLOPs): 3 = every fp32 operand as three bf16 pieces, six bf16 MFMAs per
# pair (the fp32 product to 2^-27; 2.7 x fewer matrix-pipe clocks than v_mfma_f32_16x16x4_f32), 2 = two pieces / three MFMAs (~1e-5 relative), 0 = fp32 MFMA
EXPAND_SPLIT = 22      # 22 = two scaled fp16 pieces (3 MFMAs per product, closer to fp64 than 3 bf16 pieces); 3 / 2 = bf16 pieces; 0 = fp32 MFMA
USE_S1 = True                                 # register-blocked stride-1 conv kernel (False = generic kernels, for A/B tests)
USE_IN_ROW = True                             # InstanceNorm of short rows (V <= 4096): statistics + application in one launch
IN_ROW_MAX = 4096
USE_WGRAD_WS = False                          # tiled weight gradient through a partial-sum workspace (deterministic order) instead of float atomics (30 fewer launches per step: +2 %)
USE_PATCHIFY = True                           # kernel == stride convs (PatchEmbed) as patchify + 1x1 conv (False = generic direct conv)
USE_GCONV1 = True                             # dedicated weight-gradient kernel of the 1x1x1 grouped JLC conv (False = tiled kernel)
PW_MFMA_MAX_V = 4096                          # 1x1 convs on volumes up to this many voxels use the MFMA tile kernel
BRANCH_STREAMS = True                         # independent sub-networks (M+1 decoders; encoder conv chain vs PWA chain) run on forked HIP streams
MODALITY_STREAMS = 1                          # 1: per-modality halves of a PWA block on forked streams; 2: + PatchEmbed / PatchMerging
IN_EPS = 1e-5      # nn.InstanceNorm3d default (reference common_function.py:63-66)
LN_EPS = 1e-6      # reference attention_utils.py:15

# ------------------------------------------------------------------------------------------------
# dropout RNG state: device int64[2] = {seed, step}; kernels hash (seed, step, site, element index)
# ------------------------------------------------------------------------------------------------
_site_counter = itertools.count(1)
_rng_state = {}


_branch_streams = {}


def _record(ts, stream):
    for t in ts:
        if isinstance(t, (list, tuple)):
            _record(t, stream)
        elif torch.is_tensor(t) and t.is_cuda:
            t.record_stream(stream)


def run_branches(fns, device, tag: str = "branches", uses=None):
    """Run independent closures `fns` (each returns a tensor or a tuple/list of tensors) on forked HIP streams and join them on
    the current stream.  `uses[k]` = the tensors branch k reads that were allocated on another stream: they are `record_stream`-ed on
    the branch's stream, otherwise the caching allocator may hand their memory to a new tensor as soon as the host drops the last
    reference -- in the backward pass that is while the branch's (saved-tensor-reading) kernels are still queued, and the first training
    step then computes a gradient from recycled memory.  The autograd engine replays every backward node on the stream its forward ran on, so the backward
    passes of the branches overlap too; under hipGraph capture the fork/join becomes parallel branches of the graph.  The branches
    are chains of small kernels (a 4^3 .. 32^3 decoder level rarely fills 256 CUs), which is what makes the overlap pay."""
    if not BRANCH_STREAMS or len(fns) < 2:
        return [f() for f in fns]
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    cur = torch.cuda.current_stream(device)
    key = (str(device), len(fns), tag)
    if key not in _branch_streams:
        _branch_streams[key] = [torch.cuda.Stream(device=device) for _ in fns]
    outs = []
    for k_, (s_, f) in enumerate(zip(_branch_streams[key], fns)):
        s_.wait_stream(cur)
        if uses is not None:
            _record(uses[k_], s_)
        with torch.cuda.stream(s_):
            outs.append(f())
    for s_, o in zip(_branch_streams[key], outs):
        cur.wait_stream(s_)
        for t in (o if isinstance(o, (tuple, list)) else (o,)):
            for u in (t if isinstance(t, (tuple, list)) else (t,)):
                if torch.is_tensor(u):
                    u.record_stream(cur)
    return outs


_streams_ready = set()


def ensure_streams(device, n_modalities: int):
    """Create every side stream the model uses (encoder conv chain, M modality branches, M+1 decoder branches) BEFORE the first kernel of the
    first forward, then synchronise once.  Streams created lazily in the middle of the first forward gave a wrong first-iteration gradient
    for the last node of the encoder conv chain (a cross-stream ordering the runtime only honoured once all queues existed;
    AMD_SERIALIZE_KERNEL=3 or this eager creation make the first step equal to the later ones: tests/test_hip_model_gpu.py)."""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), n_modalities)
    if key in _streams_ready or not BRANCH_STREAMS:
        return
    side_stream(device, "encoder_conv")
    for n, tag in ((n_modalities, "modalities"), (n_modalities + 1, "branches")):
        k = (str(device), n, tag)
        if n >= 2 and k not in _branch_streams:
            _branch_streams[k] = [torch.cuda.Stream(device=device) for _ in range(n)]
    torch.cuda.synchronize(device)
    _streams_ready.add(key)


def branch_stream_list(device, n: int, tag: str = "branches"):
    """the streams run_branches uses for `n` branches with this tag (empty when branch streams are off or not created yet)"""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return list(_branch_streams.get((str(device), n, tag), [])) if BRANCH_STREAMS else []


def all_side_streams(device):
    """every stream this module has forked work onto on `device` (branch / modality lists and named side streams)"""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out = []
    for k, v in _branch_streams.items():
        if k[0] != str(device):
            continue
        out.extend(v if isinstance(v, list) else [v])
    return out


def side_stream(device, name: str) -> "torch.cuda.Stream":
    """a named, cached side stream of `device` (one per role, e.g. the conv chain of the encoder)"""
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (str(device), name)
    if key not in _branch_streams:
        _branch_streams[key] = torch.cuda.Stream(device=device)
    return _branch_streams[key]


def new_dropout_site() -> int:
    return next(_site_counter)


def reset_dropout_sites():
    """Called at the top of VeloxSeg.__init__: site ids are then a function of the architecture only, so two models built
    from the same config draw the same dropout streams for the same (seed, step)."""
    global _site_counter
    _site_counter = itertools.count(1)


def rng_state(device) -> torch.Tensor:
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())      # "cuda" and "cuda:0" must name the same state
    key = str(device)
    if key not in _rng_state:
        _rng_state[key] = torch.tensor([12345, 0], dtype=torch.int64, device=device)
    return _rng_state[key]


def manual_seed(seed: int, device="cuda"):
    st = rng_state(torch.device(device) if not isinstance(device, torch.device) else device)
    st.copy_(torch.tensor([seed, 0], dtype=torch.int64))


RNG_INPLACE = False      # hipGraph capture (engine.TrainEngine(use_graph=True)): the captured step must bump the SAME tensor on every replay
_rng_keep = {}           # device -> the {seed, step} tensors of the most recent training forwards (kept alive for their backward passes)
_rng_inc = {}


def advance_rng(device):
    """New dropout step.  Every training forward gets its OWN {seed, step} tensor (the previous ones stay alive for the last 32 forwards): the
    kernels read {seed, step} at execution time through the pointer their autograd node captured in forward, so a second forward before the
    first backward (micro-batching, two models on one device) can no longer change the masks an earlier forward's backward regenerates."""
    st = rng_state(device)
    if RNG_INPLACE:
        st[1:2].add_(1)
        return
    key = str(st.device)
    inc = _rng_inc.get(key)
    if inc is None:
        inc = _rng_inc[key] = torch.tensor([0, 1], dtype=torch.int64, device=st.device)
    keep = _rng_keep.setdefault(key, [])
    keep.append(st)
    if len(keep) > 32:
        del keep[0]
    _rng_state[key] = st + inc


def grad_buf(p: torch.Tensor) -> torch.Tensor:
    """Running gradient buffer of a parameter (created zeroed on first use)."""
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


_HOST_FLAGS = ("USE_S1", "USE_EXPAND_MFMA", "USE_GCONV1", "USE_WGRAD_WS", "USE_PATCHIFY", "USE_IN_ROW", "PW_MFMA_MAX_V", "IN_ROW_MAX", "WGRAD_UNTILED")
_CPP = None


def _push_host_flags(m):
    m.set_flags(s1=USE_S1, expand_mfma=USE_EXPAND_MFMA, gconv1=USE_GCONV1, wgrad_ws=USE_WGRAD_WS, patchify=USE_PATCHIFY, in_row=USE_IN_ROW,
                pw_mfma_max_v=PW_MFMA_MAX_V, in_row_max=IN_ROW_MAX, in_eps=IN_EPS, ln_eps=LN_EPS, wgrad_untiled=WGRAD_UNTILED)


def cpp_module(reload: bool = False):
    """veloxseg_amd._vxops (csrc/_vxops.cpp, built by __graft_entry__.build): the host side of the operators and the owner of the torch.ops.veloxseg
    schemas, configured with this module's flags when it is first loaded; a module that is missing or does not import raises"""
    global _CPP
    if _CPP is None or reload:
        try:
            H.LIB.load()
            from . import _vxops
        except ImportError as e:
            raise RuntimeError("veloxseg_amd: the C++ operator module veloxseg_amd._vxops cannot be imported (" + str(e)[:200] + "); build it with "
                               "`python -c 'import __graft_entry__ as g; g.build()'`") from e
        _vxops.set_expand_split(EXPAND_SPLIT)
        _vxops.set_tile_min_c(TILE_MIN_C)
        _push_host_flags(_vxops)
        _CPP = _vxops
    return _CPP


def set_host_flags(**kw):
    """Set kernel-choice flags (the names of _HOST_FLAGS) here AND in the C++ operator bodies, which make the choice; returns the previous
    values of the flags it was given, so that `old = set_host_flags(...)` / `finally: set_host_flags(**old)` restores them."""
    unknown = sorted(set(kw) - set(_HOST_FLAGS))
    if unknown:
        raise TypeError(f"set_host_flags: unknown flag(s) {unknown}; known: {_HOST_FLAGS}")
    g = globals()
    old = {k: g[k] for k in kw}
    g.update(kw)
    _push_host_flags(cpp_module())
    return old


def _ops():
    """torch.ops.veloxseg, with the extension that registers it loaded"""
    cpp_module()
    return torch.ops.veloxseg


_PRECISION = "fp32"
BF16_STORAGE = os.environ.get("VELOXSEG_BF16_STORAGE", "1") != "0"      # (tests assign it as well)


def set_precision(mode: str):
    """"fp32" (default: every product in fp32, the parity mode) or "bf16": the opt-in mode of BASELINE configs[1] -- bf16 MFMA operands with fp32
    accumulation in the patch-expand layers (forward, input and weight gradient; 49 % of the training FLOPs) and in the JLC grouped convolutions (forward,
    input and weight gradient; 29 %), fp32 tensors in HBM, fp32 norms / soft-max / loss.  Judged by Dice, not by the fp32 logit tolerance (tests/test_bf16_gpu.py).  Process-wide; TrainEngine(precision=...) sets it."""
    global _PRECISION
    if mode not in ("fp32", "bf16"):
        raise ValueError("precision must be 'fp32' or 'bf16'")
    m = cpp_module()
    m.set_bf16_expand(mode == "bf16")
    # round 6: the bf16 mode also STORES 16-bit tensors (VELOXSEG_BF16_STORAGE=0: operands only, the mode of rounds 2-5, for the A/B): the block-internal tensors of the JLC blocks
    # at the 32^3 level (y_k, o, dn, d_o, g_k) and the full-resolution heads / reconstructions with their gradients; fp32: statistics, sums, soft-max, loss, master weights,
    # flat gradients, AdamW, every block-boundary tensor
    m.set_act_bf16(mode == "bf16" and BF16_STORAGE)
    # the stem DownConv (k7 s4, conv_blocks.py:4-21) on plain fp16 operands in the bf16 mode (one MFMA per step instead of three, half the LDS)
    H.call("vx_conv_mfma_set_stem_pieces", 1 if mode == "bf16" else 2)
    # the JLC grouped convolutions and their weight gradients on the matrix pipe (csrc/jlc_mfma.hip): 3 bf16 pieces per operand (six piece products = the fp32
    # product) in the fp32 mode, ONE piece (plain bf16 operands, fp32 accumulation) in the bf16 mode
    H.call("vx_jlc_tz_set_pieces", 1 if mode == "bf16" else 22)     # 22 = two scaled fp16 pieces (22 significant bits, three piece products: csrc/jlc_mfma.hip)
    _PRECISION = mode


def get_precision() -> str:
    return _PRECISION


def rs_ptr(device, p):
    """address of the {seed, step} tensor for the C++ nodes (0 without dropout)"""
    return rng_state(device).data_ptr() if p > 0 else 0


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


def _check(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise RuntimeError(f"veloxseg_amd.{what}: input is on {x.device}; the VeloxSeg hot path runs only on an MI355X "
                           "(HIP kernels, no CPU fallback)")
    if x.dtype != torch.float32:
        raise RuntimeError(f"veloxseg_amd.{what}: expected float32, got {x.dtype}")
    if x.device.index != torch.cuda.current_device():
        raise RuntimeError(f"veloxseg_amd.{what}: tensor lives on cuda:{x.device.index} but the current device is cuda:{torch.cuda.current_device()}; "
                           "kernels launch on the current device's stream -- wrap the call in torch.cuda.device(tensor.device)")


# ------------------------------------------------------------------------------------------------
# convolutions
# ------------------------------------------------------------------------------------------------
# The model reaches the seven C++-registered operators THROUGH THE DISPATCHER (torch.ops.veloxseg.*: Autograd / CUDA / Meta keys registered by csrc/_vxops.cpp) wherever
# the call has the schema's form; forms the schemas do not carry (two-pointer concat input, the "feeds an InstanceNorm" hint) call the node directly.  A taped step
# replays captured launches, so the extra dispatcher hop costs the eager path only.


def conv3d(x, w, b=None, *, x2=None, stride=1, padding=0, groups=1, pixel_shuffle=1, out_bf16=False):
    """Conv3d (+ optional channel-concat input, + optional PixelShuffle store).  out_bf16 (bf16 storage mode, patch-expand layers only): the output is a bfloat16 tensor
    -- the full-resolution logits / reconstructions -- and the backward accepts a bfloat16 gradient; ignored wherever the 16-bit kernels do not apply."""
    K = int(w.shape[2])
    if x2 is not None:
        return cpp_module().conv(x, x2, w, b, K, int(stride), int(padding), int(groups), int(pixel_shuffle))
    if out_bf16 and _PRECISION == "bf16" and BF16_STORAGE:
        return cpp_module().conv_h(x, w, b, K, int(stride), int(padding), int(groups), int(pixel_shuffle))
    return _ops().conv3d(x, w, b, int(stride), int(padding), int(groups), int(pixel_shuffle))


def conv_transpose_k2s2(x, w, b, feeds_instnorm: bool = False):
    """feeds_instnorm: the output goes straight into an InstanceNorm (UpConv): the bias gradient is zero by construction and is not computed"""
    if not feeds_instnorm and b is not None:
        return _ops().conv_transpose_k2s2(x, w, b)
    return cpp_module().upconv_k2s2(x, w, b, bool(feeds_instnorm))


# ------------------------------------------------------------------------------------------------
# InstanceNorm (+ activation, + n-way sum, + residual)
# ------------------------------------------------------------------------------------------------
def instnorm_sum(ys: Sequence[torch.Tensor], act: bool = False, res: Optional[torch.Tensor] = None):
    """(res) + sum_k act(InstanceNorm(y_k)), 1..3 inputs (the kernels take three; a fourth raises)."""
    return _ops().instance_norm_sum(list(ys), bool(act), res)


# ------------------------------------------------------------------------------------------------
# channels-first LayerNorm
# ------------------------------------------------------------------------------------------------
def layernorm_cf(x, gamma, beta):
    return _ops().layer_norm_cf(x, gamma, beta)


# ------------------------------------------------------------------------------------------------
# element-wise
# ------------------------------------------------------------------------------------------------
def gelu_dropout(a, p: float = 0.0, site: int = 0):
    return cpp_module().gelu(a, float(p), int(site), rs_ptr(a.device, p))


def residual_dropout(x, z, alpha: float = 1.0, p: float = 0.0, site: int = 0):
    """out = alpha * x + dropout(z)  (x may be None)."""
    return cpp_module().axpy(x, z, float(alpha), float(p), int(site), rs_ptr(z.device, p))


class _AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        _check(a, "add")
        a, b = _c(a), _c(b)
        out = torch.empty_like(a)
        H.call("vx_add", H.P(a), H.P(b), None, H.P(out), a.numel(), H.stream_ptr())
        return out

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _AddFn.apply(a, b)


# ------------------------------------------------------------------------------------------------
# composite blocks: ONE autograd node for a whole JLC block / transformer FFN tail
# ------------------------------------------------------------------------------------------------
# The fine-grained operators above cost ~45 us of host time each per step (autograd node + allocations), and the step is host-bound once
# the GPU side overlaps on several streams.  A composite is ONE C++ autograd node (csrc/_vxops.cpp JLCFn / FFNFn) that runs the
# block on its fused kernels where they apply and otherwise the forward / backward bodies of those operators in a fixed order; the dropout
# streams are identical either way.
USE_COMPOSITE = True


def weights_epoch_bump():
    """the parameters changed through raw pointers (TrainEngine's fused AdamW): weight images kept for inference (jlc_prefetch(keep=True)) are stale from here on"""
    return int(cpp_module().weights_epoch_bump())


def weights_epoch() -> int:
    return int(cpp_module().weights_epoch())


def jlc_prefetch(mod, grid, stream, keep: bool = False) -> bool:
    """Build the weight images of JLC block `mod` (its next forward runs on a `grid` = (D, H, W) volume) on `stream`, ahead of the block: the block's forward then launches
    no preparation kernels (csrc/_vxops.cpp jlc_prep_into / jlc_fwd_f).  The image buffer is the block's own and is re-used every step; an event recorded on `stream` is left
    on the block and waited for by its forward.  Returns False where the block builds nothing ahead (VALU convolutions)."""
    m = cpp_module()
    if len(mod.spatial_convs) != 3:
        return False
    convs = [seq[0] for seq in mod.spatial_convs]
    w = convs[0].weight
    if not w.is_cuda:
        return False
    C, G = int(w.shape[0]), int(convs[0].groups)
    kind, n = m.jlc_img_plan(C, G, int(grid[0]), int(grid[1]), int(grid[2]))
    if kind == 0:
        return False
    bufs = mod.__dict__.setdefault("_pf_img", {})                # one buffer per image kind: a tape holds the address of the one it was captured with
    img = bufs.get(int(kind))
    if img is None or img.numel() < n or img.device != w.device:
        img = bufs[int(kind)] = torch.empty(int(n), device=w.device, dtype=torch.float32)          # (allocated on the CURRENT stream, before the side stream is entered)
    with torch.cuda.stream(stream):
        ok = m.jlc_prep_into(convs[0].weight, convs[1].weight, convs[2].weight, img, C, G, int(grid[0]), int(grid[1]), int(grid[2]), stream.cuda_stream, bool(keep))
        if ok and not keep:          # (keep: inference -- the images are built once on the stream the forwards run on, nobody waits for an event)
            ev = torch.cuda.Event()
            ev.record(stream)
            mod._pf_ev = ev
    return bool(ok)


def expand_prefetch(conv, stream, keep: bool = False) -> bool:
    """Both weight images of a patch-expand layer (`conv`: the 3^3 convolution in front of PixelShuffle(4)) built on `stream` ahead of its forward (fp16-piece mode;
    csrc/_vxops.cpp expand_prep_into): the layer's forward and input gradient then launch their matrix kernels only.  The buffers are the layer's own, re-used every step.
    The caller joins `stream` before the layer runs (the engine's encoder-forward stage does)."""
    m = cpp_module()
    w = conv.weight
    if not w.is_cuda or w.dim() != 5:
        return False
    n = int(m.expand_img_floats(int(w.shape[0])))
    if n <= 0 or tuple(w.shape[1:]) != (16, 3, 3, 3):
        return False
    bufs = getattr(conv, "_pf_wt", None)
    if bufs is None or bufs[0].numel() < n or bufs[0].device != w.device:
        bufs = conv._pf_wt = (torch.empty(n, device=w.device, dtype=torch.float32), torch.empty(n, device=w.device, dtype=torch.float32))
    with torch.cuda.stream(stream):
        return bool(m.expand_prep_into(w, bufs[0], bufs[1], stream.cuda_stream, bool(keep)))


def jlc_block(x, mod, p: float, site: int):
    """x + sum_k GELU(IN(gconv_k(x))) =: o ;  out = o + Drop(conv2(GELU(conv1(IN(o)))))   (reference conv_blocks.py:41-75) as one autograd node"""
    convs = [seq[0] for seq in mod.spatial_convs]
    if len(convs) > 3:
        raise RuntimeError(f"veloxseg_amd.jlc_block: {len(convs)} spatial convolutions; the node and its kernels take at most 3")
    ev = mod.__dict__.pop("_pf_ev", None)                      # images prepared ahead on a side stream (jlc_prefetch): this stream waits for them
    if ev is not None:
        torch.cuda.current_stream(x.device).wait_event(ev)
    l1, l2 = mod.channel_conv[1], mod.channel_conv[3]
    w = [c.weight for c in convs] + [None] * (3 - len(convs))
    b = [c.bias for c in convs] + [None] * (3 - len(convs))
    return cpp_module().jlc(x, w[0], w[1], w[2], b[0], b[1], b[2], convs[0].groups, l1.weight, l1.bias, l2.weight, l2.bias, float(p), int(site), rs_ptr(x.device, p))


def ffn_tail(y, norm, ffn, p: float):
    """out = y + Drop(linear2(Drop(GELU(linear1(LN(y))))))   (reference PWA.py:437 with attention_utils.py:45-71) as one autograd node"""
    return cpp_module().ffn(y, norm.weight, norm.bias, ffn.linear1.weight, ffn.linear1.bias, ffn.linear2.weight, ffn.linear2.bias, float(p), int(ffn.site1), int(ffn.site2),
                            rs_ptr(y.device, p))


# ------------------------------------------------------------------------------------------------
# fused per-voxel chains of a PWA transformer block, all modalities in one launch (csrc/pwa_fused.hip)
# ------------------------------------------------------------------------------------------------
# channel stages (FFN tail of a PWA block, channel MLP of a JLC block) with >= this many channels run on the tile-GEMM chains of csrc/pwa_fused.hip (pwa_post / inmlp +
# grouped weight gradients) even where csrc/mlp.hip has an instance: at C = 32 (16^3 grids) mlp.hip's per-block weight staging and in-kernel weight-gradient
# flush cost 45-90 us per launch for 0.5 GFLOP; the tile kernels take 15-25 us (autopet128 747 -> 756 patches/s, autopet96 1061 -> 1079)
TILE_MIN_C = 32
USE_PWA_FUSED = True      # A/B (tests): False = LN, q / k / v, mix, FFN as separate launches per modality


def _ptrs(vals):
    """host array of device pointers (None -> NULL); the caller keeps it alive across the call"""
    return (H.ctypes.c_void_p * len(vals))(*[(v if v else None) for v in vals])


def _submit_wgrad(fn):
    """run fn(stream_ptr) now on the current stream, or -- while the engine defers weight gradients (csrc/_vxops.cpp WgradQueue) -- queue it with the
    other weight-gradient launches of the pass; fn owns its operands"""
    cpp_module().wgrad_submit_py(int(H.stream_ptr() or 0), int(torch.cuda.current_device()), fn)


WGG_JOBS, WGG_FOLDS = 24, 16          # capacity of one vx_pw_wgrad_group launch (csrc/pointwise.hip)
_wgg_pending = {}                     # (device, stream) -> [jobs, folds] collected while the engine defers weight gradients


def _wgrad_group(jobs, folds, st):
    """jobs: [(x, dy, dw, db or None, Cin, Cout, V, B)], folds: [(part, dgamma, dbeta, C, rows)] -> as few launches as the capacity allows"""
    jobs, folds = list(jobs), list(folds)
    while jobs or folds:
        j, jobs = jobs[:WGG_JOBS], jobs[WGG_JOBS:]
        f, folds = folds[:WGG_FOLDS], folds[WGG_FOLDS:]
        jp = _ptrs([v for q in j for v in (H.P(q[0]), H.P(q[1]), H.P(q[2]), H.P(q[3]))])
        jd = (H.ctypes.c_long * max(1, 4 * len(j)))(*[int(v) for q in j for v in q[4:8]])
        fp = _ptrs([v for q in f for v in (H.P(q[0]), H.P(q[1]), H.P(q[2]))])
        fd = (H.ctypes.c_int * max(1, 2 * len(f)))(*[int(v) for q in f for v in q[3:5]])
        H.call("vx_pw_wgrad_group", H.ctypes.addressof(jp) if j else None, H.ctypes.addressof(jd) if j else None, len(j),
               H.ctypes.addressof(fp) if f else None, H.ctypes.addressof(fd) if f else None, len(f), st)


def _submit_wgrad_jobs(jobs, folds):
    """The weight-gradient jobs / LayerNorm-parameter folds of one fused chain.  Immediate mode: one grouped launch now.  While the engine defers weight
    gradients, the jobs of EVERY chain of the pass submitted from this stream are pooled and leave in one or two grouped launches when the queue is joined
    (13 launches at the end of the encoder backward -> 2)."""
    if not jobs and not folds:
        return
    if not cpp_module().wgrad_deferring():
        _wgrad_group(jobs, folds, H.stream_ptr())
        return
    key = (int(torch.cuda.current_device()), int(H.stream_ptr() or 0))
    pend = _wgg_pending.get(key)
    fresh = pend is None
    if fresh:
        pend = _wgg_pending[key] = [[], []]
    # the jobs go into the pool BEFORE the flush closure is submitted: in side-stream deferral the queue auto-flushes every VX_WG_FLUSH closures, and a flush
    # that ran at once on an empty pool would pop it and orphan the jobs appended afterwards (their weight gradients silently lost)
    pend[0].extend(jobs)
    pend[1].extend(folds)
    if fresh:
        def flush(st, key=key):
            p_ = _wgg_pending.pop(key, None)
            if p_ is not None:
                _wgrad_group(p_[0], p_[1], st)
        _submit_wgrad(flush)


def _gb(p):
    return grad_buf(p) if (p is not None and p.requires_grad) else None


class _LnPwFn(torch.autograd.Function):
    """For every modality m: xn = LN(x_m), out_{m,s} = W_{m,s} xn + b_{m,s} (s < NS), all in ONE launch; s2d = PatchMerging's 8-way gather first.
    Returns the M * NS projections followed (not s2d) by the M inputs passed through: whoever adds x_m as a residual later takes the pass-through,
    so that its gradient arrives HERE and is added inside the backward kernel instead of by an autograd add launch."""

    @staticmethod
    def forward(ctx, M, NS, s2d, eps, *args):
        xs = [_c(t) for t in args[:M]]
        _check(xs[0], "pwa_pre")
        per = 2 + 2 * NS
        prm = [list(args[M + m * per: M + (m + 1) * per]) for m in range(M)]
        B = xs[0].shape[0]
        dev = xs[0].device
        if s2d:
            C0 = xs[0].shape[1]
            g = [int(v) // 2 for v in xs[0].shape[2:]]
            C = 8 * C0
        else:
            C = xs[0].shape[1]
            g = [int(v) for v in xs[0].shape[2:]]
        V = g[0] * g[1] * g[2]
        J = [int(prm[0][2 + 2 * s_].shape[0]) for s_ in range(NS)]
        Jc = (H.ctypes.c_int * 3)(*(J + [0] * (3 - NS)))
        xn = [torch.empty((B, C, *g), device=dev, dtype=torch.float32) for _ in range(M)]
        outs = [[torch.empty((B, J[s_], *g), device=dev, dtype=torch.float32) for s_ in range(NS)] for _ in range(M)]
        vals = []
        for m in range(M):
            gam, bet = prm[m][0], prm[m][1]
            ws = [prm[m][2 + 2 * s_] for s_ in range(NS)] + [None] * (3 - NS)
            bs = [prm[m][3 + 2 * s_] for s_ in range(NS)] + [None] * (3 - NS)
            os_ = outs[m] + [None] * (3 - NS)
            vals += [H.P(xs[m]), H.P(gam), H.P(bet), H.P(ws[0]), H.P(bs[0]), H.P(ws[1]), H.P(bs[1]), H.P(ws[2]), H.P(bs[2]), H.P(xn[m]), H.P(os_[0]), H.P(os_[1]), H.P(os_[2])]
        arr = _ptrs(vals)
        H.call("vx_ln_pw_fwd", H.ctypes.addressof(arr), M, NS, H.ctypes.addressof(Jc), B, C, V, float(eps), int(s2d), g[0], g[1], g[2], H.stream_ptr())
        ctx.save_for_backward(*xs, *xn)
        ctx.prm, ctx.geo = prm, (M, NS, int(s2d), float(eps), B, C, V, g, J)
        flat = [t for o in outs for t in o]
        if s2d:
            return tuple(flat)
        return tuple(flat) + tuple(args[:M])

    @staticmethod
    def backward(ctx, *grads):
        M, NS, s2d, eps, B, C, V, g, J = ctx.geo
        xs, xn = ctx.saved_tensors[:M], ctx.saved_tensors[M:]
        prm = ctx.prm
        dev = xs[0].device
        douts = [[grads[m * NS + s_] for s_ in range(NS)] for m in range(M)]
        dres = [None] * M if s2d else list(grads[M * NS:])
        for m in range(M):
            for s_ in range(NS):
                douts[m][s_] = _c(douts[m][s_]) if douts[m][s_] is not None else torch.zeros((B, J[s_], *g), device=dev, dtype=torch.float32)
        rows = H.query("vx_ln_pw_tiles", B, V) if not s2d else B * ((V + 15) // 16)
        parts = [torch.empty((rows, 2 * C), device=dev, dtype=torch.float32) for _ in range(M)]
        dxs = [torch.empty_like(x) for x in xs]
        Jc = (H.ctypes.c_int * 3)(*(J + [0] * (3 - NS)))
        vals = []
        for m in range(M):
            ws = [prm[m][2 + 2 * s_] for s_ in range(NS)] + [None] * (3 - NS)
            ds_ = douts[m] + [None] * (3 - NS)
            dr = _c(dres[m]) if dres[m] is not None else None
            vals += [H.P(xs[m]), H.P(prm[m][0]), H.P(ws[0]), H.P(ws[1]), H.P(ws[2]), H.P(ds_[0]), H.P(ds_[1]), H.P(ds_[2]), H.P(dr), H.P(dxs[m]), H.P(parts[m])]
        arr = _ptrs(vals)
        H.call("vx_ln_pw_bwd", H.ctypes.addressof(arr), M, NS, H.ctypes.addressof(Jc), B, C, V, eps, s2d, g[0], g[1], g[2], H.stream_ptr())
        jobs, folds = [], []
        for m in range(M):
            for s_ in range(NS):
                w_, b_ = prm[m][2 + 2 * s_], prm[m][3 + 2 * s_]
                if w_.requires_grad:
                    jobs.append((xn[m], douts[m][s_], grad_buf(w_), _gb(b_), C, J[s_], V, B))
            if prm[m][0].requires_grad:
                folds.append((parts[m], grad_buf(prm[m][0]), grad_buf(prm[m][1]), C, rows))
        _submit_wgrad_jobs(jobs, folds)
        return (None, None, None, None) + tuple(dxs) + (None,) * (len(prm) * len(prm[0]))


def ln_pw_ok(C, J, V, s2d=False):
    Jc = (H.ctypes.c_int * 3)(*(list(J) + [0] * (3 - len(J))))
    return bool(H.query("vx_ln_pw_ok", int(C), len(J), H.ctypes.addressof(Jc), int(V), int(bool(s2d))))


def pwa_pre(xs, norms, projs):
    """xs[m] -> ([q_m, k_m, v_m] per modality, x pass-throughs); norms[m] = LayerNorm module, projs[m] = the three ParamConv3d of modality m"""
    M = len(xs)
    args = list(xs)
    for m in range(M):
        args += [norms[m].weight, norms[m].bias]
        for c in projs[m]:
            args += [c.weight, c.bias]
    out = _LnPwFn.apply(M, 3, False, LN_EPS, *args)
    return [list(out[3 * m: 3 * m + 3]) for m in range(M)], list(out[3 * M:])


class _FanOutFn(torch.autograd.Function):
    """n aliases of every tensor of a list, one per consumer.  Backward: the n gradients of every tensor are summed in ONE launch for the whole list (vx_add_many)
    instead of n - 1 aten `add`s per tensor that the autograd engine would issue one by one as the consumers' gradients arrive (6.5 us each on the critical path of
    the encoder backward: the per-modality transformer features feed the mixer, the decoders and the next level's patch merge)."""

    @staticmethod
    def forward(ctx, n, *xs):
        ctx.n = n
        return tuple(x.view_as(x) for x in xs for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        import ctypes
        n = ctx.n
        k = len(gs) // n
        out = []
        groups = [[g for g in gs[i * n:(i + 1) * n] if g is not None] for i in range(k)]
        todo = [i for i, g in enumerate(groups) if 2 <= len(g) <= 3 and all(t.is_cuda and t.dtype == torch.float32 for t in g)]
        res = {}
        if todo:
            gc = {i: [t.contiguous() for t in groups[i]] for i in todo}
            outs = [torch.empty_like(gc[i][0]) for i in todo]
            m = len(todo)
            arr = lambda vals: (ctypes.c_void_p * m)(*vals)
            a, b = arr([H.P(gc[i][0]) for i in todo]), arr([H.P(gc[i][1]) for i in todo])
            c = arr([H.P(gc[i][2]) if len(gc[i]) == 3 else None for i in todo])
            o = arr([H.P(r) for r in outs])
            cnt = (ctypes.c_long * m)(*[gc[i][0].numel() for i in todo])
            H.call("vx_add_many", ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c), ctypes.addressof(o), ctypes.addressof(cnt), m, H.stream_ptr())
            res = dict(zip(todo, outs))
        for i, g in enumerate(groups):
            if i in res:
                out.append(res[i])
            elif not g:
                out.append(None)
            else:
                acc = g[0]
                for h in g[1:]:
                    acc = acc + h
                out.append(acc)
        return (None, *out)


def fan_out(xs, n):
    """[x0, x1, ...] -> [[n aliases of x0], [n aliases of x1], ...] whose gradients meet in one launch (training, CUDA tensors that require grad); else n references"""
    xs = list(xs)
    if not (n >= 2 and xs and torch.is_grad_enabled() and all(x.is_cuda and x.requires_grad for x in xs)):
        return [[x] * n for x in xs]
    al = _FanOutFn.apply(n, *xs)
    return [list(al[i * n:(i + 1) * n]) for i in range(len(xs))]


def patch_merge_all(xs, downs):
    """PatchMerging of every modality in one launch (attention_utils.py:127-168): 8-way gather -> LN(8C) -> 1x1 (8C -> 2C, no bias)"""
    M = len(xs)
    args = list(xs)
    for m in range(M):
        args += [downs[m].norm.weight, downs[m].norm.bias, downs[m].reduction.weight, None]
    return list(_LnPwFn.apply(M, 1, True, LN_EPS, *args))


class _PwaPostFn(torch.autograd.Function):
    """For every modality: y = alpha x + Drop(Wm s + bm); out = y + Drop(W2 Drop(GELU(W1 LN(y) + b1)) + b2)  -- one launch (PWA.py:377,433-439)"""

    @staticmethod
    def forward(ctx, M, alpha, p_mix, p_ffn, sites, *args):
        ss = [_c(t) for t in args[:M]]
        xs = [_c(t) for t in args[M:2 * M]]
        _check(ss[0], "pwa_post")
        prm = [list(args[2 * M + 8 * m: 2 * M + 8 * (m + 1)]) for m in range(M)]      # wm, bm, gamma, beta, w1, b1, w2, b2
        B, Cv = ss[0].shape[:2]
        C = xs[0].shape[1]
        R = prm[0][4].shape[0]
        V = ss[0][0, 0].numel()
        dev = ss[0].device
        ys = [torch.empty_like(x) for x in xs]
        outs = [torch.empty_like(x) for x in xs]
        rs = rng_state(dev) if (p_mix > 0 or p_ffn > 0) else None
        vals = []
        for m in range(M):
            vals += [H.P(ss[m]), H.P(xs[m])] + [H.P(t) for t in prm[m]] + [H.P(ys[m]), H.P(outs[m])] + [None] * 9 + [int(sites[3 * m]), int(sites[3 * m + 1]), int(sites[3 * m + 2])]
        arr = _ptrs(vals)
        H.call("vx_pwa_post_fwd", H.ctypes.addressof(arr), M, B, C, Cv, R, V, LN_EPS, float(alpha), H.P(rs, torch.int64), float(p_mix), float(p_ffn), H.stream_ptr())
        ctx.save_for_backward(*ss, *ys)
        ctx.prm, ctx.geo, ctx.rs, ctx.sites = prm, (M, float(alpha), float(p_mix), float(p_ffn), B, C, Cv, R, V), rs, tuple(sites)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *douts):
        M, alpha, p_mix, p_ffn, B, C, Cv, R, V = ctx.geo
        ss, ys = ctx.saved_tensors[:M], ctx.saved_tensors[M:]
        prm, sites = ctx.prm, ctx.sites
        dev = ss[0].device
        rows = H.query("vx_pwa_post_tiles", B, V)
        dsl, dxl, parts, scr = [], [], [], []
        vals = []
        for m in range(M):
            do = _c(douts[m]) if douts[m] is not None else torch.zeros_like(ys[m])
            ds_, dx_ = torch.empty_like(ss[m]), torch.empty_like(ys[m])
            part = torch.empty((rows, 2 * C), device=dev, dtype=torch.float32)
            sc = [torch.empty_like(ys[m]), torch.empty((B, R, V), device=dev, dtype=torch.float32), torch.empty((B, R, V), device=dev, dtype=torch.float32),
                  torch.empty_like(ys[m]), torch.empty_like(ys[m])]          # n, h, da, dz, dmix
            dsl.append(ds_); dxl.append(dx_); parts.append(part); scr.append(sc)
            vals += [H.P(ss[m]), None] + [H.P(t) for t in prm[m]] + [H.P(ys[m]), None, H.P(do), H.P(ds_), H.P(dx_), H.P(part)] + [H.P(t) for t in sc] + \
                    [int(sites[3 * m]), int(sites[3 * m + 1]), int(sites[3 * m + 2])]
        arr = _ptrs(vals)
        H.call("vx_pwa_post_bwd", H.ctypes.addressof(arr), M, B, C, Cv, R, V, LN_EPS, alpha, H.P(ctx.rs, torch.int64), p_mix, p_ffn, H.stream_ptr())
        jobs, folds = [], []
        for m in range(M):
            wm, bm, gam, bet, w1, b1, w2, b2 = prm[m]
            n_, h_, da_, dz_, dmix_ = scr[m]
            if w1.requires_grad:
                jobs.append((n_, da_, grad_buf(w1), _gb(b1), C, R, V, B))
            if w2.requires_grad:
                jobs.append((h_, dz_, grad_buf(w2), _gb(b2), R, C, V, B))
            if wm.requires_grad:
                jobs.append((ss[m], dmix_, grad_buf(wm), _gb(bm), Cv, C, V, B))
            if gam.requires_grad:
                folds.append((parts[m], grad_buf(gam), grad_buf(bet), C, rows))
        _submit_wgrad_jobs(jobs, folds)
        return (None, None, None, None, None) + tuple(dsl) + tuple(dxl) + (None,) * (8 * M)


def pwa_post_ok(C, Cv, R, V):
    return bool(H.query("vx_pwa_post_ok", int(C), int(Cv), int(R), int(V)))


def pwa_post(ss, xs, mixes, norms, ffns, alpha, p_mix, p_ffn, sites_mix):
    M = len(ss)
    args = list(ss) + list(xs)
    sites = []
    for m in range(M):
        args += [mixes[m].weight, mixes[m].bias, norms[m].weight, norms[m].bias, ffns[m].linear1.weight, ffns[m].linear1.bias, ffns[m].linear2.weight, ffns[m].linear2.bias]
        sites += [int(sites_mix[m]), int(ffns[m].site1), int(ffns[m].site2)]
    return list(_PwaPostFn.apply(M, float(alpha), float(p_mix), float(p_ffn), tuple(sites), *args))


def space_to_depth2(x):
    return _ops().space_to_depth2(x)


# ------------------------------------------------------------------------------------------------
# Paired-Window Attention core: gather -> attention -> scatter for all modalities
# ------------------------------------------------------------------------------------------------
def pwa_core(table, plan, cq, cv, qkv: Sequence[torch.Tensor], p_attn: float = 0.0, site: int = 0) -> List[torch.Tensor]:
    """gather -> attention -> scatter for all M = len(qkv) / 3 modalities as one autograd node; M <= 4 (more raises)"""
    return list(cpp_module().pwa_core(table, H.ctypes.addressof(plan), int(cq), int(cv), float(p_attn), int(site), rs_ptr(qkv[0].device, p_attn), list(qkv)))


# ------------------------------------------------------------------------------------------------
# up-sampling, Gram
# ------------------------------------------------------------------------------------------------
def upsample_trilinear(x, size):
    size = tuple(int(s) for s in size)
    if tuple(x.shape[2:]) == size:
        return x        # F.interpolate to the same size with align_corners=True is the identity (VeloxSeg.py:183)
    return _ops().upsample_trilinear(x, list(size))


def gram(x):
    return _ops().gram(x)


# ------------------------------------------------------------------------------------------------
# loss
# ------------------------------------------------------------------------------------------------
_LAB_KIND = {torch.int64: 0, torch.int32: 1, torch.uint8: 2}
_weight_cache = {}


def _head_weights(ws, device):
    key = (tuple(float(w) for w in ws), str(device))
    if key not in _weight_cache:
        _weight_cache[key] = torch.tensor(key[0], dtype=torch.float32, device=device)
    return _weight_cache[key]


class StagedLoss:
    """The VeloxSeg loss (utils/loss.py:52-66) taken apart for the staged training step (engine.TrainEngine): the accumulators, `finalize` and
    coefficients of the fused loss node (csrc/_vxops.cpp LossFn), but every decoder branch runs ITS part on its own stream -- the Seg branch the deep-supervision CE + Dice sums and, later, their gradients; each
    reconstruction branch its sum of squares against its channels of the input and, later, its MSE gradient -- and only the one-wave `finalize`
    (scalar loss, Dice coefficients, Gram term) sits between the forward and the backward fans.  Same arithmetic, same accumulators, same
    coefficients as the fused node; nothing here is differentiated by autograd (the gradients are handed to autograd.backward)."""

    def __init__(self, head_weights, w_rc, w_f, num_modal):
        self.head_weights, self.w_rc, self.w_f, self.M = tuple(float(w) for w in head_weights), float(w_rc), float(w_f), int(num_modal)
        self.nh = len(self.head_weights)
        self._drc, self.n_rc_expected = {}, None

    def begin(self, dev, B, C):
        """fresh accumulators (zero-filled here, i.e. before the forward fan: the branches only add)"""
        self.B, self.C = B, C
        self.seg_acc = torch.empty((self.nh * (1 + B * C * 3),), device=dev, dtype=torch.float64)      # (zeroed by the Seg branch's forward entry)
        self.rc_acc = torch.zeros((1,), device=dev, dtype=torch.float64)
        self.n_rc = 0
        self.ds = None
        self._drc, self.n_rc_expected = {}, None          # (a pass hands out only the MSE gradients its own rc_forward formed)

    def seg_forward(self, logits, labels):
        logits = [_c(t) for t in logits]
        h16 = logits[0].dtype == torch.bfloat16          # bf16 storage mode: head 0 (the full-resolution logits) is a bfloat16 tensor; the low-resolution heads stay fp32
        if not h16:
            _check(logits[0], "loss")
        nh, B, C = self.nh, self.B, self.C
        assert len(logits) == nh and logits[0].shape[0] == B and logits[0].shape[1] == C
        if labels.dtype not in _LAB_KIND:
            raise RuntimeError(f"labels must be int64/int32/uint8, got {labels.dtype}")
        labels = _c(labels)
        V = logits[0][0, 0].numel()
        st = H.stream_ptr()
        lp = [H.P(logits[0], None)] + [H.P(t) for t in logits[1:]] + [None] * (4 - nh)
        if any(tuple(t.shape[2:]) != tuple(logits[0].shape[2:]) for t in logits[1:]):
            D_, H_, W_ = (int(v) for v in logits[0].shape[2:])
            if not H.query("vx_seg_loss_ds_ok", C, D_, H_, W_):
                raise RuntimeError("veloxseg_loss: deep-supervision heads on coarser grids need C in 2..4 and W % 4 == 0 with W/4 dividing 64; up-sample them first")
            dims = (H.ctypes.c_int * (3 * max(nh - 1, 1)))(*[int(v) for t in logits[1:] for v in t.shape[2:]])
            self.ds = (dims, D_, H_, W_)
            H.call("vx_seg_loss_ds_fwd_h", *lp, H.ctypes.addressof(dims), nh, H.P(labels, None), _LAB_KIND[labels.dtype], H.P(self.seg_acc, torch.float64), B, C, D_, H_, W_, int(h16), st)
        else:
            if h16:
                raise RuntimeError("staged loss: a bfloat16 head 0 needs the fused deep-supervision kernels (heads 1.. on their own grids)")
            H.call("vx_seg_loss_fwd", *lp, nh, H.P(labels, None), _LAB_KIND[labels.dtype], H.P(self.seg_acc, torch.float64), B, C, V, st)
        self.logits, self.labels, self.V = logits, labels, V

    @staticmethod
    def _slice(x, ch_off, ch_n):
        """(pointer, floats between samples) of channels [ch_off, ch_off + ch_n) of the contiguous (B, Cx, ...) input"""
        Vx = x[0, 0].numel()
        return x.data_ptr() + 4 * ch_off * Vx, x.shape[1] * Vx, ch_n * Vx

    def rc_forward(self, rc, x, ch_off):
        """this branch's sum of squares against its channels of the input AND -- the coefficient 2 w_rc / N_rc is known already: the reconstructions cover the input, so
        N_rc = x.numel() (checked in finalize) -- its MSE gradient, in one pass (vx_sqdiff_sum_grad_bs); rc_backward hands the stored gradient out.
        A bfloat16 reconstruction (bf16 storage mode) gets a bfloat16 gradient; the sum of squares is formed in fp32 / fp64 either way."""
        rc = _c(rc)
        ptr, bstride, n = self._slice(x, ch_off, rc.shape[1])
        assert rc[0].numel() == n and x.is_contiguous()
        self.n_rc_expected = int(x.numel())
        scale = float(np.float32(2.0 * self.w_rc / float(self.n_rc_expected))) if self.w_rc != 0.0 else 0.0
        drc = torch.empty_like(rc)
        H.call("vx_sqdiff_sum_grad_bs_h", H.P(rc, None), ptr, n, bstride, rc.shape[0], H.P(self.rc_acc, torch.float64), scale, H.P(drc, None), int(rc.dtype == torch.bfloat16), H.stream_ptr())
        self._drc[int(ch_off)] = drc
        return rc

    def finalize(self, gram_seg, grams_rc, n_rc):
        """-> scalar loss (device tensor); keeps the coefficients and the Gram gradients for the backward fans"""
        dev = self.seg_acc.device
        nh, B, C, M = self.nh, self.B, self.C, self.M
        if self.n_rc_expected is not None and int(n_rc) != self.n_rc_expected:
            raise RuntimeError(f"staged loss: the reconstruction branches cover {int(n_rc)} elements, the input has {self.n_rc_expected}: the MSE gradient formed in the forward used the wrong 1 / N")
        st = H.stream_ptr()
        hw = _head_weights(self.head_weights, dev)
        self.coef = torch.empty((nh * (1 + B * C * 2) + 2,), device=dev, dtype=torch.float32)
        loss = torch.empty((1,), device=dev, dtype=torch.float32)
        gs = _c(gram_seg)
        gm = [_c(g) for g in grams_rc]
        gp = [H.P(g) for g in gm] + [None] * (4 - M)
        H.call("vx_loss_finalize", H.P(self.seg_acc, torch.float64), nh, B, C, self.V, H.P(hw), H.P(self.rc_acc, torch.float64), int(n_rc), self.w_rc,
               H.P(gs), *gp, M, gs.shape[1], self.w_f, H.P(loss), H.P(self.coef), st)
        stride = (1 + B * C * 2) * 4
        self.misc = self.coef.data_ptr() + nh * stride
        self.dgs = torch.empty_like(gs)
        self.dgm = [torch.empty_like(g) for g in gm]
        dp = [H.P(g) for g in self.dgm] + [None] * (4 - M)
        H.call("vx_gram_mse_bwd", H.P(gs), *gp, M, self.misc + 4, None, H.P(self.dgs), *dp, gs.numel(), st)
        return loss.view(())

    def seg_backward(self):
        nh, B, C = self.nh, self.B, self.C
        logits, labels = self.logits, self.labels
        h16 = logits[0].dtype == torch.bfloat16
        st = H.stream_ptr()
        stride = (1 + B * C * 2) * 4
        grads = [torch.empty_like(t) for t in logits]          # (head 0's gradient has head 0's dtype)
        lp = [H.P(logits[0], None)] + [H.P(t) for t in logits[1:]] + [None] * (4 - nh)
        gp = [H.P(grads[0], None)] + [H.P(d) for d in grads[1:]] + [None] * (4 - nh)
        if self.ds is not None:
            dims, D_, H_, W_ = self.ds
            nws = H.query("vx_seg_loss_ds_ws_floats", H.ctypes.addressof(dims), nh, B, C, D_)
            ws = torch.empty((max(nws, 1),), device=grads[0].device, dtype=torch.float32)
            H.call("vx_seg_loss_ds_bwd_h", *lp, H.ctypes.addressof(dims), nh, H.P(labels, None), _LAB_KIND[labels.dtype], self.coef.data_ptr(), stride // 4, None, *gp,
                   H.P(ws), B, C, D_, H_, W_, int(h16), st)
        else:
            H.call("vx_seg_loss_bwd4", *lp, nh, H.P(labels, None), _LAB_KIND[labels.dtype], self.coef.data_ptr(), stride // 4, None, *gp, B, C, self.V, st)
        return grads

    def rc_backward(self, rc, x, ch_off):
        drc = self._drc.get(int(ch_off))
        if drc is not None and drc.shape == rc.shape:
            return drc                                   # formed by rc_forward
        ptr, bstride, n = self._slice(x, ch_off, rc.shape[1])
        if rc.dtype != torch.float32:
            raise RuntimeError("staged loss: the gradient of a bfloat16 reconstruction is formed by rc_forward")
        drc = torch.empty_like(rc)
        H.call("vx_mse_bwd_bs", H.P(rc), ptr, n, bstride, rc.shape[0], self.misc, None, H.P(drc), H.stream_ptr())
        return drc


def veloxseg_loss(outputs: Sequence[torch.Tensor], labels: torch.Tensor, sr_labels: Optional[torch.Tensor], head_weights: Sequence[float],
                  w_rc: float, w_f: float, num_modal: int) -> torch.Tensor:
    """sum_h w_h (CE + Dice)(logits_h) + w_rc MSE(rcs, x) + w_f/M sum_m MSE(G_seg, G_m)   (utils/loss.py:52-66) as one autograd node.
    outputs = nh logits [+ rcs, G_seg, G_rc x M]; 1 <= nh <= 4 with one weight each (the node refuses anything else)."""
    return _ops().seg_loss(list(outputs), labels, sr_labels, [float(w) for w in head_weights], float(w_rc), float(w_f), int(num_modal))


def seg_only_loss(outputs: Sequence[torch.Tensor], labels: torch.Tensor, head_weights: Sequence[float]) -> torch.Tensor:
    return veloxseg_loss(outputs, labels, None, head_weights, 0.0, 0.0, 0)
