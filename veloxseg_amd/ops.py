"""The hot-path operators as registered PyTorch custom ops: torch.ops.veloxseg.* (north_star: "re-registered as custom ops backed by hand-written
HIP kernels").  Each op is the operator of veloxseg_amd.functional under a dispatcher schema; the implementation is registered for
the Autograd / CUDA / Meta keys from C++ (csrc/_vxops.cpp) and for CompositeImplicitAutograd for the two dropout operators that fetch Python-side
state; autograd records the operator's own node (a C++ autograd function whose forward and backward launch the kernels of include/veloxseg_hip.h), and
a CPU tensor raises the library's "no CPU path" error -- there is no fallback kernel behind any key.

    torch.ops.veloxseg.conv3d(x, w, b, stride, padding, groups, pixel_shuffle)        nn.Conv3d (+ PixelShuffle), conv_blocks.py / Decoder.py
    torch.ops.veloxseg.conv_transpose_k2s2(x, w, b)                                   nn.ConvTranspose3d(k=2, s=2), conv_blocks.py:29-35
    torch.ops.veloxseg.instance_norm_sum(ys, act, res)                                sum_k [GELU](InstanceNorm3d(y_k)) [+ res]
    torch.ops.veloxseg.layer_norm_cf(x, gamma, beta)                                  channels-first LayerNorm, attention_utils.py:29-43
    torch.ops.veloxseg.gelu_dropout(a, p, site) / residual_dropout(x, z, alpha, p, site)
    torch.ops.veloxseg.space_to_depth2(x) / upsample_trilinear(x, size) / gram(x)
    torch.ops.veloxseg.pwa_attention(table, qkv, grid, n, heads, small, nwin, cq, cv, p_attn, site, rng_state=None)     PWA.py:106-200,308-327
    torch.ops.veloxseg.jlc_block(x, ws, bs, groups, l1w, l1b, l2w, l2b, p, site, rng_state=None)                         conv_blocks.py:41-75
    torch.ops.veloxseg.ffn_tail(y, gamma, beta, w1, b1, w2, b2, p, site1, site2, rng_state=None)                         attention_utils.py:45-71 (LN + FFN + residual)
    torch.ops.veloxseg.seg_loss(outputs, labels, sr_labels, head_weights, w_rc, w_f, num_modal)                          utils/loss.py:52-66

The modules of veloxseg_amd.model reach the seven generic operators THROUGH the dispatcher (functional.py routes conv3d, conv_transpose_k2s2, instance_norm_sum,
layer_norm_cf, space_to_depth2, upsample_trilinear and gram to torch.ops.veloxseg.*), and so does the eager loss (functional.veloxseg_loss / seg_only_loss call
seg_loss); the other composite operators are called as functions of veloxseg_amd.functional, which hand the same C++ nodes their Python-side state.
There is one host path per operator: the C++ autograd node behind these schemas."""
import torch

from . import functional as VF

# Eleven operators are DEFINED AND REGISTERED IN C++ (csrc/_vxops.cpp: TORCH_LIBRARY(veloxseg) with Autograd / CUDA / Meta keys and a CPU key that raises): the seven
# generic ones (conv3d, conv_transpose_k2s2, instance_norm_sum, layer_norm_cf, space_to_depth2, upsample_trilinear, gram) and the four north_star names --
# pwa_attention (the window plan as integer lists, the dropout site and the {seed, step} RNG-state tensor as arguments), jlc_block, ffn_tail, seg_loss.  Importing the
# extension registers them.  gelu_dropout / residual_dropout are Python bodies under CompositeImplicitAutograd (they fetch the RNG-state tensor themselves).
CPP_OPS = ("conv3d", "conv_transpose_k2s2", "instance_norm_sum", "layer_norm_cf", "space_to_depth2", "upsample_trilinear", "gram",
           "pwa_attention", "jlc_block", "ffn_tail", "seg_loss")
VF.cpp_module()          # (raises when the extension is not built)
_lib = torch.library.Library("veloxseg", "FRAGMENT")
for _schema, _fn in (("gelu_dropout(Tensor a, float p, int site) -> Tensor", lambda a, p, site: VF.gelu_dropout(a, p, site)),
                     ("residual_dropout(Tensor? x, Tensor z, float alpha, float p, int site) -> Tensor", lambda x, z, alpha, p, site: VF.residual_dropout(x, z, alpha, p, site))):
    _lib.define(_schema)
    _lib.impl(_schema.split("(")[0], _fn, "CompositeImplicitAutograd")

OPS = ("conv3d", "conv_transpose_k2s2", "instance_norm_sum", "layer_norm_cf", "gelu_dropout", "residual_dropout", "space_to_depth2", "upsample_trilinear", "gram",
       "pwa_attention", "seg_loss", "jlc_block", "ffn_tail")
