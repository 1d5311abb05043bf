#!/usr/bin/env python3
"""Time the 32^3-level streaming entries and the loss join alone at their bench shapes (autopet128, B = 4, fp32): 20 back-to-back launches of
each C-ABI entry, microseconds per launch.  vx_in_fwd_split / vx_in_bwd_split are two kernels per call (partial sums + apply), vx_gram_fwd is a memset + a kernel."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import veloxseg_amd  # noqa
import torch
from veloxseg_amd import _hip as H

dev = torch.device("cuda")
f64 = torch.float64


def timed(name, f, reps=20):
    for _ in range(3): f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps): f()
    e1.record(); torch.cuda.synchronize()
    print(f"{name}: {e0.elapsed_time(e1) / reps * 1e3:.1f} us", flush=True)


def instnorm(B=4, C=16, V=32768, nk=2, act=1):
    BC = B * C
    ys = [torch.randn(BC, V, device=dev) for _ in range(nk)]
    res, dout, out = torch.randn(BC, V, device=dev), torch.randn(BC, V, device=dev), torch.empty(BC, V, device=dev)
    stats = [torch.empty(BC * 2, device=dev) for _ in range(nk)]
    grads = [torch.empty(BC, V, device=dev) for _ in range(nk)]
    part = torch.empty(nk * BC * 32, device=dev, dtype=f64)
    pad = [None] * (3 - nk)
    st = H.stream_ptr()
    yp, sp, gp = [H.P(y) for y in ys] + pad, [H.P(s) for s in stats] + pad, [H.P(g) for g in grads] + pad
    timed(f"vx_in_fwd_split BC={BC} V={V} nk={nk} act={act} res", lambda: H.call("vx_in_fwd_split", *yp, *sp, H.P(part, f64), nk, act, H.P(res), H.P(out), BC, V, 1e-5, st))
    timed(f"vx_in_bwd_split BC={BC} V={V} nk={nk} act={act}", lambda: H.call("vx_in_bwd_split", H.P(dout), *yp, *sp, H.P(part, f64), nk, act, *gp, None, BC, V, st))


def gram(B=4, C=16, V=32768):
    x, dG = torch.randn(B, C, V, device=dev), torch.randn(B, C, C, device=dev)
    G, dx = torch.empty(B, C, C, device=dev), torch.empty(B, C, V, device=dev)
    st = H.stream_ptr()
    timed(f"vx_gram_fwd B={B} C={C} V={V}", lambda: H.call("vx_gram_fwd", H.P(x), H.P(G), B, C, V, st))
    timed(f"vx_gram_bwd B={B} C={C} V={V}", lambda: H.call("vx_gram_bwd", H.P(x), H.P(dG), H.P(dx), B, C, V, st))


def patch_wgrad(B=4, M=2, Cout=16, Do=32):
    x = torch.randn(B, M, 4 * Do, 4 * Do, 4 * Do, device=dev)          # one modality (Cin = 1) of the M-channel input, read in place
    dy = torch.randn(B, Cout, Do, Do, Do, device=dev)
    dw, db = torch.zeros(Cout, 64, device=dev), torch.zeros(Cout, device=dev)
    st = H.stream_ptr()
    timed(f"vx_patch_embed_bwd_weight B={B} Cin=1 Cout={Cout} grid={Do}^3",
          lambda: H.call("vx_patch_embed_bwd_weight", x.data_ptr(), M * 64 * Do ** 3, H.P(dy), H.P(dw), H.P(db), B, 1, Cout, Do, Do, Do, st))


def finalize(nh=4, B=4, C=2, V=128 ** 3, M=2, Cg=16):
    acc = torch.rand(nh * (1 + B * C * 3), device=dev, dtype=f64) * V
    rc = torch.rand(1, device=dev, dtype=f64)
    hw = torch.tensor([1.0, 0.5, 0.25, 0.125][:nh], device=dev)
    gs = torch.randn(B, Cg, Cg, device=dev)
    gm = [torch.randn(B, Cg, Cg, device=dev) for _ in range(M)]
    coef, loss = torch.empty(nh * (1 + B * C * 2) + 2, device=dev), torch.empty(1, device=dev)
    st = H.stream_ptr()
    timed(f"vx_loss_finalize nh={nh} B={B} C={C} M={M} Cg={Cg}",
          lambda: H.call("vx_loss_finalize", H.P(acc, f64), nh, B, C, V, H.P(hw), H.P(rc, f64), B * M * V, 1.0, H.P(gs), *([H.P(g) for g in gm] + [None] * (4 - M)), M, Cg, 1.0,
                         H.P(loss), H.P(coef), st))


if __name__ == "__main__":
    instnorm()
    gram()
    patch_wgrad()
    finalize()
