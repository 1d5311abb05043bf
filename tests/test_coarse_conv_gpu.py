"""The coarse-level convolutions through the C ABI against fp64 oracles on integer-valued data (tests/coarse_conv_ref.py): vx_jlc_cl_fwd /
vx_jlc_cl_bwd (csrc/jlc_cl.hip: the operand ring and the single-read staging) and the k3 s2 path of vx_conv_mfma_fwd / vx_conv_mfma_bwd_data (csrc/conv_mfma.hip: two
register buffers, one (tap, channel step) stream).  Results are compared with `==`; only the sum-of-squares partials carry a tolerance (rtol 1e-6 against fp64).
Outputs start as NaN between canaries, so an element that is not written, or one written outside, fails.

The ring depth is a compile-time constant of the library (VX_CL_RING, 8): the width-8 cases have a K = 3 stream of 7 entries, shorter than the ring."""
import pytest
import torch

import coarse_conv_ref as R
from exact_ref import Guard, exact

pytestmark = pytest.mark.gpu


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


def _cl_setup(H, name):
    B, C, G, (D, Hh, W) = R.CL_CASES[name]
    assert R.cl_magnitude(name) < R.LIMIT          # (on the reference: every sum of the case is exact in fp32)
    assert H.query("vx_jlc_cl_ok", C, G, D, Hh, W) == 1
    t = {k: v.cuda() for k, v in R.cl_inputs(name).items()}
    img = torch.full((H.query("vx_jlc_cl_img_floats", C, G),), float("nan"), device="cuda")
    H.call("vx_jlc_cl_prep", H.P(t["w1"]), H.P(t["w3"]), H.P(t["w5"]), H.P(img), C, G, H.stream_ptr())
    return t, img


@pytest.mark.parametrize("name", sorted(R.CL_CASES))
def test_jlc_cl_fwd_returns_the_integers(name):
    H = _H()
    B, C, G, (D, Hh, W) = R.CL_CASES[name]
    t, img = _cl_setup(H, name)
    ref = R.cl_reference(name)
    nslot = H.query("vx_jlc_cl_ntiles", C, G, D, Hh, W)
    assert nslot == R.cl_slots(D * Hh * W)[0]
    ys = [Guard((B, C, D, Hh, W)) for _ in range(3)]
    part = Guard((3, B * C, nslot, 2), torch.float64)
    H.call("vx_jlc_cl_fwd", H.P(t["x"]), H.P(img), H.P(t["b1"]), H.P(t["b3"]), H.P(t["b5"]), ys[0].ptr, ys[1].ptr, ys[2].ptr, part.ptr, B, C, G, D, Hh, W, H.stream_ptr())
    torch.cuda.synchronize()
    for g, what in zip(ys + [part], ("y1", "y3", "y5", "part")):
        g.check(f"vx_jlc_cl_fwd {name} {what}")
    for g, k in zip(ys, (1, 3, 5)):
        exact(g.t, ref[f"y{k}"], f"vx_jlc_cl_fwd {name} y{k}")
    exact(part.t[..., 0], ref["part"][..., 0], f"vx_jlc_cl_fwd {name} per-slot sums")
    got, want = part.t[..., 1].cpu(), ref["part"][..., 1]
    assert bool(torch.isfinite(got).all())
    assert torch.allclose(got, want, rtol=1e-6, atol=0.0), f"sum-of-squares partials: {float(((got - want).abs() / want.abs().clamp_min(1.0)).max()):.3e}"


@pytest.mark.parametrize("name", sorted(R.CL_CASES))
def test_jlc_cl_bwd_returns_the_integers(name):
    H = _H()
    B, C, G, (D, Hh, W) = R.CL_CASES[name]
    t, img = _cl_setup(H, name)
    ref = R.cl_reference(name)
    dx = Guard((B, C, D, Hh, W))
    H.call("vx_jlc_cl_bwd", H.P(t["g1"]), H.P(t["g3"]), H.P(t["g5"]), H.P(img), H.P(t["d_o"]), dx.ptr, B, C, G, D, Hh, W, H.stream_ptr())
    dx0 = Guard((B, C, D, Hh, W))                  # d_o = NULL: the convolutions alone
    H.call("vx_jlc_cl_bwd", H.P(t["g1"]), H.P(t["g3"]), H.P(t["g5"]), H.P(img), None, dx0.ptr, B, C, G, D, Hh, W, H.stream_ptr())
    torch.cuda.synchronize()
    dx.check(f"vx_jlc_cl_bwd {name} dx")
    dx0.check(f"vx_jlc_cl_bwd {name} dx (no d_o)")
    exact(dx.t, ref["dx"], f"vx_jlc_cl_bwd {name} dx")
    exact(dx0.t, ref["dx"] - R.cl_inputs(name)["d_o"].double(), f"vx_jlc_cl_bwd {name} dx (no d_o)")


@pytest.mark.parametrize("name", sorted(R.CM_CASES))
def test_downconv_k3s2_fwd_and_input_gradient_return_the_integers(name):
    H = _H()
    B, Cin, Cout, (D, Hh, W) = R.CM_CASES[name]
    assert R.cm_magnitude(name) < R.LIMIT
    assert H.query("vx_conv_mfma_ok", Cin, Cout, D, Hh, W, 3, 2, 1, 1, 1) == 1
    t = {k: v.cuda() for k, v in R.cm_inputs(name).items()}
    ref = R.cm_reference(name)
    st = H.stream_ptr()
    y, wsf = Guard(tuple(ref["y"].shape)), Guard((H.query("vx_conv_mfma_ws_floats", Cin, Cout, 3, 0),))
    H.call("vx_conv_mfma_fwd", H.P(t["x"]), H.P(t["w"]), H.P(t["b"]), y.ptr, wsf.ptr, B, Cin, D, Hh, W, Cout, 3, 2, 1, st)
    nb = H.query("vx_conv_mfma_ws_floats", Cin, Cout, 3, 1)
    dx, wsb = Guard(tuple(ref["dx"].shape)), Guard((nb,))
    H.call("vx_conv_mfma_bwd_data", H.P(t["dy"]), H.P(t["w"]), dx.ptr, wsb.ptr, B, Cin, D, Hh, W, Cout, 3, 2, 1, 0, st)
    dxa, wsa = Guard(tuple(ref["dx"].shape), fill=t["dx0"]), Guard((nb,))
    H.call("vx_conv_mfma_bwd_data", H.P(t["dy"]), H.P(t["w"]), dxa.ptr, wsa.ptr, B, Cin, D, Hh, W, Cout, 3, 2, 1, 1, st)
    torch.cuda.synchronize()
    for g, what in ((y, "y"), (wsf, "forward workspace"), (dx, "dx"), (wsb, "workspace"), (dxa, "dx accumulate"), (wsa, "workspace (accumulate)")):
        g.check(f"vx_conv_mfma {name} {what}")
    exact(y.t, ref["y"], f"vx_conv_mfma_fwd {name}")
    exact(dx.t, ref["dx"], f"vx_conv_mfma_bwd_data {name} accumulate=0")
    exact(dxa.t, ref["dx_acc"], f"vx_conv_mfma_bwd_data {name} accumulate=1")
