"""The premises of tests/coarse_conv_ref.py, proven on the CPU for every case the GPU tests run (tests/test_coarse_conv_gpu.py)."""
import pytest
import torch
import torch.nn.functional as F

import coarse_conv_ref as R


@pytest.mark.parametrize("name", sorted(R.CL_CASES))
def test_jlc_cases_are_exact_in_fp32_and_their_pieces_are_exact(name):
    B, C, G, sp = R.CL_CASES[name]
    assert R.cl_magnitude(name) < R.LIMIT
    t, ref = R.cl_inputs(name), R.cl_reference(name)
    V = sp[0] * sp[1] * sp[2]
    Cg = C // G
    assert Cg in (8, 16) and max(sp) <= 8
    # every staged (sample, group) volume has a maximum of 1 or 2: v * 2^e is then a multiple of 2^12 below 2^14, one fp16 piece holds it and the other is zero
    for key in ("x", "g1", "g3", "g5"):
        mx = t[key].abs().reshape(B, G, Cg * V).amax(2)
        assert bool(((mx == 1) | (mx == 2)).all()), key
    for k in (1, 3, 5):
        y32 = F.conv3d(t["x"], t[f"w{k}"], t[f"b{k}"], padding=k // 2, groups=G)
        assert bool((y32.double() == ref[f"y{k}"]).all())
        assert bool((ref[f"y{k}"] == ref[f"y{k}"].round()).all())
    # the slots partition the voxels: they fold to the statistics of the whole tensor
    nslot, tpw = R.cl_slots(V)
    assert ref["part"].shape == (3, B * C, nslot, 2) and 16 * tpw * nslot >= V
    for i, k in enumerate((1, 3, 5)):
        y = ref[f"y{k}"].reshape(B * C, V)
        assert bool((ref["part"][i, :, :, 0].sum(1) == y.sum(1)).all())
        assert bool((ref["part"][i, :, :, 1].sum(1) == (y * y).sum(1)).all())
    assert bool((ref["dx"] == ref["dx"].round()).all())


def test_jlc_cases_cover_the_paths_of_the_kernel():
    slots = {n: R.cl_slots(c[3][0] * c[3][1] * c[3][2]) for n, c in R.CL_CASES.items()}
    assert any(tpw == 2 for _, tpw in slots.values()) and any(tpw == 1 for _, tpw in slots.values())
    widths = {c[1] // c[2] for c in R.CL_CASES.values()}
    assert widths == {8, 16}
    # a wave without a tile, a ragged last tile, rows shorter than 4 voxels
    assert any((c[3][0] * c[3][1] * c[3][2] + 15) // 16 < 4 for c in R.CL_CASES.values())
    assert any((c[3][0] * c[3][1] * c[3][2]) % 16 for c in R.CL_CASES.values())
    assert any(c[3][2] < 4 for c in R.CL_CASES.values())


@pytest.mark.parametrize("name", sorted(R.CM_CASES))
def test_downconv_cases_are_exact_in_fp32(name):
    B, Cin, Cout, sp = R.CM_CASES[name]
    assert R.cm_magnitude(name) < R.LIMIT
    assert all(s % 2 == 0 for s in sp) and Cout % 4 == 0
    t, ref = R.cm_inputs(name), R.cm_reference(name)
    y32 = F.conv3d(t["x"], t["w"], t["b"], stride=2, padding=1)
    assert bool((y32.double() == ref["y"]).all())
    assert ref["dx"].shape == t["x"].shape
    # the transposed convolution is the adjoint of the forward: <conv(x), dy> == <x, conv^T(dy)> (integers: exactly)
    lhs = (F.conv3d(t["x"].double(), t["w"].double(), None, stride=2, padding=1) * t["dy"].double()).sum()
    assert float(lhs) == float((t["x"].double() * ref["dx"]).sum())
    assert bool((ref["dx_acc"] - ref["dx"] == t["dx0"].double()).all())


def test_downconv_cases_cover_the_group_tails():
    ks = {n: (c[1] * 27 + 3) // 4 for n, c in R.CM_CASES.items()}
    assert any(k % 8 for k in ks.values()) and any(k % 8 == 0 for k in ks.values())
    assert any((c[2] // 4) % 8 for c in R.CM_CASES.values())
