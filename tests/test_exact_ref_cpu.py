"""The premise of tests/test_exact_linear_gpu.py, proved on the CPU for EVERY row of the case table (tests/exact_ref.py CASES):
  - sum |x_i| |w_i| + |prefill| per output element -- the operation itself on the absolute values of the operands, in fp64 -- stays below 2^24, so every partial
    sum of every summation order is an integer (or a dyadic fraction of few bits) that fp32 holds exactly;
  - torch's own fp32 CPU result of the same operation equals the fp64 oracle, value for value.
The reference alone meets the condition the GPU test imposes on the kernels.  A row that fails here is a badly chosen row, not a kernel bug."""
import pytest
import torch

import exact_ref as E


def test_generators_are_seeded_small_integers():
    a, b = E.ints(4, 5, 6, seed=3), E.ints(4, 5, 6, seed=3)
    assert a.dtype == torch.float32 and torch.equal(a, b) and not torch.equal(a, E.ints(4, 5, 6, seed=4))
    assert torch.equal(a, a.round()) and float(a.min()) == -3.0 and float(a.max()) == 3.0
    p = E.prefill(1000, seed=1)
    assert torch.equal(p, p.round()) and float(p.min()) == -8.0 and float(p.max()) == 8.0


def test_comparison_is_by_value_and_reports_the_first_mismatch():
    ref = torch.tensor([0.0, 1.0, 2.0], dtype=torch.float64)
    assert E.mismatch(torch.tensor([-0.0, 1.0, 2.0]), ref, "x") is None
    m = E.mismatch(torch.tensor([0.0, float("nan"), 3.0]), ref, "x")
    assert "2 of 3" in m and "index 1" in m
    with pytest.raises(AssertionError):
        E.exact(torch.tensor([0.0, 1.0, 2.5]), ref, "x")


def test_table_ids_are_unique_and_every_family_has_a_batch_of_three():
    assert len(set(E.ROW_IDS)) == len(E.ROW_IDS)
    for fam in ("direct", "s1", "mfma", "stem", "gather", "down_wgrad", "jlc_gather", "gconv1", "pw", "upconv", "expand", "patchify", "patch_embed"):
        assert any(r.get("B") == 3 for r in E.rows(fam)), fam


@pytest.mark.parametrize("fam,row", E.ROWS, ids=E.ROW_IDS)
def test_row_is_exact_in_fp32(fam, row):
    ref = E.reference(fam, row)
    mag = E.magnitude(fam, row)
    f32 = E.operate(row, {n: v.float() for n, v in E.inputs(fam, row).items()})
    assert set(ref) == set(mag) == set(f32)
    for name, r in ref.items():
        assert r.dtype == torch.float64 and f32[name].dtype == torch.float32
        bound = float(mag[name].max()) + 8.0                      # (+ the largest prefill of a `+=` destination)
        assert bound < E.LIMIT, f"{fam}-{row['id']} {name}: sum |x||w| + |prefill| = {bound} reaches 2^24"
        assert bool((mag[name] >= r.abs()).all())
        E.exact(f32[name], r, f"{fam}-{row['id']} {name}: torch fp32 on the CPU against the fp64 oracle")
