"""The premise of tests/test_norm_loss_fp64_gpu.py, proved without a GPU: every row of tests/stable_ref.py keeps the fp32 oracle inside the
input condition (so the yardstick can never be loose enough to hide a kernel bug), the fp32 oracle passes its own bound, and the LayerNorm bound SEPARATES right
from wrong: two-sweep statistics pass on every row, the one-sweep pivot form fails wherever channel 0 is the outlier."""
import pytest
import torch

import stable_ref as S

ALL = [(op, r) for op in S.TABLES for r in S.rows(op)]
LN_WIDE = [r for r in S.LN_ROWS if r["family"] == "first_outlier" and r["shape"][1] >= 64]
LN_C16 = [r for r in S.LN_ROWS if r["family"] == "first_outlier" and r["shape"][1] == 16]


@pytest.mark.parametrize("op,row", ALL, ids=[f"{op}-{r['id']}" for op, r in ALL])
def test_row_keeps_the_input_condition_and_fp32_oracle_passes_its_bound(op, row):
    c = S.case(op, row)
    assert set(c["r64"]) == set(c["r32"]) and c["r64"]
    for name, r64 in c["r64"].items():
        r32 = c["r32"][name]
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{op} {row['id']} {name}: the oracle is not finite"
        ok, rel = S.condition(r64, r32)
        assert ok, f"{op} {row['id']} {name}: max|ref32-ref64| / M = {rel:.3e} breaks the cap {S.CAP:g}"
        S.check(r32, r64, r32, f"{op} {row['id']} {name} (ref32 as got)", op)


def test_bound_constants_and_zero_reference():
    assert S.FACTOR == 8.0 and S.FLOOR == 16.0 * 2.0 ** -24 and S.CAP == 1e-4
    assert all(f >= S.FACTOR for f in S.FACTORS.values()) and "layernorm" not in S.FACTORS
    z = torch.zeros(5, dtype=torch.float64)
    S.check(torch.zeros(5), z, torch.zeros(5), "exact zeros")
    assert S.violation(torch.full((5,), 1e-30), z, torch.zeros(5), "M == 0") is not None          # M == 0: the bound is 0
    assert S.violation(torch.tensor([float("nan")]), torch.ones(1, dtype=torch.float64), torch.ones(1), "nan") is not None
    r64 = torch.tensor([1.0, -2.0], dtype=torch.float64)
    r32 = torch.tensor([1.0 + 2e-7, -2.0])
    e32 = float((r32.double() - r64).abs().max())
    lim = 8 * e32 + S.FLOOR * 2.0
    assert S.violation((r64 + 0.99 * lim).float().double(), r64, r32, "inside") is None
    assert S.violation(r64 + 1.5 * lim, r64, r32, "outside") is not None


@pytest.mark.parametrize("row", S.LN_ROWS, ids=S.ids("layernorm"))
def test_layernorm_two_sweep_statistics_pass_the_bound(row):
    c = S.case("layernorm", row)
    B, C = row["shape"][:2]
    assert S.ln_path(B, C, c["tensors"][0][0, 0].numel()) == row["path"]
    got = S.ln_restated(c["tensors"][0], *c["params"], "two_sweep", row["path"])
    S.check(got, c["r64"]["out0"], c["r32"]["out0"], f"two-sweep {row['id']}", "layernorm")


@pytest.mark.parametrize("row", LN_WIDE + LN_C16, ids=[r["id"] for r in LN_WIDE + LN_C16])
def test_layernorm_pivot_statistics_fail_the_bound_when_channel_0_is_the_outlier(row):
    """guards the GPU test against being loosened: a bound the one-sweep pivot form passes would pass the kernel this suite was written to catch"""
    c = S.case("layernorm", row)
    got = S.ln_restated(c["tensors"][0], *c["params"], "pivot", row["path"])
    m = S.violation(got, c["r64"]["out0"], c["r32"]["out0"], f"pivot {row['id']}", "layernorm")
    assert m is not None, f"{row['id']}: the pivot form passes the bound"
    # ... and it is the algorithm, not the precision: the same form with the outlier in the LAST channel is at reference accuracy
    last = next(r for r in S.LN_ROWS if r["shape"] == row["shape"] and r["family"] == "last_outlier")
    cl = S.case("layernorm", last)
    S.check(S.ln_restated(cl["tensors"][0], *cl["params"], "pivot", last["path"]), cl["r64"]["out0"], cl["r32"]["out0"], f"pivot {last['id']}", "layernorm")


def test_tables_are_well_formed():
    for op in S.TABLES:
        rs = S.rows(op)
        assert rs and len({r["id"] for r in rs}) == len(rs), op
        assert all(isinstance(r.get("branch"), str) and r["branch"] for r in rs), op
    # InstanceNorm: every row length of the issue, the three variants, every family; B C = 6 with C = 3
    vol = {s["id"]: s["sp"][0] * s["sp"][1] * s["sp"][2] for s in S.IN_SHAPES}
    assert sorted(vol.values()) == [2, 255, 257, 1000, 2049, 4096, 4097, 4800, 8381, 8448]
    assert {s["sp"] for s in S.IN_SHAPES} >= {(1, 17, 241), (20, 20, 12), (17, 17, 29), (16, 16, 33)}
    assert S.IN_B * S.IN_C == 6 and S.IN_C == 3 and set(S.IN_VARIANTS) == {(1, False, False), (2, False, True), (3, True, True)}
    want = {s["id"]: (S.IN_V2_FAMILIES if s["id"] == "v2" else S.IN_FAMILIES) for s in S.IN_SHAPES}          # (two-element rows: see IN_V2_FAMILIES)
    assert {(r["shape"], r["n"], r["family"]) for r in S.IN_ROWS} == {(s, n, f) for s in vol for n in (1, 2, 3) for f in want[s]}
    assert set(S.IN_V2_FAMILIES) == {"plain", "offset", "scale_down", "constant"}
    assert set(S.IN_FAMILIES) >= {"plain", "offset", "scale_up", "scale_down", "constant", "spike"}
    # LayerNorm: the nine shapes on their three paths, all eight families
    assert {(s["shape"], s["path"]) for s in S.LN_SHAPES} == {((2, 16, 4, 6, 8), "thread"), ((1, 32, 5, 7, 9), "thread"), ((1, 64, 17, 32, 32), "thread"),
                                                              ((2, 128, 4, 4, 4), "lanes16"), ((2, 100, 2, 3, 3), "lanes16"), ((1, 64, 3, 5, 2), "lanes16"),
                                                              ((2, 1024, 2, 2, 2), "lanes64"), ((3, 256, 5, 7, 9), "lanes64"), ((1, 300, 3, 3, 3), "lanes64")}
    assert len(S.LN_FAMILIES) == 8 and len(S.LN_ROWS) == 72
    for s in S.LN_SHAPES:
        B, C, d, h, w = s["shape"]
        assert S.ln_path(B, C, d * h * w) == s["path"]
    # loss: every value of every axis
    L = S.LOSS_ROWS
    assert {r["C"] for r in L} == {2, 3, 4, 5, 8} and {r["nh"] for r in L} == {1, 4} and {r["lab"] for r in L} == {"int64", "int32", "uint8"}
    assert {r["vol"] for r in L} == {(8, 8, 8), (16, 16, 20), (5, 7, 9), (9, 15, 17)} and {r["M"] for r in L} == {0, 1, 2}
    assert {r["family"] for r in L} == set(S.LOSS_FAMILIES)
    for vol_ in ((8, 8, 8), (16, 16, 20), (5, 7, 9), (9, 15, 17)):                     # every volume with a vectorisable and a scalar-forward class count
        assert {r["C"] <= 4 for r in L if r["vol"] == vol_} == {True, False}
    for fam in ("empty_foreground_soft", "empty_foreground_bg12"):
        assert {r["vol"] for r in L if r["family"] == fam} & {(5, 7, 9), (9, 15, 17)} and {r["vol"] for r in L if r["family"] == fam} & {(8, 8, 8), (16, 16, 20)}
    D = S.DS_ROWS
    assert {r["family"] for r in D} == {"empty_foreground_bg12", "empty_foreground_soft", "confident_wrong", "common_offset"}
    assert {r["vol"] for r in D} == {(8, 8, 16), (16, 16, 32)} and {r["columns"] for r in D} == {0, 1} and S.DS_FACTORS == (2, 4, 8)
    for fam in ("confident_wrong", "common_offset"):
        assert {(r["vol"], r["columns"]) for r in D if r["family"] == fam} == {(v, c) for v in ((8, 8, 16), (16, 16, 32)) for c in (0, 1)}
    assert {r["vol"] for r in D if r["family"].startswith("empty_foreground")} == {(8, 8, 16), (16, 16, 32)}
    # Gram and up-sampling
    assert {(r["C"], r["sp"][0] * r["sp"][1] * r["sp"][2], r["scale"]) for r in S.GRAM_ROWS} == {(C, V, s) for C, V in ((16, 1024), (17, 1029), (32, 2048), (31, 125), (8, 4100))
                                                                                                 for s in (1.0, 1e3)}
    assert {(r["lo"], r["hi"]) for r in S.UP_ROWS} == {((4, 6, 3), (16, 24, 12)), ((2, 2, 2), (32, 32, 32)), ((3, 5, 7), (7, 11, 13))}


def test_families_are_what_they_say():
    x = S.family_rows("constant", 7, 300, 5, 0.0)
    assert bool((x == x[:, :1]).all()) and float(x.float().sum(1).sub(300 * x[:, 0]).abs().max()) == 0.0
    x = S.family_rows("scale_down", 4, 1000, 5, 0.0)
    assert float(x.double().var(1, unbiased=False).max()) < S.LN_EPS < S.IN_EPS
    x = S.family_rows("spike", 6, 50, 5, 0.0)
    assert bool(((x == 1e4).sum(1) == 1).all())
    x = S.family_rows("offset", 6, 4096, 5, S.IN_OFFSET, 1.0)
    assert 900 < float((x.double().mean(1) / x.double().std(1)).min())
    lab, lg = S.loss_labels_logits("empty_foreground_bg12", 2, 3, (4, 4, 4), 1, 3)
    assert int(lab[0].max()) == 0 and int(lab[1].max()) > 0 and float(lg[0][0, 0].mean()) > 11
    lab, _ = S.loss_labels_logits("absent_class", 2, 4, (4, 4, 4), 1, 3)
    assert 3 not in lab.unique().tolist() and {1, 2} <= set(lab.unique().tolist())
    lab, _ = S.loss_labels_logits("all_foreground", 2, 3, (4, 4, 4), 1, 3)
    assert int(lab.min()) == 1
    lab, lg = S.loss_labels_logits("confident_wrong", 2, 3, (4, 4, 4), 1, 3)
    assert int((lg[0].argmax(1, keepdim=True) != lab).sum()) >= lab.numel() // 7
