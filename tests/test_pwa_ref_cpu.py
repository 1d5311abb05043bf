"""The premises of tests/test_pwa_exact_gpu.py, proved on the CPU for EVERY row of the tables in tests/pwa_ref.py:
  A. aten's max_pool3d follows the scan rule `val > best or isnan(val)` -- values AND indices -- on every row and data kind, so the rule the kernels are held to is
     aten's and not a reading of it; every planted position exists;
  B. torch's fp32 oracle.scatter_windows and its autograd stay inside the derived bounds 12 u S and (12 + n) u S against the fp64 restatement; the kernel-selection
     column of the table is the predicate of csrc/pwa.hip;
  C. the exactly solvable attention regimes are what the table says: both kinds of query exist, the integer sums are exact in fp32, exp(-128) is 0 in fp32.
A row that fails here is a badly chosen row or a wrong oracle, not a kernel bug."""
import pytest
import torch

import pwa_ref as R
from oracle import veloxseg_oracle as O

G_IDS = [r["id"] for r in R.GATHER_ROWS]
S_IDS = [r["id"] for r in R.SCATTER_ROWS]
A_IDS = [r["id"] for r in R.ATTN_ROWS]


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ====================================================================================================================== A
@pytest.mark.parametrize("row", R.GATHER_ROWS, ids=G_IDS)
def test_gather_table_positions_exist(row):
    pl = R.make_plan(row)
    pooled = sorted({R._prod(s) for s in pl["small"] if R._prod(s) > 1})
    assert pooled and pooled == sorted(row["nan_at"]), "one entry per pooled cell size"
    for s in pl["small"]:
        csz = R._prod(s)
        if csz == 1:
            continue
        want = row["nan_at"][csz]
        assert want == R.nan_positions(csz) and all(0 <= p < csz for p in want) and len(set(want)) == len(want)
        assert {0, 1, csz - 1} <= set(want) and R.lanes(csz) - 1 in want
        assert R._prod([g // k for g, k in zip(row["grid"], s)]) >= max(R.GATHER_CELLS, len(want)), "a planting would fall outside the volume"


def test_gather_table_reaches_every_position_role_and_kernel():
    assert any(R.lanes(c) < c and R.lanes(c) in p for r in R.GATHER_ROWS for c, p in r["nan_at"].items()), "no row has a cell wider than its lanes (position T)"
    assert any(r["cq"] % 8 == 0 and r["cv"] % 8 == 0 for r in R.GATHER_ROWS) and any(r["cq"] % 8 and r["cq"] % 4 == 0 for r in R.GATHER_ROWS)      # <8> and <4>
    assert any(r["cq"] % 4 for r in R.GATHER_ROWS) and any(r["grid"][2] % 4 for r in R.GATHER_ROWS) and any(1 in R.make_plan(r)["n"] for r in R.GATHER_ROWS)
    assert len(set(G_IDS)) == len(G_IDS)


@pytest.mark.parametrize("kind", R.GATHER_KINDS)
@pytest.mark.parametrize("row", R.GATHER_ROWS, ids=G_IDS)
def test_aten_max_pool_follows_the_scan_rule(row, kind):
    pl = R.make_plan(row)
    for k, x in enumerate(R.gather_sources(row, kind)):
        c = row["cv"] if k % 3 == 2 else row["cq"]
        tok, idx = R.pool_aten(x, pl, c)
        tok2, idx2 = R.pool_aten(x, pl, c, pool=R.pool_scan)
        assert same_bits(tok, tok2), f"{kind}: values of tensor {k}"          # (NaNs included: both sides copy the input's NaN)
        assert torch.equal(idx, idx2), f"{kind}: indices of tensor {k}"
        if not bool(torch.isnan(x).any()):
            assert same_bits(tok, O.gather_windows(x, pl, c)), "the partition is oracle.gather_windows"
        # the saved index points at the token's value
        B = x.shape[0]
        ref = R.gather_bwd_reference(idx, tok, pl, c).view(B, -1)
        xv = x.reshape(B, -1)
        hit = R.gather_bwd_reference(idx, torch.ones_like(tok), pl, c).view(B, -1) == 1
        assert same_bits(ref[hit], xv[hit])


@pytest.mark.parametrize("row", R.GATHER_ROWS, ids=G_IDS)
def test_gather_kinds_show_what_they_are_for(row):
    pl = R.make_plan(row)
    off = R.woff(pl)
    first_pooled = next(i for i, s in enumerate(pl["small"]) if R._prod(s) > 1)
    ref = {kind: R.gather_reference(row, kind) for kind in R.GATHER_KINDS}
    for kind in ("ties", "zeros", "neg_inf", "randn"):
        assert not any(bool(torch.isnan(t).any()) for t, _ in ref[kind])
    t = ref["zeros"][0][0][:, :, off[first_pooled]:]
    assert bool(((t == 0) & torch.signbit(t)).any()) and bool(((t == 0) & ~torch.signbit(t)).any()), "both signs of zero must reach a token"
    assert bool((ref["neg_inf"][0][0] == -R.INF).any())
    for kind, per_scale in (("inf_nan", 2), ("two_nans", 2), ("all_nan", 1)):
        for (t, _), c in zip(ref[kind], (row["cq"], row["cq"], row["cv"])):
            pooled = sum(1 for s in pl["small"] if R._prod(s) > 1)
            assert int(torch.isnan(t).sum()) == per_scale * pooled * R.MAXB * row["heads"] * c * R.MAXM, kind
    want = sum(len(p) for s in pl["small"] for cz, p in row["nan_at"].items() if R._prod(s) == cz)
    assert int(torch.isnan(ref["nan_at"][0][0]).sum()) == want * R.MAXB * row["heads"] * row["cq"] * R.MAXM, "every single NaN must reach its token"
    assert not bool(torch.isinf(ref["inf_nan"][0][0]).any()), "a NaN beats +inf wherever it stands"
    d = R.gather_dtok(row)
    assert all(bool((g != 0).all()) and torch.equal(g, g.round()) and float(g.abs().max()) == 3 for g in d)


# ====================================================================================================================== B
@pytest.mark.parametrize("row", R.SCATTER_ROWS, ids=S_IDS)
def test_scatter_kernel_selection_column(row):
    pl, c = R.make_plan(row), row["c"]
    for B in (1, 2):
        assert [R.scatter_bwd_kind(pl, c, B, i) for i in range(pl["nb"])] == row["kinds"]
        assert [R.scatter_bwd_kind(pl, c, B, i, ident=0) for i in range(pl["nb"])] == [3] * pl["nb"]
        assert not R.scatter_w_declines(pl, c, B) and R.scatter_w_declines(pl, c, B, ident=0)
        assert R.scatter_one_launch(pl, c, B) and not R.scatter_one_launch(pl, c, B, ident=0)
    assert pl["nb"] <= 4 and max(max(s) for s in pl["small"]) <= 8


def test_scatter_table_reaches_every_kernel():
    kinds = {k for r in R.SCATTER_ROWS for k in r["kinds"]}
    assert kinds == {0, 1, 2}                                                  # (3, the general kernel: every scale of every row with the identity knob off)
    assert {r["M"] for r in R.SCATTER_ROWS} == {1, 2, 3}
    assert any(r["c"] % 4 for r in R.SCATTER_ROWS) and any(r["c"] % 4 == 0 for r in R.SCATTER_ROWS)
    assert len(set(S_IDS)) == len(S_IDS)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("row", R.SCATTER_ROWS, ids=S_IDS)
def test_fp32_scatter_oracle_is_inside_the_derived_bounds(row, B):
    ref = R.scatter_reference(row, B)
    pl, c = R.make_plan(row), row["c"]
    outs, dtok = R.scatter_operate(row, B)
    worst = 0.0
    for m in range(row["M"]):
        assert bool((ref["out_S"][m] >= ref["out"][m].abs()).all())
        ok, ratio, text = R.bound_report(outs[m], ref["out"][m], ref["out_S"][m], 12)
        assert ok, f"forward, modality {m}: {text}"
        worst = max(worst, ratio)
    assert bool((ref["dtok_S"] >= ref["dtok"].abs()).all()) and bool((ref["dtok_n"] >= 1).all()) and torch.equal(ref["dtok_n"], ref["dtok_n"].round())
    ok, ratio_a, text = R.bound_report(dtok, ref["dtok"], ref["dtok_S"], 12 + ref["dtok_n"])
    assert ok, f"adjoint: {text}"
    print(f"{row['id']} B={B}: torch fp32 forward err / (u S) <= {worst:.2f}, adjoint <= {ratio_a:.2f}; n up to {int(ref['dtok_n'].max())}")
    # the identity scale is a copy
    nI, l, hc = R.ident_windows(pl), R._prod(pl["n"]), row["heads"] * c
    tok, dout = R.scatter_inputs(row, B)
    for m in range(row["M"]):
        assert torch.equal(R.partition(ref["out"][m][:, :hc], pl, 0, c), tok[:, :, :nI, m * l:(m + 1) * l].double())


# ====================================================================================================================== C
def test_exp_of_the_off_bias_is_zero_in_fp32():
    x = torch.tensor(R.OFF_BIAS, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)          # exp(x) as exp2(x log2 e), in fp32
    assert float(torch.exp2(x)) == 0.0 and float(torch.exp(torch.tensor(R.OFF_BIAS, dtype=torch.float32))) == 0.0
    assert float(torch.exp2(torch.tensor(0.0) * torch.tensor(1.4426950408889634))) == 1.0


@pytest.mark.parametrize("row", R.ATTN_ROWS, ids=A_IDS)
def test_attention_regimes(row):
    pl, M, h = R.make_plan(row), row["M"], row["heads"]
    n, l = pl["n"], R._prod(pl["n"])
    V = R.attn_v(row).double()
    assert (pl["c_qk"], pl["c_v"]) in {(4, 4), (8, 8), (8, 16), (16, 16), (16, 32), (4, 8), (4, 16), (8, 32), (16, 64), (8, 64), (32, 32)}, "no kernel for these head widths"
    ref = R.attn_reference(row, "uniform")
    assert bool((ref["count"] == M * l).all()) and float(ref["S"].max()) < 2.0 ** 24
    assert torch.equal(ref["total"], V.sum(3, keepdim=True).expand_as(V)) and bool((ref["top"] == 0).all())
    seen = set()
    for bias in R.ATTN_BIASES[1:]:
        ref = R.attn_reference(row, bias)
        assert float(ref["S"].max()) < 2.0 ** 24
        for a in range(h):
            roff = R.attn_head_offset(n, a, bias)
            seen.add(roff)
            inw, tgt = R.attn_targets(n, roff)
            inw_q, tgt_q = inw.repeat(M), tgt.repeat(M)
            assert torch.equal(ref["count"][a], torch.where(inw_q, torch.tensor(float(M), dtype=torch.float64), torch.tensor(float(M * l), dtype=torch.float64)))
            if any(roff):
                assert bool(inw.any()) and bool((~inw).any()), f"offset {roff}: queries of both kinds"
            else:
                assert bool(inw.all())
            # a query whose target lies in its window returns the mean over the modalities of V[m, t + r]; the others the window mean
            Vm = V[:, a].view(V.shape[0], V.shape[2], M, l, -1)
            want_in = Vm[:, :, :, tgt[inw]].sum(2)
            got = ref["total"][:, a].view(V.shape[0], V.shape[2], M, l, -1)          # (the sums are integers: exact; O = total / count)
            for m in range(M):
                assert torch.equal(got[:, :, m][:, :, inw], want_in)
                if bool((~inw).any()):
                    assert torch.equal(got[:, :, m][:, :, ~inw], Vm.sum((2, 3))[:, :, None].expand(-1, -1, int((~inw).sum()), -1))
            assert torch.equal(ref["top"][a], torch.where(inw_q, torch.tensor(0.0, dtype=torch.float64), torch.tensor(R.OFF_BIAS, dtype=torch.float64)))
    assert seen == set(R.attn_offsets(n)), "every offset on some head"


def test_attention_table_reaches_both_divisor_kinds():
    ls = {(R._prod(R.make_plan(r)["n"]), r["M"]) for r in R.ATTN_ROWS}
    assert {8, 27, 32, 64, 216} == {l for l, _ in ls} and {1, 2, 3} == {M for _, M in ls}
    p2 = [bool(R.attn_reference(r, "uniform")["pow2"].all()) for r in R.ATTN_ROWS]
    assert any(p2) and not all(p2)
