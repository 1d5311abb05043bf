"""The premise of tests/test_attn_fp64_gpu.py, proved without a GPU: every case of tests/attn_ref.py keeps the fp32 oracle inside the input
condition and `ref32` inside its own bound; the planted structure exists (sharp rows are sharp, the ramps put the row maximum in the last / first 64-key slab); the
kernels' arithmetic restated in fp32 -- (a) the online soft-max over 64-key slabs with 1, 2 and 4 merged partial states, (b) the backward from the fp32 LSE,
(c) the same backward on two fp16 pieces per operand -- stays inside the bound of the path it restates; and three wrong forms do not: (d) no maximum subtraction,
(e) one fp16 piece per operand, (f) partial states merged without the rescale.  Loosening the bound until (e) passes makes this file fail."""
import math

import pytest
import torch

import attn_ref as A
import stable_ref as S

FWD, BWD = ("O", "LSE"), ("dQ", "dK", "dV", "dtable")
F16_PATHS = ("f16_aligned", "f16_ragged", "f16_m1")


def _ref(rid, family, p):
    r = A.ROW[rid]
    return (r["geo"], r["M"], r["B"], family, p)


# reference -> the f16-pipe backward paths that run on it
F16_OPS = {}
for _rid, _f, _p in A.CASES:
    if A.ROW[_rid]["path"] in F16_PATHS:
        F16_OPS.setdefault(_ref(_rid, _f, _p), set()).add("attn_bwd_" + A.ROW[_rid]["path"])
F16_REFS = sorted(F16_OPS)
F16_IDS = [A.REF_IDS[A.REFS.index(r)] for r in F16_REFS]
RAMPS = [r for r in A.REFS if r[3] in ("ramp_up", "ramp_down")]
OVERFLOW = [r for r in A.REFS if r[3] in ("one_hot", "offset")]


def _ids(refs):
    return [A.REF_IDS[A.REFS.index(r)] for r in refs]


def _misses(got, c, names, op=None):
    return [m for m in (A.violation(got[n], c["r64"][n], c["r32"][n], n, op) for n in names) if m]


@pytest.mark.parametrize("ref", A.REFS, ids=A.REF_IDS)
def test_case_keeps_the_input_condition_and_fp32_oracle_passes_its_bound(ref):
    c = A.case(*ref)
    assert set(c["r64"]) == set(c["r32"]) == set(A.NAMES)
    for name in A.NAMES:
        r64, r32 = c["r64"][name], c["r32"][name]
        assert r64.dtype == torch.float64 and r32.dtype == torch.float32
        assert bool(torch.isfinite(r64).all()) and bool(torch.isfinite(r32).all()), f"{ref} {name}: the oracle is not finite"
        ok, rel = A.condition(r64, r32)
        assert ok, f"{ref} {name}: max|ref32-ref64| / M = {rel:.3e} breaks the cap {S.CAP:g}"
        S.check(r32, r64, r32, f"{ref} {name} (ref32 as got)")


@pytest.mark.parametrize("ref", A.REFS, ids=A.REF_IDS)
def test_the_oracle_restates_window_attention(ref):
    """same numbers as oracle.window_attention + oracle.relative_bias (with the restated Philox mask under dropout), bit for bit in double"""
    c = A.case(*ref)
    d, inp, p = c["d"], c["inp"], ref[4]
    bias = A.O.relative_bias(inp["table"].double(), A.O.relative_position_index(d["n"]), d["l"])
    masks = dict(seed=A.SEED, step=A.STEP, sites={"k": A.SITE}) if p > 0 else None
    want = A.O.window_attention(inp["q"].double(), inp["k"].double(), inp["v"].double(), bias, d["M"], p, p > 0, masks, "k")
    assert torch.equal(want, c["r64"]["O"])


@pytest.mark.parametrize("ref", A.REFS, ids=A.REF_IDS)
def test_fp32_restatements_of_the_forward_and_backward_pass_the_bound(ref):
    """(a) at 1, 2 and 4 partial states, with libm's exp and with the device's exp2(x log2 e); (b) fed by (a), as the library feeds its backward"""
    c = A.case(*ref)
    d, inp, keep = c["d"], c["inp"], c["keep"]
    bad = []
    for exp in (torch.exp, A.exp_fast):
        for splits in (1, 2, 4):
            fwd = A.forward_online(inp, d, splits, keep, exp=exp)
            bad += [f"(a) {splits} states, {exp.__name__}: {m}" for m in _misses(fwd, c, FWD)]
        fwd = A.forward_online(inp, d, 1, keep, exp=exp)
        bad += [f"(b) {exp.__name__}: {m}" for m in _misses(A.backward_restated(inp, d, fwd, keep, exp=exp), c, BWD)]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("ref", F16_REFS, ids=F16_IDS)
def test_two_fp16_pieces_pass_the_bound_of_their_path_and_one_piece_misses_it(ref):
    """(c) inside the bound at the factor tests/stable_ref.py grants the f16-pipe paths; (e) outside it on EVERY family: a factor wide enough for one piece fails here"""
    c = A.case(*ref)
    d, inp, keep = c["d"], c["inp"], c["keep"]
    fwd = A.forward_online(inp, d, 1, keep)
    two, one = A.backward_restated(inp, d, fwd, keep, 2), A.backward_restated(inp, d, fwd, keep, 1)
    for op in sorted(F16_OPS[ref]):
        bad = _misses(two, c, BWD, op)
        assert not bad, f"(c) {op}:\n" + "\n".join(bad)
        assert _misses(one, c, BWD, op), f"(e) {op}: one fp16 piece per operand passes the bound (factor {S.FACTORS.get(op, S.FACTOR):g})"


@pytest.mark.parametrize("ref", OVERFLOW, ids=_ids(OVERFLOW))
def test_exp_without_the_maximum_is_not_finite(ref):
    c = A.case(*ref)
    got = A.forward_no_max(c["inp"], c["d"])
    assert not bool(torch.isfinite(got["O"]).all()) and not bool(torch.isfinite(got["LSE"]).all()), f"(d) {ref}: exp(s) stays finite, the family does not reach overflow"


@pytest.mark.parametrize("ref", RAMPS, ids=_ids(RAMPS))
def test_ramps_plant_the_maximum_in_an_end_slab_and_a_merge_without_rescale_misses(ref):
    c = A.case(*ref)
    d, inp, keep = c["d"], c["inp"], c["keep"]
    top = A.scores(inp, d, torch.float64).argmax(-1) // A.SLAB
    last = (d["ML"] - 1) // A.SLAB
    assert bool((top == (last if ref[3] == "ramp_up" else 0)).all()), f"{ref}: a row maximum lies outside the {'last' if ref[3] == 'ramp_up' else 'first'} slab"
    for splits in (2, 4):
        got = A.forward_online(inp, d, splits, keep, rescale=False)
        if last == 0:                                                # one slab: nothing to merge, the form IS (a)
            assert not _misses(got, c, FWD)
        else:
            assert _misses(got, c, FWD), f"(f) {ref}: {splits} states merged without the rescale pass the bound"


def test_sharp_rows_are_sharp():
    """the median of the largest soft-max weight over the rows of a family: above 0.8 on `sharp`, above 0.999 on `one_hot`, flat on `plain`.  Per case `sharp` must
    give more than half of the rows more than half of their weight on ONE key; the pooled median is the one the thresholds are stated for (q x 10 gives logits of
    standard deviation 10 whatever the width, and the gap between the two largest of n draws narrows with n and with a heavier tail: 1024 keys of width 8 give 0.78,
    128 keys of width 2 give 0.71, 54 keys of width 4 give 0.89)"""
    pooled = {}
    for ref in A.REFS:
        if ref[3] in ("sharp", "one_hot", "plain") and not ref[4]:
            pm = A.p_max(A.case(*ref)).reshape(-1)
            med = float(pm.median())
            print(f"median p_max {A.REF_IDS[A.REFS.index(ref)]}: {med:.4f}")
            pooled.setdefault(ref[3], []).append(pm)
            if ref[3] == "sharp":
                assert med > 0.5, (ref, med)
            elif ref[3] == "one_hot":
                assert med > 0.999, (ref, med)
            else:
                assert med < 0.5, (ref, med)
    assert float(torch.cat(pooled["sharp"]).median()) > 0.8 and float(torch.cat(pooled["one_hot"]).median()) > 0.999
    assert float(torch.cat(pooled["plain"]).median()) < 0.2


def test_the_case_table_is_well_formed():
    assert len(set(A.CASE_IDS)) == len(A.CASES) and len({r["id"] for r in A.ROWS}) == len(A.ROWS)
    assert all(isinstance(r["branch"], str) and r["branch"] for r in A.ROWS)
    assert set(A.FAMILIES) == {"plain", "sharp", "one_hot", "bias_sharp", "offset", "ramp_up", "ramp_down", "tiny", "dO_big", "dO_small", "v_outlier", "q_outlier"}
    for r in A.ROWS:
        assert A.elements(r["geo"], r["M"], r["B"]) <= A.MAX_ELEMENTS, r["id"]
        assert set(r["knobs"]) <= set(A.KNOBS) and r["path"] in A.BWD_PATHS and r["fwd"] in A.FWD_PATHS
    paths = {r["path"] for r in A.ROWS}
    assert paths == set(A.BWD_PATHS) and {r["fwd"] for r in A.ROWS} == set(A.FWD_PATHS)
    for path in paths:
        rows = [r for r in A.ROWS if r["path"] == path]
        small = min(rows, key=lambda r: A.elements(r["geo"], r["M"], r["B"]) if set(r["families"]) == set(A.FAMILIES) else 1 << 62)
        assert set(small["families"]) == set(A.FAMILIES), f"{path}: no row runs every family"
        assert all(set(r["families"]) >= set(A.CORE) or not r["families"] for r in rows)
        assert any(set(r["drop"]) == {"plain", "sharp"} for r in rows), f"{path}: no dropout row"
        assert any(r["nofold"] for r in rows), f"{path}: no row runs vx_pwa_attn_bwd_nofold + fold"
    valu = [r for r in A.ROWS if r["path"] == "valu"]
    assert {(r["knobs"].get("fused_bwd", 1), r["knobs"].get("split", 0)) for r in valu} >= {(1, 0), (1, 1), (1, 2), (1, 4), (0, 0), (0, 1), (0, 2), (0, 4)}
    assert any(r["knobs"].get("valu_bits") == 1 and r["drop"] for r in valu)
    assert {A.dims(r["geo"], r["M"], r["B"])["l"] for r in valu} >= {27, 64, 216} and any(r["M"] == 3 for r in valu)
    assert {(A.dims(r["geo"], r["M"], r["B"])["cq"], A.dims(r["geo"], r["M"], r["B"])["cv"]) for r in valu} >= {(2, 4), (32, 32)}
    assert {A.dims(r["geo"], r["M"], r["B"])["l"] for r in A.ROWS if r["path"] == "f16_ragged"} == {27, 216, 32, 125}
    assert {A.dims(r["geo"], r["M"], r["B"])["l"] for r in A.ROWS if r["path"] == "f16_aligned"} == {64, 512}
    assert sum(1 for r in A.ROWS if r["path"] == "mfma1" and r["M"] == 1) == 2


def test_factors_are_granted_to_the_f16_pipe_paths_only():
    """the fp32 paths stay at FACTOR; a granted factor is a power of two (DESIGN.md section 36 carries the measured ratio beside each)"""
    attn = {k: v for k, v in S.FACTORS.items() if k.startswith("attn_")}
    assert set(attn) <= {"attn_bwd_" + p for p in F16_PATHS}
    assert all(v >= S.FACTOR and math.log2(v).is_integer() for v in attn.values())
    assert S.FACTOR == 8.0 and S.FLOOR == 16.0 * 2.0 ** -24 and S.CAP == 1e-4
