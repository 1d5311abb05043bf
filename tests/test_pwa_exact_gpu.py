"""The paired-window attention path of csrc/pwa.hip against exact and derived-bound oracles, straight through the C ABI (tables, inputs and
references: tests/pwa_ref.py; their premises: tests/test_pwa_ref_cpu.py).

  A. gather (max-pool + window partition): tokens, saved arg-max indices and the routed gradient, BIT FOR BIT against F.max_pool3d(return_indices=True) on the CPU:
     ties, signed zeros, all -inf cells, +inf with NaN, a single NaN at the first / last load of lane 0 and of the other lanes, two NaNs, an all-NaN cell.
  B. scatter and its adjoints against fp64, per element: |err| <= 12 u S forward, (12 + n) u S adjoint, S = sum |w| |t| from the same operator on absolute values,
     n = the number of accumulated terms; exactly 0 where S = 0; the identity scale is a copy and compared as bits.
  C. attention forward with q = k = 0 and a bias table that is uniform or one-hot (0 / -128): value for value where the divisor is a power of two, 2 u |ref| elsewhere.

Every destination and workspace is an exact_ref.Guard: `=` outputs start as NaN, index tensors as -1, `+=` destinations as integers in [-8, 8] that the reference
adds; a declined call (return value 1) must leave its prefill untouched; `*_set_*` knobs are restored in `finally`."""
import contextlib
import ctypes

import pytest
import torch

import exact_ref as E
import pwa_ref as R
from exact_ref import Guard

pytestmark = pytest.mark.gpu

U = R.U
LSE_ATOL, LSE_RTOL = 3e-5, 3e-4          # the tolerance of test_pwa_core (tests/test_hip_ops_gpu.py)
IDX_CANARY = 0x5A5A5A


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


@contextlib.contextmanager
def knob(H, name, value, default):
    H.call(name, value)
    try:
        yield
    finally:
        H.call(name, default)


class Run:
    """the guards and device operands of one test; done() synchronises and checks every canary"""

    def __init__(self, H, row):
        self.H, self.guards, self.keep, self.seed = H, [], [], R._seed(row["id"], 900)
        self.pl = R.make_plan(row)
        self.plan = H.make_plan(row["grid"], self.pl["n"], row["heads"], self.pl["small"], self.pl["nwin"])
        self.pp, self.st = ctypes.addressof(self.plan), H.stream_ptr()

    def out(self, shape, dtype=torch.float32):
        g = Guard(tuple(shape), dtype, fill=-1, canary=IDX_CANARY) if dtype == torch.int32 else Guard(tuple(shape), dtype)
        self.guards.append(g)
        return g

    def acc(self, shape):
        self.seed += 1
        p = E.prefill(*shape, seed=self.seed)
        g = Guard(tuple(shape), fill=p)
        self.guards.append(g)
        return g, p.double()

    def dev(self, t):
        self.keep.append(t.contiguous().cuda())
        return self.keep[-1]

    def ptrs(self, tensors, n=None):
        """a host array of device pointers (kept alive with the test)"""
        p = [t.ptr if isinstance(t, Guard) else t.data_ptr() for t in tensors]
        arr = (ctypes.c_void_p * (n or len(p)))(*(p + [None] * ((n or len(p)) - len(p))))
        self.keep.append(arr)
        return ctypes.addressof(arr)

    def done(self, what):
        torch.cuda.synchronize()
        for i, g in enumerate(self.guards):
            g.check(f"{what} (buffer {i})")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits_or_nan(got, ref, what):
    """equal as bits wherever the reference is no NaN, NaN exactly where it is one"""
    g, nan = got.detach().cpu(), torch.isnan(ref)
    gn = torch.isnan(g)
    assert torch.equal(gn, nan), f"{what}: {int((gn & ~nan).sum())} NaNs the reference does not have, {int((nan & ~gn).sum())} NaNs of the reference missing (of {int(nan.sum())})"
    bad = (bits(g) != bits(ref)) & ~nan
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ in their bits; first: got {float(g[bad][0])!r}, want {float(ref[bad][0])!r}"


MB = [(1, 1), (1, 2), (3, 1), (3, 2)]
MB_IDS = [f"M{m}_B{b}" for m, b in MB]
G_IDS = [r["id"] for r in R.GATHER_ROWS]
S_IDS = [r["id"] for r in R.SCATTER_ROWS]
A_IDS = [r["id"] for r in R.ATTN_ROWS]


# ====================================================================================================================== A. gather
def _gather_dsrc_reference(row, pl, ref, dtok, M):
    l = R._prod(pl["n"])
    return [R.gather_bwd_reference(ref[k % 3][1][:, :, :, (k // 3) * l:(k // 3 + 1) * l], dtok[k % 3][:, :, :, (k // 3) * l:(k // 3 + 1) * l], pl,
                                   row["cv"] if k % 3 == 2 else row["cq"]) for k in range(3 * M)]


@pytest.mark.parametrize("M,B", MB, ids=MB_IDS)
@pytest.mark.parametrize("kind", R.GATHER_KINDS)
@pytest.mark.parametrize("row", R.GATHER_ROWS, ids=G_IDS)
def test_fused_gather_is_aten_max_pool(row, kind, M, B):
    """vx_pwa_gather_all_fwd / _bwd under vx_pwa_gather_set_vec 0, 1 and 2: tokens, arg-max indices of the pooled scales, dsrc"""
    H = _H()
    run = Run(H, row)
    pl, cq, cv, h = run.pl, row["cq"], row["cv"], row["heads"]
    off, l = R.woff(pl), R._prod(pl["n"])
    pooled0 = off[next(i for i, s in enumerate(pl["small"]) if R._prod(s) > 1)]
    src = [run.dev(t) for t in R.gather_sources(row, kind, M, B)]
    ref = R.gather_reference(row, kind, M, B)
    dtok_cpu = R.gather_dtok(row, M, B)
    dtok = [run.dev(t) for t in dtok_cpu]
    dref = _gather_dsrc_reference(row, pl, ref, dtok_cpu, M)
    got = {}
    for vec in (0, 1, 2):
        with knob(H, "vx_pwa_gather_set_vec", vec, 1):
            tok = [run.out((B, h, off[-1], M * l, c)) for c in (cq, cq, cv)]
            idx = [run.out((B, h, off[-1], M * l, c), torch.int32) for c in (cq, cq, cv)]
            H.call("vx_pwa_gather_all_fwd", run.ptrs(src), *[t.ptr for t in tok], *[t.ptr for t in idx], run.pp, cq, cv, M, B, run.st)
            dst = [run.out(t.shape) for t in src]
            H.call("vx_pwa_gather_all_bwd", *[H.P(t) for t in dtok], *[t.ptr for t in idx], run.ptrs(dst), run.pp, cq, cv, M, B, run.st)      # (reads the indices this form saved)
        got[vec] = (tok, idx, dst)
    run.done(f"gather_all {row['id']} {kind}")
    for vec, (tok, idx, dst) in got.items():
        for j, name in enumerate("qkv"):
            same_bits_or_nan(tok[j].t, ref[j][0], f"{kind}, knob {vec}: tokens of {name}")
            gi, ri = idx[j].t.cpu()[:, :, pooled0:], ref[j][1][:, :, pooled0:].to(torch.int32)
            bad = gi != ri
            assert not bool(bad.any()), f"{kind}, knob {vec}: {int(bad.sum())} of {bad.numel()} saved indices of {name} differ from aten's; first: got {int(gi[bad][0])}, want {int(ri[bad][0])}"
        for k in range(3 * M):
            assert torch.equal(bits(dst[k].t), bits(dref[k])), f"{kind}, knob {vec}: dsrc {k} (every element is written: zero except dsrc[idx] = dtok)"


@pytest.mark.parametrize("M,B", MB, ids=MB_IDS)
@pytest.mark.parametrize("kind", R.GATHER_KINDS)
@pytest.mark.parametrize("row", R.GATHER_ROWS, ids=G_IDS)
def test_per_modality_gather_is_aten_max_pool(row, kind, M, B):
    """vx_pwa_gather_fwd with m = 0 .. M - 1 into one token tensor; vx_pwa_gather_bwd, which recomputes the arg-max from src"""
    H = _H()
    run = Run(H, row)
    pl, h = run.pl, row["heads"]
    off, l = R.woff(pl), R._prod(pl["n"])
    src = [run.dev(t) for t in R.gather_sources(row, kind, M, B)]
    ref = R.gather_reference(row, kind, M, B)
    dtok_cpu = R.gather_dtok(row, M, B)
    dref = _gather_dsrc_reference(row, pl, ref, dtok_cpu, M)
    res = []
    for j, c in ((0, row["cq"]), (2, row["cv"])):
        tok = run.out((B, h, off[-1], M * l, c))
        dtok = run.dev(dtok_cpu[j])
        dst = []
        for m in range(M):
            H.call("vx_pwa_gather_fwd", H.P(src[3 * m + j]), tok.ptr, run.pp, c, m, M, B, run.st)
            dst.append(run.out(src[3 * m + j].shape))
            H.call("vx_pwa_gather_bwd", H.P(src[3 * m + j]), H.P(dtok), dst[m].ptr, run.pp, c, m, M, B, run.st)
        res.append((j, tok, dst))
    run.done(f"gather {row['id']} {kind}")
    for j, tok, dst in res:
        same_bits_or_nan(tok.t, ref[j][0], f"{kind}: tokens of {'qkv'[j]}")
        for m in range(M):
            assert torch.equal(bits(dst[m].t), bits(dref[3 * m + j])), f"{kind}: dsrc of {'qkv'[j]}, modality {m}"


# ====================================================================================================================== B. scatter
def _inside(got, ref, S, mult, what, worst):
    ok, ratio, text = R.bound_report(got, ref, S, mult)
    worst[what.split(":")[0]] = max(worst.get(what.split(":")[0], 0.0), ratio)
    assert ok, f"{what}: {text}"


def _ident_bits(got, ref, what):
    """the identity scale copies: the fp64 reference is exact and compared as bits (+ 0.0: a sum of signed zeros in the reference is +0.0, as is the kernels')"""
    assert torch.equal(bits(got), bits((ref + 0.0).float())), f"{what}: the identity scale must be a copy"


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("row", R.SCATTER_ROWS, ids=S_IDS)
def test_scatter_forward_inside_the_derived_bound(row, B):
    """vx_pwa_scatter_fwd (per modality) and vx_pwa_scatter_fwd_all; vx_pwa_gather_set_vec 1: four channels per lane where c % 4 == 0, 0: the scalar kernel"""
    H = _H()
    run = Run(H, row)
    pl, c, M, h = run.pl, row["c"], row["M"], row["heads"]
    ref = R.scatter_reference(row, B)
    tok = run.dev(R.scatter_inputs(row, B)[0])
    shape = (B, pl["nb"] * h * c, *row["grid"])
    got = []
    for vec in (0, 1):
        with knob(H, "vx_pwa_gather_set_vec", vec, 1):
            one = [run.out(shape) for _ in range(M)]
            for m in range(M):
                H.call("vx_pwa_scatter_fwd", H.P(tok), one[m].ptr, run.pp, c, m, M, B, run.st)
            every = [run.out(shape) for _ in range(M)]
            H.call("vx_pwa_scatter_fwd_all", H.P(tok), run.ptrs(every, 4), run.pp, c, M, B, run.st)
        form = "four channels per lane" if vec and c % 4 == 0 else "scalar"
        got += [(f"forward {form}: vx_pwa_scatter_fwd, knob {vec}", one), (f"forward {form}: vx_pwa_scatter_fwd_all, knob {vec}", every)]
    run.done(f"scatter forward {row['id']}")
    worst = {}
    for what, outs in got:
        for m in range(M):
            _inside(outs[m].t, ref["out"][m], ref["out_S"][m], 12, f"{what}, modality {m}", worst)
            _ident_bits(outs[m].t[:, :h * c], ref["out"][m][:, :h * c], f"{what}, modality {m}")
    print(f"scatter {row['id']} B={B}: largest err / (u S): " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("row", R.SCATTER_ROWS, ids=S_IDS)
def test_scatter_adjoints_inside_the_derived_bound(row, B):
    """vx_pwa_scatter_bwd (+=, per modality), _bwd_all (+=), _bwd_all_w and _bwd_all_wz (NaN-filled destination, the extra buffer zeroed) under
    vx_pwa_scatter_set_ident 0 / 1 x vx_pwa_scatter_set_merged 0 / 2: with the identity knob on every scale takes the kernel of the table's `kinds` column (identity,
    per-token gather, separable), per scale or in the one launch; with it off every scale takes the general kernel and _w / _wz decline"""
    H = _H()
    run = Run(H, row)
    pl, c, M, h = run.pl, row["c"], row["M"], row["heads"]
    ref = R.scatter_reference(row, B)
    dout = [run.dev(t) for t in R.scatter_inputs(row, B)[1]]
    dptr = run.ptrs(dout, 4)
    shape = tuple(ref["dtok"].shape)
    nI = R.ident_windows(pl)
    got = []
    for ident in (1, 0):
        kinds = [R.scatter_bwd_kind(pl, c, B, i, ident) for i in range(pl["nb"])]
        assert kinds == (row["kinds"] if ident else [3] * pl["nb"])
        declines = R.scatter_w_declines(pl, c, B, ident)
        for merged in (0, 2):
            tag = f"adjoint kinds {sorted(set(kinds))} {'one launch' if merged and R.scatter_one_launch(pl, c, B, ident) else 'per scale'}"
            with knob(H, "vx_pwa_scatter_set_ident", ident, 1), knob(H, "vx_pwa_scatter_set_merged", merged, 1):
                if merged == 0:                                  # (the per-modality entry never takes the one launch)
                    d, p = run.acc(shape)
                    for m in range(M):
                        H.call("vx_pwa_scatter_bwd", H.P(dout[m]), d.ptr, run.pp, c, m, M, B, run.st)
                    got.append((f"{tag}: vx_pwa_scatter_bwd ident={ident}", d, p))
                d, p = run.acc(shape)
                H.call("vx_pwa_scatter_bwd_all", dptr, d.ptr, run.pp, c, M, B, run.st)
                got.append((f"{tag}: vx_pwa_scatter_bwd_all ident={ident} merged={merged}", d, p))
                for entry in ("vx_pwa_scatter_bwd_all_w", "vx_pwa_scatter_bwd_all_wz"):
                    d = run.out(shape)
                    extra = run.out((4 * 1237,)) if entry.endswith("wz") else None
                    rc = H.query(entry, dptr, d.ptr, run.pp, c, M, B, *((extra.ptr, extra.t.numel()) if extra else ()), run.st)
                    assert rc == (1 if declines else 0), f"{entry} ident={ident} merged={merged}: returned {rc}"
                    got.append((f"{tag}: {entry} ident={ident} merged={merged}", d, None if declines else 0.0, extra))
    run.done(f"scatter adjoint {row['id']}")
    worst = {}
    for what, d, p, *rest in got:
        extra = rest[0] if rest else None
        if p is None:                                            # declined: nothing may have been written
            assert bool(torch.isnan(d.t).all()), f"{what}: declined, but wrote its destination"
            assert extra is None or bool(torch.isnan(extra.t).all()), f"{what}: declined, but wrote the extra buffer"
            continue
        prefilled = torch.is_tensor(p)                           # `+=`: the prefill is one more accumulated term of weight 1
        want, S, n = ref["dtok"] + p, ref["dtok_S"] + (p.abs() if prefilled else 0.0), ref["dtok_n"] + (1 if prefilled else 0)
        _inside(d.t, want, S, 12 + n, what, worst)
        _ident_bits(d.t[:, :, :nI], want[:, :, :nI], what)
        if extra is not None:
            assert bool((bits(extra.t) == 0).all()), f"{what}: the extra buffer must come back all zero"
    print(f"scatter {row['id']} B={B}: largest err / (u S): " + "; ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


# ====================================================================================================================== C. attention forward
@pytest.mark.parametrize("bias", R.ATTN_BIASES)
@pytest.mark.parametrize("row", R.ATTN_ROWS, ids=A_IDS)
def test_attention_forward_in_its_exact_regimes(row, bias):
    """vx_pwa_attn_fwd, p_drop 0, q = k = 0, V integers, under vx_pwa_attn_set_mfma 3 / 0 x vx_pwa_attn_set_split 0 / 1 / 2 / 4"""
    H = _H()
    run = Run(H, row)
    pl, M, h, B = run.pl, row["M"], row["heads"], R.ATTN_B
    cq, cv, ML, Nt = pl["c_qk"], pl["c_v"], M * R._prod(pl["n"]), R.woff(pl)[-1]
    ref = R.attn_reference(row, bias)
    q, k = run.dev(torch.zeros(B, h, Nt, ML, cq)), run.dev(torch.zeros(B, h, Nt, ML, cq))
    v, table = run.dev(R.attn_v(row)), run.dev(R.attn_table(row, bias))
    seed = run.dev(torch.zeros(2, dtype=torch.int64))
    got = []
    for mfma in (3, 0):
        for split in (0, 1, 2, 4):
            with knob(H, "vx_pwa_attn_set_mfma", mfma, 3), knob(H, "vx_pwa_attn_set_split", split, 0):
                o, lse = run.out((B, h, Nt, ML, cv)), run.out((B, h, Nt, ML))
                H.call("vx_pwa_attn_fwd", H.P(q), H.P(k), H.P(v), H.P(table), o.ptr, lse.ptr, run.pp, B, M, cq, cv, H.P(seed, torch.int64), 0, 0.0, run.st)
            got.append((f"{bias}, mfma {mfma}, split {split}", o, lse))
    run.done(f"attention {row['id']} {bias}")
    pow2 = ref["pow2"][None, :, None, :, None].expand_as(ref["O"])
    for what, o, lse in got:
        g = o.t.detach().double().cpu()
        bad = ~(g == ref["O"]) & pow2
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {int(pow2.sum())} outputs with a power-of-two divisor differ; first: got {float(g[bad][0])!r}, want {float(ref['O'][bad][0])!r}"
        err = (g - ref["O"]).abs()
        bad = ~(err <= 2 * U * ref["O"].abs())
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} outputs beyond 2 u |ref|; largest err / (u |ref|) = {float((err / (U * ref['O'].abs()))[ref['O'] != 0].max()):.3f}"
        gl, rl = lse.t.detach().double().cpu(), ref["lse"][None, :, None, :].expand(B, h, Nt, ML)
        assert bool(((gl - rl).abs() <= LSE_ATOL + LSE_RTOL * rl.abs()).all()), f"{what}: LSE, largest error {float((gl - rl).abs().max()):.3e}"
