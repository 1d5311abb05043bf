"""Oracles for the paired-window attention path of csrc/pwa.hip: tables of rows, input builders and fp64 / aten references.

  A. gather   = max-pool + window partition, held BIT FOR BIT to F.max_pool3d(return_indices=True) on the CPU: ties, signed zeros, -inf cells, +inf and NaN.
  B. scatter  = per-window trilinear up-sampling and its adjoints against fp64 with a DERIVED per-element bound: the same operator on the absolute values gives
                S = sum |w| |t|; forward |err| <= 12 u S (three nested lerps), adjoint |err| <= (12 + n) u S with n = the number of accumulated terms.
  C. attention forward in the regimes it solves exactly: q = k = 0, so the scores are the relative bias; a table that is uniform, or 0 at one offset and -128
     elsewhere (exp(-128) flushes to 0 in fp32): the output is a mean of integers.

CPU-only at import (tests/test_pwa_ref_cpu.py proves the premises on every row without a GPU; tests/test_pwa_exact_gpu.py runs the kernels on the same rows)."""
import functools
import torch
import torch.nn.functional as F

import exact_ref as E
from oracle import veloxseg_oracle as O

U = 2.0 ** -24              # unit roundoff of fp32
NAN, INF = float("nan"), float("inf")
MAXB, MAXM = 2, 3           # inputs are built once at the largest batch / modality count; smaller cases take a prefix


def _seed(rid, extra=0):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(rid)) + 7919 * extra) % 100003


def _prod(v):
    return int(v[0]) * int(v[1]) * int(v[2])


def make_plan(r):
    """the window geometry of a row (channel counts are the row's own, not the plan's)"""
    return O.plan_pwa(r["grid"], r["big"], [1, 1, 1], 2, r["heads"], r.get("mdh", 4), r.get("C", 4))


def woff(pl):
    off = [0]
    for nw in pl["nwin"]:
        off.append(off[-1] + _prod(nw))
    return off


# ====================================================================================================================== A. gather
def lanes(csz):
    """T of vx_pwa_gather_all_fwd*: the lanes that share a pooled cell (a power of two, 64 at the most)"""
    T = 1
    while T < 64 and T < csz:
        T <<= 1
    return T


def nan_positions(csz):
    """in-cell scan positions of the `nan_at` kind: the first and the last load of lane 0 (0, T, where T < csz) and of the other lanes (1, T - 1, csz - 1)"""
    T = lanes(csz)
    return sorted({p for p in (0, 1, T - 1, T, csz - 1) if 0 <= p < csz})


def _g(id, grid, big, heads, cq, cv, nan_at):
    return dict(id=id, grid=grid, big=big, heads=heads, cq=cq, cv=cv, nan_at=nan_at)


# `nan_at`: {cell size: scan positions} spelt out per row (test_pwa_ref_cpu.py holds it to nan_positions, so the table cannot quietly shrink)
GATHER_ROWS = [
    _g("16_four_scales", [16, 16, 16], [2, 2, 2], 2, 4, 8, {8: [0, 1, 7], 64: [0, 1, 63], 512: [0, 1, 63, 64, 511]}),     # cells up to 8^3: T = 64 lanes x 8 loop trips
    _g("aniso", [16, 16, 8], [4, 4, 2], 1, 8, 8, {8: [0, 1, 7], 64: [0, 1, 63]}),
    _g("w12", [12, 12, 12], [3, 3, 3], 1, 4, 4, {8: [0, 1, 7], 64: [0, 1, 63]}),
    _g("w6_rows_not_x4", [6, 6, 6], [3, 3, 3], 2, 4, 8, {8: [0, 1, 7]}),
    _g("token_axis_of_1", [8, 8, 2], [4, 4, 1], 2, 4, 4, {8: [0, 1, 7]}),
    _g("scalar_channels_3_5", [8, 8, 8], [2, 2, 2], 1, 3, 5, {8: [0, 1, 7], 64: [0, 1, 63]}),                          # c % 4 != 0: the one-lane kernels under every knob
]
GATHER_KINDS = ("ties", "zeros", "neg_inf", "inf_nan", "nan_at", "two_nans", "all_nan", "randn")
GATHER_CELLS = 5            # every pooled scale of every row has at least this many cells (the plantings use cells 0 .. 4)


def gather_row(rid):
    return next(r for r in GATHER_ROWS if r["id"] == rid)


def cell_voxel(grid, s, cell, pos):
    """(d, h, w) of in-cell scan position `pos` of the pooled cell with flat number `cell`"""
    pn = [g // k for g, k in zip(grid, s)]
    p2, p1, p0 = cell % pn[2], (cell // pn[2]) % pn[1], cell // (pn[2] * pn[1])
    w, h, d = pos % s[2], (pos // s[2]) % s[1], pos // (s[2] * s[1])
    return p0 * s[0] + d, p1 * s[1] + h, p2 * s[2] + w


@functools.lru_cache(maxsize=None)
def _gather_sources(rid, kind):
    r = gather_row(rid)
    pl, grid, h = make_plan(r), r["grid"], r["heads"]
    out = []
    for k in range(3 * MAXM):
        c = r["cv"] if k % 3 == 2 else r["cq"]
        shape = (MAXB, pl["nb"] * h * c, *grid)
        g = torch.Generator().manual_seed(_seed(rid, 10 * k + GATHER_KINDS.index(kind)))
        if kind == "ties":
            x = torch.randint(0, 3, shape, generator=g).float()
        else:
            x = torch.randn(shape, generator=g)
        if kind == "zeros":
            x = -x.abs() - 1.0                                                   # every other value is below -1: a planted zero is its cell's maximum
        for i, s in enumerate(pl["small"]):
            csz = _prod(s)
            if csz == 1:
                continue
            sl, T = slice(i * h * c, (i + 1) * h * c), lanes(csz)

            def put(cell, pos, val):
                d, hh, w = cell_voxel(grid, s, cell, pos)
                x[:, sl, d, hh, w] = val

            def fill(cell, val):
                d, hh, w = cell_voxel(grid, s, cell, 0)
                x[:, sl, d:d + s[0], hh:hh + s[1], w:w + s[2]] = val

            if kind == "zeros":
                put(0, 0, -0.0), put(0, csz - 1, 0.0)                            # -0.0 first: the token is -0.0
                put(1, 0, 0.0), put(1, csz - 1, -0.0)                            # +0.0 first
                put(2, 1, -0.0), put(2, 2, 0.0)                                  # neighbours
            elif kind == "neg_inf":
                fill(0, -INF)
            elif kind == "inf_nan":
                put(0, 0, INF), put(0, csz - 1, NAN)
                put(1, 0, NAN), put(1, csz - 1, INF)
            elif kind == "nan_at":
                for j, pos in enumerate(r["nan_at"][csz]):
                    put(j, pos, NAN)
            elif kind == "two_nans":
                put(0, 0, NAN), put(0, csz - 1, NAN)                             # lane 0 and the last lane
                put(1, 1, NAN), put(1, min(T + 1, csz - 1), NAN)                 # (cells wider than T: twice in lane 1)
            elif kind == "all_nan":
                fill(0, NAN)
        out.append(x)
    return out


def gather_sources(r, kind, M=MAXM, B=MAXB):
    """3 M source volumes (q, k, v per modality), CPU fp32, never modified"""
    return [t[:B] for t in _gather_sources(r["id"], kind)[:3 * M]]


def partition(p, pl, i, c):
    """window partition of scale i: (B, h c, P0, P1, P2) -> (B, h, N_i, l, c); the reshape of oracle.gather_windows, for values and for indices alike"""
    B, h, n = p.shape[0], pl["heads"], pl["n"]
    N0, N1, N2 = pl["nwin"][i]
    p = p.reshape(B, h, c, N0, n[0], N1, n[1], N2, n[2])
    return p.permute(0, 1, 3, 5, 7, 4, 6, 8, 2).reshape(B, h, N0 * N1 * N2, n[0] * n[1] * n[2], c)


def pool_aten(x, pl, c, pool=None):
    """-> tokens (B, h, Ntot, l, c) fp32 and the arg-max voxel of every token (int64; the flattened (d H + h) W + w of its channel's volume; 1x1x1 cells: the voxel
    itself) by F.max_pool3d(return_indices=True) -- or by `pool(x_i, s)`, the scan restatement of the CPU premise test"""
    B, h, nb = x.shape[0], pl["heads"], pl["nb"]
    V = _prod(pl["grid"])
    xv = x.view(B, nb, h * c, *pl["grid"])
    toks, idxs = [], []
    for i, s in enumerate(pl["small"]):
        if _prod(s) == 1:
            v, ix = xv[:, i], torch.arange(V).view(1, 1, *pl["grid"]).expand(B, h * c, *pl["grid"])
        elif pool is None:
            v, ix = F.max_pool3d(xv[:, i], kernel_size=s, stride=s, return_indices=True)
        else:
            v, ix = pool(xv[:, i], s)
        toks.append(partition(v, pl, i, c))
        idxs.append(partition(ix, pl, i, c))
    return torch.cat(toks, 2), torch.cat(idxs, 2)


def pool_scan(x, s):
    """aten's rule restated: scan each cell in (d, h, w) order, start from (-inf, first voxel), update on `val > best or isnan(val)`"""
    B, C, D, H, W = x.shape
    P = (D // s[0], H // s[1], W // s[2])
    cells = x.view(B, C, P[0], s[0], P[1], s[1], P[2], s[2]).permute(0, 1, 2, 4, 6, 3, 5, 7).reshape(B, C, *P, _prod(s))
    best, pos = torch.full(cells.shape[:-1], -INF), torch.zeros(cells.shape[:-1], dtype=torch.int64)
    for e in range(cells.shape[-1]):
        val = cells[..., e]
        upd = (val > best) | torch.isnan(val)
        best, pos = torch.where(upd, val, best), torch.where(upd, torch.full_like(pos, e), pos)
    p0, p1, p2 = torch.meshgrid(*[torch.arange(k) for k in P], indexing="ij")
    d, hh, w = pos // (s[1] * s[2]), (pos // s[2]) % s[1], pos % s[2]
    return best, ((p0 * s[0] + d) * H + (p1 * s[1] + hh)) * W + (p2 * s[2] + w)


@functools.lru_cache(maxsize=None)
def _gather_reference(rid, kind):
    r = gather_row(rid)
    pl = make_plan(r)
    return [pool_aten(x, pl, r["cv"] if k % 3 == 2 else r["cq"]) for k, x in enumerate(_gather_sources(rid, kind))]


def gather_reference(r, kind, M=MAXM, B=MAXB):
    """per kind (q, k, v): tokens (B, h, Ntot, M l, c) and arg-max voxels, the modalities concatenated as the kernels lay them out"""
    ref = _gather_reference(r["id"], kind)
    return [(torch.cat([ref[3 * m + j][0][:B] for m in range(M)], 3), torch.cat([ref[3 * m + j][1][:B] for m in range(M)], 3)) for j in range(3)]


@functools.lru_cache(maxsize=None)
def _gather_dtok(rid):
    r = gather_row(rid)
    pl = make_plan(r)
    shape = (MAXB, r["heads"], woff(pl)[-1], MAXM * _prod(pl["n"]))
    return [E.ints(*shape, c, seed=_seed(rid, 500 + j), lo=1, hi=3) * (2.0 * E.ints(*shape, c, seed=_seed(rid, 600 + j), lo=0, hi=1) - 1.0)
            for j, c in enumerate((r["cq"], r["cq"], r["cv"]))]


def gather_dtok(r, M=MAXM, B=MAXB):
    """token gradients of q, k, v: random non-zero integers (+-1 .. +-3)"""
    l = _prod(make_plan(r)["n"])
    return [t[:B, :, :, :M * l].contiguous() for t in _gather_dtok(r["id"])]


def gather_bwd_reference(idx, dtok, pl, c):
    """dsrc (B, nb h c, grid) of ONE modality: zero except dsrc[idx] = dtok (idx, dtok: that modality's (B, h, Ntot, l, c) slices)"""
    B, h = idx.shape[0], pl["heads"]
    dsrc = torch.zeros(B, pl["nb"] * h * c, _prod(pl["grid"]))
    off = woff(pl)
    for i in range(pl["nb"]):
        ix = idx[:, :, off[i]:off[i + 1]].permute(0, 1, 4, 2, 3).reshape(B, h * c, -1)
        g = dtok[:, :, off[i]:off[i + 1]].permute(0, 1, 4, 2, 3).reshape(B, h * c, -1)
        dsrc[:, i * h * c:(i + 1) * h * c].scatter_(2, ix, g)
    return dsrc.view(B, -1, *pl["grid"])


# ====================================================================================================================== B. scatter
def _s(id, grid, big, heads, c, M, kinds):
    return dict(id=id, grid=grid, big=big, heads=heads, c=c, M=M, kinds=kinds)


# `kinds`: the adjoint kernel vx_scatter_bwd_kind selects per scale with the identity knob on (0 identity, 1 per-token gather, 2 separable); with the knob off every
# scale takes the general kernel (3).  test_pwa_ref_cpu.py holds the column to the predicate as csrc/pwa.hip writes it.
SCATTER_ROWS = [
    _s("two_scales", [16, 16, 16], [8, 8, 8], 2, 8, 2, [0, 1]),
    _s("scales_incl_separable", [32, 32, 32], [4, 4, 4], 1, 4, 2, [0, 1, 2, 2]),
    _s("one_modality", [8, 8, 8], [4, 4, 4], 4, 32, 1, [0, 1]),
    _s("single_scale", [4, 4, 4], [4, 4, 4], 2, 16, 2, [0]),
    _s("96_L1", [24, 24, 24], [3, 3, 3], 1, 4, 2, [0, 1, 2, 2]),
    _s("aniso_three_modalities", [16, 16, 8], [4, 4, 2], 2, 8, 3, [0, 1, 2]),
    _s("token_axis_of_1_c3", [8, 8, 2], [4, 4, 1], 2, 3, 2, [0, 1]),                     # c = 3: the scalar forward under every knob
]
SC_TAPS, SC_GATHER_MAX, SC_SEP_T2 = 12, 2, 8         # VX_SC_TAPS, vx_scatter_gather_max, VX_SC_SEP_T2 of csrc/pwa.hip


def scatter_row(rid):
    return next(r for r in SCATTER_ROWS if r["id"] == rid)


def scatter_bwd_kind(pl, c, B, i, ident=1):
    """vx_scatter_bwd_kind as written: smax <= 2, the LDS sizes, the grid limits"""
    s, n, h = pl["small"][i], pl["n"], pl["heads"]
    if s == [1, 1, 1] and ident:
        return 0
    bw = [n[k] * s[k] for k in range(3)]
    nv, smax, nmax = _prod(bw), max(s), max(n)
    shm2 = 4 * ((nv + 3) // 4 * 4 + 3 * nmax * SC_TAPS * 2 + 3 * nmax)
    if smax <= SC_GATHER_MAX and shm2 <= 64 * 1024 and c <= 65535 and ident:
        return 1
    shm3 = 4 * (bw[1] * bw[2] + bw[1] * n[2] + _prod(n) + n[2] * bw[2] + n[1] * bw[1])
    if ident and shm3 <= 60 * 1024 and B * h * c <= 65535:
        return 2
    return 3


def scatter_w_declines(pl, c, B, ident=1):
    """vx_pwa_scatter_bwd_all_w / _wz return 1 and launch nothing: nb <= 4 holds for every plan; scale 0 must be the only identity scale"""
    kinds = [scatter_bwd_kind(pl, c, B, i, ident) for i in range(pl["nb"])]
    return kinds[0] != 0 or any(k == 0 for k in kinds[1:])


def scatter_one_launch(pl, c, B, ident=1):
    """vx_scatter_bwd_merged with the knob at 2 takes the row: every scale of kind 0, 1 or 2, separable scales with n2 <= VX_SC_SEP_T2 and windows below 2^22 voxels"""
    for i in range(pl["nb"]):
        k = scatter_bwd_kind(pl, c, B, i, ident)
        nv = _prod([pl["n"][a] * pl["small"][i][a] for a in range(3)])
        if k > 2 or (k == 2 and (pl["n"][2] > SC_SEP_T2 or nv >= 1 << 22)):
            return False
    return True


def _weights(n_in, n_out, how):
    A = O.interp_matrix(n_in, n_out).double()                   # the fp32-computed weights, cast
    return A if how == "w" else (A.abs() if how == "abs" else (A != 0).double())


def scatter(tok, pl, c, how="w"):
    """oracle.scatter_windows in fp64: (B, h, Ntot, l, c) -> (B, nb h c, grid).  how = "w": the operator; "abs": on |w| (its operand is |t|); "nz": the indicator of
    a non-zero weight (pushing ones through counts the terms)"""
    B, h, n, g = tok.shape[0], pl["heads"], pl["n"], pl["grid"]
    outs, off = [], woff(pl)
    for i, s in enumerate(pl["small"]):
        N0, N1, N2 = pl["nwin"][i]
        t = tok[:, :, off[i]:off[i + 1]].reshape(B, h, N0, N1, N2, n[0], n[1], n[2], c)
        A0, A1, A2 = (_weights(n[k], n[k] * s[k], how) for k in range(3))
        t = torch.einsum("bhxyzijkc,Ii->bhxyzIjkc", t, A0)
        t = torch.einsum("bhxyzijkc,Jj->bhxyziJkc", t, A1)
        t = torch.einsum("bhxyzijkc,Kk->bhxyzijKc", t, A2)
        outs.append(t.permute(0, 1, 8, 2, 5, 3, 6, 4, 7).reshape(B, h * c, g[0], g[1], g[2]))
    return torch.cat(outs, 1)


def scatter_adjoint(douts, pl, c, how="w"):
    """the autograd of `scatter` over the M modalities: douts[m] (B, nb h c, grid) -> dtok (B, h, Ntot, M l, c)"""
    M, B, l = len(douts), douts[0].shape[0], _prod(pl["n"])
    tok = torch.zeros(B, pl["heads"], woff(pl)[-1], M * l, c, dtype=douts[0].dtype, requires_grad=True)
    outs = [scatter(tok[:, :, :, m * l:(m + 1) * l], pl, c, how) for m in range(M)]
    return torch.autograd.grad(outs, tok, list(douts))[0]


@functools.lru_cache(maxsize=None)
def _scatter_inputs(rid):
    r = scatter_row(rid)
    pl, c, M = make_plan(r), r["c"], r["M"]
    tok = E.ints(MAXB, r["heads"], woff(pl)[-1], M * _prod(pl["n"]), c, seed=_seed(rid, 1))
    dout = [E.ints(MAXB, pl["nb"] * r["heads"] * c, *r["grid"], seed=_seed(rid, 2 + m)) for m in range(M)]
    return tok, dout


def scatter_inputs(r, B):
    """tokens and output gradients: integers in [-3, 3], CPU fp32, never modified"""
    tok, dout = _scatter_inputs(r["id"])
    return tok[:B], [d[:B] for d in dout]


def scatter_operate(r, B):
    """forward per modality and adjoint through oracle.scatter_windows itself, in torch's fp32: what the CPU premise test holds to the bounds"""
    pl, c, M = make_plan(r), r["c"], r["M"]
    tok, dout = scatter_inputs(r, B)
    l = _prod(pl["n"])
    t = tok.clone().requires_grad_(True)
    outs = [O.scatter_windows(t[:, :, :, m * l:(m + 1) * l], pl, c) for m in range(M)]
    return [o.detach() for o in outs], torch.autograd.grad(outs, t, list(dout))[0]


@functools.lru_cache(maxsize=None)
def _scatter_reference(rid, B):
    r = scatter_row(rid)
    pl, c, M = make_plan(r), r["c"], r["M"]
    tok, dout = scatter_inputs(r, B)
    l = _prod(pl["n"])
    td, dd = tok.double(), [d.double() for d in dout]
    return dict(out=[scatter(td[:, :, :, m * l:(m + 1) * l], pl, c) for m in range(M)],
                out_S=[scatter(td[:, :, :, m * l:(m + 1) * l].abs(), pl, c, "abs") for m in range(M)],
                dtok=scatter_adjoint(dd, pl, c), dtok_S=scatter_adjoint([d.abs() for d in dd], pl, c, "abs"),
                dtok_n=scatter_adjoint([torch.ones_like(d) for d in dd], pl, c, "nz"))


def scatter_reference(r, B):
    """fp64: out[m], out_S[m] = sum |w| |t| per voxel; dtok, dtok_S, dtok_n = the number of voxels with a non-zero weight on each token element"""
    return _scatter_reference(r["id"], B)


def ident_windows(pl):
    """window range [0, n) of the identity scale (1x1x1 cells; scale 0 of every row): a copy, compared as bits"""
    assert pl["small"][0] == [1, 1, 1]
    return woff(pl)[1]


def bound_report(got, ref, S, mult):
    """(ok, largest err / (u S), text): |got - ref| <= mult u S per element (mult: a number or a tensor); where S == 0 the result must be exactly 0"""
    g = got.detach().double().cpu()
    err = (g - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, INF), err)          # (a NaN left of the prefill)
    lim = mult * U * S
    ok = bool((err <= lim).all())
    pos = S > 0
    ratio = float((err[pos] / (U * S[pos])).max()) if bool(pos.any()) else 0.0
    worst = int((err - lim).argmax())
    return ok, ratio, f"largest err / (u S) = {ratio:.3f}; worst element {worst}: got {float(g.reshape(-1)[worst])!r}, want {float(ref.reshape(-1)[worst])!r}, S = {float(S.reshape(-1)[worst])!r}"


# ====================================================================================================================== C. attention forward
def _a(id, grid, big, heads, mdh, C, M):
    return dict(id=id, grid=grid, big=big, heads=heads, mdh=mdh, C=C, M=M)


ATTN_ROWS = [
    _a("l2_like", [12, 12, 12], [6, 6, 6], 2, 8, 32, 2),          # the five PWA_CASES of tests/test_hip_ops_gpu.py: l = 216 and 27 ...
    _a("l1_like", [8, 8, 8], [2, 2, 2], 1, 4, 16, 2),             # l = 8
    _a("single_modality", [8, 8, 8], [4, 4, 4], 2, 8, 32, 1),     # l = 64, M = 1
    _a("aniso", [8, 8, 4], [4, 4, 2], 1, 4, 16, 2),               # l = 32
    _a("l4_like", [3, 3, 3], [3, 3, 3], 4, 16, 128, 2),           # l = 27, four heads
    _a("three_modalities", [6, 6, 6], [3, 3, 3], 1, 4, 16, 3),    # M = 3: M l = 81, a divisor that is no power of two in either regime
]
ATTN_B = 2
ATTN_BIASES = ("uniform", "one_hot_0", "one_hot_1", "one_hot_2")     # one_hot_s: head a takes offset number (a + s) % 3
OFF_BIAS = -128.0


def attn_row(rid):
    return next(r for r in ATTN_ROWS if r["id"] == rid)


def attn_offsets(n):
    return [(0, 0, 0), (1, 0, -1), (n[0] - 1, n[1] - 1, n[2] - 1)]


def attn_head_offset(n, a, bias):
    return attn_offsets(n)[(a + int(bias[-1])) % 3]


def attn_table(r, bias):
    """(Tsz, heads) fp32.  Entry ((d0 + n0 - 1)(2 n1 - 1) + d1 + n1 - 1)(2 n2 - 1) + d2 + n2 - 1 is read by the pair with query - key = d, so the key at query + r reads
    the entry of d = -r"""
    n = make_plan(r)["n"]
    Tsz = (2 * n[0] - 1) * (2 * n[1] - 1) * (2 * n[2] - 1)
    if bias == "uniform":
        return torch.zeros(Tsz, r["heads"])
    t = torch.full((Tsz, r["heads"]), OFF_BIAS)
    for a in range(r["heads"]):
        d = [-x for x in attn_head_offset(n, a, bias)]
        t[((d[0] + n[0] - 1) * (2 * n[1] - 1) + d[1] + n[1] - 1) * (2 * n[2] - 1) + d[2] + n[2] - 1, a] = 0.0
    return t


@functools.lru_cache(maxsize=None)
def _attn_v(rid):
    r = attn_row(rid)
    pl = make_plan(r)
    return E.ints(ATTN_B, r["heads"], woff(pl)[-1], r["M"] * _prod(pl["n"]), pl["c_v"], seed=_seed(rid, 3))


def attn_v(r):
    """V: integers in [-3, 3] (q = k = 0)"""
    return _attn_v(r["id"])


def attn_targets(n, roff):
    """per query token t: (its target t + r lies in the window, the target's token index)"""
    c = torch.stack(torch.meshgrid(*[torch.arange(k) for k in n], indexing="ij")).flatten(1).T + torch.tensor(roff)
    inw = ((c >= 0) & (c < torch.tensor(n))).all(1)
    return inw, (c[:, 0] * n[1] + c[:, 1]) * n[2] + c[:, 2]


@functools.lru_cache(maxsize=None)
def _attn_reference(rid, bias):
    r = attn_row(rid)
    pl, M = make_plan(r), r["M"]
    l = _prod(pl["n"])
    idx = O.relative_position_index(pl["n"])
    s = attn_table(r, bias).double()[idx.reshape(-1)].view(l, l, -1).permute(2, 0, 1).repeat(1, M, M)          # (heads, M l, M l): the scores
    top = s.max(-1).values
    sel = (s == top[..., None]).double()               # exp(s - max): 1 at the row's maxima, exp(-128) -> 0 elsewhere
    count = sel.sum(-1)
    total = torch.einsum("hij,bhnjc->bhnic", sel, attn_v(r).double())
    ci = count.long()
    return dict(O=total / count[None, :, None, :, None], lse=top + torch.log(count), count=count, pow2=(ci & (ci - 1)) == 0, total=total, top=top,
                S=torch.einsum("hij,bhnjc->bhnic", sel, attn_v(r).double().abs()))


def attn_reference(r, bias):
    """fp64: O (B, heads, Ntot, M l, c_v); lse, count and pow2 (heads, M l): the row's log-sum-exp, its number of maximal keys, and whether that divisor is a power of two"""
    return _attn_reference(r["id"], bias)
