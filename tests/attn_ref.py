"""fp64 oracle, sharp and shifted soft-max inputs, the case table and fp32 restatements for the paired-window attention CORE: the forward
kernels vx_pwa_attn_fwd_k (csrc/pwa.hip) / the MFMA forward (csrc/pwa_mfma.hip) and the six backward paths behind vx_pwa_attn_bwd.

The oracle restates oracle.window_attention with the bias of oracle.relative_bias on TOKENS -- Q, K (B, heads, Ntot, M l, c_qk), V (B, heads, Ntot, M l, c_v), keys
modality-major, as vx_pwa_attn_fwd takes them; the gather and scatter stay out, so no max-pool kink enters -- and returns O, LSE = logsumexp(s) and, through
autograd for a seeded cotangent dO, dQ, dK, dV and dtable.  With dropout the soft-max weights are multiplied by the restated Philox mask
(oracle.philox.attn_scales, flat (B, heads, Ntot, M l, M l) order) before `@ V`; LSE is unaffected.  It runs in double (ref64) and in single (ref32) and the bound,
the input condition and their constants are those of tests/stable_ref.py:

    max |got - ref64|  <=  FACTOR * max |ref32 - ref64|  +  FLOOR * max |ref64|          input condition: max |ref32 - ref64| <= CAP * max |ref64|

CPU-only at import.  tests/test_attn_ref_cpu.py proves the premise on every case (the condition, ref32 under its own bound, the planted structure, the fp32
restatements of the kernels' arithmetic inside the bound and three wrong forms outside it); tests/test_attn_fp64_gpu.py runs the kernels on the same cases."""
import functools
import math

import torch

import stable_ref as S
from oracle import philox
from oracle import veloxseg_oracle as O

figures, limit, violation, condition = S.figures, S.limit, S.violation, S.condition
NAMES = ("O", "LSE", "dQ", "dK", "dV", "dtable")
SLAB = 64                      # keys per slab of the forward kernels (VX_KV_ROWS)
P_DROP = 0.2
SEED, STEP, SITE = 77, 3, 9    # the {seed, step} pair and the site id (`dstream`) of the dropout cases: the arguments of attn_scales


# ---------------------------------------------------------------------------------------------------------------------- geometries
# id: (grid, big, heads, min_dim_head, C)  ->  l tokens per window and modality, head widths c_qk / c_v (oracle.plan_pwa)
GEOS = {
    "l64c4": ([16, 16, 16], [4, 4, 4], 1, 4, 12),           # 73 windows over three scales
    "l512c8": ([8, 8, 8], [8, 8, 8], 2, 8, 8),              # one window of 512 tokens per head
    "l27c4": ([12, 12, 12], [3, 3, 3], 1, 4, 12),           # 73 windows, ragged chunk
    "l216c4": ([6, 6, 6], [6, 6, 6], 1, 4, 4),              # one window, 14 tiles of 16 tokens, seven 64-key slabs at M = 2
    "l32c4": ([8, 8, 4], [4, 4, 2], 1, 4, 8),               # anisotropic, half a 64-token chunk
    "l125c8": ([10, 10, 10], [5, 5, 5], 2, 8, 16),
    "l64c16v32": ([4, 4, 4], [4, 4, 4], 4, 16, 128),
    "l64c8v16": ([8, 8, 8], [4, 4, 4], 2, 8, 64),
    "l27c16v32": ([3, 3, 3], [3, 3, 3], 4, 16, 128),
    "l64c2v4": ([4, 4, 4], [4, 4, 4], 1, 2, 4),             # head widths only the VALU dispatch instantiates
    "l27c32": ([3, 3, 3], [3, 3, 3], 1, 32, 32),            # the same, the widest pair
    "l27m3": ([6, 6, 6], [3, 3, 3], 1, 4, 16),              # carries M = 3
}


def _prod(v):
    return int(v[0]) * int(v[1]) * int(v[2])


@functools.lru_cache(maxsize=None)
def dims(geo, M, B):
    """the window geometry of a case as plain numbers (+ the plan of oracle.plan_pwa under "pl")"""
    grid, big, heads, mdh, C = GEOS[geo]
    pl = O.plan_pwa(grid, big, [1, 1, 1], 2, heads, mdh, C)
    n = pl["n"]
    l = _prod(n)
    return dict(pl=pl, grid=grid, n=n, l=l, ML=M * l, M=M, B=B, heads=heads, Nt=sum(_prod(w) for w in pl["nwin"]), cq=pl["c_qk"], cv=pl["c_v"],
                Tsz=(2 * n[0] - 1) * (2 * n[1] - 1) * (2 * n[2] - 1))


def elements(geo, M, B):
    d = dims(geo, M, B)
    return B * d["heads"] * d["Nt"] * d["ML"] ** 2


# ---------------------------------------------------------------------------------------------------------------------- families
FAMILIES = ("plain", "sharp", "one_hot", "bias_sharp", "offset", "ramp_up", "ramp_down", "tiny", "dO_big", "dO_small", "v_outlier", "q_outlier")
CORE = ("plain", "sharp", "ramp_up")
# `q_outlier`: one query row of every window x Q_OUTLIER.  That row's soft-max is one-hot with logits of Q_OUTLIER x a few units, and its large dS carries the
# rounding of the logits into dK.  Decided on the CPU alone: at 1e3 the fp32 ORACLE resolves dK to 1.04e-4 M on the c 16 / 32 row, outside the input condition
# (CAP = 1e-4); at 300 the condition holds (worst 3.3e-5 M) but restatement (b) -- the kernels' own formula in plain fp32 -- uses 1.06 of the bound on dV of that row,
# so the family would test the yardstick, not the kernel; at 100 the oracle is at 5.1e-6 M, (b) uses at most 0.77 of its bound, and the row still sets the
# chunk-maximum scale of the f16 pieces 100 x above its neighbours.
Q_OUTLIER = 100.0


def _seed(*parts):
    return S._seed("attn", *parts)


@functools.lru_cache(maxsize=None)
def inputs(geo, M, B, family):
    """{"q", "k", "v", "table", "dO"}: fp32 CPU tensors, never modified.  Every family transforms the same seeded randn tokens of its geometry"""
    d = dims(geo, M, B)
    h, Nt, ML, cq, cv = d["heads"], d["Nt"], d["ML"], d["cq"], d["cv"]
    s = _seed(geo, M, B)
    q, k = S.randn(B, h, Nt, ML, cq, seed=s), S.randn(B, h, Nt, ML, cq, seed=s + 1)
    v, dO = S.randn(B, h, Nt, ML, cv, seed=s + 2), S.randn(B, h, Nt, ML, cv, seed=s + 3)
    table = S.randn(d["Tsz"], h, seed=s + 4, scale=0.5)
    if family == "sharp":
        q = q * 10.0
    elif family == "one_hot":
        q = q * 100.0
    elif family == "bias_sharp":
        table = table * 40.0
    elif family == "offset":
        table = table + 100.0
    elif family in ("ramp_up", "ramp_down"):
        j = torch.arange(ML, dtype=torch.float32)
        ramp = 6.0 * (j if family == "ramp_up" else (ML - 1) - j) / ML
        k = 0.1 * k + ramp.view(1, 1, 1, ML, 1)
        q = q.abs() + 1.0
    elif family == "tiny":
        q, v = q * 1e-4, v * 1e4
    elif family == "dO_big":
        dO, v = dO * 1e4, v * 30.0
    elif family == "dO_small":
        dO, v = dO * 1e-4, v * 0.03
    elif family in ("v_outlier", "q_outlier"):
        at = torch.randint(0, ML, (B, h, Nt), generator=S._gen(s + 5))
        sel = torch.zeros(B, h, Nt, ML, 1).scatter_(3, at.view(B, h, Nt, 1, 1), 1.0).bool()
        if family == "v_outlier":
            v = torch.where(sel, torch.full_like(v, 1e4), v)
        else:
            q = torch.where(sel, q * Q_OUTLIER, q)
    elif family != "plain":
        raise KeyError(family)
    return dict(q=q, k=k, v=v, table=table, dO=dO)


@functools.lru_cache(maxsize=None)
def mask(geo, M, B, p):
    """the restated keep mask x 1 / (1 - p) of the attention site, (B, heads, Ntot, M l, M l) fp32; None without dropout"""
    if not p > 0:
        return None
    d = dims(geo, M, B)
    shp = (B, d["heads"], d["Nt"], d["ML"], d["ML"])
    return philox.attn_scales(SEED, STEP, SITE, math.prod(shp), p).view(shp)


# ---------------------------------------------------------------------------------------------------------------------- the oracle
def _bias_index(d):
    return O.relative_position_index(d["n"])[:d["l"], :d["l"]].reshape(-1)


def oracle(inp, d, dtype, keep=None):
    """oracle.window_attention + oracle.relative_bias on tokens in `dtype`, with LSE and the gradients for the cotangent dO"""
    q, k, v, table = (inp[x].detach().to(dtype).requires_grad_(True) for x in ("q", "k", "v", "table"))
    l, M = d["l"], d["M"]
    bias = O.relative_bias(table, O.relative_position_index(d["n"]), l)                      # (heads, l, l)
    s = torch.einsum("bhnic,bhnjc->bhnij", q, k) / (q.shape[-1] ** 0.5)
    s = s + bias.repeat(1, M, M)[None, :, None]
    w = torch.softmax(s, -1)
    if keep is not None:
        w = w * keep.to(dtype)
    out = torch.einsum("bhnij,bhnjc->bhnic", w, v)
    g = torch.autograd.grad(out, [q, k, v, table], inp["dO"].to(dtype))
    return dict(O=out.detach(), LSE=torch.logsumexp(s.detach(), -1), dQ=g[0], dK=g[1], dV=g[2], dtable=g[3])


@functools.lru_cache(maxsize=None)
def case(geo, M, B, family, p=0.0):
    """inputs, dims, mask and both references of one case (computed once; rows that differ only in their knobs share it)"""
    d, inp, keep = dims(geo, M, B), inputs(geo, M, B, family), mask(geo, M, B, p)
    return dict(d=d, inp=inp, keep=keep, r64=oracle(inp, d, torch.float64, keep), r32=oracle(inp, d, torch.float32, keep))


def p_max(c):
    """(B, heads, Ntot, M l): the largest soft-max weight of every row, from the fp64 scores"""
    d, inp = c["d"], c["inp"]
    return torch.exp(scores(inp, d, torch.float64) - c["r64"]["LSE"][..., None]).max(-1).values


def scores(inp, d, dtype=torch.float32):
    """(q * scale) . k + bias as the fp32 kernels form them (the scale is folded into q)"""
    q, k = inp["q"].to(dtype), inp["k"].to(dtype)
    scale = torch.tensor(1.0 / math.sqrt(d["cq"]), dtype=dtype)
    bias = O.relative_bias(inp["table"].to(dtype), O.relative_position_index(d["n"]), d["l"])
    return torch.einsum("bhnic,bhnjc->bhnij", q * scale, k) + bias.repeat(1, d["M"], d["M"])[None, :, None]


# ---------------------------------------------------------------------------------------------------------------------- fp32 restatements (CPU premise only)
LOG2E = 1.4426950408889634


def exp_fast(x):
    """the device's fast exponential: exp2(x * log2 e), the product rounded to fp32"""
    return torch.exp2(x * torch.tensor(LOG2E, dtype=x.dtype))


def forward_online(inp, d, splits=1, keep=None, rescale=True, exp=torch.exp):
    """(a) the forward of vx_pwa_attn_fwd_k in fp32: split t of `splits` walks the 64-key slabs t, t + splits, .. with a running maximum, rescaling its sum and
    its accumulator at every slab; the partial states are then merged with exp(m_t - m).  `rescale` False = wrong form (f): the states are merged as they are"""
    s = scores(inp, d)
    v = inp["v"]
    ML = d["ML"]
    nslab = -(-ML // SLAB)
    splits = min(splits, nslab)
    states = []
    for t in range(splits):
        m = torch.full(s.shape[:-1], -float("inf"))
        lsum = torch.zeros(s.shape[:-1])
        acc = torch.zeros(s.shape[:-1] + (d["cv"],))
        for j in range(t, nslab, splits):
            sl = slice(j * SLAB, min(ML, (j + 1) * SLAB))
            mn = torch.maximum(m, s[..., sl].max(-1).values)
            alpha = exp(m - mn)
            p = exp(s[..., sl] - mn[..., None])
            lsum = lsum * alpha + p.sum(-1)
            pd = p if keep is None else p * keep[..., sl]
            acc = acc * alpha[..., None] + torch.einsum("bhnij,bhnjc->bhnic", pd, v[..., sl, :])
            m = mn
        states.append((m, lsum, acc))
    m, lsum, acc = states[0]
    for m2, l2, a2 in states[1:]:
        mn = torch.maximum(m, m2)
        a1, b2 = (exp(m - mn), exp(m2 - mn)) if rescale else (torch.ones_like(m), torch.ones_like(m))
        lsum, acc, m = lsum * a1 + l2 * b2, acc * a1[..., None] + a2 * b2[..., None], mn
    return dict(O=acc / lsum[..., None], LSE=m + torch.log(lsum))


def forward_no_max(inp, d):
    """wrong form (d): exp(s) without the maximum subtracted"""
    p = torch.exp(scores(inp, d))
    return dict(O=torch.einsum("bhnij,bhnjc->bhnic", p, inp["v"]) / p.sum(-1, keepdim=True), LSE=torch.log(p.sum(-1)))


def _pow2(mx, target):
    """the power of two that brings `mx` into [2^(target-1), 2^target) (1 where mx == 0), as vx_a_exp"""
    e = target - (torch.floor(torch.log2(mx.double().clamp_min(1e-300))) + 1)
    return torch.where(mx > 0, torch.exp2(e.clamp(-60, 60)), torch.ones_like(e)).float()


def chunk_scale(x, target, d):
    """(B, heads, Ntot, M l, 1): per token the power of two 2^e that brings the largest |x| of its CHUNK -- 64 consecutive tokens of every modality of the window, the
    query chunk / key block of vx_pwa_attn_bwd1h_k -- into [2^(target-1), 2^target)"""
    M, l = d["M"], d["l"]
    LP = -(-l // 64) * 64
    y = torch.zeros(x.shape[:3] + (M, LP, x.shape[-1]))
    y[..., :l, :] = x.view(x.shape[:3] + (M, l, x.shape[-1]))
    mx = y.view(x.shape[:3] + (M, LP // 64, 64, x.shape[-1])).abs().amax((3, 5, 6), keepdim=True)
    sc = _pow2(mx, target).expand(x.shape[:3] + (M, LP // 64, 64, 1))
    return sc.reshape(x.shape[:3] + (M, LP, 1))[..., :l, :].reshape(x.shape[:3] + (M * l, 1))


def split(y, n):
    """y as the sum of n in {1, 2} fp16 pieces, hi = fp16(y), lo = fp16(y - hi): the exact fp32 value the MFMA sees"""
    hi = y.half().float()
    return hi + (y - hi).half().float() if n == 2 else hi


def pieces(x, sc, n):
    return split(x * sc, n) / sc


def backward_restated(inp, d, fwd, keep=None, n_pieces=0, exp=torch.exp):
    """(b) the backward as the kernels form it, in fp32: p = exp(s - lse) from the fp32 LSE of the forward, delta = sum dO O, dS = p (dP - delta);
    n_pieces = 2: (c) as vx_pwa_attn_bwd1h_k feeds the f16 matrix pipe: q, k (scaled below 2^10 by their chunk's maximum), v, dO (below 2^5) enter every product as two
    fp16 pieces, and so do p x mask (unscaled) into dV and dS (in the units of its dO and V scales) into dQ / dK; delta stays fp32.  1: wrong form (e), one piece"""
    q, k, v, dO = inp["q"], inp["k"], inp["v"], inp["dO"]
    delta = (dO * fwd["O"]).sum(-1)
    if n_pieces:
        sv, sd = chunk_scale(v, 5, d), chunk_scale(dO, 5, d)
        q, k, v, dO = pieces(q, chunk_scale(q, 10, d), n_pieces), pieces(k, chunk_scale(k, 10, d), n_pieces), pieces(v, sv, n_pieces), pieces(dO, sd, n_pieces)
    scale = torch.tensor(1.0 / math.sqrt(d["cq"]))
    if n_pieces:                                                                               # exp2(fma(S, c, bias2 - lse2)): log2(e) folded into c, the staged bias and lse
        L = torch.tensor(LOG2E)
        bias2 = O.relative_bias(inp["table"] * L, O.relative_position_index(d["n"]), d["l"]).repeat(1, d["M"], d["M"])[None, :, None]
        p = torch.exp2(torch.einsum("bhnic,bhnjc->bhnij", q, k) * (scale * L) + (bias2 - (fwd["LSE"] * L)[..., None]))
    else:
        p = exp(scores(inp, d) - fwd["LSE"][..., None])
    dP = torch.einsum("bhnic,bhnjc->bhnij", dO, v)
    pd = p
    if keep is not None:
        dP, pd = dP * keep, p * keep
    dS = p * (dP - delta[..., None])
    dSm = dS                                                                                   # (the bias gradient sums the fp32 dS)
    if n_pieces:
        u = sd * sv.transpose(-1, -2)                                                          # (.., M l, M l): the units of dS at (query chunk, key block)
        pd, dS = split(pd, n_pieces), split(dS * u, n_pieces) / u
    l, M, h = d["l"], d["M"], d["heads"]
    dbias = dSm.sum((0, 2)).view(h, M, l, M, l).sum((1, 3))                                    # (heads, l, l)
    dtable = torch.zeros(d["Tsz"], h).index_add_(0, _bias_index(d), dbias.reshape(h, l * l).t().contiguous())
    return dict(dQ=torch.einsum("bhnij,bhnjc->bhnic", dS, k) * scale, dK=torch.einsum("bhnij,bhnic->bhnjc", dS, q) * scale,
                dV=torch.einsum("bhnij,bhnic->bhnjc", pd, dO), dtable=dtable)


# ---------------------------------------------------------------------------------------------------------------------- the case table
# knob: (setter, default)
KNOBS = {"mfma": ("vx_pwa_attn_set_mfma", 3), "split": ("vx_pwa_attn_set_split", 0), "fused_bwd": ("vx_pwa_attn_set_fused_bwd", 1),
         "f16_bwd": ("vx_pwa_attn_set_f16_bwd", 1), "f16_bwd_ragged": ("vx_pwa_attn_set_f16_bwd_ragged", 1), "f16_bwd_m1": ("vx_pwa_attn_set_f16_bwd_m1", 0),
         "valu_bits": ("vx_pwa_attn_set_valu_bits", 0)}
# backward path -> the answers of (vx_pwa_attn_bwd1h_ok, vx_pwa_attn_bwd1_ok, vx_pwa_attn_mfma_ok & 2) that select it in vx_pwa_attn_bwd
BWD_PATHS = {"f16_aligned": (1, None, None), "f16_ragged": (1, None, None), "f16_m1": (1, None, None), "mfma1": (0, 1, None), "mfma2": (0, 0, 2), "valu": (0, 0, 0)}
FWD_PATHS = {"mfma": 1, "valu": 0}                                                          # vx_pwa_attn_mfma_ok & 1


def _row(id, geo, M, B, path, fwd, knobs, branch, families=CORE, drop=(), nofold=False):
    grid, big, heads, mdh, C = GEOS[geo]
    return dict(id=id, geo=geo, grid=grid, big=big, heads=heads, mdh=mdh, C=C, M=M, B=B, path=path, fwd=fwd, knobs=knobs, branch=branch, families=tuple(families),
                drop=tuple(drop), nofold=nofold)


_F32 = {"mfma": 11, "f16_bwd": 0}
_DROP = ("plain", "sharp")
ROWS = [
    # ---- backward on the f16 pipe (default knobs where the windows are aligned); forward MFMA where l % 64 == 0
    _row("f16-l64c4", "l64c4", 2, 2, "f16_aligned", "mfma", {}, "64-token windows, c 4: one query chunk per window", FAMILIES, _DROP, True),
    _row("f16-l512c8", "l512c8", 2, 1, "f16_aligned", "mfma", {}, "512-token windows, c 8: eight query chunks, the scales of Q / dO change per chunk"),
    _row("f16r-l27c4", "l27c4", 2, 2, "f16_ragged", "valu", {"f16_bwd_ragged": 2}, "27 tokens in a padded 64-token chunk", FAMILIES, _DROP, True),
    _row("f16r-l216c4", "l216c4", 2, 3, "f16_ragged", "valu", {"f16_bwd_ragged": 2}, "216 tokens: three full chunks and a ragged fourth"),
    _row("f16r-l32c4", "l32c4", 2, 2, "f16_ragged", "valu", {"f16_bwd_ragged": 2}, "32 tokens, anisotropic window"),
    _row("f16r-l125c8", "l125c8", 2, 1, "f16_ragged", "valu", {"f16_bwd_ragged": 2}, "125 tokens, c 8, two heads"),
    _row("f16m1-l64c4", "l64c4", 1, 2, "f16_m1", "mfma", {"f16_bwd_m1": 1}, "one modality: the MF = 1 instance", FAMILIES, _DROP, True),
    # ---- backward on the fp32 one-pass MFMA kernel for every geometry it covers
    _row("mfma1-l64c16v32", "l64c16v32", 2, 2, "mfma1", "mfma", _F32, "c 16 / 32, one key block", FAMILIES, _DROP, True),
    _row("mfma1-l64c8v16", "l64c8v16", 2, 2, "mfma1", "mfma", _F32, "c 8 / 16, two window scales"),
    _row("mfma1-l27c16v32", "l27c16v32", 2, 2, "mfma1", "valu", _F32, "27 tokens: padded 16-token tiles"),
    _row("mfma1-few-l64c8v16", "l64c8v16", 1, 2, "mfma1", "mfma", _F32, "M = 1, few windows: split queries, dK / dV summed with float atomics"),
    _row("mfma1-few-l64c16v32", "l64c16v32", 1, 2, "mfma1", "mfma", _F32, "M = 1, few windows, c 16 / 32"),
    _row("mfma1-l216c4", "l216c4", 2, 3, "mfma1", "valu", _F32, "14 key tiles = four key blocks: dQ summed with float atomics"),
    # ---- the two-kernel MFMA backward
    _row("mfma2-l64c4", "l64c4", 2, 2, "mfma2", "mfma", {"mfma": 5}, "64-token windows", FAMILIES, _DROP, True),
    _row("mfma2-l512c8", "l512c8", 2, 1, "mfma2", "mfma", {"mfma": 5}, "512-token windows"),
    _row("mfma2-l64c16v32", "l64c16v32", 2, 2, "mfma2", "mfma", {"mfma": 5}, "c 16 / 32"),
    # ---- VALU forward and backward: one launch / two launches x the key split (clamped to the slab count: 4 needs l = 216 at M = 2)
    _row("valu-l27c4", "l27c4", 2, 2, "valu", "valu", {"mfma": 0}, "27 tokens, one ragged slab, automatic split", FAMILIES, _DROP, True),
    _row("valu-l216c4-s4", "l216c4", 2, 3, "valu", "valu", {"mfma": 0, "split": 4}, "seven slabs in four partial states, one launch", FAMILIES),
    _row("valu-l216c4-s4-two", "l216c4", 2, 3, "valu", "valu", {"mfma": 0, "split": 4, "fused_bwd": 0}, "seven slabs in four partial states, two launches"),
    _row("valu-l216c4-s2", "l216c4", 2, 3, "valu", "valu", {"mfma": 0, "split": 2}, "two partial states, one launch"),
    _row("valu-l216c4-s1-two", "l216c4", 2, 3, "valu", "valu", {"mfma": 0, "split": 1, "fused_bwd": 0}, "one state over seven slabs, two launches"),
    _row("valu-l64c4-s1", "l64c4", 2, 2, "valu", "valu", {"mfma": 0, "split": 1}, "64 tokens, two slabs in one state, one launch"),
    _row("valu-l64c4-s2-two", "l64c4", 2, 2, "valu", "valu", {"mfma": 0, "split": 2, "fused_bwd": 0}, "64 tokens, one slab per state, two launches"),
    _row("valu-l64c4-bits", "l64c4", 2, 2, "valu", "valu", {"mfma": 0, "valu_bits": 1}, "the backward reads the forward's keep bits", (), _DROP),
    _row("valu-l27c4-two", "l27c4", 2, 2, "valu", "valu", {"mfma": 0, "fused_bwd": 0}, "27 tokens, two launches"),
    _row("valu-l64c2v4-s2", "l64c2v4", 2, 2, "valu", "valu", {"mfma": 0, "split": 2}, "c 2 / 4: VALU dispatch only"),
    _row("valu-l64c2v4-two", "l64c2v4", 2, 2, "valu", "valu", {"mfma": 0, "split": 1, "fused_bwd": 0}, "c 2 / 4, two launches"),
    _row("valu-l27c32", "l27c32", 2, 2, "valu", "valu", {"mfma": 0}, "c 32 / 32: VALU dispatch only"),
    _row("valu-l27m3", "l27m3", 3, 2, "valu", "valu", {"mfma": 0}, "three modalities: 81 keys, slabs of 20 tokens per modality in the dQ pass"),
    _row("valu-l27m3-two", "l27m3", 3, 2, "valu", "valu", {"mfma": 0, "split": 2, "fused_bwd": 0}, "three modalities, two states, two launches"),
]
ROW = {r["id"]: r for r in ROWS}
# (row id, family, p_drop) of every GPU case
CASES = [(r["id"], f, 0.0) for r in ROWS for f in r["families"]] + [(r["id"], f, P_DROP) for r in ROWS for f in r["drop"]]
CASE_IDS = [f"{rid}-{f}{'-drop' if p else ''}" for rid, f, p in CASES]
# the distinct references behind them
REFS = sorted({(ROW[rid]["geo"], ROW[rid]["M"], ROW[rid]["B"], f, p) for rid, f, p in CASES})
REF_IDS = [f"{g}-M{M}-B{B}-{f}{'-drop' if p else ''}" for g, M, B, f, p in REFS]
MAX_ELEMENTS = 4 << 20


def row_case(rid, family, p=0.0):
    r = ROW[rid]
    return case(r["geo"], r["M"], r["B"], family, p)
