"""fp64 oracles, ill-conditioned inputs and the error bound for the NON-LINEAR reduction kernels: InstanceNorm (csrc/norm.hip), channels-first
LayerNorm, the segmentation / reconstruction / Gram loss (csrc/loss.hip, csrc/loss_ds.hip), the Gram matrix and trilinear up-sampling.

The yardstick of a case is the error of the fp32 ORACLE on the very same input.  With r64 / r32 the functions of oracle/veloxseg_oracle.py run in double / single
precision (outputs and, through autograd, every gradient) and M = max |r64|, a compared tensor `got` must satisfy

    max |got - r64|  <=  FACTOR * max |r32 - r64|  +  FLOOR * M            FACTOR = 8, FLOOR = 16 * 2^-24

An input that is hard for every fp32 implementation loosens its own bound, an easy one tightens it; FACTOR is three bits for summation order, fma contraction and
device against host erff / expf; FLOOR covers tensors the CPU oracle happens to get exactly (M == 0: the kernel must return exact zeros).  So that the yardstick can
never hide a kernel bug, every row also has to satisfy the INPUT CONDITION max |r32 - r64| <= CAP * M with CAP = 1e-4 (tests/test_stable_ref_cpu.py checks every row).

This module is CPU-only at import.  The case tables are plain data; every row names the dispatch branch it is there for.  tests/test_stable_ref_cpu.py proves the
premise (the condition, that r32 passes its own bound, and that the LayerNorm bound separates the two-sweep statistics from the one-sweep pivot form, both restated
below from their formulas); tests/test_norm_loss_fp64_gpu.py runs the kernels on the same rows."""
import functools

import torch

from oracle import veloxseg_oracle as O

FACTOR = 8.0
FLOOR = 16.0 * 2.0 ** -24
CAP = 1e-4
# per-operator factors under the measured-ratio rule of DESIGN.md sections 32 and 36: the next power of two at or above twice the ratio max |got - ref64| / max |ref32 - ref64|
# measured on an MI355X, granted only where a CPU restatement of the path's own arithmetic shows a ratio of the same size on the same row (tests/attn_ref.py restatement
# (c): two fp16 pieces carry 22 mantissa bits).  The norm and loss operators of section 32 need none.
FACTORS = {
    "attn_bwd_f16_aligned": 64.0,       # measured 18.67 (l = 512, c 8, `ramp_up`, dQ); restated 17.77 on the same row
    "attn_bwd_f16_ragged": 64.0,        # measured 27.45 (l = 27, c 4, `q_outlier`, dV); restated 20.12 on the same row, 21.90 at its largest (`ramp_up`, dQ)
    "attn_bwd_f16_m1": 64.0,            # measured 23.84 (l = 64, c 4, M = 1, `one_hot`, dV); restated 15.18 on the same row, 21.44 at its largest (`ramp_up`, dQ)
}

IN_EPS, LN_EPS = 1e-5, 1e-6


# ---------------------------------------------------------------------------------------------------------------------- oracles and the bound
def _run(fn, tensors, params, cots, dtype):
    ts = [t.detach().to(dtype).requires_grad_(True) for t in tensors]
    ps = [p.detach().to(dtype).requires_grad_(True) for p in params]
    outs = fn(*ts, *ps)
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    grads = torch.autograd.grad(outs, ts + ps, [c.to(dtype) for c in cots], allow_unused=False)
    res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
    res.update({f"d_in{i}": g for i, g in enumerate(grads[:len(ts)])})
    res.update({f"d_par{i}": g for i, g in enumerate(grads[len(ts):])})
    return res


def ref64(fn, tensors, params, cots):
    """outputs and all gradients of the oracle function `fn(*tensors, *params)` on .double() copies: {"out0".., "d_in0".., "d_par0"..}"""
    return _run(fn, tensors, params, cots, torch.float64)


def ref32(fn, tensors, params, cots):
    return _run(fn, tensors, params, cots, torch.float32)


def figures(got, r64, r32):
    """(max |got - r64|, max |r32 - r64|, M) in fp64; a NaN or Inf in `got` gives an infinite error"""
    r = r64.detach().double().cpu().reshape(-1)
    g = got.detach().double().cpu().reshape(-1)
    s = r32.detach().double().cpu().reshape(-1)
    assert g.numel() == r.numel() == s.numel(), (g.numel(), r.numel(), s.numel())
    err = (g - r).abs()
    e = float(err.max()) if bool(torch.isfinite(g).all()) else float("inf")
    return e, float((s - r).abs().max()), float(r.abs().max())


def limit(e32, M, op=None):
    return FACTORS.get(op, FACTOR) * e32 + FLOOR * M


def violation(got, r64, r32, what, op=None):
    """None, or the report of a tensor that misses the bound"""
    e, e32, M = figures(got, r64, r32)
    lim = limit(e32, M, op)
    if e <= lim:
        return None
    ratio = e / e32 if e32 > 0 else float("inf")
    return f"{what}: max|got-ref64| = {e:.3e} > bound {lim:.3e} (max|ref32-ref64| = {e32:.3e}, M = {M:.3e}, ratio {ratio:.1f})"


def check(got, r64, r32, what, op=None):
    m = violation(got, r64, r32, what, op)
    assert m is None, m


def condition(r64, r32):
    """the input condition of one compared tensor: (holds, max |r32 - r64| / M)"""
    _, e32, M = figures(r32, r64, r32)
    return e32 <= CAP * M, (e32 / M if M > 0 else 0.0)


# ---------------------------------------------------------------------------------------------------------------------- generators
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def randn(*shape, seed, scale=1.0):
    return torch.randn(tuple(int(s) for s in shape), generator=_gen(seed)) * scale


def _quarter_steps(n, seed):
    """n multiples of 0.25 in [-2, 2]: sums of up to 2^20 of them are exact in fp32, so a `constant` row has mean == value and variance == 0 exactly"""
    return torch.randint(-8, 9, (int(n),), generator=_gen(seed)).float() * 0.25


NORM_FAMILIES = ("plain", "offset", "scale_up", "scale_down", "constant", "spike")
IN_FAMILIES = NORM_FAMILIES
LN_FAMILIES = NORM_FAMILIES + ("first_outlier", "last_outlier")


def family_rows(family, R, N, seed, offset, sigma=1.0):
    """(R, N) fp32: R rows of N elements, the family applied along each row; `offset` in units of sigma for "offset", `sigma` scales "plain" and "offset" only"""
    x = randn(R, N, seed=seed)
    if family == "plain":
        return x * sigma
    if family == "offset":
        return (x + offset) * sigma
    if family == "scale_up":
        return x * 1e4
    if family == "scale_down":                        # variance 1e-8: below both eps
        return x * 1e-4
    if family == "constant":
        return _quarter_steps(R, seed + 1).view(R, 1).expand(R, N).contiguous()
    if family == "spike":
        x = x * 1e-2
        at = torch.randint(0, N, (R,), generator=_gen(seed + 2))
        x[torch.arange(R), at] = 1e4
        return x
    if family == "first_outlier":
        x[:, 0] += 1000.0
        return x
    if family == "last_outlier":
        x[:, -1] += 1000.0
        return x
    raise KeyError(family)


def _seed(*parts):
    s = "/".join(str(p) for p in parts)
    return sum(ord(c) * (i + 1) for i, c in enumerate(s)) % 100003


# ---------------------------------------------------------------------------------------------------------------------- InstanceNorm
IN_VARIANTS = ((1, False, False), (2, False, True), (3, True, True))          # (inputs, GELU, residual)
IN_OFFSET = 1000.0                                                             # in units of sigma


def _in_shape(id, sp, branch, families=None, sigma=1.0, offset=IN_OFFSET):
    return dict(id=id, sp=tuple(sp), branch=branch, families=families or IN_FAMILIES, sigma=sigma, offset=offset)


# A row of TWO elements normalises to +-sqrt(var / (var + eps)) whatever its values, and its gradient is proportional to eps / (var + eps): once var is far above
# eps that gradient is the difference of two nearly equal numbers and NO fp32 evaluation resolves it (fp32 oracle at unit variance: 2e-3 M; at variance 1e8 or with
# a 1e4 spike: pure noise).  The input condition therefore admits V = 2 only where eps takes part: sigma = 3e-3 (var ~ eps) for `plain` and `offset`, with the offset
# shrunk to 30 sigma (at 1000 sigma the mean's own rounding is 1e-4 of the spread), `scale_down` and `constant`; `scale_up` and `spike` have no well-conditioned
# two-element form.
IN_V2_FAMILIES = ("plain", "offset", "scale_down", "constant")


IN_SHAPES = [
    _in_shape("v2", (1, 1, 2), "row kernel R=1, the smallest legal row", families=IN_V2_FAMILIES, sigma=3e-3, offset=30.0),
    _in_shape("v255", (3, 5, 17), "row kernel R=1, ragged last slot"),
    _in_shape("v257", (1, 1, 257), "row kernel R=2, ragged last slot"),
    _in_shape("v1000", (10, 10, 10), "row kernel R=4"),
    _in_shape("v2049", (1, 3, 683), "row kernel R=16 (9 slots), ragged"),
    _in_shape("v4096", (16, 16, 16), "row kernel R=16, full"),
    _in_shape("v4097", (1, 17, 241), "long rows S=1, odd V: scalar and 16-byte blocks in one launch, tail elements"),
    _in_shape("v4800", (20, 20, 12), "long rows S=1, aligned"),
    _in_shape("v8381", (17, 17, 29), "long rows S=2, odd V"),
    _in_shape("v8448", (16, 16, 33), "long rows S=2, aligned"),
]
IN_B, IN_C = 2, 3                                                              # B C = 6 rows: bc V mod 4 takes several values at odd V
IN_ROWS = [dict(id=f"{s['id']}-n{n}{'g' if act else ''}{'r' if res else ''}-{fam}", shape=s["id"], sp=s["sp"], branch=s["branch"], n=n, act=act, res=res, family=fam,
                sigma=s["sigma"], offset=s["offset"])
           for s in IN_SHAPES for (n, act, res) in IN_VARIANTS for fam in s["families"]]


def in_case(row):
    """tensors = the n inputs (+ the residual), the oracle function and the cotangent"""
    shp = (IN_B, IN_C) + row["sp"]
    V = shp[2] * shp[3] * shp[4]
    s = _seed("in", row["id"])
    n, act, res = row["n"], row["act"], row["res"]
    ts = [family_rows(row["family"], IN_B * IN_C, V, s + 10 * k, row["offset"], row["sigma"]).view(shp) for k in range(n)]
    if res:
        ts.append(randn(*shp, seed=s + 77))

    def fn(*t):
        out = t[n] if res else 0
        for y in t[:n]:
            z = O.instnorm(y, IN_EPS)
            out = out + (O.gelu(z) if act else z)
        return out

    return dict(fn=fn, tensors=ts, params=[], cots=[randn(*shp, seed=s + 99)])


# ---------------------------------------------------------------------------------------------------------------------- LayerNorm
LN_OFFSET = 100.0
LN_SHAPES = [
    dict(id="t_c16", shape=(2, 16, 4, 6, 8), path="thread", branch="thread per voxel, C < 64"),
    dict(id="t_c32", shape=(1, 32, 5, 7, 9), path="thread", branch="thread per voxel, C < 64, odd volume"),
    dict(id="t_c64_big", shape=(1, 64, 17, 32, 32), path="thread", branch="thread per voxel, C >= 64 with B V > 16384"),
    dict(id="l16_c128", shape=(2, 128, 4, 4, 4), path="lanes16", branch="16 lanes per voxel"),
    dict(id="l16_c100", shape=(2, 100, 2, 3, 3), path="lanes16", branch="16 lanes per voxel, C no multiple of 16, partly filled block"),
    dict(id="l16_c64", shape=(1, 64, 3, 5, 2), path="lanes16", branch="16 lanes per voxel, smallest C"),
    dict(id="l64_c1024", shape=(2, 1024, 2, 2, 2), path="lanes64", branch="64 lanes per voxel"),
    dict(id="l64_c256", shape=(3, 256, 5, 7, 9), path="lanes64", branch="64 lanes per voxel, B V = 945 (last block partly filled)"),
    dict(id="l64_c300", shape=(1, 300, 3, 3, 3), path="lanes64", branch="64 lanes per voxel, C no multiple of 64"),
]
LN_ROWS = [dict(id=f"{s['id']}-{fam}", shape=s["shape"], path=s["path"], branch=s["branch"], family=fam) for s in LN_SHAPES for fam in LN_FAMILIES]


def ln_path(B, C, V):
    """the launcher's choice (csrc/norm.hip: vx_ln_use_lanes / vx_ln_wide_lanes)"""
    if B * V <= 16384 and C >= 64:
        return "lanes64" if (B * V <= 1024 and C >= 256) else "lanes16"
    return "thread"


def ln_case(row):
    shp = row["shape"]
    B, C = shp[:2]
    V = shp[2] * shp[3] * shp[4]
    s = _seed("ln", row["id"])
    x = family_rows(row["family"], B * V, C, s, LN_OFFSET).view(B, V, C).permute(0, 2, 1).contiguous().view(shp)
    gamma, beta = 1.0 + 0.2 * randn(C, seed=s + 1), 0.2 * randn(C, seed=s + 2)
    return dict(fn=lambda x, w, b: O.layernorm_cf(x, w, b, LN_EPS), tensors=[x], params=[gamma, beta], cots=[randn(*shp, seed=s + 3)])


# ... the two ways to form the per-voxel statistics, restated in fp32 from their formulas with the kernels' three summation shapes (no fma; torch rounds every
# element-wise operation to fp32): `serial` = one thread walks the channels in order; `lanes16` / `lanes64` = lane l sums channels l, l + L, .. in order, then the
# lanes meet in a butterfly (lane ^= L/2, .., 1)
def _sum_shape(terms, path):
    """terms: (C, N) fp32 -> (N,) sums in the order of the path"""
    C, N = terms.shape
    if path == "thread":
        s = torch.zeros(N)
        for c in range(C):
            s = s + terms[c]
        return s
    L = 16 if path == "lanes16" else 64
    K = -(-C // L)
    pad = torch.zeros(K * L, N)
    pad[:C] = terms
    pad = pad.view(K, L, N)
    lanes = torch.zeros(L, N)
    for k in range(K):
        take = min(L, C - k * L)                       # (a lane whose channel is past C adds nothing)
        lanes[:take] = lanes[:take] + pad[k, :take]
    idx = torch.arange(L)
    o = L // 2
    while o > 0:
        lanes = lanes + lanes[idx ^ o]
        o //= 2
    return lanes[0]


def ln_restated(x, gamma, beta, form, path, eps=LN_EPS):
    """channels-first LayerNorm in fp32 with statistics by `form`: "pivot" = one sweep of d = x - x[0]: mean = x[0] + mean(d), var = mean(d^2) - mean(d)^2;
    "two_sweep" = mean, then mean of the squares centred on it"""
    shp = x.shape
    B, C = shp[:2]
    xc = x.float().reshape(B, C, -1).permute(1, 0, 2).reshape(C, -1)          # (C, B V)
    fC = torch.tensor(float(C))
    if form == "pivot":
        d = xc - xc[0:1]
        md = _sum_shape(d, path) / fC
        var = _sum_shape(d * d, path) / fC - md * md
        var = torch.clamp(var, min=0.0)
        u = xc[0] + md
    elif form == "two_sweep":
        u = _sum_shape(xc, path) / fC
        d = xc - u
        var = _sum_shape(d * d, path) / fC
    else:
        raise KeyError(form)
    r = 1.0 / torch.sqrt(var + torch.tensor(eps))
    out = gamma.float().view(C, 1) * ((xc - u) * r) + beta.float().view(C, 1)
    return out.view(C, B, -1).permute(1, 0, 2).reshape(shp)


# ---------------------------------------------------------------------------------------------------------------------- loss
LOSS_FAMILIES = ("plain", "confident_right", "confident_wrong", "empty_foreground_soft", "empty_foreground_bg12", "absent_class", "all_foreground", "common_offset",
                 "rc_scale_1e3")
LAB_DTYPES = {"int64": torch.int64, "int32": torch.int32, "uint8": torch.uint8}
HEAD_WEIGHTS = {1: (1.0,), 4: (0.4, 0.3, 0.2, 0.1)}
W_RC, W_F, GRAM_SIDE, LOSS_B = 0.5, 2.0, 8, 2
VOL_BRANCH = {(8, 8, 8): "one block", (16, 16, 20): "two blocks of the vectorised kernel", (5, 7, 9): "scalar forward and bwd4<1>",
              (9, 15, 17): "two blocks of the scalar forward"}


def _loss_row(C, nh, lab, vol, family, M):
    """M = 0: VF.seg_only_loss; M in {1, 2}: VF.veloxseg_loss with M reconstructions and M + 1 Gram matrices"""
    cb = "vectorised kernels" if C <= 4 else "scalar forward"
    return dict(id=f"c{C}_h{nh}_{lab}_{'x'.join(map(str, vol))}_{family}_m{M}", C=C, nh=nh, lab=lab, vol=tuple(vol), family=family, M=M,
                branch=f"C = {C}: {cb}; volume: {VOL_BRANCH[tuple(vol)]}")


LOSS_ROWS = [
    _loss_row(2, 4, "int64", (8, 8, 8), "plain", 2),
    _loss_row(3, 1, "int32", (8, 8, 8), "plain", 1),
    _loss_row(4, 4, "uint8", (8, 8, 8), "confident_right", 2),
    _loss_row(4, 4, "int64", (16, 16, 20), "plain", 1),
    _loss_row(2, 1, "uint8", (16, 16, 20), "empty_foreground_bg12", 0),
    _loss_row(3, 4, "int64", (16, 16, 20), "confident_wrong", 0),
    _loss_row(4, 4, "int32", (16, 16, 20), "empty_foreground_soft", 2),
    _loss_row(4, 4, "int64", (16, 16, 20), "common_offset", 0),
    _loss_row(5, 4, "int32", (16, 16, 20), "confident_wrong", 0),
    _loss_row(3, 1, "uint8", (16, 16, 20), "all_foreground", 0),
    _loss_row(5, 4, "int64", (8, 8, 8), "plain", 2),
    _loss_row(8, 1, "int32", (8, 8, 8), "absent_class", 0),
    _loss_row(5, 4, "uint8", (8, 8, 8), "confident_wrong", 0),
    _loss_row(8, 4, "uint8", (9, 15, 17), "plain", 0),
    _loss_row(5, 1, "int64", (9, 15, 17), "common_offset", 0),
    _loss_row(4, 1, "int64", (9, 15, 17), "all_foreground", 0),
    _loss_row(2, 4, "int64", (9, 15, 17), "empty_foreground_bg12", 0),
    _loss_row(8, 4, "int32", (9, 15, 17), "empty_foreground_soft", 1),
    _loss_row(3, 4, "int64", (5, 7, 9), "plain", 2),
    _loss_row(2, 1, "int32", (5, 7, 9), "empty_foreground_soft", 0),
    _loss_row(4, 4, "uint8", (5, 7, 9), "confident_wrong", 0),
    _loss_row(5, 4, "int64", (5, 7, 9), "confident_right", 0),
    _loss_row(3, 4, "int32", (8, 8, 8), "absent_class", 0),
    _loss_row(2, 4, "int64", (8, 8, 8), "common_offset", 0),
    _loss_row(2, 4, "int64", (8, 8, 8), "rc_scale_1e3", 2),
    _loss_row(3, 4, "int64", (5, 7, 9), "rc_scale_1e3", 1),
    _loss_row(4, 1, "uint8", (8, 8, 8), "empty_foreground_bg12", 1),
]


def loss_labels_logits(family, B, C, sp, nh, seed, low=None, offset=1e4):
    """labels (B, 1, *sp) int64 and nh logit tensors; `low` = the grids of heads 1.. for the deep-supervision kernels (families that edit logits per voxel then
    edit head 0 only, the one on the label grid)"""
    g = _gen(seed)
    lab = torch.randint(0, C, (B, 1) + tuple(sp), generator=g)
    if family in ("empty_foreground_soft", "empty_foreground_bg12"):
        lab[0] = 0
    elif family == "absent_class":
        lab[lab == C - 1] = 0
    elif family == "all_foreground":
        lab = torch.randint(1, C, (B, 1) + tuple(sp), generator=g)
    grids = [tuple(sp)] + ([tuple(sp)] * (nh - 1) if low is None else [tuple(t) for t in low])
    logits = [randn(B, C, *grids[h], seed=seed + 1 + h) for h in range(nh)]
    onehot = torch.zeros(B, C, *sp).scatter_(1, lab, 1.0)
    seventh = (torch.arange(lab[0, 0].numel()).view(1, 1, *sp) % 7 == 3).float()
    for h in range(nh):
        full = grids[h] == tuple(sp)
        if family == "confident_right" and full:                                  # six voxels of seven: the label's logit + 12.  (On EVERY voxel the whole gradient is
            logits[h] = logits[h] + 12.0 * onehot * (1.0 - seventh)               # 1 - p ~ 1e-5, which the fp32 oracle itself resolves to 1.8e-4 M only: outside the condition.)
        elif family == "confident_wrong" and full:                                # every 7th voxel: a wrong class + 40
            wrong = torch.zeros(B, C, *sp).scatter_(1, (lab + 1) % C, 1.0)
            logits[h] = logits[h] + 40.0 * wrong * seventh
        elif family == "empty_foreground_bg12":
            logits[h][0, 0] += 12.0
        elif family == "common_offset":
            logits[h] = logits[h] + offset
    return lab, logits


def loss_case(row):
    B, C, nh, M, sp = LOSS_B, row["C"], row["nh"], row["M"], row["vol"]
    s = _seed("loss", row["id"])
    lab, logits = loss_labels_logits(row["family"], B, C, sp, nh, s)
    w = HEAD_WEIGHTS[nh]
    if M == 0:
        return dict(fn=lambda *t: sum(wi * O.seg_loss(l, lab) for wi, l in zip(w, t)), tensors=logits, params=[], cots=[torch.ones(())], labels=lab, sr=None, weights=w)
    sc = 1e3 if row["family"] == "rc_scale_1e3" else 1.0
    rc, sr = randn(B, M, *sp, seed=s + 20, scale=sc), randn(B, M, *sp, seed=s + 21, scale=sc)
    grams = [randn(B, GRAM_SIDE, GRAM_SIDE, seed=s + 30 + i, scale=0.1) for i in range(1 + M)]
    cfg = {"deep_Loss_weight": list(w), "RC_Loss_weight": W_RC, "Feature_Loss_weight": W_F}
    return dict(fn=lambda *t: O.loss(list(t), lab, sr.to(t[0].dtype), M, cfg), tensors=logits + [rc] + grams, params=[], cots=[torch.ones(())], labels=lab, sr=sr, weights=w)


# ... the fused deep-supervision kernels (csrc/loss_ds.hip): head 0 on the label grid, heads 1..3 on grids coarser by `factors`
DS_FACTORS = (2, 4, 8)
# the common offset of these rows is 1e3, not 1e4: the coarse heads are INTERPOLATED first, and an interpolated logit near 1e4 carries a rounding of 5e-4 that
# reaches the gradients of the fp32 oracle at 2.3e-4 M to 2.6e-4 M (the input condition caps them at 1e-4 M); near 1e3 it is 3e-5
DS_COMMON_OFFSET = 1e3
DS_ROWS = [dict(id=f"c{C}_{lab}_{'x'.join(map(str, vol))}_{fam}_{'columns' if col else 'rows'}", C=C, lab=lab, vol=vol, family=fam, columns=col,
                branch=f"fused deep supervision, {'column owners' if col else 'row sweep'}")
           for (C, lab, vol, fam) in ((2, "int64", (8, 8, 16), "empty_foreground_bg12"), (3, "uint8", (8, 8, 16), "confident_wrong"), (4, "int32", (8, 8, 16), "common_offset"),
                                      (4, "int64", (16, 16, 32), "empty_foreground_soft"), (2, "int32", (16, 16, 32), "confident_wrong"), (3, "uint8", (16, 16, 32), "common_offset"))
           for col in (1, 0)]


def ds_case(row):
    B, C, sp = LOSS_B, row["C"], row["vol"]
    s = _seed("ds", row["id"].rsplit("_", 1)[0])                                  # both thread maps see the same input
    low = [tuple(max(n // f, 2) for n in sp) for f in DS_FACTORS]
    lab, heads = loss_labels_logits(row["family"], B, C, sp, 4, s, low=low, offset=DS_COMMON_OFFSET)
    w = HEAD_WEIGHTS[4]

    def fn(*t):
        up = [t[0]] + [upsample(h, sp) for h in t[1:]]
        return sum(wi * O.seg_loss(u, lab) for wi, u in zip(w, up))

    return dict(fn=fn, tensors=heads, params=[], cots=[torch.ones(())], labels=lab, weights=w)


# ---------------------------------------------------------------------------------------------------------------------- Gram, up-sampling
def upsample(x, size):
    """oracle.veloxseg_oracle.upsample_trilinear in the dtype of x (its interpolation matrices restate the fp32 index / weight arithmetic, converted exactly)"""
    Ad, Ah, Aw = (O.interp_matrix(x.shape[2 + i], size[i]).to(x.dtype) for i in range(3))
    x = torch.einsum("bcdhw,Dd->bcDhw", x, Ad)
    x = torch.einsum("bcdhw,Hh->bcdHw", x, Ah)
    return torch.einsum("bcdhw,Ww->bcdhW", x, Aw)


GRAM_ROWS = [dict(id=f"c{C}_v{V}_x{sc:g}", C=C, sp=sp, scale=sc, branch=br)
             for C, V, sp, br in ((16, 1024, (8, 8, 16), "one full 1024-voxel block, one channel group, compile-time C = 16 backward"),
                                  (17, 1029, (3, 7, 49), "two blocks, ragged unaligned tail, second channel group with one channel"),
                                  (32, 2048, (8, 16, 16), "two blocks, both channel groups full, compile-time C = 32 backward"),
                                  (31, 125, (5, 5, 5), "one partly filled block, second channel group partly filled, scalar backward"),
                                  (8, 4100, (4, 25, 41), "five blocks, aligned tail of 4 voxels, half a channel group"))
             for sc in (1.0, 1e3)]
GRAM_B = 2


def gram_case(row):
    s = _seed("gram", row["id"])
    x = randn(GRAM_B, row["C"], *row["sp"], seed=s, scale=row["scale"])
    return dict(fn=O.gram, tensors=[x], params=[], cots=[randn(GRAM_B, row["C"], row["C"], seed=s + 1)])


UP_ROWS = [dict(id="4x6x3_to_16x24x12", BC=(2, 3), lo=(4, 6, 3), hi=(16, 24, 12), branch="rows of 12: the 16-byte store kernel"),
           dict(id="2x2x2_to_32x32x32", BC=(1, 2), lo=(2, 2, 2), hi=(32, 32, 32), branch="ratio 31: every output between the same two inputs"),
           dict(id="3x5x7_to_7x11x13", BC=(2, 2), lo=(3, 5, 7), hi=(7, 11, 13), branch="odd extents: the scalar store kernel")]


def up_case(row):
    s = _seed("up", row["id"])
    hi = row["hi"]
    return dict(fn=lambda x: upsample(x, hi), tensors=[randn(*row["BC"], *row["lo"], seed=s)], params=[], cots=[randn(*row["BC"], *hi, seed=s + 1)])


# ---------------------------------------------------------------------------------------------------------------------- the tables as one
TABLES = {"instnorm": (IN_ROWS, in_case), "layernorm": (LN_ROWS, ln_case), "loss": (LOSS_ROWS, loss_case), "loss_ds": (DS_ROWS, ds_case), "gram": (GRAM_ROWS, gram_case),
          "upsample": (UP_ROWS, up_case)}


def rows(op):
    return TABLES[op][0]


def ids(op):
    return [r["id"] for r in TABLES[op][0]]


@functools.lru_cache(maxsize=4)
def _case(op, rid):
    r = next(x for x in TABLES[op][0] if x["id"] == rid)
    c = TABLES[op][1](r)
    c["r64"] = ref64(c["fn"], c["tensors"], c["params"], c["cots"])
    c["r32"] = ref32(c["fn"], c["tensors"], c["params"], c["cots"])
    return c


def case(op, row):
    """the row's inputs (fp32 CPU tensors, never modified), its oracle function and both references (computed once per row, a few rows kept)"""
    return _case(op, row["id"])
