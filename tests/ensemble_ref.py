"""Torch / numpy restatement of the ensemble kernels (csrc/ensemble.hip) and of utils/ensemble.py's weight rule, for the tests only.

fp64 side: soft-max, weighted mean and entropy, written from the definitions (no torch.softmax).  fp32 side: the accumulation chain of vx_softmax_accumulate as
separate tensor operations (a product, then a sum: two roundings, which no CPU tensor op contracts), and the arg-max rule of the inference kernels."""
import numpy as np
import torch


def softmax64(logits: torch.Tensor, dim: int = 1) -> torch.Tensor:
    """fp64 soft-max from its definition; inf - inf = NaN makes a column with a +inf and a column of -inf only all-NaN, a NaN spreads through the sum, and a -inf
    beside a finite maximum gives exp(-inf) = 0 exactly: the special values of torch.softmax"""
    x = logits.double()
    m = x.max(dim=dim, keepdim=True).values             # (torch's max hands a NaN on)
    e = torch.exp(x - m)
    return e / e.sum(dim=dim, keepdim=True)


def normalise_weights(weights, n):
    """w_i / sum(w) in fp64, rounded to fp32; None: float32(1 / n) each"""
    if weights is None:
        return [float(np.float32(1.0 / n))] * n
    w = np.asarray(weights, dtype=np.float64)
    return [float(np.float32(x)) for x in w / w.sum()]


def mean64(logits_list, weights=None, dim: int = 1) -> torch.Tensor:
    """the weighted mean of the fp64 soft-max, with the fp32 weights the kernels get"""
    w = normalise_weights(weights, len(logits_list))
    return sum(wi * softmax64(x, dim) for wi, x in zip(w, logits_list))


def entropy64(p: torch.Tensor, dim: int = 1) -> torch.Tensor:
    """-sum p ln p in fp64, 0 ln 0 = 0"""
    p = p.double()
    t = torch.where(p == 0, torch.zeros_like(p), -p * torch.log(p))
    return t.sum(dim=dim, keepdim=True)


def accumulate32(psum, p32: torch.Tensor, weight: float) -> torch.Tensor:
    """the fp32 chain of one vx_softmax_accumulate call on fp32 probabilities p32: t = w * p; psum = psum + t (psum None: the first call, 0 + t)"""
    assert p32.dtype == torch.float32
    t = p32 * torch.tensor(weight, dtype=torch.float32)
    base = torch.zeros_like(t) if psum is None else psum
    return base + t


def argmax_rule(x: torch.Tensor, dim: int = 1) -> torch.Tensor:
    """uint8 index of the first NaN of a column, else of its first maximum (vx_sw_finalize, vx_argmax_channels), keepdim"""
    K = x.shape[dim]
    idx = torch.arange(K).view([-1 if d == dim else 1 for d in range(x.dim())]).expand_as(x)
    nan = torch.isnan(x)
    first_nan = torch.where(nan, idx, torch.full_like(idx, K)).min(dim=dim, keepdim=True).values
    clean = torch.where(nan, torch.full_like(x, -float("inf")), x)
    top = clean.max(dim=dim, keepdim=True).values
    first_max = torch.where(clean == top, idx, torch.full_like(idx, K)).min(dim=dim, keepdim=True).values
    return torch.where(first_nan < K, first_nan, first_max).to(torch.uint8)


def exact_columns(K: int, shape, seed: int):
    """logits (K, *shape) drawn from {0, -inf} with m zeros per column, so every probability is exactly 0 or fl(1 / m) -- s = m is exact and the IEEE quotient is the
    correctly rounded one --, and the fp32 probabilities themselves.  m in {1, 2, 4} as far as K allows, where 1 / m is a power of two and w * p exact, and also
    m in {3, 5}: there w * p is rounded, so a product contracted into an fma shows in the bits.  The first columns are special: all -inf, one with a +inf, one
    with a NaN (all-NaN probabilities)"""
    g = torch.Generator().manual_seed(seed)
    V = int(np.prod(shape))
    ms = [m for m in (1, 2, 4, 3, 5) if m <= K]
    x = torch.full((K, V), -float("inf"))
    p = torch.zeros((K, V))
    for v in range(V):
        m = ms[int(torch.randint(0, len(ms), (1,), generator=g))]
        on = torch.randperm(K, generator=g)[:m]
        x[on, v] = 0.0
        p[on, v] = float(np.float32(1.0) / np.float32(m))
    n = min(3, V)
    special = [torch.full((K,), -float("inf")), torch.zeros(K), torch.zeros(K)]
    special[1][K - 1] = float("inf")
    special[2][0] = float("nan")
    for v in range(n):
        x[:, v] = special[v]
        p[:, v] = float("nan")
    return x.view(K, *shape), p.view(K, *shape)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """fp32 tensors equal as int32 bytes, except that any NaN equals any NaN (at the same positions)"""
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or not torch.equal(torch.isnan(a), torch.isnan(b)):
        return False
    ok = ~torch.isnan(a)
    return torch.equal(a.view(torch.int32)[ok], b.view(torch.int32)[ok])
