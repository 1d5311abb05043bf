"""CPU restatement of the dropout masks the HIP kernels draw -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The product's masks are a pure function of ({seed, step}, site id, element index) (veloxseg_amd/csrc/vx_common.h, "counter-based RNG for
dropout"), so the oracle can apply the very masks a training step on the device applied.  This module states that function again in numpy
uint64 arithmetic; it shares no code with the product.

  * Philox4x32 with `rounds` rounds (7 in the product); the key is bumped by (0x9E3779B9, 0xBB67AE85) after every round.  Counter words
    (ctr lo, ctr hi, stream lo, stream hi), key words (seed lo, seed hi).
  * seed' = seed + 0x9E3779B97F4A7C15 * step  (mod 2^64), from the {seed, step} int64 pair of veloxseg_amd.functional.rng_state.
  * the stream is the dropout site id (veloxseg_amd.functional.new_dropout_site).
  * 24-bit sites (positional, projection, FFN, JLC): element idx of the dropped tensor, flat in (B, C, D, H, W) order, uses word idx & 3 of
    philox(seed', site, idx >> 2); it is kept iff float(word >> 8) * 2^-24 >= p (fp32), and a kept element is scaled by the fp32 value 1 / (1 - p).
  * attention sites: element idx of the (B, heads, N, ML, ML) soft-max weights uses the 16-bit chunk idx & 7 of philox(seed', site, idx >> 3)
    (word chunk >> 1, low half first); kept iff chunk >= thr16 = min(65535, uint(p * 65536 + 0.5)), scale 65536 / (65536 - thr16) (fp32).
    p is thereby quantised to thr16 / 65536: 6554 / 65536 = 0.100006 at p = 0.1; the scale keeps the mask unbiased for that rate.
"""
from __future__ import annotations

import numpy as np
import torch

_U64 = np.uint64
_M32 = _U64(0xFFFFFFFF)
_PH_M0, _PH_M1 = _U64(0xD2511F53), _U64(0xCD9E8D57)
_PH_W0, _PH_W1 = _U64(0x9E3779B9), _U64(0xBB67AE85)
GOLDEN64 = 0x9E3779B97F4A7C15
ROUNDS = 7
_CHUNK = 1 << 21          # counters per numpy pass (bounds the temporaries at ~100 MB)


def mix_seed(seed: int, step: int) -> int:
    """the key the kernels draw with for the {seed, step} pair (two's-complement int64 values read as uint64)"""
    return ((int(seed) & 0xFFFFFFFFFFFFFFFF) + GOLDEN64 * (int(step) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF


def philox4x32(ctr, stream: int, key: int, rounds: int = ROUNDS) -> np.ndarray:
    """(..., 4) uint32 words of Philox4x32-`rounds` for the uint64 counters `ctr` (array) under one 64-bit stream id and one 64-bit key"""
    ctr = np.asarray(ctr, dtype=_U64)
    c0, c1 = ctr & _M32, ctr >> _U64(32)
    s = int(stream) & 0xFFFFFFFFFFFFFFFF
    c2 = np.full_like(ctr, s & 0xFFFFFFFF)
    c3 = np.full_like(ctr, s >> 32)
    k = int(key) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = _U64(k & 0xFFFFFFFF), _U64(k >> 32)
    for _ in range(rounds):
        p0 = _PH_M0 * c0                      # 32 x 32 -> 64 bits: exact in uint64
        p1 = _PH_M1 * c2
        c0, c1, c2, c3 = (p1 >> _U64(32)) ^ c1 ^ k0, p1 & _M32, (p0 >> _U64(32)) ^ c3 ^ k1, p0 & _M32
        k0 = (k0 + _PH_W0) & _M32
        k1 = (k1 + _PH_W1) & _M32
    return np.stack([c0, c1, c2, c3], -1).astype(np.uint32)


def _words(seed: int, step: int, site: int, n_ctr: int):
    key = mix_seed(seed, step)
    for lo in range(0, n_ctr, _CHUNK):
        hi = min(n_ctr, lo + _CHUNK)
        yield lo, philox4x32(np.arange(lo, hi, dtype=_U64), site, key)


def keep_scale(p: float) -> float:
    """fp32 1 / (1 - p) of the 24-bit sites"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def attn_thr16(p: float) -> int:
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    return 0 if p <= 0 else (65535 if t >= np.float32(65535.0) else int(t))


def attn_keep_scale(p: float) -> float:
    return float(np.float32(65536.0) / (np.float32(65536.0) - np.float32(attn_thr16(p))))


def site_scales(seed: int, step: int, site: int, n: int, p: float) -> torch.Tensor:
    """fp32 (n,): 0 or 1 / (1 - p) for elements 0 .. n-1 of a 24-bit dropout site"""
    out = np.empty(n, dtype=np.float32)
    if n == 0:
        return torch.from_numpy(out)
    pf, sc = np.float32(p), np.float32(keep_scale(p))
    for lo, w in _words(seed, step, site, (n + 3) // 4):
        bits = w.reshape(-1)[: n - 4 * lo]
        u = (bits >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        out[4 * lo: 4 * lo + bits.size] = np.where(u >= pf, sc, np.float32(0.0))
    return torch.from_numpy(out)


def attn_scales(seed: int, step: int, site: int, n: int, p: float) -> torch.Tensor:
    """fp32 (n,): 0 or 65536 / (65536 - thr16) for elements 0 .. n-1 of an attention dropout site"""
    out = np.empty(n, dtype=np.float32)
    if n == 0:
        return torch.from_numpy(out)
    thr, sc = np.uint32(attn_thr16(p)), np.float32(attn_keep_scale(p))
    for lo, w in _words(seed, step, site, (n + 7) // 8):
        halves = np.stack([w & np.uint32(0xFFFF), w >> np.uint32(16)], -1).reshape(-1)[: n - 8 * lo]
        out[8 * lo: 8 * lo + halves.size] = np.where(halves >= thr, sc, np.float32(0.0))
    return torch.from_numpy(out)


def apply(x: torch.Tensor, seed: int, step: int, site: int, p: float, attn: bool = False) -> torch.Tensor:
    """x times the restated mask of dropout site `site` (x flat in its own memory order, which is the kernels' index order)"""
    f = attn_scales if attn else site_scales
    s = f(seed, step, site, x.numel(), p).view(x.shape).to(device=x.device, dtype=x.dtype)
    return x * s
