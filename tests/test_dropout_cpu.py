"""CPU checks of the dropout-mask restatement (oracle/philox.py) and of the model's dropout site ids.

The restatement is what tests/test_dropout_parity_gpu.py holds the HIP kernels to, and what the dropout-on golden
(tests/golden/g1_48_m2_drop.pt, checked by tests/test_oracle_golden.py) was generated with, so its generator must be right on
its own: Philox4x32 is pinned here against known answers of an independent implementation.
"""
import numpy as np
import pytest
import torch

from oracle import philox as P
from recipe import CASES, DROP_CASES, dropout_sites

# Philox4x32-10 known answers: rocRAND's host-callable rocrand_device::philox4x32_10_engine::ten_rounds(counter, key) (ROCm
# include/rocrand/rocrand_philox4x32_10.h; protected, called from a derived class in a one-off host program).  The first three are also the
# known-answer vectors Random123 publishes for philox4x32_10.  Rows: (counter words x, y, z, w), (key words x, y) -> 4 output words.
KAT_PHILOX4X32_10 = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
    ((0x00000007, 0x00000000, 0x00000003, 0x00000000), (0x00003039, 0x00000000), (0xf0e5fd73, 0x02e3c8e3, 0x2139402c, 0xf976d670)),
    ((0x00000001, 0x00000002, 0x0000002a, 0x00000000), (0xdeadbeef, 0x00000001), (0x34e40014, 0x8ceccc45, 0xfa412f3e, 0x4193cc2e)),
]


@pytest.mark.parametrize("ctr,key,want", KAT_PHILOX4X32_10)
def test_philox4x32_10_known_answers(ctr, key, want):
    """the round function, the key schedule and the word order, at 10 rounds (the product draws 7 rounds of the same function)"""
    c = ctr[0] | (ctr[1] << 32)
    stream = ctr[2] | (ctr[3] << 32)
    k = key[0] | (key[1] << 32)
    got = P.philox4x32(np.array([c, c], dtype=np.uint64), stream, k, rounds=10)
    assert got.dtype == np.uint32 and got.shape == (2, 4)
    assert [int(v) for v in got[0]] == list(want) and [int(v) for v in got[1]] == list(want)


def test_seed_mixing_and_index_layout():
    """seed' = seed + 0x9E3779B97F4A7C15 * step (mod 2^64); element idx of a 24-bit site is word idx & 3 of counter idx >> 2, element idx of
    an attention site is 16-bit chunk idx & 7 (low half first) of counter idx >> 3"""
    assert P.mix_seed(5, 0) == 5
    assert P.mix_seed(2 ** 64 - 1, 1) == (0x9E3779B97F4A7C15 - 1)
    assert P.mix_seed(0x1_2345_6789, 3) == (0x1_2345_6789 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64
    seed, step, site, p = 0x1_0000_0003, 2, 9, 0.3
    key = P.mix_seed(seed, step)
    w = P.philox4x32(np.arange(4, dtype=np.uint64), site, key)
    s = P.site_scales(seed, step, site, 13, p).numpy()
    for idx in range(13):
        u = np.float32(int(w[idx >> 2][idx & 3]) >> 8) * np.float32(2.0 ** -24)
        assert s[idx] == (np.float32(1) / (np.float32(1) - np.float32(p)) if u >= np.float32(p) else 0.0)
    a = P.attn_scales(seed, step, site, 29, p).numpy()
    thr = P.attn_thr16(p)
    for idx in range(29):
        word = int(w[idx >> 3][(idx & 7) >> 1])
        chunk = (word >> (16 * (idx & 1))) & 0xFFFF
        assert a[idx] == (np.float32(P.attn_keep_scale(p)) if chunk >= thr else 0.0)


def test_attention_rate_quantisation():
    """the attention sites represent p as thr16 / 65536 (deliberately: 16 random bits per decision) and scale kept weights by
    65536 / (65536 - thr16), so the mask stays unbiased for the rate it draws: p = 0.1 -> thr16 = 6554, an effective rate of 0.100006"""
    assert P.attn_thr16(0.1) == 6554 and abs(6554 / 65536 - 0.100006) < 1e-6
    assert P.attn_keep_scale(0.1) == float(np.float32(65536.0 / (65536 - 6554)))
    assert P.attn_thr16(0.0) == 0 and P.attn_thr16(0.9999999) == 65535
    assert P.keep_scale(0.1) == float(np.float32(1.0) / np.float32(0.9))
    n = 1 << 20
    for p in (0.1, 0.3):
        for f, rate, sc in ((P.site_scales, p, P.keep_scale(p)), (P.attn_scales, P.attn_thr16(p) / 65536, P.attn_keep_scale(p))):
            m = f(123, 4, 17, n, p)
            drop = float((m == 0).double().mean())
            assert abs(drop - rate) < 5 * (rate * (1 - rate) / n) ** 0.5, (f.__name__, p, drop)
            assert set(torch.unique(m).tolist()) == {0.0, sc}


def _all_configs():
    import bench
    out = [(n, c) for n, (c, _) in CASES.items()] + [(n, c) for n, (c, _) in DROP_CASES.items()]
    return out + [("bench:" + n, c) for n, (c, _) in bench.WORKLOADS.items()]


@pytest.mark.parametrize("name,cfg", _all_configs(), ids=lambda v: v if isinstance(v, str) else "")
def test_site_ids_positive_unique(name, cfg):
    """every dropout site of the model draws its own stream: ids positive and pairwise different, one per (module, modality), and the numbering
    is a function of the architecture only (two models built from one config agree)"""
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    model = VeloxSeg(**cfg)
    sites = dropout_sites(model)
    ids = list(sites.values())
    assert ids and all(i > 0 for i in ids), sites
    assert len(set(ids)) == len(ids), sorted(ids)
    M = len(cfg["in_ch"])
    depths = cfg.get("depths", [2, 2, 2, 2])
    conv_depths = cfg.get("conv_depths", [1, 1, 1, 1])
    n_blocks = sum(depths)
    n_jlc = sum(conv_depths) + (1 + M) * sum(conv_depths[:3])
    assert len(ids) == M + n_blocks * (1 + M + 2 * M) + n_jlc, (len(ids), sorted(sites))
    assert dropout_sites(VeloxSeg(**cfg)) == sites


def test_masks_differ_across_sites_steps_samples():
    """sanity of the restatement as the kernels use it: different sites, steps and seeds draw different masks, and the two samples of a batch
    (consecutive index ranges of one site) are not copies of each other"""
    n, p = 4 * 48 * 24 * 24 * 24, 0.1
    base = P.site_scales(0x1_2345_6789, 3, 5, 2 * n, p)
    for other in (P.site_scales(0x1_2345_6789, 3, 6, 2 * n, p), P.site_scales(0x1_2345_6789, 4, 5, 2 * n, p),
                  P.site_scales(0x2_2345_6789, 3, 5, 2 * n, p)):
        agree = float(((base == 0) == (other == 0)).double().mean())
        assert agree < 0.85, agree               # independent masks agree on 1 - 2p(1-p) = 0.82 of the elements
    b0, b1 = base[:n], base[n:]
    assert float(((b0 == 0) == (b1 == 0)).double().mean()) < 0.85
    a = P.attn_scales(0x1_2345_6789, 3, 5, 2 * n, p)
    assert float(((a == 0) == (base == 0)).double().mean()) < 0.85      # the two schemes do not alias on one site
