"""The data movers of csrc/pwa.hip through the C ABI: the channel-vectorised window gather (forward and backward) against the one-lane-per-channel kernels
(vx_pwa_gather_set_vec(0)), bit for bit; the one-launch scatter adjoint against the per-scale launches (vx_pwa_scatter_set_merged(0))."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import veloxseg_oracle as O  # noqa: E402  (window geometry only)


def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(tuple(shape), generator=g)


def bits(t):
    return t.contiguous().view(torch.int32)


def _plan(grid, big, heads):
    from veloxseg_amd import _hip as H
    pl = O.plan_pwa(grid, big, [1, 1, 1], 2, heads, 4, 4)
    return pl, H.make_plan(grid, pl["n"], heads, pl["small"], pl["nwin"])


# grid, big window, heads, c_qk, c_v                                   covers
GATHER_GEOMETRIES = [([16, 16, 16], [2, 2, 2], 2, 4, 8),             # four scales, cells up to 8^3; two heads, 4 and 8 channels
                     ([16, 16, 8], [4, 4, 2], 1, 8, 8),              # anisotropic; 8 channels per lane
                     ([12, 12, 12], [3, 3, 3], 1, 4, 4),             # W = 12: row tails, cells 1 / 2 / 4
                     ([6, 6, 6], [3, 3, 3], 2, 4, 8)]                # W % 4 != 0: the fall-back
GATHER_IDS = ["16_four_scales", "aniso", "w12", "w6_fallback"]


def _gather_sources(kind, pl, heads, cq, cv, M, B, grid):
    """3 M volumes (q, k, v per modality).  `randn`; `ties`: integer values in {0, 1, 2}, so every pooled cell has several maxima and the first-index rule decides;
    `nan`: randn with one NaN per pooled scale at the first, at a middle and at the last voxel of three different cells"""
    nb = pl["nb"]
    out = []
    for k in range(3 * M):
        c = cv if k % 3 == 2 else cq
        shape = (B, nb * heads * c, *grid)
        if kind == "ties":
            g = torch.Generator().manual_seed(100 + k)
            x = torch.randint(0, 3, shape, generator=g).float()
        else:
            x = rnd(*shape, seed=10 + k)
        if kind == "nan":
            for i, s in enumerate(pl["small"]):
                if s == [1, 1, 1]:
                    continue
                last_cell = [(g_ // s_ - 1) * s_ for g_, s_ in zip(grid, s)]
                mid = (s[0] * s[1] * s[2]) // 2
                md, mh, mw = mid // (s[1] * s[2]), (mid // s[2]) % s[1], mid % s[2]
                sl = slice(i * heads * c, (i + 1) * heads * c)
                x[:, sl, 0, 0, 0] = float("nan")                                                          # first voxel of cell (0, 0, 0)
                x[:, sl, md, mh, s[2] + mw] = float("nan")                                                # middle of cell (0, 0, 1)
                x[:, sl, last_cell[0] + s[0] - 1, last_cell[1] + s[1] - 1, last_cell[2] + s[2] - 1] = float("nan")    # last voxel of the last cell
        out.append(x)
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("M", [1, 2, 3])
@pytest.mark.parametrize("grid,big,heads,cq,cv", GATHER_GEOMETRIES, ids=GATHER_IDS)
def test_vectorised_gather_keeps_the_bits_of_the_per_channel_kernels(grid, big, heads, cq, cv, M, B):
    """vx_pwa_gather_all_fwd / _bwd, default path (1) and the four-voxels-per-thread backward at any size (2) against vx_pwa_gather_set_vec(0): tokens, arg-max indices
    (pooled scales) and dsrc are the same bits; every destination starts as NaN (indices: -1), so an element that was not written shows"""
    from veloxseg_amd import _hip as H
    d = dev()
    pl, plan = _plan(grid, big, heads)
    pp, st = ctypes.addressof(plan), H.stream_ptr()
    pooled0 = next((plan.woff[i] for i in range(plan.nb) if pl["small"][i] != [1, 1, 1]), plan.Ntot)       # first window of the pooled scales
    for kind in ("randn", "ties", "nan"):
        src = [t.to(d) for t in _gather_sources(kind, pl, heads, cq, cv, M, B, grid)]
        arr = (ctypes.c_void_p * (3 * M))(*[H.P(t) for t in src])
        dtok = [rnd(B, heads, plan.Ntot, M * plan.l, c, seed=70 + j).to(d) for j, c in enumerate((cq, cq, cv))]
        res = {}
        try:
            for on in (0, 1, 2):            # 2: the four-voxels-per-thread backward at any size (by default it takes large volumes only)
                H.call("vx_pwa_gather_set_vec", on)
                tok = [torch.full((B, heads, plan.Ntot, M * plan.l, c), float("nan"), device=d) for c in (cq, cq, cv)]
                idx = [torch.full(t.shape, -1, device=d, dtype=torch.int32) for t in tok]
                H.call("vx_pwa_gather_all_fwd", ctypes.addressof(arr), *[H.P(t) for t in tok], *[H.P(t, torch.int32) for t in idx], pp, cq, cv, M, B, st)
                dst = [torch.full_like(t, float("nan")) for t in src]
                darr = (ctypes.c_void_p * (3 * M))(*[H.P(t) for t in dst])
                ref_idx = res[0][1] if on else idx           # the backward of both forms reads the indices of the per-channel forward (every scale written)
                H.call("vx_pwa_gather_all_bwd", *[H.P(t) for t in dtok], *[H.P(t, torch.int32) for t in ref_idx], ctypes.addressof(darr), pp, cq, cv, M, B, st)
                torch.cuda.synchronize()
                res[on] = (tok, idx, dst)
        finally:
            H.call("vx_pwa_gather_set_vec", 1)
        for on in (1, 2):
            for j in range(3):
                assert torch.equal(bits(res[on][0][j]), bits(res[0][0][j])), f"{kind}: tokens {j}"
                assert torch.equal(res[on][1][j][:, :, pooled0:], res[0][1][j][:, :, pooled0:]), f"{kind}: indices {j}"
                assert bool((res[0][1][j][:, :, pooled0:] >= 0).all()) and bool((res[on][1][j][:, :, pooled0:] >= 0).all()), f"{kind}: an index was not written"
                if kind != "nan":
                    assert bool(torch.isfinite(res[on][0][j]).all()), f"{kind}: a token was not written"
            for k in range(3 * M):
                assert bool(torch.isfinite(res[on][2][k]).all()), f"{kind}: dsrc {k} has an element that was not written (knob {on})"
                assert torch.equal(res[on][2][k], res[0][2][k]), f"{kind}: dsrc {k} (knob {on})"
        if kind == "ties" and pooled0 < plan.Ntot:
            # the first-index rule itself, not only agreement: the saved arg-max is the first voxel (flattened d, h, w order) that holds its cell's maximum
            q0, i = src[0][0].cpu(), plan.nb - 1
            s, c = pl["small"][i], cq
            cell = q0[i * heads * c, :s[0], :s[1], :s[2]].reshape(-1)
            first = int((cell == cell.max()).nonzero()[0])
            want = ((first // (s[1] * s[2])) * grid[1] + (first // s[2]) % s[1]) * grid[2] + first % s[2]
            assert int(res[1][1][0][0, 0, plan.woff[i], 0, 0]) == want


SCATTER_GEOMETRIES = [([16, 16, 16], [8, 8, 8], 2, 8, 2), ([32, 32, 32], [4, 4, 4], 1, 4, 2), ([8, 8, 8], [4, 4, 4], 4, 32, 1), ([4, 4, 4], [4, 4, 4], 2, 16, 2),
                      ([24, 24, 24], [3, 3, 3], 1, 4, 2), ([16, 16, 8], [4, 4, 2], 2, 8, 3)]
SCATTER_IDS = ["two_scales", "scales_incl_separable", "one_modality", "single_scale", "96_L1", "aniso_three_modalities"]


@pytest.mark.parametrize("grid,big,heads,c,M", SCATTER_GEOMETRIES, ids=SCATTER_IDS)
def test_one_launch_scatter_adjoint_equals_the_per_scale_launches(grid, big, heads, c, M):
    """vx_pwa_scatter_bwd_all_w / _all_wz / _all with every scale in one launch (each token element has one owning block) into a NaN-filled destination, against the
    per-scale launches into a zeroed one: the same bits where every scale was a sole owner before (cells up to 2^3), the tolerance of
    test_scatter_adjoint_into_an_unzeroed_destination for the wide-cell scales, which added with float atomics; bit-identical from run to run; the extra buffer zeroed"""
    from veloxseg_amd import _hip as H
    d = dev()
    pl, plan = _plan(grid, big, heads)
    B = 2
    pp, st = ctypes.addressof(plan), H.stream_ptr()
    dout = [rnd(B, plan.nb * heads * c, *grid, seed=60 + m).to(d) for m in range(M)]
    ptrs = (ctypes.c_void_p * 4)(*([t.data_ptr() for t in dout] + [None] * (4 - M)))
    ref = torch.zeros(B, heads, plan.Ntot, M * plan.l, c, device=d)
    try:
        H.call("vx_pwa_scatter_set_merged", 0)
        H.call("vx_pwa_scatter_bwd_all", ctypes.addressof(ptrs), H.P(ref), pp, c, M, B, st)
        torch.cuda.synchronize()
    finally:
        H.call("vx_pwa_scatter_set_merged", 1)
    got = [torch.full_like(ref, float("nan")) for _ in range(3)]
    extra = torch.full((4 * 1237,), float("nan"), device=d)
    try:
        H.call("vx_pwa_scatter_set_merged", 2)              # (by default the one launch is taken from B * M = 8 volumes on)
        assert H.query("vx_pwa_scatter_bwd_all_w", ctypes.addressof(ptrs), H.P(got[0]), pp, c, M, B, st) == 0
        assert H.query("vx_pwa_scatter_bwd_all_w", ctypes.addressof(ptrs), H.P(got[1]), pp, c, M, B, st) == 0
        assert H.query("vx_pwa_scatter_bwd_all_wz", ctypes.addressof(ptrs), H.P(got[2]), pp, c, M, B, H.P(extra), extra.numel(), st) == 0
        acc = torch.zeros_like(ref)
        H.call("vx_pwa_scatter_bwd_all", ctypes.addressof(ptrs), H.P(acc), pp, c, M, B, st)          # "+=" into a zeroed destination, the same launch
        torch.cuda.synchronize()
    finally:
        H.call("vx_pwa_scatter_set_merged", 1)
    assert float(ref.abs().max()) > 0 and bool(torch.isfinite(got[0]).all())
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2]) and torch.equal(got[0], acc), "the one-launch adjoint must be reproducible"
    assert float(extra.abs().max()) == 0.0
    if all(max(s) <= 2 for s in pl["small"]):
        assert torch.equal(got[0], ref)
    else:
        a, b = got[0].cpu().double(), ref.cpu().double()
        err, tol = (a - b).abs(), 2e-6 * max(1.0, float(b.abs().max())) + 1e-5 * b.abs()
        print(f"scatter adjoint, one launch vs per scale: max abs err {float(err.max()):.3e}, ref max {float(b.abs().max()):.3e}")
        assert bool((err <= tol).all()), f"max abs err {float(err.max()):.3e} (ref max {float(b.abs().max()):.3e})"
