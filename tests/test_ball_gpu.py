"""vx_morph_ball (csrc/morphology.hip), the ball_* functions of utils/morphology.py and the normalised surface Dice of utils/metric/surface.py against the numpy /
scipy oracle of tests/ball_ref.py.  tests/test_ball_cpu.py holds the oracle to the definition.

Exact integer work: every comparison in this file is `==`.  Kernel outputs of the C-ABI tests sit between 64-element canaries (exact_ref.Guard) and are prefilled
with a sentinel; inputs are checked unwritten; a refused call raises and leaves its prefill.  The kernel's grid-stride loop takes a second trip in
test_above_the_grid_cap."""
import math

import numpy as np
import pytest
import torch

import ball_ref as R
import distance_ref as DR
import morphology_ref as MR
from exact_ref import Guard

pytestmark = pytest.mark.gpu

I64_CANARY, I64_FILL = 0x5A5A5A5A5A5A, -7
DILATE, ERODE = 0, 1
UNIT = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module", autouse=True)
def stream_pool_left_where_it_was():
    """as in tests/test_morphology_gpu.py: this module leaves torch's round-robin pool of 32 streams at the position it found it (one full turn recorded on the way
    in, streams drawn until that turn's last one comes up again on the way out)"""
    turn = [torch.cuda.Stream().cuda_stream for _ in range(32)]
    yield
    if len(set(turn)) == 32:
        for _ in range(32):
            if torch.cuda.Stream().cuda_stream == turn[-1]:
                break


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


def _M():
    from veloxseg_amd.utils import morphology as M
    return M


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()
    return t if dtype is None else t.to(dtype)


def same(got, want, what):
    g = got.detach().cpu().numpy().astype(np.int64).reshape(-1) if torch.is_tensor(got) else np.asarray(got).astype(np.int64).reshape(-1)
    w = np.asarray(want).astype(np.int64).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} elements against {w.size}"
    bad = g != w
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first flat index {i}: got {g[i]:#x}, want {w[i]:#x}")


def guard(n):
    return Guard((n,), torch.int64, fill=I64_FILL, canary=I64_CANARY)


def rows_of(tau, spacing):
    M = _M()
    return M.pack_rows(M.BallElement(tau, spacing).half_widths)


def abi_ball(words, shape, rows, op, border_value, gate=None):
    """vx_morph_ball through the C ABI on host arrays -> the output words (numpy int64).  gate: None, "in" (the input buffer itself) or an array of words"""
    H = _H()
    src, rec = dev(words), dev(np.asarray(rows, dtype=np.int32))
    g = None if gate is None else (src if isinstance(gate, str) else dev(gate))
    keep, keep_rec, keep_g = src.clone(), rec.clone(), None if g is None else g.clone()
    out = guard(MR.words(shape))
    H.call("vx_morph_ball", src.data_ptr(), None if g is None else g.data_ptr(), out.ptr, *shape, rec.data_ptr(), rec.numel(), op, border_value, H.stream_ptr())
    torch.cuda.synchronize()
    out.check("vx_morph_ball out")
    assert torch.equal(src, keep) and torch.equal(rec, keep_rec) and (g is None or torch.equal(g, keep_g)), "vx_morph_ball wrote an input"
    return out.t.cpu().numpy()


def oracle(mask, tau, spacing, op, border_value):
    return (R.erode if op == ERODE else R.dilate)(mask, tau, spacing, border_value)


# ====================================================================================================================== the kernel against the oracle
@pytest.mark.parametrize("k", range(len(R.ELEMENTS)))
def test_ball_equals_reference(k):
    tau, spacing = R.ELEMENTS[k]
    rows = rows_of(tau, spacing)
    if k == 0:
        assert R.unpack_rows(rows) == [(0, 0, 0)]
    shapes = R.ABI_SHAPES
    if k == len(R.ELEMENTS) - 1:
        shapes, radii = R.LARGE_SHAPES, _M().BallElement(tau, spacing).radii
        assert radii == (9, 9, 63) and all(r >= n - 1 for shape in shapes for r, n in zip(radii, shape)), "the large element no longer spans its volumes"
    for i, shape in enumerate(shapes):
        m = R.mask_for(shape, 350 + 10 * k + i)
        words, ones = MR.pack(m), MR.tail_ones(shape)
        for op in (DILATE, ERODE):
            src = MR.pack(1 - m) if op == ERODE else words          # sparse sites for the dilation, sparse holes for the erosion
            mm = 1 - m if op == ERODE else m
            for bv in (0, 1):
                want = MR.pack(oracle(mm, tau, spacing, op, bv))
                what = f"tau {tau} on {spacing}, {shape}: op {op}, border {bv}"
                same(abi_ball(src, shape, rows, op, bv), want, what)
                if ones.any():
                    same(abi_ball(src | ones, shape, rows, op, bv), want, what + ", input tails set")


@pytest.mark.parametrize("shape", R.WIDE_SHAPES)
def test_half_width_63_across_both_word_seams_and_faces(shape):
    tau, spacing = R.WIDE
    el = _M().BallElement(tau, spacing)
    assert el.radii == (1, 1, 63) and int(el.half_widths.max()) == 63, "the wide case no longer has r_x = 63 with r_z = r_y = 1"
    rows = rows_of(tau, spacing)
    D, Hh, W = shape
    single = np.zeros(shape, dtype=np.uint8)
    single[D // 2, Hh // 2, 64] = 1                                  # reaches x = 1 .. 127: both seams of word 1
    ends = np.zeros(shape, dtype=np.uint8)
    ends[0, 0, 0] = ends[-1, -1, -1] = ends[0, -1, 63] = 1           # spreads past both faces
    for name, m in (("one voxel at x = 64", single), ("voxels at the faces", ends), ("bernoulli", R.mask_for(shape, 77, 0.03))):
        ones = MR.tail_ones(shape)
        for op in (DILATE, ERODE):
            mm = 1 - m if op == ERODE else m
            for bv in (0, 1):
                same(abi_ball(MR.pack(mm) | ones, shape, rows, op, bv), MR.pack(oracle(mm, tau, spacing, op, bv)), f"{name} in {shape}: op {op}, border {bv}")
    want = np.zeros(shape, dtype=np.uint8)
    want[D // 2, Hh // 2, 1:128] = 1
    got = abi_ball(MR.pack(single), shape, rows, DILATE, 0).view(np.uint64).reshape(D, Hh, -1)
    assert got[D // 2, Hh // 2, 0] == np.uint64(0xFFFFFFFFFFFFFFFE) and got[D // 2, Hh // 2, 1] == np.uint64(0xFFFFFFFFFFFFFFFF), "the centre row is not x = 1 .. 127"


def test_gate():
    shape, (tau, spacing) = (4, 5, 130), R.ELEMENTS[3]
    rows = rows_of(tau, spacing)
    m = MR.inner_boundary(DR.ball(shape, (2, 2, 60), 2) | DR.ball(shape, (1, 3, 120), 1), 6)
    other = MR.inner_boundary(DR.ball(shape, (2, 3, 62), 2) | R.mask_for(shape, 5, 0.02), 6)
    words, ones, nw = MR.pack(m), MR.tail_ones(shape), MR.words(shape)
    full = MR.pack(np.ones(shape, dtype=np.uint8))
    for op, bv in ((DILATE, 0), (ERODE, 1), (DILATE, 1), (ERODE, 0)):
        want = MR.pack(oracle(m, tau, spacing, op, bv))
        what = f"op {op}, border {bv}"
        same(abi_ball(words, shape, rows, op, bv, None), want, "no gate, " + what)
        same(abi_ball(words, shape, rows, op, bv, full), want, "a gate of ones, " + what)
        same(abi_ball(words, shape, rows, op, bv, full | ones), want, "a gate of ones with its tails set, " + what)
        same(abi_ball(words, shape, rows, op, bv, MR.pack(other)), want & MR.pack(other), "a sparse gate, " + what)
        same(abi_ball(words, shape, rows, op, bv, np.zeros(nw, dtype=np.int64)), np.zeros(nw, dtype=np.int64), "a gate of zeros, " + what)
        same(abi_ball(words | ones, shape, rows, op, bv, "in"), want & words, "gate == in, " + what)
    assert (MR.pack(oracle(m, tau, spacing, DILATE, 0)) & MR.pack(other)).any() and (MR.pack(other) & ~MR.pack(oracle(m, tau, spacing, DILATE, 0))).any()


def test_garbage_records_stay_inside_out():
    """the entry cannot validate the list: any int32s are read as (signed byte, signed byte, 6 bits) and every fetch is bounds-checked"""
    rng = np.random.default_rng(3535)
    wild = rng.integers(-2 ** 31, 2 ** 31, 24, dtype=np.int64).astype(np.int32)
    near = ((rng.integers(-2, 3, 24) & 0xff) | ((rng.integers(-3, 4, 24) & 0xff) << 8) | (rng.integers(0, 2 ** 16, 24) << 16)).astype(np.uint32).view(np.int32)
    for shape in ((7, 9, 11), (3, 4, 130)):
        m = R.mask_for(shape, 99, 0.1)
        for rows in (wild, near, np.concatenate([wild[:8], near[:8]])):
            for op, bv in ((DILATE, 0), (ERODE, 1), (DILATE, 1), (ERODE, 0)):
                mm = 1 - m if op == ERODE else m
                same(abi_ball(MR.pack(mm) | MR.tail_ones(shape), shape, rows, op, bv), MR.pack(R.apply_rows(mm, rows, op, bv)), f"garbage records in {shape}: op {op}, border {bv}")


def test_above_the_grid_cap():
    """one thread per word and no tile: W = 1 makes every voxel a word, and just above 256 x cap of them the loop takes its second trip"""
    H = _H()
    cap = H.query("vx_morph_grid_cap")
    shape = (256 * cap // 1024 + 1, 1024, 1)
    assert 256 * cap < MR.words(shape) < 1.01 * 256 * cap, "the volume no longer sits just above the grid cap"
    rows = rows_of(1.0, UNIT)
    assert sorted(R.unpack_rows(rows)) == [(-1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)]          # the 6-neighbourhood
    m = MR.bernoulli(shape, 0.05, 61)
    m[0, 0, 0] = m[-1, -1, -1] = 1
    words = m.reshape(-1).astype(np.int64)                           # W = 1: a word is a voxel
    gate = MR.bernoulli(shape, 0.3, 62).reshape(-1).astype(np.int64)
    want = MR.dilate(m, 6, 1).reshape(-1).astype(np.int64)
    assert np.array_equal(abi_ball(words, shape, rows, DILATE, 0), want), "above the cap"
    assert np.array_equal(abi_ball(words, shape, rows, DILATE, 0, gate), want & gate), "above the cap, gated"
    assert np.array_equal(abi_ball(1 - words, shape, rows, ERODE, 1), 1 - want), "above the cap, erosion"


def test_refused_calls_leave_the_prefill():
    H = _H()
    shape = (4, 5, 70)
    nw = MR.words(shape)
    src, gate = torch.zeros(nw, dtype=torch.int64, device="cuda"), torch.zeros(nw, dtype=torch.int64, device="cuda")
    rows = dev(rows_of(1.0, UNIT))
    out = guard(nw)
    st, cap = H.stream_ptr(), H.query("vx_morph_ball_max_rows")
    ball = lambda **kw: (kw.get("src", src.data_ptr()), kw.get("gate", gate.data_ptr()), kw.get("out", out.ptr), *kw.get("shape", shape), kw.get("rows", rows.data_ptr()),
                         kw.get("n", rows.numel()), kw.get("op", 0), kw.get("bv", 0), st)
    for args, msg in ((ball(src=None), "null"), ((src.data_ptr(), None, None, *shape, rows.data_ptr(), 5, 0, 0, st), "null"), (ball(rows=None), "null"),
                      (ball(src=out.ptr), "neither in nor gate"), (ball(gate=out.ptr), "neither in nor gate"), (ball(shape=(4, 0, 70)), "bad sizes"),
                      (ball(shape=(2048, 1024, 1024)), "bad sizes"), (ball(n=0), "rows"), (ball(n=-2), "rows"), (ball(n=cap + 1), "rows"), (ball(op=2), "op"), (ball(op=-1), "op"),
                      (ball(bv=2), "border_value"), (ball(bv=-1), "border_value")):
        with pytest.raises(RuntimeError, match=msg):
            H.call("vx_morph_ball", *args)
    torch.cuda.synchronize()
    out.check("refused call")
    assert bool((out.t == I64_FILL).all()), "a refused call wrote out"
    assert not bool(src.any()) and not bool(gate.any())
    el = _M().BallElement(40.0)                                      # more rows than a call takes
    assert el.n_rows > cap
    with pytest.raises(ValueError, match=str(cap)):
        _M().ball_dilation(torch.zeros(shape, dtype=torch.uint8, device="cuda"), el, method="ball")
    with pytest.raises(ValueError, match="63"):
        _M().ball_dilation(torch.zeros(shape, dtype=torch.uint8, device="cuda"), 70.0, method="ball")
    x = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    for fn, bv in ((_M().ball_dilation, 1), (_M().ball_erosion, 0)):
        with pytest.raises(ValueError, match="edt"):
            fn(x, 1.0, border_value=bv, method="edt")
    with pytest.raises(ValueError, match="method"):
        _M().ball_dilation(x, 1.0, method="tile")
    with pytest.raises(ValueError, match="no labels"):
        _M().ball_dilation(_M().pack(x), 1.0, label=1)


# ====================================================================================================================== the library
IDENTITY = ((UNIT, 2.5), (R.ANISO, 4.0), ((0.7, 0.7, 0.7), 5.0))


@pytest.mark.parametrize("spacing,tau", IDENTITY)
def test_identity_on_the_device(spacing, tau, monkeypatch):
    """two routes to the same bits: the row-list kernel and the exact distance transform compared with q"""
    M = _M()
    from veloxseg_amd.utils import distance as Dm
    q = M.sq_threshold(tau)
    surf = dev(R.ball_surface())
    solid = dev((DR.ball((24, 40, 70), (9, 14, 20), 7) | DR.ball((24, 40, 70), (14, 25, 50), 9)).astype(np.uint8))
    want_d = Dm.distance_to(surf, spacing, squared=True) <= q
    want_e = Dm.distance_transform_edt(solid, spacing, squared=True) > q
    assert bool(want_d.any()) and not bool(want_d.all()) and bool((want_e != (solid != 0)).any())
    by_ball_d, by_ball_e = M.ball_dilation(surf, tau, spacing, method="ball"), M.ball_erosion(solid, tau, spacing, 1, method="ball")
    assert torch.equal(by_ball_d != 0, want_d), "ball_dilation against the thresholded transform"
    assert torch.equal(by_ball_e != 0, want_e), "ball_erosion (border 1) against the thresholded transform of the complement"
    assert torch.equal(M.ball_dilation(surf, tau, spacing, method="edt"), by_ball_d) and torch.equal(M.ball_erosion(solid, tau, spacing, 1, method="edt"), by_ball_e)
    for switch in (0, 10 ** 9):                                      # method=None on either side of the switch
        monkeypatch.setattr(M, "BALL_ROWS_SWITCH", switch)
        assert torch.equal(M.ball_dilation(surf, tau, spacing), by_ball_d) and torch.equal(M.ball_erosion(solid, tau, spacing, 1), by_ball_e)
        assert torch.equal(M.ball_erosion(solid, tau, spacing), M.ball_erosion(solid, tau, spacing, method="ball")), "border 0 has no transform route: the kernel serves"


def test_library_equals_reference():
    M = _M()
    lab = MR.volumes()["multiclass_10x12x70"]
    m = (lab != 0).astype(np.uint8)
    fns = ((M.ball_dilation, R.dilate), (M.ball_erosion, R.erode), (M.ball_opening, R.opening), (M.ball_closing, R.closing))
    for tau, spacing in ((1.5, UNIT), (4.0, R.ANISO)):
        for fn, ref in fns:
            for bv in (0, 1):
                what = f"{fn.__name__}, tau {tau} on {spacing}, border {bv}"
                got = fn(dev(lab), tau, spacing, bv)
                assert got.dtype == torch.uint8 and got.shape == lab.shape
                same(got, ref(m, tau, spacing, bv), what)
                same(fn(dev(lab), tau, spacing, bv, method="ball"), ref(m, tau, spacing, bv), what + ', method="ball"')
            p = fn(M.pack(dev(lab)), tau, spacing)
            assert isinstance(p, M.PackedMask)
            same(M.unpack(p), ref(m, tau, spacing), f"{fn.__name__} of a packed mask")
            same(fn(dev(lab), tau, spacing, label=2), ref(lab == 2, tau, spacing), f"{fn.__name__} of one class")
            same(fn(dev(lab), M.BallElement(tau, spacing)), ref(m, tau, spacing), f"{fn.__name__} with a ready element")
    other = MR.bernoulli(lab.shape, 0.6, 71)
    batch = dev(np.stack([m, other])[:, None])
    got = M.ball_closing(batch, 2.0, (1.0, 1.0, 2.0))
    assert got.shape == batch.shape and got.dtype == torch.uint8
    same(got[0, 0], R.closing(m, 2.0, (1.0, 1.0, 2.0)), "batch sample 0")
    same(got[1, 0], R.closing(other, 2.0, (1.0, 1.0, 2.0)), "batch sample 1")
    b = M.ball_erosion(dev(m).bool(), 1.0)
    assert b.dtype == torch.bool
    same(b, R.erode(m, 1.0), "a bool tensor")
    same(M.ball_dilation(dev(m), 0.0), m, "radius 0 is the identity")
    el = M.BallElement(2.0)
    assert el.rows("cuda") is el.rows("cuda"), "the record list is made once per device"
    same(M.unpack(M.ball_dilation(M.ball_erosion(M.pack(dev(m)), el), el)), R.opening(m, 2.0), "erosion then dilation, packed in between")


# ====================================================================================================================== the metrics
def _check_pair(a, b, tau, spacing, what):
    from veloxseg_amd.utils.metric import surface as S
    da, db = dev(a), dev(b)
    assert S.surface_overlap(da, db, tau, spacing) == R.surface_overlap(a, b, tau, spacing), f"counts of {what}"
    got = S.normalized_surface_dice(da, db, tau, spacing)
    assert isinstance(got, float) and got == R.normalized_surface_dice(a, b, tau, spacing), f"surface Dice of {what}"
    assert S.normalized_surface_dice(db, da, tau, spacing) == R.normalized_surface_dice(b, a, tau, spacing), f"surface Dice of {what}, swapped"
    return got


@pytest.mark.parametrize("spacing", DR.SURFACE_SPACINGS)
@pytest.mark.parametrize("name", list(DR.surface_cases()))
def test_surface_dice_equals_reference(name, spacing):
    a, b = DR.surface_cases()[name]
    for tau in R.METRIC_TAUS:
        got = _check_pair(a, b, tau, spacing, f"{name}, tau {tau} on {spacing}")
        if name == "identical":
            assert got == 2.0 / (2.0 + 1e-8)


@pytest.mark.parametrize("spacing", DR.SURFACE_SPACINGS)
def test_surface_dice_of_brats_regions(spacing):
    out, tgt = DR.brats_maps()
    for tau in R.METRIC_TAUS:
        for region, fn in (("et", lambda x: x == 3), ("tc", lambda x: (x == 1) | (x == 3)), ("wt", lambda x: x != 0)):
            _check_pair(fn(out).astype(np.uint8), fn(tgt).astype(np.uint8), tau, spacing, f"{region}, tau {tau} on {spacing}")


def test_surface_dice_beyond_the_kernel_cap_and_conventions():
    from veloxseg_amd.utils.metric import metrics as Mb, surface as S
    M = _M()
    a, b = DR.surface_cases()["offset_balls"]
    assert M.BallElement(40.0).n_rows > _H().query("vx_morph_ball_max_rows") and M.BallElement(100.0).n_rows is None
    for tau in (40.0, 100.0):                                        # too many rows; a radius above 63 voxels: the distance transform serves
        _check_pair(a, b, tau, None if tau == 40.0 else UNIT, f"offset_balls at tau {tau}")
    da, db, zero = dev(a), dev(b), torch.zeros(a.shape, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="first supplied"):
        S.surface_overlap(zero, db, 1.0)
    with pytest.raises(RuntimeError, match="second supplied"):
        S.normalized_surface_dice(da, zero, 1.0)
    assert math.isnan(Mb.get_surface_dice(zero[None, None], db[None, None], 1.0)) and math.isnan(Mb.get_surface_dice(da[None, None], zero[None, None], 1.0))
    assert Mb.get_surface_dice(db[None, None], da[None, None], 2.5, DR.SPACINGS[2]) == R.surface_dice_or_nan(b, a, 2.5, DR.SPACINGS[2])
    assert Mb.get_surface_dice(db[None, None].bool(), da[None, None].float(), 1.0) == R.surface_dice_or_nan(b, a, 1.0)
    p = S.surface_overlap(M.pack(da), M.pack(db), 1.0)
    assert p == R.surface_overlap(a, b, 1.0), "packed masks in"
