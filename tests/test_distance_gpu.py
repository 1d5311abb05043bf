"""The distance-transform kernels (csrc/distance.hip), the Python surface built on them (utils/distance.py, utils/metric/surface.py) and the reference-named wrappers
against the numpy oracle of tests/distance_ref.py.

The squared map is held to `==`: the definition fixes every rounding, and tests/test_distance_cpu.py holds the oracle to the brute-force definition and to
scipy.ndimage.distance_transform_edt on every input used here; this file needs no scipy.  The distances are held within 1 ulp of np.sqrt(oracle) (a correctly rounded
square root, one unit of slack; the test prints whether every element was equal).  surface_distances is `==` the oracle's array (np.sqrt of its squared values: `__dsqrt_rn` is correctly rounded), hd and hd95 are `==` as Python floats; asd and assd within (n - 1) 2^-53 relative,
the bound of an fp64 sum of n non-negative terms in any order.  Kernel outputs of the C-ABI tests sit between canaries (exact_ref.Guard) and are prefilled; a refused
call raises and leaves its prefill untouched.  Every grid-stride loop takes a second trip in test_above_the_grid_cap."""
import math

import numpy as np
import pytest
import torch

import distance_ref as R
import morphology_ref as MR
from exact_ref import Guard

pytestmark = pytest.mark.gpu

FILL = -7.0


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()
    return t if dtype is None else t.to(dtype)


def same(got, want, what):
    """bit equality of two fp64 arrays (+inf == +inf; a NaN anywhere fails)"""
    g = (got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)).reshape(-1)
    w = np.asarray(want, dtype=np.float64).reshape(-1)
    assert g.dtype == np.float64 and g.size == w.size, f"{what}: {g.dtype} x {g.size} against float64 x {w.size}"
    bad = ~(g == w)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first flat index {i}: got {g[i]!r}, want {w[i]!r}")


def abi_sq(mask, spacing, invert=0, tails=False):
    """vx_edt_sq through the C ABI on a host mask of the SET bits -> (D, H, W) fp64 device tensor out of a guarded, prefilled buffer"""
    H = _H()
    words = MR.pack(mask)
    if tails:
        words = words | MR.tail_ones(mask.shape)
    src = dev(words)
    keep = src.clone()
    out = Guard(mask.shape, torch.float64, fill=FILL)
    H.call("vx_edt_sq", src.data_ptr(), invert, out.ptr, *mask.shape, *spacing, H.stream_ptr())
    torch.cuda.synchronize()
    out.check("vx_edt_sq")
    assert torch.equal(src, keep), "vx_edt_sq wrote its input"
    return out.t


# ====================================================================================================================== the squared map
@pytest.mark.parametrize("name", list(R.cases()))
def test_squared_map_equals_oracle(name):
    m, spacing = R.cases()[name]
    same(abi_sq(m, spacing), R.oracle_sq(name), name)


def test_lines_at_the_extent_cap():
    cap = _H().query("vx_edt_max_extent")
    for name, (m, spacing) in R.cap_cases(cap).items():
        same(abi_sq(m, spacing), R.edt_sq(m, spacing), name)


@pytest.mark.parametrize("name", ["9x33x65_bern30", "9x33x65_bern97", "17x40x130_bern2", "17x40x130_bern30", "17x40x130_corner", "17x40x130_none", "17x40x130_all"])
def test_invert_and_tail_bits(name):
    """sites as the CLEAR bits of the complement (invert 1), on widths that are no multiple of 64, with the input's tail bits clear and set: a clear tail bit taken
    for a site under invert 1, or a set one under invert 0, changes the map"""
    m, spacing = R.cases()[name]
    assert m.shape[2] % 64
    want = R.oracle_sq(name)
    for tails in (False, True):
        same(abi_sq(~m, spacing, 1, tails), want, f"{name}: invert 1, tails {tails}")
        same(abi_sq(m, spacing, 0, tails), want, f"{name}: invert 0, tails {tails}")


def test_single_passes():
    """vx_edt_pass: the three passes one by one give the map of vx_edt_sq; pass 0 alone is t_z of the integer column distance"""
    H = _H()
    m, spacing = R.cases()["17x40x130_bern2"]
    src = dev(MR.pack(m))
    out = Guard(m.shape, torch.float64, fill=FILL)
    H.call("vx_edt_pass", 0, src.data_ptr(), 0, out.ptr, *m.shape, spacing[0], H.stream_ptr())
    torch.cuda.synchronize()
    same(out.t, _column_only(m, spacing[0]), "pass 0")
    H.call("vx_edt_pass", 1, None, 0, out.ptr, *m.shape, spacing[1], H.stream_ptr())
    H.call("vx_edt_pass", 2, None, 0, out.ptr, *m.shape, spacing[2], H.stream_ptr())
    torch.cuda.synchronize()
    out.check("vx_edt_pass")
    same(out.t, R.oracle_sq("17x40x130_bern2"), "passes 0, 1, 2")


def _column_only(m, sz):
    """t_z of the distance to the nearest site of the same (y, x) column, +inf for a column without one"""
    out = np.full(m.shape, np.inf)
    for z in range(m.shape[0]):
        cand = np.where(m[z][None], R.term(np.arange(m.shape[0]) - z, sz)[:, None, None], np.inf)
        out = np.minimum(out, cand)
    return out


def test_two_runs_give_equal_bits():
    for name in ("40x36x70_bern2", "17x40x130_balls"):
        m, spacing = R.cases()[name]
        assert torch.equal(abi_sq(m, spacing), abi_sq(m, spacing)), name


# ====================================================================================================================== the second loop trip
def test_above_the_grid_cap():
    """per kernel the smallest volume at which its grid-stride loop takes a second trip (distance_ref.grid_cap_shapes); sites on a lattice, the expectation by
    arithmetic (tests/test_distance_cpu.py checks that arithmetic against the oracle on small volumes)"""
    H = _H()
    cap = H.query("vx_edt_grid_cap")
    shapes = R.grid_cap_shapes(cap)
    (_, Hh, W), _ = shapes["z"]
    assert 256 * cap < Hh * W
    (D, Hh, _), _ = shapes["x"]
    assert 256 * cap < D * Hh
    (D, Hh, W), _ = shapes["y"]
    assert Hh <= 128 and cap < D * ((W + 31) // 32)
    spacing = R.SPACINGS[2]
    for which, (shape, period) in shapes.items():
        sites = R.lattice_sites(shape, period)
        want = R.lattice_sq(shape, period, spacing)
        got = abi_sq(sites, spacing)
        assert torch.equal(got, dev(want)), f"squared map above the cap of the {which} pass"
        if which != "x":
            continue
        # count, gather and square root above the cap: W = 1 makes every voxel a row and a word
        st, n = H.stream_ptr(), int(sites.sum())
        pick = np.zeros(shape, dtype=bool)
        pick.reshape(-1)[::3] = True
        bits = dev(MR.pack(pick))
        counts = Guard((shape[0] * shape[1],), torch.int32, fill=-7, canary=0x5A5A5A5A)
        H.call("vx_bits_count", bits.data_ptr(), *shape, counts.ptr, st)
        offsets = torch.cumsum(counts.t, 0, dtype=torch.int64) - counts.t
        out = Guard((int(pick.sum()),), torch.float64, fill=FILL)
        H.call("vx_edt_gather", got.data_ptr(), bits.data_ptr(), offsets.data_ptr(), out.ptr, *shape, st)
        root = Guard(shape, torch.float64, fill=got)
        H.call("vx_edt_sqrt", root.ptr, root.t.numel(), st)
        torch.cuda.synchronize()
        for g in (counts, out, root):
            g.check("above the grid cap")
        assert torch.equal(counts.t, dev(pick.reshape(-1).astype(np.int32))), "row counts above the cap"
        assert torch.equal(out.t, dev(want[pick])), "gather above the cap"
        _within_one_ulp(root.t, np.sqrt(want), "square root above the cap")
        assert n > 0


# ====================================================================================================================== distances and the python layer
def _within_one_ulp(got, want, what):
    g, w = got.detach().cpu().numpy().reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert g.dtype == np.float64 and g.size == w.size
    fin = np.isfinite(w)
    assert np.array_equal(g[~fin], w[~fin]), f"{what}: the infinite elements differ"
    err = np.abs(g[fin] - w[fin])
    equal = bool((err == 0).all())
    print(f"{what}: {int(fin.sum())} finite elements, every one equal to np.sqrt: {equal}; largest error {float((err / np.spacing(w[fin])).max()) if fin.any() else 0.0:.2f} ulp")
    assert bool((err <= np.spacing(w[fin])).all()), f"{what}: more than 1 ulp from np.sqrt of the oracle"
    return equal


@pytest.mark.parametrize("name", ["1x1x70_corner", "9x33x65_bern2", "17x40x130_balls", "40x36x70_bern30", "40x36x70_plane", "5x1x3_none"])
def test_distances_within_one_ulp(name):
    from veloxseg_amd.utils import distance as Dm
    m, spacing = R.cases()[name]
    want_sq = R.oracle_sq(name)
    got = Dm.distance_to(dev(m.astype(np.uint8)), spacing)
    assert got.dtype == torch.float64 and got.shape == m.shape
    _within_one_ulp(got, np.sqrt(want_sq), f"distance_to {name}")
    same(Dm.distance_to(dev(m.astype(np.uint8)), spacing, squared=True), want_sq, f"distance_to(squared) {name}")
    # scipy's form: the distance of the foreground ~m to the background m
    _within_one_ulp(Dm.distance_transform_edt(dev((~m).astype(np.uint8)), spacing), np.sqrt(want_sq), f"distance_transform_edt {name}")


def test_python_layer_inputs():
    from veloxseg_amd.utils import distance as Dm, morphology as M
    (a, sa), (b, _) = R.cases()["9x33x65_bern30"], R.cases()["9x33x65_bern97"]
    wa, wb = R.edt_sq(~a, sa), R.edt_sq(~b, sa)
    batch = dev(np.stack([a, b])[:, None].astype(np.uint8))
    got = Dm.distance_transform_edt(batch, sa, squared=True)
    assert got.shape == batch.shape and got.dtype == torch.float64
    same(got[0, 0], wa, "batch sample 0")
    same(got[1, 0], wb, "batch sample 1")
    for t in (dev(a), dev(a.astype(np.int32)), dev(a.astype(np.int64)) * 5, dev(a.astype(np.float32)) * 0.5, dev(a.astype(np.float64))):
        got = Dm.distance_transform_edt(t, sa, squared=True)
        assert got.shape == a.shape
        same(got, wa, f"a {t.dtype} input")
    lab = dev(np.where(a, 3, np.where(b, 1, 0)).astype(np.uint8))
    same(Dm.distance_transform_edt(lab, sa, squared=True, label=3), wa, "label=3")
    same(Dm.distance_transform_edt(lab.float(), sa, squared=True, label=3), wa, "label=3 of a float map")
    p = M.pack(dev(a.astype(np.uint8)))
    same(Dm.distance_transform_edt(p, sa, squared=True), wa, "a packed mask")
    same(Dm.distance_to(M.inner_boundary(p, 6), sa, squared=True), R.edt_sq(MR.inner_boundary(a, 6), sa), "pack -> boundary -> transform without an unpack")
    same(Dm.distance_transform_edt(dev(a.astype(np.uint8)), squared=True), R.edt_sq(~a), "default sampling")
    same(Dm.distance_transform_edt(dev(a.astype(np.uint8)), 2.0, squared=True), R.edt_sq(~a, (2.0, 2.0, 2.0)), "scalar sampling")
    assert bool(torch.isposinf(Dm.distance_transform_edt(torch.ones((3, 4, 5), dtype=torch.uint8, device="cuda"))).all()), "no background: +inf everywhere"
    cap = _H().query("vx_edt_max_extent")
    with pytest.raises(ValueError, match="exceed"):
        Dm.distance_to(torch.zeros((1, 1, cap + 1), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="no labels"):
        Dm.distance_transform_edt(p, label=1)


# ====================================================================================================================== refusals
def test_refused_abi_calls_leave_the_prefill():
    H = _H()
    cap = H.query("vx_edt_max_extent")
    shape = (4, 5, 70)
    nw = MR.words(shape)
    src = torch.zeros(nw, dtype=torch.int64, device="cuda")
    out = Guard(shape, torch.float64, fill=FILL)
    counts = Guard((20,), torch.int32, fill=-7, canary=0x5A5A5A5A)
    offs = torch.zeros(20, dtype=torch.int64, device="cuda")
    st = H.stream_ptr()
    sq = lambda **kw: ("vx_edt_sq", (kw.get("src", src.data_ptr()), kw.get("invert", 0), kw.get("out", out.ptr), *kw.get("shape", shape), *kw.get("s", (1.0, 1.0, 1.0)), st))
    one = lambda axis, s=1.0, **kw: ("vx_edt_pass", (axis, kw.get("src", src.data_ptr()), kw.get("invert", 0), out.ptr, *kw.get("shape", shape), s, st))
    calls = [(sq(src=None), "null"), (sq(out=None), "null"), (sq(invert=2), "invert"), (sq(shape=(4, 0, 70)), "bad sizes"), (sq(shape=(-4, 5, 70)), "bad sizes"),
             (sq(shape=(4, 5, cap + 1)), "bad sizes"), (sq(shape=(cap + 1, 5, 7)), "bad sizes"), (sq(shape=(cap, cap, cap)), "bad sizes"),
             (sq(s=(float("nan"), 1.0, 1.0)), "spacing"), (sq(s=(1.0, float("inf"), 1.0)), "spacing"), (sq(s=(1.0, 1.0, 0.0)), "spacing"), (sq(s=(1.0, -2.0, 1.0)), "spacing"),
             (one(0, src=None), "null"), (one(3), "axis"), (one(1, float("nan")), "spacing"), (one(2, 0.0), "spacing"), (one(1, shape=(4, cap + 1, 70)), "bad sizes"),
             (one(0, invert=-1), "invert"),
             (("vx_edt_sqrt", (out.ptr, 0, st)), "bad size"), (("vx_edt_sqrt", (None, 10, st)), "null"),
             (("vx_bits_count", (src.data_ptr(), 4, 5, 0, counts.ptr, st)), "bad sizes"), (("vx_bits_count", (None, *shape, counts.ptr, st)), "null"),
             (("vx_edt_gather", (out.ptr, src.data_ptr(), offs.data_ptr(), out.ptr, 4, 5, cap + 1, st)), "bad sizes"),
             (("vx_edt_gather", (out.ptr, src.data_ptr(), None, out.ptr, *shape, st)), "null")]
    for (name, args), msg in calls:
        with pytest.raises(RuntimeError, match=msg):
            H.call(name, *args)
    torch.cuda.synchronize()
    out.check("refused call: out")
    counts.check("refused call: counts")
    assert bool((out.t == FILL).all()) and bool((counts.t == -7).all()), "a refused call wrote its output"
    assert not bool(src.any())


# ====================================================================================================================== surface metrics
def _rel_bound(n):
    return (n - 1) * 2.0 ** -53


@pytest.mark.parametrize("spacing", R.SURFACE_SPACINGS)
@pytest.mark.parametrize("name", list(R.surface_cases()))
def test_surface_metrics_equal_oracle(name, spacing):
    from veloxseg_amd.utils.metric import surface as S
    a, b = R.surface_cases()[name]
    ta, tb = dev(a), dev(b)
    for (x, y), (hx, hy) in (((ta, tb), (a, b)), ((tb, ta), (b, a))):
        got = S.surface_distances(x, y, spacing, squared=True)
        assert got.dtype == torch.float64 and got.dim() == 1
        same(got, R.surface_sq(hx, hy, spacing), f"{name}: squared surface distances")
        same(S.surface_distances(x, y, spacing), R.surface_distances(hx, hy, spacing), f"{name}: surface distances")
    hd, hd95, asd, assd = S.hd(ta, tb, spacing), S.hd95(ta, tb, spacing), S.asd(ta, tb, spacing), S.assd(ta, tb, spacing)
    assert all(isinstance(v, float) for v in (hd, hd95, asd, assd))
    print(f"{name} {spacing}: hd {hd!r} hd95 {hd95!r} asd {asd!r} assd {assd!r}; oracle {R.hd(a, b, spacing)!r} {R.hd95(a, b, spacing)!r} {R.asd(a, b, spacing)!r} {R.assd(a, b, spacing)!r}")
    assert hd == R.hd(a, b, spacing) and hd95 == R.hd95(a, b, spacing)
    n_ab, n_ba = int(R.surface(a).sum()), int(R.surface(b).sum())
    want_asd, want_assd = R.asd(a, b, spacing), R.assd(a, b, spacing)
    assert abs(asd - want_asd) <= _rel_bound(n_ab) * want_asd
    assert abs(assd - want_assd) <= _rel_bound(max(n_ab, n_ba)) * want_assd
    assert S.hd95(tb, ta, spacing) == hd95 and S.hd(tb, ta, spacing) == hd, "hd and hd95 are symmetric"
    if name == "identical":
        assert hd == hd95 == asd == assd == 0.0


def test_surface_metrics_inputs_and_empty_masks():
    from veloxseg_amd.utils import morphology as M
    from veloxseg_amd.utils.metric import surface as S
    a, b = R.surface_cases()["offset_balls"]
    sp = R.SURFACE_SPACINGS[1]
    want = R.hd95(a, b, sp)
    ta, tb = dev(a), dev(b)
    forms = {"uint8": (ta, tb), "int32": (ta.int(), tb.int()), "int64": (ta.long() * 4, tb.long()), "bool": (ta.bool(), tb.bool()),
             "float": ((ta == 1).float(), (tb == 1).float()), "five axes": (ta[None, None], tb[None, None]), "packed": (M.pack(ta), M.pack(tb)),
             "mixed": (ta.bool(), tb[None, None].double() * 0.25)}
    for what, (x, y) in forms.items():
        assert S.hd95(x, y, sp) == want, what
    assert S.hd95(ta, tb, np.array(sp)) == want and S.hd95(ta, tb) == R.hd95(a, b)
    zero = torch.zeros_like(ta)
    for fn in (S.surface_distances, S.hd, S.hd95, S.asd, S.assd):
        with pytest.raises(RuntimeError, match="first supplied array does not contain"):
            fn(zero, tb)
        with pytest.raises(RuntimeError, match="second supplied array does not contain"):
            fn(ta, zero)
        with pytest.raises(RuntimeError, match="first supplied array does not contain"):
            fn(zero.float(), zero)
    with pytest.raises(ValueError, match="differ in shape"):
        S.hd(ta, tb[:, :, :-1])
    with pytest.raises(ValueError, match="one"):
        S.hd(torch.stack([ta, ta])[:, None], torch.stack([tb, tb])[:, None])
    assert S.hd95(ta, tb, sp) == S.hd95(ta, tb, sp), "two runs differ"


def test_reference_named_wrappers():
    from veloxseg_amd.utils.metric import metrics as Mb, metrics_brats as Mr
    a, b = R.surface_cases()["nested_boxes"]
    sp = R.SURFACE_SPACINGS[1]
    gt, pred = dev(a)[None, None], dev(b)[None, None]
    zero = torch.zeros_like(gt)
    for fn in (Mb.get_hausdorff, Mr.HD95):
        assert fn(gt, pred, sp) == R.reference_hd95(a, b, sp) and fn(gt, pred) == R.reference_hd95(a, b)
        assert fn(gt.float(), pred.float(), sp) == R.reference_hd95(a, b, sp), "float masks, as the reference passes them"
        assert math.isnan(fn(zero, pred)) and math.isnan(fn(gt, zero)) and math.isnan(fn(zero.float(), zero.float()))
        assert isinstance(fn(gt, pred), float)
    out, tgt = R.brats_maps()
    to, tt = dev(out)[None, None], dev(tgt)[None, None]
    for spacing in ((1, 1, 1), sp):
        assert Mr.cal_hd95(to, tt, spacing) == R.cal_hd95(out, tgt, spacing)
        assert Mr.cal_hd95(to.float(), tt.float(), spacing) == R.cal_hd95(out, tgt, spacing), "float label maps"
    no_et = np.where(out == 3, 1, out)                      # the prediction lacks class 3: ET is nan, and so is the average; TC and WT are numbers
    got, want = Mr.cal_hd95(dev(no_et)[None, None], tt, sp), R.cal_hd95(no_et, tgt, sp)
    assert math.isnan(got[0]) and math.isnan(got[1]) and math.isnan(want[0]) and math.isnan(want[1]) and got[2:] == want[2:]
    assert all(math.isnan(v) for v in Mr.cal_hd95(torch.zeros_like(to), tt))
