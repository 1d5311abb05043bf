"""The numpy oracle of the distance-transform kernels (tests/distance_ref.py) against the brute-force definition, against scipy.ndimage.distance_transform_edt on every
input tests/test_distance_gpu.py uses, and -- for the surface metrics -- against medpy's formulas restated with scipy's binary_erosion, distance_transform_edt and
np.percentile; the header symbols; every refusal of the C entries (they answer before anything is launched, so also on a machine without a GPU) and of the Python
surface.  No GPU.  That both command lines still refuse --use_hd95 is held by tests/test_ensemble_cpu.py."""
import math

import numpy as np
import pytest
import torch

import distance_ref as R

SMALL = (7, 9, 11)


def _scipy():
    return pytest.importorskip("scipy.ndimage")


# ---------------------------------------------------------------------------------------------------------------------- the oracle's premise
@pytest.mark.parametrize("spacing", R.SPACINGS)
@pytest.mark.parametrize("density", [0.02, 0.3])
def test_separable_equals_brute_force_equals_scipy(density, spacing):
    m = np.random.default_rng(int(density * 100)).random(SMALL) < density
    assert m.any()
    brute = R.brute_sq(m, spacing)
    assert np.array_equal(R.edt_sq(m, spacing), brute)
    assert np.array_equal(_scipy().distance_transform_edt(~m, sampling=spacing), np.sqrt(brute))


def test_separable_equals_brute_force_on_degenerate_volumes():
    for shape in ((1, 1, 1), (1, 1, 9), (6, 1, 2), (3, 4, 1)):
        for pattern in R.PATTERNS:
            m = R.sites(shape, pattern, 3)
            assert np.array_equal(R.edt_sq(m, R.SPACINGS[2]), R.brute_sq(m, R.SPACINGS[2])), (shape, pattern)
    assert np.isposinf(R.edt_sq(np.zeros(SMALL, dtype=bool))).all() and not R.edt_sq(np.ones(SMALL, dtype=bool)).any()


@pytest.mark.parametrize("name", list(R.cases()))
def test_oracle_equals_scipy_on_every_gpu_input(name):
    m, spacing = R.cases()[name]
    if not m.any():                                         # scipy's result without any site is unspecified; ours is defined
        assert np.isposinf(R.oracle_sq(name)).all()
        return
    assert np.array_equal(np.sqrt(R.oracle_sq(name)), _scipy().distance_transform_edt(~m, sampling=spacing))


def test_oracle_equals_scipy_at_the_extent_cap():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    cap = _hip.query("vx_edt_max_extent")
    assert 2 * 8 * cap <= 160 * 1024, "two workgroups holding one line each no longer fit a CU's LDS"
    for name, (m, spacing) in R.cap_cases(cap).items():
        assert max(m.shape) == cap and m.size == 2 * cap
        assert np.array_equal(np.sqrt(R.edt_sq(m, spacing)), _scipy().distance_transform_edt(~m, sampling=spacing)), name


def test_lattice_arithmetic_equals_the_oracle():
    """the expectation of the GPU file's grid-cap case, on small volumes with the same periods"""
    for shape, period in (((5, 30, 37), (1, 9, 11)), ((23, 17, 1), (7, 5, 1)), ((20, 2, 40), (6, 2, 9))):
        for spacing in (R.SPACINGS[0], R.SPACINGS[2]):
            assert np.array_equal(R.lattice_sq(shape, period, spacing), R.edt_sq(R.lattice_sites(shape, period), spacing)), (shape, period)
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    cap = _hip.query("vx_edt_grid_cap")
    g = R.grid_cap_shapes(cap)
    (_, H, W), _ = g["z"]
    assert 256 * cap < H * W < 1.01 * 256 * cap
    (D, H, _), _ = g["x"]
    assert 256 * cap < D * H < 1.01 * 256 * cap
    (D, H, W), _ = g["y"]
    assert H <= 128 and cap < D * ((W + 31) // 32) < 1.01 * cap


# ---------------------------------------------------------------------------------------------------------------------- surface metrics: medpy restated with scipy
def _medpy_surface_distances(result, reference, voxelspacing):
    """medpy 0.4 metric/binary.py: __surface_distances with connectivity=1"""
    ndi = _scipy()
    result, reference = np.atleast_1d(result.astype(bool)), np.atleast_1d(reference.astype(bool))
    footprint = ndi.generate_binary_structure(result.ndim, 1)
    if 0 == np.count_nonzero(result):
        raise RuntimeError("The first supplied array does not contain any binary object.")
    if 0 == np.count_nonzero(reference):
        raise RuntimeError("The second supplied array does not contain any binary object.")
    result_border = result ^ ndi.binary_erosion(result, structure=footprint, iterations=1)
    reference_border = reference ^ ndi.binary_erosion(reference, structure=footprint, iterations=1)
    dt = ndi.distance_transform_edt(~reference_border, sampling=voxelspacing)
    return dt[result_border]


@pytest.mark.parametrize("spacing", R.SURFACE_SPACINGS)
@pytest.mark.parametrize("name", list(R.surface_cases()))
def test_surface_oracle_equals_medpy_restated(name, spacing):
    a, b = R.surface_cases()[name]
    ab, ba = _medpy_surface_distances(a, b, spacing), _medpy_surface_distances(b, a, spacing)
    assert np.array_equal(R.surface_distances(a, b, spacing), ab) and np.array_equal(R.surface_distances(b, a, spacing), ba)
    assert R.hd95(a, b, spacing) == float(np.percentile(np.hstack((ab, ba)), 95))
    assert R.hd(a, b, spacing) == float(max(ab.max(), ba.max()))
    assert R.asd(a, b, spacing) == float(ab.mean()) and R.assd(a, b, spacing) == float(np.mean((ab.mean(), ba.mean())))
    if name == "identical":
        assert R.hd(a, b, spacing) == R.hd95(a, b, spacing) == R.asd(a, b, spacing) == R.assd(a, b, spacing) == 0.0
    else:
        assert R.hd(a, b, spacing) >= R.hd95(a, b, spacing) > 0.0


def test_surface_oracle_raises_on_an_empty_mask_and_brats_regions():
    a, _ = R.surface_cases()["nested_boxes"]
    with pytest.raises(RuntimeError, match="first supplied"):
        R.surface_distances(np.zeros_like(a), a)
    with pytest.raises(RuntimeError, match="second supplied"):
        R.surface_distances(a, np.zeros_like(a))
    assert math.isnan(R.reference_hd95(np.zeros_like(a), a)) and math.isnan(R.reference_hd95(a, np.zeros_like(a)))
    out, tgt = R.brats_maps()
    avg, et, tc, wt = R.cal_hd95(out, tgt, R.SPACINGS[2])
    assert all(v > 0.0 and math.isfinite(v) for v in (avg, et, tc, wt))
    assert et == float(np.percentile(np.hstack((_medpy_surface_distances(out == 3, tgt == 3, R.SPACINGS[2]), _medpy_surface_distances(tgt == 3, out == 3, R.SPACINGS[2]))), 95))


def test_percentile_of_square_roots_from_the_squared_order_statistics():
    """what hd95 does on the host: the two bracketing order statistics of the SQUARED values, their square roots, numpy's linear rule"""
    from veloxseg_amd.utils.preprocess import linear_lerp, linear_ranks
    rng = np.random.default_rng(5)
    for n in list(range(1, 60)) + [101, 1000, 4321]:
        sq = np.sort(rng.random(n) * 50.0)
        v, lo, hi = linear_ranks(n, 95.0)
        assert linear_lerp(math.sqrt(sq[lo]), math.sqrt(sq[hi]), v, lo) == float(np.percentile(np.sqrt(sq), 95)), n


# ---------------------------------------------------------------------------------------------------------------------- header and refusals
def test_header_symbols():
    from veloxseg_amd import _hip
    protos = _hip.parse_header()
    names = lambda f: [n for _, n in protos[f][1]]
    assert names("vx_edt_sq") == ["bits", "invert", "out_sq", "D", "H", "W", "sz", "sy", "sx", "stream"]
    assert [t for t, _ in protos["vx_edt_sq"][1]][6:9] == ["double"] * 3
    assert names("vx_edt_pass") == ["axis", "bits", "invert", "io", "D", "H", "W", "spacing", "stream"]
    assert names("vx_edt_sqrt") == ["x", "n", "stream"] and names("vx_bits_count") == ["bits", "D", "H", "W", "counts", "stream"]
    assert names("vx_edt_gather") == ["values", "bits", "offsets", "out", "D", "H", "W", "stream"]
    assert protos["vx_edt_max_extent"][1] == [] and protos["vx_edt_grid_cap"][1] == []


def test_entries_refuse_bad_arguments_without_gpu():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    cap = _hip.query("vx_edt_max_extent")
    assert cap == 2048 and _hip.query("vx_edt_grid_cap") >= 1
    ok = dict(bits=4096, invert=0, out=8192, D=3, H=4, W=70, sz=1.0, sy=1.0, sx=1.0)          # pointers that are never dereferenced

    def sq(**kw):
        a = dict(ok, **kw)
        _hip.call("vx_edt_sq", a["bits"], a["invert"], a["out"], a["D"], a["H"], a["W"], a["sz"], a["sy"], a["sx"], None)

    def one(axis, spacing=1.0, **kw):
        a = dict(ok, **kw)
        _hip.call("vx_edt_pass", axis, a["bits"], a["invert"], a["out"], a["D"], a["H"], a["W"], spacing, None)
    for kw in (dict(bits=None), dict(out=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            sq(**kw)
    for axis, kw in ((0, dict(bits=None)), (0, dict(out=None)), (1, dict(out=None)), (2, dict(out=None))):
        with pytest.raises(RuntimeError, match="null pointer"):
            one(axis, **kw)
    sizes = [dict(D=0), dict(H=0), dict(W=0), dict(D=-1), dict(H=-3), dict(W=-70), dict(D=cap + 1), dict(H=cap + 1), dict(W=cap + 1), dict(D=cap, H=cap, W=cap)]
    for kw in sizes:
        with pytest.raises(RuntimeError, match="bad sizes"):
            sq(**kw)
        with pytest.raises(RuntimeError, match="bad sizes"):
            one(1, **kw)
        with pytest.raises(RuntimeError, match="bad sizes"):
            _hip.call("vx_bits_count", 4096, kw.get("D", 3), kw.get("H", 4), kw.get("W", 70), 8192, None)
        with pytest.raises(RuntimeError, match="bad sizes"):
            _hip.call("vx_edt_gather", 4096, 8192, 12288, 16384, kw.get("D", 3), kw.get("H", 4), kw.get("W", 70), None)
    for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.0, -1.5):
        for key in ("sz", "sy", "sx"):
            with pytest.raises(RuntimeError, match="spacing"):
                sq(**{key: bad})
        for axis in (0, 1, 2):
            with pytest.raises(RuntimeError, match="spacing"):
                one(axis, bad)
    for inv in (-1, 2):
        with pytest.raises(RuntimeError, match="invert"):
            sq(invert=inv)
        with pytest.raises(RuntimeError, match="invert"):
            one(0, invert=inv)
    for axis in (-1, 3):
        with pytest.raises(RuntimeError, match="axis"):
            one(axis)
    for args, msg in (((None, 5, None), "null pointer"), ((4096, 0, None), "bad size"), ((4096, -1, None), "bad size"), ((4096, 2 ** 31, None), "bad size")):
        with pytest.raises(RuntimeError, match=msg):
            _hip.call("vx_edt_sqrt", *args)
    for args in ((None, 3, 4, 70, 8192, None), (4096, 3, 4, 70, None, None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            _hip.call("vx_bits_count", *args)
    for k in range(4):
        ptrs = [4096, 8192, 12288, 16384]
        ptrs[k] = None
        with pytest.raises(RuntimeError, match="null pointer"):
            _hip.call("vx_edt_gather", *ptrs, 3, 4, 70, None)


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    from veloxseg_amd.utils import distance as Dm
    from veloxseg_amd.utils.metric import metrics as Mb, metrics_brats as Mr, surface as S
    x = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for fn in (Dm.distance_transform_edt, Dm.distance_to):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x.float())
        for bad in ((1.0, 2.0), (1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), (float("inf"), 1.0, 1.0), -1.0):
            with pytest.raises(ValueError, match="spacings"):
                fn(x, sampling=bad)
    for fn in (S.surface_distances, S.hd, S.hd95, S.asd, S.assd):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x.float(), x.float())
    for fn in (Mb.get_hausdorff, Mr.HD95, Mr.cal_hd95):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x[None, None], x[None, None])
    assert Dm._sampling(None, "t") == (1.0, 1.0, 1.0) and Dm._sampling(2, "t") == (2.0, 2.0, 2.0) and Dm._sampling(np.array([1.5, 0.75, 2]), "t") == (1.5, 0.75, 2.0)
