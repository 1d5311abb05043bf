"""The ball element and the normalised surface Dice without a GPU: the squared threshold, BallElement's tables against the brute-force
element of tests/ball_ref.py, the identity  dilation by the ball == (squared distance <= q) == (scipy's distance <= tau)  that ties the new kernel to the existing
transform, the metric's oracle against the formula written out on scipy's distances, the header prototypes, every refusal of vx_morph_ball (it answers before
anything is launched) and the Python layer's refusals."""
import math

import numpy as np
import pytest
import torch

import ball_ref as R
import distance_ref as DR

SMALL = (7, 9, 11)
UNIT = (1.0, 1.0, 1.0)
PAIRS = ((UNIT, 0.0), (UNIT, 1.0), (UNIT, math.sqrt(5.0)), ((0.7, 0.7, 0.7), 2.0), (R.ANISO, 4.0), (R.ANISO, 6.6))


def _scipy():
    return pytest.importorskip("scipy.ndimage")


def _M():
    from veloxseg_amd.utils import morphology as M
    return M


# ---------------------------------------------------------------------------------------------------------------------- the squared threshold
def test_sq_threshold_brackets_tau():
    M = _M()
    taus = [0.0, 1.0, math.sqrt(2.0), math.sqrt(5.0), 2.5, 1e-200, 1e160] + list(np.random.default_rng(35).random(2000) * 40.0) + \
        list(np.exp(np.random.default_rng(36).normal(0.0, 3.0, 1000)))
    for tau in taus:
        q = M.sq_threshold(float(tau))
        assert q == R.sq_threshold(tau)
        assert math.sqrt(q) <= tau < math.sqrt(math.nextafter(q, math.inf)), tau
    assert M.sq_threshold(0.0) == 0.0
    for tau, sq in ((1.0, 1.0), (2.5, 6.25)):              # q is the LARGEST such double: a few ulps above tau^2, whose square root still rounds to tau
        assert sq <= M.sq_threshold(tau) < sq * (1 + 2.0 ** -50) and math.sqrt(M.sq_threshold(tau)) == tau
    assert M.sq_threshold(math.sqrt(2.0)) >= 2.0 and M.sq_threshold(math.sqrt(5.0)) >= 5.0          # fl(sqrt(n)) is a radius that reaches the offsets of squared length n
    assert M.sq_threshold(math.nextafter(math.sqrt(5.0), 0.0)) < 5.0
    for bad in (-1.0, -1e-300, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="radius"):
            M.sq_threshold(bad)


# ---------------------------------------------------------------------------------------------------------------------- the element
@pytest.mark.parametrize("spacing", [UNIT, (0.7, 0.7, 0.7), R.ANISO])
def test_element_tables_equal_brute_force(spacing):
    M = _M()
    top = 6 * max(spacing)
    taus = [0.0, min(spacing), math.sqrt(2.0), math.sqrt(3.0), math.sqrt(5.0), 2.5, 6 * min(spacing), top] + list(np.random.default_rng(7).random(12) * top)
    for tau in taus:
        el = M.BallElement(tau, spacing)
        want = R.half_widths(R.element(float(tau), spacing))          # (asserts every row a symmetric interval)
        assert el.q == R.sq_threshold(tau) and el.radii == R.radii(tau, spacing)
        assert el.half_widths.dtype == np.int8 and el.half_widths.shape == (2 * el.radii[0] + 1, 2 * el.radii[1] + 1)
        assert np.array_equal(el.half_widths, want), (tau, spacing)
        assert el.n_rows == int((want >= 0).sum()) and int(el.half_widths.max()) == el.radii[2]
        assert el.half_widths[el.radii[0], el.radii[1]] == el.radii[2], "the centre row is the widest"
        rows = M.pack_rows(el.half_widths)
        assert rows.dtype == np.int32 and rows.size == el.n_rows
        assert sorted(R.unpack_rows(rows)) == sorted(R.unpack_rows(R.pack_rows(want)))
        back = np.full_like(want, -1)
        for dz, dy, hw in R.unpack_rows(rows):
            back[dz + el.radii[0], dy + el.radii[1]] = hw
        assert np.array_equal(back, want), "the records do not round-trip"
    assert max(R.radii(top, spacing)) >= 6
    one = M.BallElement(0.0, spacing)
    assert one.radii == (0, 0, 0) and one.n_rows == 1 and R.unpack_rows(M.pack_rows(one.half_widths)) == [(0, 0, 0)]


def test_known_unit_grid_elements():
    M = _M()
    count = lambda tau: int((M.BallElement(tau).half_widths.astype(int) * 2 + 1).clip(0).sum())
    assert [count(t) for t in (1.0, math.sqrt(2.0), math.sqrt(3.0), 2.0)] == [7, 19, 27, 33]
    wide = M.BallElement(*R.WIDE)
    assert wide.radii == (1, 1, 63) and wide.n_rows == 9
    big = M.BallElement(200.0)
    assert big.radii == (200, 200, 200) and big.half_widths is None and big.n_rows is None


# ---------------------------------------------------------------------------------------------------------------------- the identity
@pytest.mark.parametrize("density", [0.02, 0.3])
def test_dilation_by_the_ball_is_the_thresholded_transform(density):
    ndi = _scipy()
    m = np.random.default_rng(int(density * 100)).random(SMALL) < density
    assert m.any()
    for spacing, tau in PAIRS:
        q = R.sq_threshold(tau)
        by_structure = R.dilate(m, tau, spacing)
        assert np.array_equal(by_structure, DR.edt_sq(m, spacing) <= q), (spacing, tau)
        assert np.array_equal(by_structure, ndi.distance_transform_edt(~m, sampling=spacing) <= tau), (spacing, tau)
        assert np.array_equal(R.erode(m, tau, spacing, 1), DR.edt_sq(~m, spacing) > q), (spacing, tau)
        rows = _M().pack_rows(_M().BallElement(tau, spacing).half_widths)
        for op, bv, want in ((0, 0, by_structure), (1, 1, R.erode(m, tau, spacing, 1)), (0, 1, R.dilate(m, tau, spacing, 1)), (1, 0, R.erode(m, tau, spacing, 0))):
            assert np.array_equal(R.apply_rows(m, rows, op, bv), want), (spacing, tau, op, bv)


# ---------------------------------------------------------------------------------------------------------------------- the metric's oracle
@pytest.mark.parametrize("spacing", DR.SURFACE_SPACINGS)
@pytest.mark.parametrize("name", list(DR.surface_cases()))
def test_nsd_oracle_is_the_formula_on_scipy_distances(name, spacing):
    ndi = _scipy()
    a, b = DR.surface_cases()[name]

    def sd(x, y):
        fp = ndi.generate_binary_structure(3, 1)
        xb, yb = (x != 0) ^ ndi.binary_erosion(x != 0, structure=fp), (y != 0) ^ ndi.binary_erosion(y != 0, structure=fp)
        return ndi.distance_transform_edt(~yb, sampling=spacing)[xb]
    for tau in R.METRIC_TAUS:
        a_to_b, b_to_a = sd(a, b), sd(b, a)
        tp_a, tp_b = np.sum(a_to_b <= tau) / len(a_to_b), np.sum(b_to_a <= tau) / len(b_to_a)
        fp, fn = np.sum(a_to_b > tau) / len(a_to_b), np.sum(b_to_a > tau) / len(b_to_a)
        assert R.normalized_surface_dice(a, b, tau, spacing) == float((tp_a + tp_b) / (tp_a + tp_b + fp + fn + 1e-8))
        # the counts from the squared oracle distances and q: the comparison the device makes
        q = R.sq_threshold(tau)
        sa, sb = DR.surface_sq(a, b, spacing), DR.surface_sq(b, a, spacing)
        assert R.surface_overlap(a, b, tau, spacing) == (int((sa <= q).sum()), sa.size, int((sb <= q).sum()), sb.size)
    if name == "identical":
        assert R.normalized_surface_dice(a, b, 0.0, spacing) == 2.0 / (2.0 + 1e-8)


def test_nsd_oracle_refuses_empty_masks():
    a, _ = DR.surface_cases()["nested_boxes"]
    with pytest.raises(RuntimeError, match="first supplied"):
        R.surface_overlap(np.zeros_like(a), a, 1.0)
    with pytest.raises(RuntimeError, match="second supplied"):
        R.surface_overlap(a, np.zeros_like(a), 1.0)
    assert math.isnan(R.surface_dice_or_nan(np.zeros_like(a), a, 1.0)) and math.isnan(R.surface_dice_or_nan(a, np.zeros_like(a), 1.0))


# ---------------------------------------------------------------------------------------------------------------------- header and refusals
def test_header_prototypes():
    from veloxseg_amd import _hip
    protos = _hip.parse_header()
    assert protos["vx_morph_ball_max_rows"] == ("int", [])
    assert protos["vx_morph_ball"] == ("int", [("const unsigned long long*", "in"), ("const unsigned long long*", "gate"), ("unsigned long long*", "out"), ("int", "D"),
                                               ("int", "H"), ("int", "W"), ("const int*", "rows"), ("int", "n_rows"), ("int", "op"), ("int", "border_value"),
                                               ("void*", "stream")])


def test_entry_refuses_bad_arguments_without_gpu():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    cap = _hip.query("vx_morph_ball_max_rows")
    assert cap == 4096 and 4 * cap <= 64 * 1024, "the record list no longer fits the LDS a workgroup may take"
    ok = dict(src=4096, gate=8192, out=12288, D=3, H=4, W=70, rows=16384, n=5, op=0, bv=0)          # pointers that are never dereferenced

    def ball(**kw):
        a = dict(ok, **kw)
        _hip.call("vx_morph_ball", a["src"], a["gate"], a["out"], a["D"], a["H"], a["W"], a["rows"], a["n"], a["op"], a["bv"], None)
    for kw in (dict(src=None), dict(out=None), dict(rows=None), dict(src=None, gate=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            ball(**kw)
    for kw in (dict(out=4096), dict(out=8192), dict(gate=4096, out=4096)):
        with pytest.raises(RuntimeError, match="neither in nor gate"):
            ball(**kw)
    for kw in (dict(D=0), dict(H=0), dict(W=0), dict(D=-1), dict(H=-3), dict(W=-70), dict(D=2048, H=1024, W=1024), dict(D=65536, H=65536, W=1)):
        with pytest.raises(RuntimeError, match="bad sizes"):
            ball(**kw)
    for n in (0, -1, cap + 1, 2 ** 31 - 1):
        with pytest.raises(RuntimeError, match="rows"):
            ball(n=n)
    for op in (-1, 2):
        with pytest.raises(RuntimeError, match="op"):
            ball(op=op)
    for bv in (-1, 2):
        with pytest.raises(RuntimeError, match="border_value"):
            ball(bv=bv)


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    M = _M()
    from veloxseg_amd.utils.metric import metrics as Mb, surface as S
    x = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for fn in (M.ball_dilation, M.ball_erosion, M.ball_opening, M.ball_closing):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, 1.0)
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="radius"):
                fn(x, bad)
        for bad in ((1.0, 2.0), (1.0, 0.0, 1.0), (1.0, float("nan"), 1.0), -1.0):
            with pytest.raises(ValueError, match="spacings"):
                fn(x, 1.0, bad)
        with pytest.raises(ValueError, match="border_value"):
            fn(x, 1.0, None, 2)
    for bad in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="radius"):
            M.BallElement(bad)
    with pytest.raises(ValueError, match="spacings"):
        M.BallElement(1.0, (1.0, -1.0, 1.0))
    for fn in (S.surface_overlap, S.normalized_surface_dice):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x, x, 1.0)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x.float(), x.float(), 1.0)
        with pytest.raises(ValueError, match="radius"):
            fn(x, x, -1.0)
        with pytest.raises(ValueError, match="spacings"):
            fn(x, x, 1.0, (1.0, 2.0))
    for c in (2, 3, 0):
        with pytest.raises(ValueError, match="connectivity"):
            S.normalized_surface_dice(x, x, 1.0, None, c)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Mb.get_surface_dice(x[None, None], x[None, None], 1.0)
