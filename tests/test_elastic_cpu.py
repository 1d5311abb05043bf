"""CPU: the premises of tests/elastic_ref.py (with a zero field or none it is affine_ref's rule on every exact row of affine_ref; its own exact rows are exact in
fp32; it agrees with torch's grid_sample in fp64 within a derived bound; the off-dyadic seed leaves out less than its cap), the noise against the Philox restatement,
the weights, the draw order of Rand3DElasticd, the configuration, the record layouts against the header, and every refusal of the three C entries and of the Python
surface (nothing here launches a kernel)."""
import math
import re

import numpy as np
import pytest
import torch

import affine_ref as R
import augment_stats_ref as SR
import elastic_ref as E
from oracle.philox import philox4x32


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def _same_values(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


# ====================================================================================================================== premises of the oracle
@pytest.mark.parametrize("row", R.EXACT_ROWS, ids=lambda r: r["id"])
def test_zero_field_is_the_affine_rule(row):
    A, c = R.record_values(R.row_matrix(row), row["n"])
    zero = np.zeros((3,) + tuple(row["out"]), dtype=np.float32)
    x = R.image(row)
    for a, b in zip(E.coords(A, c, row["out"]), R.coords(A, c, row["out"])):
        assert _same_values(a, b)
    for mode in (0, 1):
        for pad in (0, 1):
            want = R.reference(row, mode, pad)
            assert _same_values(E.sample(x, A, c, row["out"], mode, pad, R.CVAL), want), f"{row['id']} mode {mode} pad {pad}: no field"
            assert _same_values(E.sample(x, A, c, row["out"], mode, pad, R.CVAL, zero, 2.0), want), f"{row['id']} mode {mode} pad {pad}: a zero field"
            assert _same_values(E.sample(x, A, c, row["out"], mode, pad, R.CVAL, zero, 2.0, dtype=np.float32), want)
    for code in (1, 8):
        for pad in (0, 1):
            assert _same_values(E.sample(R.label(row, code), A, c, row["out"], 1, pad, R.CVAL, zero, 0.5), R.reference(row, 1, pad, code))


@pytest.mark.parametrize("row", E.EXACT_ROWS, ids=lambda r: r["id"])
def test_exact_rows_are_exact_in_fp32(row):
    A, c = R.record_values(R.row_matrix(row), row["n"])
    f = E.field(row)
    assert f.dtype == np.float32 and f.shape == (3,) + tuple(row["out"]) and bool((f * 4 == np.rint(f * 4)).all()) and float(np.abs(f).max()) <= 3 and row["m"] in (1.0, 2.0, 0.5)
    for a32, a64 in zip(E.coords(A, c, row["out"], f, row["m"], np.float32), E.coords(A, c, row["out"], f, row["m"], np.float64)):
        assert _same_values(a32, a64)
    x = R.image(row)
    for mode in (0, 1):
        for pad in (0, 1):
            got32 = E.sample(x, A, c, row["out"], mode, pad, E.CVAL, f, row["m"], dtype=np.float32)
            assert _same_values(got32, E.reference(row, mode, pad)), f"{row['id']} mode {mode} pad {pad}: fp32 and fp64 evaluation differ"


def test_rows_are_moved_by_their_fields_and_hold_ties_and_outside_samples():
    moved = ties = outside = 0
    for row in E.EXACT_ROWS:
        A, c = R.record_values(R.row_matrix(row), row["n"])
        moved += int(not _same_values(E.reference(row, 0, 0), E.sample(R.image(row), A, c, row["out"], 0, 0, E.CVAL)))
        s = E.coords(A, c, row["out"], E.field(row), row["m"])
        ties += int(any(bool(((sa - np.floor(sa)) == 0.5).any()) for sa in s))
        outside += int(any(bool(((sa < 0) | (sa > n - 1)).any()) for sa, n in zip(s, row["n"])))
    assert moved >= len(E.EXACT_ROWS) - 7 and ties >= len(E.EXACT_ROWS) // 2 and outside >= len(E.EXACT_ROWS) // 2          # (a one-voxel-thick source hides some moves)


# ====================================================================================================================== the independent pin: torch.nn.functional.grid_sample
PIN_SEED, PIN_N = 3, (12, 10, 14)


def _pin_case(seed=PIN_SEED):
    """random data, a random rotation + scale, and a smooth random field (sigma 1.5 on this small grid) of up to two voxels"""
    rs = np.random.RandomState(seed)
    x = rs.standard_normal(PIN_N)
    m = R.matrix(rs.uniform(-0.6, 0.6, 3), rs.uniform(0.8, 1.2, 3), rs.uniform(-1, 1, 3))
    f = np.stack([E.smooth64(rs.uniform(-1, 1, PIN_N), E.weights64(1.5).astype(np.float32)) for _ in range(3)])
    f = (f * (2.0 / np.abs(f).max())).astype(np.float32)
    return x, m, f


def test_restatement_against_grid_sample_in_fp64():
    """torch.nn.functional.grid_sample (CPU, fp64, align_corners=True) takes NORMALISED coordinates g = 2 s / (n - 1) - 1 and turns them back with ((g + 1) / 2) (n - 1):
    the division, the subtraction, the addition and the product each round once (the halving is exact), each relative to a quantity of at most |s| + (n - 1), so its
    coordinate differs from s by at most delta = 4 * 2^-53 * (max|s| + max(n - 1)): a few ulp of the extent.  The interpolant is piecewise linear with slope at most
    G = the largest neighbour difference per axis (taken with the zero frame under `zeros`), so the value moves by at most 3 delta G; grid_sample weighs the eight
    corners by products of three factors where the rule nests three lerps, a few fp64 roundings on either side: + 32 * 2^-53 max|x|.  Nearest (nearbyint on both
    sides) is compared outside delta of a .5 tie; at most 1 % of the voxels may be left out."""
    x, m, f = _pin_case()
    A, c = R.record_values(m, PIN_N)
    A, c = A.astype(np.float64), c.astype(np.float64)
    mag = 1.0
    s = E.coords(A, c, PIN_N, f, mag)
    n1 = [v - 1 for v in PIN_N]
    delta = 4 * 2.0 ** -53 * (max(float(np.abs(sa).max()) for sa in s) + max(n1))
    grid = torch.from_numpy(np.stack([2.0 * s[2] / n1[2] - 1.0, 2.0 * s[1] / n1[1] - 1.0, 2.0 * s[0] / n1[0] - 1.0], axis=-1))[None]
    xt = torch.from_numpy(x)[None, None]
    hi = n1
    for pad, name in ((0, "border"), (1, "zeros")):
        G = R.neighbour_difference(x, 0.0 if pad else None)
        bound = 3 * delta * G + 32 * 2.0 ** -53 * float(np.abs(x).max())
        ref = torch.nn.functional.grid_sample(xt, grid, mode="bilinear", padding_mode=name, align_corners=True)[0, 0].numpy()
        err = float(np.abs(E.sample(x, A, c, PIN_N, 0, pad, 0.0, f, mag) - ref).max())
        print(f"grid_sample pin, trilinear {name}: max |difference| {err:.3e}, bound {bound:.3e} (delta {delta:.3e}, G {G:.3f})")
        assert err <= bound
        skip = E.near_tie(A, c, PIN_N, f, mag, [0, 0, 0], hi, pad, delta)
        share = float(skip.mean())
        assert share <= 0.01, f"nearest {name}: {share:.4f} of the voxels lie within delta of a tie"
        ref = torch.nn.functional.grid_sample(xt, grid, mode="nearest", padding_mode=name, align_corners=True)[0, 0].numpy()
        bad = (E.sample(x, A, c, PIN_N, 1, pad, 0.0, f, mag) != ref) & ~skip
        assert not bad.any(), f"nearest {name}: {int(bad.sum())} voxels differ away from ties"
    # the field matters here: without it the restatement is somewhere else entirely
    assert float(np.abs(E.sample(x, A, c, PIN_N, 0, 0, 0.0) - E.sample(x, A, c, PIN_N, 0, 0, 0.0, f, mag)).max()) > 0.1


def off_dyadic_case():
    """affine_ref's rotation + scale case at 24^3 and the restated device field (sigma 5) under OFF_FIELD_SEED, its magnitude set for OFF_DISPLACEMENT voxels"""
    x, m = R.off_dyadic_case(E.OFF_SEED)
    V = int(np.prod(E.OFF_N))
    half = E.weights64(E.OFF_SIGMA).astype(np.float32)
    f = np.stack([E.smooth32(p.reshape(E.OFF_N), half, True) for p in E.noise_planes([E.OFF_FIELD_SEED], 3, V)])
    return x, m, f, E.off_magnitude(f)


def test_off_dyadic_seed_stays_under_the_cap():
    x, m, f, mag = off_dyadic_case()
    A, c = R.record_values(m, E.OFF_N)
    eps = E.coord_bound(A, c, E.OFF_N, f, mag)
    assert 0 < eps < 1e-4 and 2.9 < mag * float(np.abs(f).max()) < 3.1
    hi = [v - 1 for v in E.OFF_N]
    for pad in (0, 1):
        assert float(E.near_tie(A, c, E.OFF_N, f, mag, [0, 0, 0], hi, pad, eps).mean()) <= 0.01
        bound = 3 * eps * R.neighbour_difference(x, 2.0 if pad else None) + R.gamma(9) * float(np.abs(x).max())
        err = np.abs(E.sample(x, A, c, E.OFF_N, 0, pad, 2.0, f, mag, dtype=np.float32).astype(np.float64) - E.sample(x, A, c, E.OFF_N, 0, pad, 2.0, f, mag))
        assert float(err.max()) <= bound                               # the fp32 evaluation of the rule on the CPU already sits inside the bound the GPU test uses


# ====================================================================================================================== noise
def test_noise_restatement():
    A = _A()
    assert E.STREAM == A.ELASTIC_STREAM != A.AUG_NOISE_STREAM and E.STREAM > 1 << 40
    key, V = 0x1234567890ABCDEF, 4099
    planes = E.noise_planes([key, 99], 6, V)
    assert planes.dtype == np.float32 and planes.shape == (6, V)
    w = philox4x32(np.arange((3 * V + 3) // 4, dtype=np.uint64), E.STREAM, key).reshape(-1)[:3 * V]
    want = ((w >> np.uint32(8)).astype(np.float64) - 8388608.0) / 8388608.0
    assert _same_values(planes[:3].reshape(-1), want)                  # exact in fp32: plane j of a field is its elements j V .. j V + V - 1, quads straddle the planes
    assert float(planes.min()) >= -1.0 and float(planes.max()) < 1.0 and float(planes.min()) < -0.99 and float(planes.max()) > 0.99
    assert abs(float(planes.mean())) < 0.02 and bool((planes * 2.0 ** 23 == np.rint(planes * 2.0 ** 23)).all())
    # planes of one field use disjoint counters / words, fields use their own keys: no two planes agree anywhere near fully
    for i in range(6):
        for j in range(i + 1, 6):
            assert float((planes[i] == planes[j]).mean()) < 0.01
    assert _same_values(E.noise_planes([99], 3, V), planes[3:]) and _same_values(E.uniforms(key, 5, 7), planes[:3].reshape(-1)[7:12])
    # the extremes of the map
    assert np.float32((0 - 8388608) * 2.0 ** -23) == -1.0 and np.float32(((0xFFFFFFFF >> 8) - 8388608) * 2.0 ** -23) == np.float32(1.0 - 2.0 ** -23)


# ====================================================================================================================== weights
def test_weights():
    A = _A()
    for sigma, tail in ((0.1, 1), (1.0 / 6.0, 1), (5.0, 15), (13.0, 39), (16.0, 48)):
        w = A.elastic_weights(sigma)
        assert w.dtype == np.float32 and w.size == tail + 1 == E.tail_of(sigma) + 1
        t = 1.0 / (sigma * math.sqrt(2.0))
        want = np.array([0.5 * (math.erf((k + 0.5) * t) - math.erf((k - 0.5) * t)) for k in range(tail + 1)])
        assert np.array_equal(w, want.astype(np.float32)) and np.array_equal(w, E.weights64(sigma).astype(np.float32))
        assert 0.99 < float(w[0] + 2 * w[1:].sum()) <= 1.0 + 1e-6
    # gaussian_weights' formula at the other truncation: where both tables reach, the values are the same
    assert np.array_equal(A.elastic_weights(3.0)[:10], A.gaussian_weights(3.0)[:10]) and A.elastic_weights(3.0).size == 10 and A.gaussian_weights(3.0).size == 13
    assert A.ELASTIC_MAX_TAIL == E.MAX_TAIL == 48 and A.ELASTIC_MAX_SIGMA == E.MAX_SIGMA == 16.0
    for bad in (16.0001, 17, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            A.elastic_weights(bad)
    # the smoothing restatement is the blur restatement with one vector
    x = np.random.RandomState(0).standard_normal((5, 6, 7))
    w = A.elastic_weights(1.0)
    fw = E.full(w)
    assert fw.size == 2 * w.size - 1 and np.array_equal(fw, fw[::-1]) and np.array_equal(E.smooth64(x, w), SR.blur64(x, (fw, fw, fw)))


def test_dyadic_smoothing_cases_are_exact_in_fp32():
    """the premise of the GPU test's `==`: on every shape and tail the fp32 rule, with or without a fused multiply-add, gives the fp64 values"""
    A = _A()
    shapes = E.smooth_shapes(A.ELASTIC_ROWS, A.ELASTIC_TILE_W, A.ELASTIC_STRIP, A.ELASTIC_TILE_LINE)
    assert shapes[2][0] * shapes[2][1] > A.ELASTIC_ROWS and shapes[2][2] == A.ELASTIC_TILE_W + 1 and shapes[3][1:] == (A.ELASTIC_TILE_LINE + 1, A.ELASTIC_STRIP + 1)
    assert shapes[4][0] == A.ELASTIC_TILE_LINE + 1 and shapes[1] == (5, 5, 5) and max(E.SMOOTH_TAILS) == A.ELASTIC_MAX_TAIL
    for case, shape in enumerate(shapes):
        x = E.dyadic_data(shape, len(E.SMOOTH_TAILS), 100 * case)
        assert float(np.abs(x).max()) <= 64 and bool((x == np.rint(x)).all()) and bool((x[:, 0, 0, 0] != 0).all()) and bool((x[:, -1, -1, -1] != 0).all())
        for i, tail in enumerate(E.SMOOTH_TAILS):
            h = E.dyadic_half(tail, 10 * case + i)
            assert h.size == tail + 1 and h[0] == 0.5 and (tail == 0 or (h[1] != 0 and h[tail] != 0)) and float(h[0] + 2 * h[1:].sum()) <= 3.5
            want = E.smooth64(x[i], h)
            assert _same_values(E.smooth32(x[i], h, True), want) and _same_values(E.smooth32(x[i], h, False), want), f"shape {shape}, tail {tail}"
            if tail and min(shape) > 1:
                assert not _same_values(want, h[0] ** 3 * x[i])


# ====================================================================================================================== draw order, configuration
@pytest.mark.parametrize("seed", (0, 7, 12345))
def test_draw_order(seed):
    A = _A()
    kw = dict(rotate_range=(0.3, (-0.1, 0.2), 0.0), scale_range=(0.1, 0.2, (0.0, 0.3)), translate_range=(2.0, 0.0, (1.0, 3.0)))
    t = A.Rand3DElasticd(["a"], (5, 8), (100, 200), prob=0.5, **kw).set_random_state(seed)
    got = [t.draw() for _ in range(40)]
    want = E.draws(seed, 0.5, (5, 8), (100, 200), kw["rotate_range"], kw["scale_range"], kw["translate_range"], 40)
    assert any(g is None for g in got) and any(g is not None for g in got)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert g[:3] == w[:3] and list(g[3]) == w[3] and list(g[4]) == w[4] and list(g[5]) == w[5]
            assert isinstance(g[0], int) and 0 <= g[0] < 2 ** 31 - 1 and 100 <= g[1] <= 200 and 5 <= g[2] <= 8
    # a fired sample moves the stream by thirteen numbers (rand, randint, two uniforms, nine uniforms), one that does not fire by one
    t = A.Rand3DElasticd(["a"], 6.0, 150.0, prob=1.0).set_random_state(seed)
    d = t.draw()
    assert d[1:] == (150.0, 6.0, [0.0] * 3, [0.0] * 3, [1.0] * 3)
    ref = np.random.RandomState(seed)
    ref.rand()
    assert d[0] == int(ref.randint(2 ** 31 - 1))
    ref.rand(11)
    assert t.R.rand() == ref.rand()
    t = A.Rand3DElasticd(["a"], 6.0, 150.0, prob=0.0).set_random_state(seed)
    assert [t.draw() for _ in range(3)] == [None] * 3
    ref = np.random.RandomState(seed)
    ref.rand(3)
    assert t.R.rand() == ref.rand()                                     # prob = 0 draws one uniform per sample
    assert t.last_draws is None


def test_arguments():
    A = _A()
    assert A.Rand3DElasticd.takes_list is True
    t = A.Rand3DElasticd(["a", "b"], (13, 5), 120, prob=0.3, rotate_range=0.3, mode=("bilinear", "nearest"), padding_mode="constant", cval=2.0, context=True)
    assert t.sigma_range == (5.0, 13.0) and t.magnitude_range == (120.0, 120.0) and t.prob == 0.3 and t.rotate_range == [(-0.3, 0.3), (0.0, 0.0), (0.0, 0.0)]
    assert t.mode == ["bilinear", "nearest"] and t.padding_mode == "constant" and t.cval == 2.0 and t.context is True and t.spatial_size is None
    for kw in (dict(sigma_range=(5, 17)), dict(sigma_range=0.0), dict(sigma_range=(1, 2, 3)), dict(sigma_range="ab"), dict(magnitude_range=float("inf")),
               dict(magnitude_range=(1, float("nan"))), dict(mode="cubic"), dict(padding_mode="reflection"), dict(prob=1.5), dict(spatial_size=(4, 4))):
        with pytest.raises(ValueError):
            A.Rand3DElasticd(["a", "b"], **dict(dict(sigma_range=(5, 8), magnitude_range=(100, 200)), **kw))
    with pytest.raises(TypeError):
        A.BatchAssembler(["a"], "seg", [A.Rand3DElasticd(["a"], 5, 100)])


def test_spatial_config():
    A = _A()
    keys, modes = ["img0", "img1", "seg"], A.image_label_modes(2)
    plain_cfg = {"rotate_degrees": 30, "scale": 0.1, "translate": (1, 2, 3), "prob": 0.25, "padding_mode": "constant", "context": True}
    plain = A.spatial_from_config(plain_cfg, keys, modes)
    r = math.radians(30)
    assert type(plain) is A.RandAffined                                  # without the new keys: the parent's RandAffined, field for field
    assert {k: v for k, v in vars(plain).items() if k != "R"} == dict(
        keys=keys, prob=0.25, rotate_range=[(-r, r)] * 3, translate_range=[(-1.0, 1.0), (-2.0, 2.0), (-3.0, 3.0)], scale_range=[(-0.1, 0.1)] * 3, spatial_size=None,
        mode=["bilinear", "bilinear", "nearest"], padding_mode="constant", cval=0.0, context=True)
    assert type(A.spatial_from_config({}, keys, modes)) is A.RandAffined
    el = A.spatial_from_config(dict(plain_cfg, elastic_sigma=(5, 13), elastic_magnitude=150), keys, modes)
    assert type(el) is A.Rand3DElasticd and el.sigma_range == (5.0, 13.0) and el.magnitude_range == (150.0, 150.0)
    for k in ("keys", "prob", "rotate_range", "translate_range", "scale_range", "spatial_size", "mode", "padding_mode", "cval", "context"):
        assert getattr(el, k) == getattr(plain, k), k                    # the same affine ranges
    one = A.spatial_from_config({"elastic_sigma": 7}, keys, modes)
    assert type(one) is A.Rand3DElasticd and one.sigma_range == (7.0, 7.0) and one.magnitude_range == (100.0, 200.0) and one.prob == 0.5
    assert A.spatial_from_config({"elastic_magnitude": (50, 60)}, keys, modes).sigma_range == (5.0, 13.0)
    for bad in ({"shear": 0.1}, {"zoom": 0.1}, {"gamma": 1.0}, {"elastic_sigma": 6, "shear": 0.1}, {"elastic_alpha": 1}):
        with pytest.raises(ValueError, match="unknown keys"):
            A.spatial_from_config(bad, keys, modes)
    with pytest.raises(ValueError, match="sigma_range"):
        A.spatial_from_config({"elastic_sigma": 20}, keys, modes)
    with pytest.raises(ValueError, match="a number or three"):
        A.spatial_from_config({"elastic_sigma": 6, "scale": (0.1, 0.2)}, keys, modes)
    from recipe import CASES
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    cfg, _ = CASES["g2_32_m2"]
    sp = SyntheticVolumes(cfg, 2, 1, torch.device("cpu"), spatial={"rotate_degrees": 10, "context": True, "elastic_sigma": 6, "elastic_magnitude": 100})
    plain_loader = SyntheticVolumes(cfg, 2, 1, torch.device("cpu"))
    assert isinstance(sp.pipe.transforms[2], A.Rand3DElasticd) and sp.pipe.transforms[1].copy is False and len(sp.pipe.transforms) == 3
    assert sp.pipe.transforms[1].R.rand() == plain_loader.pipe.transforms[1].R.rand()          # the chain's seeds do not move
    with pytest.raises(ValueError, match="unknown keys"):
        SyntheticVolumes(cfg, 2, 1, torch.device("cpu"), spatial={"elastic_sigma": 6, "zoom": 0.1})


# ====================================================================================================================== records, entries, Python refusals
def test_record_layouts_against_the_header():
    from veloxseg_amd import _hip
    A = _A()
    protos = _hip.parse_header()
    assert [n for _, n in protos["vx_elastic_noise"][1]] == ["keys", "n_planes", "V", "out", "stream"]
    assert [n for _, n in protos["vx_elastic_smooth"][1]] == ["weights", "n_planes", "planes", "result", "D", "H", "W", "stream"]
    assert [n for _, n in protos["vx_elastic_smooth_pass"][1]] == ["weights", "n_planes", "planes", "result", "axis", "D", "H", "W", "stream"]
    assert [n for _, n in protos["vx_elastic_batch"][1]] == [n for _, n in protos["vx_affine_batch"][1]] == ["records", "n_records", "Do", "Ho", "Wo", "stream"]
    assert all(protos[n][0] == "int" for n in ("vx_elastic_noise", "vx_elastic_smooth", "vx_elastic_batch"))
    src = open(_hip.HEADER).read()
    val = lambda name: int(re.search(rf"#define {name} \(?(-?\d+)\)?", src).group(1))
    assert val("VX_ELASTIC_RECORD_BYTES") == A.ELASTIC_RECORD_BYTES == A._ELA.itemsize == 160
    assert val("VX_ELASTIC_WEIGHT_BYTES") == A.ELASTIC_WEIGHT_BYTES == A._ELW.itemsize and val("VX_ELASTIC_MAX_TAIL") == A.ELASTIC_MAX_TAIL
    assert (val("VX_ELASTIC_ROWS"), val("VX_ELASTIC_TILE_W"), val("VX_ELASTIC_STRIP"), val("VX_ELASTIC_TILE_LINE")) == (A.ELASTIC_ROWS, A.ELASTIC_TILE_W, A.ELASTIC_STRIP,
                                                                                                                    A.ELASTIC_TILE_LINE)
    assert int(re.search(r"#define VX_ELASTIC_STREAM (0x[0-9a-fA-F]+)ull", src).group(1), 16) == A.ELASTIC_STREAM
    # the first 144 bytes are an affine record, field for field
    assert A._ELA.fields["aff"][0] == A._AFF and A._ELA.fields["aff"][1] == 0 and A._AFF.itemsize == A.AFFINE_RECORD_BYTES == 144
    assert {n: A._ELA.fields[n][1] for n in A._ELA.names} == {"aff": 0, "field": 144, "m": 152, "unused": 156}
    assert {n: A._ELW.fields[n][1] for n in A._ELW.names} == {"tail": 0, "w": 4} and A._ELW.fields["w"][0].shape == (49,)
    # the LDS of the H / D pass stays below 64 KB whatever the extent
    assert (A.ELASTIC_TILE_LINE + 2 * A.ELASTIC_MAX_TAIL) * A.ELASTIC_STRIP * 4 + 4 * 49 < 64 * 1024
    assert A.ELASTIC_ROWS * (A.ELASTIC_TILE_W + 2 * A.ELASTIC_MAX_TAIL) * 4 + 4 * 49 < 64 * 1024


def test_entries_refuse_bad_arguments_without_gpu():
    """the refusals come before any launch, so they run here on host memory: every refused call raises with its message and leaves the prefilled buffers as they were"""
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    buf = np.full(4096, 7.5, dtype=np.float32)                           # `out` / `planes` / `result` of the refused calls: host memory, never dereferenced
    tab = np.zeros(512, dtype=np.uint64)
    p, t = buf.ctypes.data, tab.ctypes.data
    assert p % 16 == 0 and t % 8 == 0

    def refused(name, msg, *args):
        with pytest.raises(RuntimeError, match=msg):
            _hip.call(name, *args, None)
        assert bool((buf == 7.5).all()) and not tab.any(), f"{name}: the refused call wrote"
    # vx_elastic_noise(keys, n_planes, V, out)
    refused("vx_elastic_noise", "null pointer", None, 3, 8, p)
    refused("vx_elastic_noise", "null pointer", t, 3, 8, None)
    refused("vx_elastic_noise", "misaligned", t + 4, 3, 8, p)
    refused("vx_elastic_noise", "misaligned", t, 3, 8, p + 2)
    for n in (0, -3):
        refused("vx_elastic_noise", "no planes", t, n, 8, p)
    for v in (0, -8):
        refused("vx_elastic_noise", "non-positive plane size", t, 3, v, p)
    refused("vx_elastic_noise", "not supported", t, 3, 1 << 31, p)
    refused("vx_elastic_noise", "exceed one grid", t, 3 << 20, 1 << 30, p)
    # vx_elastic_smooth(weights, n_planes, planes, result, D, H, W)
    q = p + 4 * 2048
    refused("vx_elastic_smooth", "null pointer", None, 3, p, q, 4, 5, 6)
    refused("vx_elastic_smooth", "null pointer", t, 3, None, q, 4, 5, 6)
    refused("vx_elastic_smooth", "null pointer", t, 3, p, None, 4, 5, 6)
    refused("vx_elastic_smooth", "misaligned", t + 4, 3, p, q, 4, 5, 6)
    refused("vx_elastic_smooth", "misaligned", t, 3, p + 1, q, 4, 5, 6)
    refused("vx_elastic_smooth", "misaligned", t, 3, p, q + 2, 4, 5, 6)
    for n in (0, -1):
        refused("vx_elastic_smooth", "no planes", t, n, p, q, 4, 5, 6)
    for d in ((0, 5, 6), (4, -1, 6), (4, 5, 0)):
        refused("vx_elastic_smooth", "non-positive extent", t, 3, p, q, *d)
    refused("vx_elastic_smooth", "overlap", t, 3, p, p, 4, 5, 6)
    refused("vx_elastic_smooth", "overlap", t, 3, p, p + 4 * (3 * 120 - 1), 4, 5, 6)
    refused("vx_elastic_smooth", "overlap", t, 3, p + 4 * 10, p, 4, 5, 6)
    refused("vx_elastic_smooth", "not supported", t, 3, p, q, 1 << 11, 1 << 10, 1 << 10)
    refused("vx_elastic_smooth", "exceed one grid", t, 1 << 24, p, p + (1 << 45), 64, 64, 64)
    # vx_elastic_smooth_pass(weights, n_planes, planes, result, axis, D, H, W): the same checks, and the axis
    refused("vx_elastic_smooth_pass", "null pointer", t, 3, None, q, 2, 4, 5, 6)
    refused("vx_elastic_smooth_pass", "misaligned", t, 3, p, q + 2, 2, 4, 5, 6)
    refused("vx_elastic_smooth_pass", "no planes", t, 0, p, q, 2, 4, 5, 6)
    refused("vx_elastic_smooth_pass", "non-positive extent", t, 3, p, q, 2, 4, 0, 6)
    refused("vx_elastic_smooth_pass", "overlap", t, 3, p, p + 8, 2, 4, 5, 6)
    for axis in (-1, 3):
        refused("vx_elastic_smooth_pass", "axis", t, 3, p, q, axis, 4, 5, 6)
    refused("vx_elastic_smooth_pass", "exceed one grid", t, 1 << 24, p, p + (1 << 48), 1, 512, 64, 64)
    # vx_elastic_batch(records, n_records, Do, Ho, Wo): the checks of vx_affine_batch
    refused("vx_elastic_batch", "null pointer", None, 3, 2, 3, 4)
    refused("vx_elastic_batch", "misaligned", t + 4, 3, 2, 3, 4)
    for n in (0, -1):
        refused("vx_elastic_batch", "no records", t, n, 2, 3, 4)
    for d in ((0, 3, 4), (2, -1, 4), (2, 3, 0)):
        refused("vx_elastic_batch", "non-positive output extent", t, 3, *d)
    refused("vx_elastic_batch", "not supported", t, 1, 1 << 11, 1 << 10, 1 << 10)
    refused("vx_elastic_batch", "exceed one grid", t, 1 << 20, 1 << 10, 1 << 10, 1 << 10)


def test_python_surface_refuses_without_gpu():
    A = _A()
    # elastic_field: every argument check comes before the device is asked for
    for args, msg in ((((4, 5), [1], [5.0]), "shape"), (((4, 0, 6), [1], [5.0]), "shape"), (((4, 5, 6), [], []), "one of each"), (((4, 5, 6), [1, 2], [5.0]), "one of each"),
                      (((4, 5, 6), [-1], [5.0]), "seed"), (((4, 5, 6), [1.5], [5.0]), "seed"), (((4, 5, 6), [1 << 64], [5.0]), "seed"), (((4, 5, 6), [1], [16.5]), "sigma"),
                      (((4, 5, 6), [1], [0.0]), "sigma"), (((1 << 11, 1 << 10, 1 << 10), [1], [5.0]), "shape")):
        with pytest.raises(ValueError, match=msg):
            A.elastic_field(*args)
    with pytest.raises(ValueError, match="`out`"):
        A.elastic_field((4, 5, 6), [1], [5.0], out=torch.zeros(1, 3, 4, 5, 6))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            A.elastic_field((4, 5, 6), [1], [5.0])
    # elastic_sample: what the record adds is checked first and needs no device; then affine_sample's own checks
    x = torch.full((1, 4, 5, 6), 3.0)
    eye = A.affine_matrix()
    f = torch.zeros(3, 4, 5, 6)
    ok = (x[0], eye, "bilinear", "border", 0.0)
    for entry, exc, msg in ((ok, ValueError, "has 5 fields"), (ok + (None, 1.0, None, None), ValueError, "has 9 fields"), (ok + (None, float("nan")), ValueError, "not finite"),
                            (ok + (None, float("inf")), ValueError, "not finite"), (ok + (None, "much"), ValueError, "not a number"), (ok + ([0.0], 1.0), TypeError, "tensor or None"),
                            (ok + (f.double(), 1.0), TypeError, "float32"), (ok + (f[:, :3], 1.0), ValueError, "contiguous"), (ok + (f[:2], 1.0), ValueError, "contiguous"),
                            (ok + (torch.zeros(3, 4, 5, 12)[..., ::2], 1.0), ValueError, "contiguous"), (ok + (f, 1.0), RuntimeError, "no CPU fallback"),
                            (ok + (None, 1.0), RuntimeError, "no CPU fallback")):
        with pytest.raises(exc, match=msg):
            A.elastic_sample([entry], (4, 5, 6))
    with pytest.raises(ValueError, match="no entries"):
        A.elastic_sample([], (4, 5, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.Rand3DElasticd(["a"], 5, 100, prob=1.0)({"a": x})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.Rand3DElasticd(["a"], 5, 100, prob=1.0)([{"a": x}, {"a": x}])
    same = A.Rand3DElasticd(["a"], 5, 100, prob=0.0)([{"a": x}, {"a": x}])          # nothing fires: nothing is asked of the device
    assert all(o["a"] is x for o in same) and bool((x == 3.0).all()) and not f.any()
