"""CPU: the premises of tests/affine_ref.py (every exact row is exact in fp32, in both modes and both paddings; the rows hold ties and out-of-range samples; the
off-dyadic seed leaves out less than its cap), affine_matrix against hand-written cases, the draw order of RandAffined, the configuration, the record layout
against the header, the C entry's refusals and the refusals of the Python surface (nothing here launches a kernel)."""
import math
import re

import numpy as np
import pytest
import torch

import affine_ref as R
import eval_ref as ER


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def _same_values(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | ((a != a) & (b != b))).all())


# ====================================================================================================================== premises of the oracle
@pytest.mark.parametrize("row", R.EXACT_ROWS, ids=lambda r: r["id"])
def test_exact_rows_are_exact_in_fp32(row):
    A, c = R.record_values(R.row_matrix(row), row["n"])
    assert _same_values(A, R.MATRICES[row["matrix"]]) and _same_values(c, [0.5 * (v - 1) for v in row["n"]])          # dyadic: the record holds the matrix itself
    x = R.image(row)
    assert x.dtype == np.float32 and bool((x == np.rint(x)).all()) and float(np.abs(x).max()) <= 64
    for a32, a64 in zip(R.coords(A, c, row["out"], np.float32), R.coords(A, c, row["out"], np.float64)):
        assert _same_values(a32, a64)
    for mode in (0, 1):
        for pad in (0, 1):
            got32 = R.sample(x, A, c, row["out"], mode, pad, R.CVAL, dtype=np.float32)
            assert _same_values(got32, R.reference(row, mode, pad)), f"{row['id']} mode {mode} pad {pad}: fp32 and fp64 evaluation differ"
    if row["matrix"] == "identity" and row["out"] == row["n"]:
        for pad in (0, 1):
            assert _same_values(R.reference(row, 0, pad), x) and _same_values(R.reference(row, 1, pad), x)


def test_rows_hold_ties_and_out_of_range_samples():
    ties, outside = {0: 0.0, 1: 0.0}, 0.0
    for row in R.EXACT_ROWS:
        A, c = R.record_values(R.row_matrix(row), row["n"])
        hi = [v - 1 for v in row["n"]]
        for pad in (0, 1):
            t, o = R.shares(A, c, row["out"], [0, 0, 0], hi, pad)
            ties[pad], outside = max(ties[pad], t), max(outside, o)
    # a tie matters to BOTH modes (nearest rounds it to even, trilinear weighs it .5 / .5) and an out-of-range sample to BOTH paddings: every row runs all four
    assert ties[0] >= 0.10 and ties[1] >= 0.10 and outside >= 0.10
    named = {r["id"]: r for r in R.EXACT_ROWS}
    A, c = R.record_values(R.row_matrix(named["rot3_9x7x5_from_9x7x5"]), (9, 7, 5))
    t, o = R.shares(A, c, (9, 7, 5), [0, 0, 0], [8, 6, 4], 0)
    assert t > 0.5 and o > 0.4
    A, c = R.record_values(R.row_matrix(named["half_16x16x16_from_16x16x16"]), (16, 16, 16))
    assert R.shares(A, c, (16, 16, 16), [0, 0, 0], [15, 15, 15], 1) == (1.0, 0.0)


def test_nearest_labels_keep_their_width():
    row = R.EXACT_ROWS[0]
    for code, dt in R.LABEL_DTYPES.items():
        lab = R.label(row, code)
        assert lab.dtype == dt
        ref = R.reference(row, 1, 1, code)
        assert ref.dtype == dt and set(np.unique(ref).tolist()) <= set(np.unique(lab).tolist()) | {dt(R.CVAL)}
    assert int(R.label(row, 8).max()) == 2 ** 63 - 1 and int(R.label(row, 4).min()) == -2 ** 31


def test_z_rotation_matrix_gives_the_rotate_z_oracle():
    for r in ER.ROT_ROWS:
        x = ER.rotate_input(r)
        m = np.array([[r["cs"], -r["sn"], 0, 0], [r["sn"], r["cs"], 0, 0], [0, 0, 1, 0]], dtype=np.float64)
        A, c = R.record_values(m, x.shape[1:])
        for mode in (0, 1):
            want = ER.rotate_exact(x, r["cs"], r["sn"], mode)
            for ch in range(x.shape[0]):
                assert _same_values(R.sample(x[ch], A, c, x.shape[1:], mode, 0), want[ch]), f"{r['id']} mode {mode}"


def test_context_bounds_differ_from_window_bounds():
    parent = ER.ints(12, 11, 13, seed=5, lo=-64, hi=64)
    start, n = (3, 1, 5), (6, 7, 5)
    A, c = R.record_values(R.row_matrix(dict(matrix="rot3")), n)
    win = parent[3:9, 1:8, 5:10]
    a = R.sample(win, A, c, n, 0, 0)
    b = R.sample(parent, A, c, n, 0, 0, lo=[-s for s in start], hi=[p - 1 - s for p, s in zip(parent.shape, start)], origin=start)
    assert not _same_values(a, b)
    # with the window's own bounds the parent and the copied crop are the same source
    assert _same_values(a, R.sample(parent, A, c, n, 0, 0, lo=[0, 0, 0], hi=[v - 1 for v in n], origin=start))


def test_off_dyadic_seed_stays_under_the_cap():
    x, m = R.off_dyadic_case()
    A, c = R.record_values(m, R.OFF_N)
    eps = R.coord_bound(A, c, R.OFF_N)
    assert 0 < eps < 1e-4
    hi = [v - 1 for v in R.OFF_N]
    for pad in (0, 1):
        assert float(R.near_tie(A, c, R.OFF_N, [0, 0, 0], hi, pad, eps).mean()) <= 0.01
    # the fp32 evaluation of the rule on the CPU already sits inside the bound the GPU test uses
    for pad in (0, 1):
        bound = 3 * eps * R.neighbour_difference(x, R.CVAL if pad else None) + R.gamma(9) * max(float(np.abs(x).max()), R.CVAL)
        err = np.abs(R.sample(x, A, c, R.OFF_N, 0, pad, R.CVAL, dtype=np.float32).astype(np.float64) - R.sample(x, A, c, R.OFF_N, 0, pad, R.CVAL))
        assert float(err.max()) <= bound


# ====================================================================================================================== affine_matrix
def _angle(c, s):
    a = math.atan2(s, c)
    assert abs(math.cos(a) - c) < 1e-15 and abs(math.sin(a) - s) < 1e-15
    return a


def test_affine_matrix_hand_written_cases():
    A = _A()
    assert A.affine_matrix().shape == (3, 4) and A.affine_matrix().dtype == np.float64
    assert np.array_equal(A.affine_matrix(), np.eye(3, 4))
    c, s = 0.6, 0.8                                                             # a dyadic-free but exact pair: 0.36 + 0.64 = 1
    a = _angle(c, s)
    want = {0: [[1, 0, 0], [0, c, -s], [0, s, c]], 1: [[c, 0, s], [0, 1, 0], [-s, 0, c]], 2: [[c, -s, 0], [s, c, 0], [0, 0, 1]]}
    for axis, w in want.items():
        rot = [0.0, 0.0, 0.0]
        rot[axis] = a
        m = A.affine_matrix(rotate=rot)
        assert np.allclose(m[:, :3], w, rtol=0, atol=1e-15) and np.array_equal(m[:, 3], [0, 0, 0])
    # quarter turns put in directly: Rz(90 deg) maps p = (1, 0, 0) to (0, 1, 0)
    q = A.affine_matrix(rotate=(0, 0, math.pi / 2))[:, :3]
    assert np.allclose(q @ [1, 0, 0], [0, 1, 0], atol=1e-15) and np.allclose(q @ [0, 1, 0], [-1, 0, 0], atol=1e-15)
    # scale alone, translate alone
    assert np.array_equal(A.affine_matrix(scale=(1.25, 0.75, 0.5)), [[1.25, 0, 0, 0], [0, 0.75, 0, 0], [0, 0, 0.5, 0]])
    assert np.array_equal(A.affine_matrix(translate=(1, -2, 3.5)), [[1, 0, 0, 1], [0, 1, 0, -2], [0, 0, 1, 3.5]])
    # the composition order R @ T @ S with R = Rx @ Ry @ Rz: written out by hand for a quarter turn about x, then about z
    hx = A.affine_matrix(rotate=(math.pi / 2, 0, 0), scale=(2, 3, 4), translate=(1, 10, 100))
    assert np.allclose(hx, [[2, 0, 0, 1], [0, 0, -4, -100], [0, 3, 0, 10]], atol=1e-13)          # Rx (90): (d, h, w) -> (d, -w, h); S first, then T, then R
    hxz = A.affine_matrix(rotate=(math.pi / 2, 0, math.pi / 2))[:, :3]
    Rx, Rz = np.array([[1, 0, 0], [0, 0, -1], [0, 1, 0]]), np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    assert np.allclose(hxz, Rx @ Rz, atol=1e-15) and not np.allclose(hxz, Rz @ Rx, atol=1e-3)
    # against the restatement with homogeneous matrices, at seeded parameters
    rs = np.random.RandomState(3)
    for _ in range(8):
        rot, sc, tr = rs.uniform(-3, 3, 3), rs.uniform(0.5, 1.5, 3), rs.uniform(-5, 5, 3)
        assert np.allclose(A.affine_matrix(rot, sc, tr), R.matrix(rot, sc, tr), rtol=0, atol=1e-13)
    for bad in ((1, 2), (1, 2, float("nan")), "abc"):
        with pytest.raises(ValueError):
            A.affine_matrix(rotate=bad)


# ====================================================================================================================== draw order, configuration
@pytest.mark.parametrize("seed", (0, 7, 12345))
def test_draw_order(seed):
    A = _A()
    kw = dict(rotate_range=(0.3, (-0.1, 0.2), 0.0), scale_range=(0.1, 0.2, (0.0, 0.3)), translate_range=(2.0, 0.0, (1.0, 3.0)))
    t = A.RandAffined(["a"], prob=0.5, **kw).set_random_state(seed)
    got = [t.draw() for _ in range(40)]
    want = R.draws(seed, 0.5, kw["rotate_range"], kw["scale_range"], kw["translate_range"], 40)
    assert any(g is None for g in got) and any(g is not None for g in got)
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if g is not None:
            assert list(g[0]) == w[0] and list(g[1]) == w[1] and list(g[2]) == w[2]
    # zero ranges still draw: the stream after a fired call has moved by ten numbers, after a call that did not fire by one
    t = A.RandAffined(["a"], prob=1.0).set_random_state(seed)
    assert t.draw() == ([0.0] * 3, [0.0] * 3, [1.0] * 3)
    ref = np.random.RandomState(seed)
    ref.rand(10)
    assert t.R.rand() == ref.rand()
    t = A.RandAffined(["a"], prob=0.0).set_random_state(seed)
    assert t.draw() is None
    ref = np.random.RandomState(seed)
    ref.rand(1)
    assert t.R.rand() == ref.rand()
    # a bare number is the first axis only (MONAI's ensure_tuple); None is no range
    assert A.RandAffined(["a"], rotate_range=0.3).rotate_range == [(-0.3, 0.3), (0.0, 0.0), (0.0, 0.0)] == R.ranges(0.3)
    assert A.RandAffined(["a"]).scale_range == [(0.0, 0.0)] * 3 == R.ranges(None)


def test_rand_affined_arguments():
    A = _A()
    for kw in (dict(mode="cubic"), dict(padding_mode="reflection"), dict(prob=1.5), dict(rotate_range=(1, 2, 3, 4)), dict(spatial_size=(4, 4)), dict(spatial_size=(4, 0, 4)),
               dict(mode=("bilinear",))):
        with pytest.raises(ValueError):
            A.RandAffined(["a", "b"], **kw)
    assert A.RandAffined.takes_list is True and not getattr(A.RandFlipd, "takes_list", False)
    # the existing limits stay
    with pytest.raises(NotImplementedError):
        A.RandRotated(["a"], range_x=0.1)
    with pytest.raises(TypeError):
        A.BatchAssembler(["a"], "seg", [A.RandAffined(["a"])])


def test_compose_hands_the_list_over_whole():
    A = _A()
    seen = []

    class Whole:
        takes_list = True

        def __call__(self, data):
            seen.append(("whole", type(data)))
            return data

    class Each:
        def __call__(self, data):
            seen.append(("each", type(data)))
            return data
    A.Compose([Each(), Whole(), Each()])([{"a": 1}, {"a": 2}])
    assert seen == [("each", dict), ("each", dict), ("whole", list), ("each", dict), ("each", dict)]


def test_spatial_config():
    A = _A()
    keys, modes = ["img0", "img1", "seg"], A.image_label_modes(2)
    with pytest.raises(ValueError, match="unknown keys"):
        A.spatial_from_config({"rotate_degrees": 10, "shear": 0.1}, keys, modes)
    with pytest.raises(ValueError, match="must be a dict"):
        A.spatial_from_config([("rotate_degrees", 10)], keys, modes)
    with pytest.raises(ValueError, match="a number or three"):
        A.spatial_from_config({"scale": (0.1, 0.2)}, keys, modes)
    with pytest.raises(ValueError, match="padding_mode"):
        A.spatial_from_config({"padding_mode": "wrap"}, keys, modes)
    t = A.spatial_from_config({"rotate_degrees": 30, "scale": 0.1, "translate": (1, 2, 3), "prob": 0.25, "padding_mode": "constant", "context": True}, keys, modes)
    r = math.radians(30)
    assert t.rotate_range == [(-r, r)] * 3 and t.scale_range == [(-0.1, 0.1)] * 3 and t.translate_range == [(-1, 1), (-2, 2), (-3, 3)]
    assert t.prob == 0.25 and t.padding_mode == "constant" and t.context is True and t.mode == ["bilinear", "bilinear", "nearest"] and t.keys == keys
    t = A.spatial_from_config({"rotate_degrees": (0, 0, 15)}, keys, modes)
    assert t.rotate_range[:2] == [(0.0, 0.0)] * 2 and t.prob == 0.5 and t.padding_mode == "border" and t.context is False
    from recipe import CASES
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    cfg, _ = CASES["g2_32_m2"]
    with pytest.raises(ValueError, match="unknown keys"):
        SyntheticVolumes(cfg, 2, 1, torch.device("cpu"), spatial={"zoom": 0.1})
    plain = SyntheticVolumes(cfg, 2, 1, torch.device("cpu"))
    assert isinstance(plain.pipe.transforms[2], A.RandRotated) and plain.pipe.transforms[1].copy is True
    sp = SyntheticVolumes(cfg, 2, 1, torch.device("cpu"), spatial={"rotate_degrees": 10, "context": True})
    assert isinstance(sp.pipe.transforms[2], A.RandAffined) and sp.pipe.transforms[1].copy is False and len(sp.pipe.transforms) == 3
    assert SyntheticVolumes(cfg, 2, 1, torch.device("cpu"), spatial={"rotate_degrees": 10}).pipe.transforms[1].copy is True
    # the chain's seeds do not move: the crop of the spatial loader draws what the plain loader's crop draws
    assert sp.pipe.transforms[1].R.rand() == plain.pipe.transforms[1].R.rand()


# ====================================================================================================================== record, entry, Python refusals
def test_record_layout_against_the_header():
    from veloxseg_amd import _hip
    A = _A()
    ret, args = _hip.parse_header()["vx_affine_batch"]
    assert ret == "int" and [n for _, n in args] == ["records", "n_records", "Do", "Ho", "Wo", "stream"]
    src = open(_hip.HEADER).read()
    assert int(re.search(r"#define VX_AFFINE_RECORD_BYTES (\d+)", src).group(1)) == A.AFFINE_RECORD_BYTES == A._AFF.itemsize
    assert {n: A._AFF.fields[n][1] for n in A._AFF.names} == {"src": 0, "dst": 8, "stride": 16, "n": 40, "lo": 52, "hi": 64, "dtype": 76, "mode": 80, "pad": 84, "cval": 88,
                                                              "A": 92, "c": 128, "unused": 140}


def test_entry_refuses_bad_arguments_without_gpu():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    ok = dict(records=4096, n_records=3, Do=2, Ho=3, Wo=4)                        # a pointer that is never dereferenced

    def call(**kw):
        a = dict(ok, **kw)
        _hip.call("vx_affine_batch", a["records"], a["n_records"], a["Do"], a["Ho"], a["Wo"], None)
    with pytest.raises(RuntimeError, match="null pointer"):
        call(records=None)
    with pytest.raises(RuntimeError, match="misaligned"):
        call(records=4100)
    for n in (0, -1):
        with pytest.raises(RuntimeError, match="no records"):
            call(n_records=n)
    for kw in (dict(Do=0), dict(Ho=-1), dict(Wo=0)):
        with pytest.raises(RuntimeError, match="non-positive output extent"):
            call(**kw)
    with pytest.raises(RuntimeError, match="exceed one grid"):
        call(n_records=1 << 20, Do=1 << 10, Ho=1 << 10, Wo=1 << 10)


def test_python_surface_refuses_cpu_tensors():
    A = _A()
    x = torch.zeros(1, 4, 5, 6)
    eye = A.affine_matrix()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.affine_sample([(x[0], eye, "bilinear", "border", 0.0)], (4, 5, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.RandAffined(["a"], prob=1.0)({"a": x})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.RandAffined(["a"], prob=1.0)([{"a": x}, {"a": x}])
    with pytest.raises(ValueError, match="no entries"):
        A.affine_sample([], (4, 5, 6))
    for size in ((4, 5), (4, 0, 6), (4, 5, -1)):
        with pytest.raises(ValueError, match="out_size"):
            A.affine_sample([(x[0], eye, "bilinear", "border", 0.0)], size)
