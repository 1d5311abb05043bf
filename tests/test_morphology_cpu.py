"""The numpy oracle of the mask-morphology kernels (tests/morphology_ref.py) against scipy.ndimage on every input tests/test_morphology_gpu.py uses, the multi-class
hole rule on hand-built cases, and Postprocess.from_config with the morphology keys.  No GPU."""
import numpy as np
import pytest
import torch

import morphology_ref as R

ndi = pytest.importorskip("scipy.ndimage")
ITERATIONS = (1, 2, 5)


def structure(connectivity):
    return ndi.generate_binary_structure(3, R.MAX_NONZERO[connectivity])


def test_offsets_are_scipys_structures():
    for c, n in zip(R.CONNECTIVITIES, (7, 19, 27)):
        s = np.zeros((3, 3, 3), dtype=bool)
        for o in R.offsets(c):
            s[tuple(d + 1 for d in o)] = True
        assert len(R.offsets(c)) == n and np.array_equal(s, structure(c))


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(R.volumes()))
def test_oracle_equals_scipy(name, connectivity):
    m = R.volumes()[name] != 0
    s = structure(connectivity)
    for n in ITERATIONS:
        for bv in (0, 1):
            assert np.array_equal(R.dilate(m, connectivity, n, bv), ndi.binary_dilation(m, s, n, border_value=bv)), ("dilate", n, bv)
            assert np.array_equal(R.erode(m, connectivity, n, bv), ndi.binary_erosion(m, s, n, border_value=bv)), ("erode", n, bv)
        assert np.array_equal(R.opening(m, connectivity, n), ndi.binary_opening(m, s, n)), ("opening", n)
        assert np.array_equal(R.closing(m, connectivity, n), ndi.binary_closing(m, s, n)), ("closing", n)
    assert np.array_equal(R.fill_holes(m.astype(np.uint8), connectivity), ndi.binary_fill_holes(m, s)), "fill_holes"
    assert np.array_equal(R.inner_boundary(m, connectivity), m & ~ndi.binary_erosion(m, s)), "inner boundary"


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_single_voxels_and_long_runs(connectivity):
    s = structure(connectivity)
    for shape in R.seam_shapes():
        big = sum(shape) + 5                               # more iterations than any extent: stationary
        for pos in R.single_voxels(shape):
            m = np.zeros(shape, dtype=bool)
            m[pos] = True
            assert np.array_equal(R.clipped_element(shape, pos, connectivity), ndi.binary_dilation(m, s)), (shape, pos)
            assert np.array_equal(R.dilate(m, connectivity), ndi.binary_dilation(m, s))
            assert np.array_equal(R.erode(~m, connectivity, 1, 1), ndi.binary_erosion(~m, s, border_value=1))
        m = np.zeros(shape, dtype=bool)
        m[0, 0, 0] = True
        assert R.dilate(m, connectivity, big).all() and np.array_equal(R.dilate(m, connectivity, big), ndi.binary_dilation(m, s, big))
        assert not R.erode(~m, connectivity, big, 1).any() and not R.erode(np.ones(shape), connectivity, big).any()
        assert R.erode(np.ones(shape), connectivity, big, 1).all() and not R.dilate(np.zeros(shape), connectivity, big).any()


def test_six_connected_growth_needs_the_sum_of_the_extents():
    """a corner voxel fills a 5 x 5 x 5 volume after 12 six-connected dilations, not 5: an iteration count may be cut at D + H + W, not at the largest extent"""
    m = np.zeros((5, 5, 5), dtype=np.uint8)
    m[0, 0, 0] = 1
    assert not R.dilate(m, 6, 11).all() and R.dilate(m, 6, 12).all() and R.dilate(m, 26, 4).all()


def test_pack_layout():
    m = np.zeros((2, 3, 70), dtype=np.uint8)
    m[0, 0, 0] = m[0, 0, 63] = m[0, 0, 64] = m[1, 2, 69] = 1
    w = R.pack(m).view(np.uint64).reshape(2, 3, 2)
    assert w[0, 0, 0] == (1 | (1 << 63)) and w[0, 0, 1] == 1 and w[1, 2, 1] == 1 << 5 and int((w != 0).sum()) == 3
    assert R.words((2, 3, 70)) == 12 and R.tail_ones((2, 3, 70)).view(np.uint64)[1] == (0xFFFFFFFFFFFFFFFF << 6) & 0xFFFFFFFFFFFFFFFF
    assert not R.tail_ones((2, 3, 64)).any()


# ---------------------------------------------------------------------------------------------------------------------- the multi-class hole rule
def test_hole_rule_hand_built():
    # a 1-D-like corridor in a 3 x 3 x W volume would touch faces; use 5 x 5 x 5 blocks with a one-voxel cavity at the centre
    block = np.ones((5, 5, 5), dtype=np.uint8)
    block[2, 2, 2] = 0
    want = np.ones((5, 5, 5), dtype=np.uint8)
    assert np.array_equal(R.fill_holes(block, 6), want) and np.array_equal(R.fill_holes(block, 26), want)
    two = block.copy()
    two[2, 2, 3] = 2                                       # a face neighbour of the cavity holds another class
    assert np.array_equal(R.fill_holes(two, 6), two) and np.array_equal(R.fill_holes(two, 26), two)
    diag = block.copy()
    diag[1, 1, 1] = 2                                      # a corner neighbour: seen at 26 only
    filled = diag.copy()
    filled[2, 2, 2] = 1
    assert np.array_equal(R.fill_holes(diag, 6), filled) and np.array_equal(R.fill_holes(diag, 18), filled) and np.array_equal(R.fill_holes(diag, 26), diag)
    sevens = block * 7
    want7 = np.full((5, 5, 5), 7, dtype=np.uint8)
    assert np.array_equal(R.fill_holes(sevens, 6), want7) and np.array_equal(R.fill_holes(sevens, 6, [7]), want7) and np.array_equal(R.fill_holes(sevens, 6, [1, 2]), sevens)
    assert np.array_equal(R.fill_holes(sevens, 6, []), want7)
    face = block.copy()
    face[2, 2, 0:3] = 0                                    # the cavity runs to the face x = 0
    assert np.array_equal(R.fill_holes(face, 6), face)


def test_constructed_hole_cases():
    v = R.hole_cases()
    n = lambda a: int((a != 0).sum())
    shell = v["closed_shell"]
    assert n(R.fill_holes(shell, 6)) - n(shell) == 3 * 4 * 5 and n(R.fill_holes(shell, 26)) - n(shell) == 60
    pin = v["diagonal_pinhole"]
    assert n(R.fill_holes(pin, 6)) - n(pin) == 60 and n(R.fill_holes(pin, 18)) - n(pin) == 60 and np.array_equal(R.fill_holes(pin, 26), pin)
    assert np.array_equal(R.fill_holes(v["cavity_at_face"], 6), v["cavity_at_face"])
    for x in (63, 64):
        f = R.fill_holes(v[f"one_voxel_x{x}"], 6)
        assert f[1, 1, x] == 1 and n(f) - n(v[f"one_voxel_x{x}"]) == 1
    big = v["across_cc_tiles"]
    assert n(R.fill_holes(big, 6)) - n(big) == 7 * 7 * 15
    two = v["two_classes"]
    assert np.array_equal(R.fill_holes(two, 6), two) and n(R.fill_holes((two != 0).astype(np.uint8), 6)) - n(two) == 60
    isl = v["island"]
    assert np.array_equal(R.fill_holes(isl, 6), isl)
    mixed = v["applied_labels"]
    both, only3 = R.fill_holes(mixed, 6), R.fill_holes(mixed, 6, [3])
    assert int((both == 3).sum()) - int((mixed == 3).sum()) == 60 and int((both == 5).sum()) - int((mixed == 5).sum()) == 60
    assert int((only3 == 3).sum()) == int((both == 3).sum()) and np.array_equal(only3 == 5, mixed == 5)
    rnd = v["bern_12x12x70_p80"]
    assert n(R.fill_holes(rnd, 6)) > n(R.fill_holes(rnd, 26)) >= n(rnd)


def test_label_map_forms_hand_built():
    lab = np.zeros((1, 1, 9), dtype=np.uint8)
    lab[0, 0] = [1, 0, 0, 2, 2, 0, 1, 0, 1]
    assert R.dilate_labels(lab, 6, 1, [1, 2])[0, 0].tolist() == [1, 1, 2, 2, 2, 1, 1, 1, 1]          # class 1 first: it takes the free voxels next to it
    assert R.dilate_labels(lab, 6, 1, [2, 1])[0, 0].tolist() == [1, 1, 2, 2, 2, 2, 1, 1, 1]
    assert R.dilate_labels(lab, 6, 1)[0, 0].tolist() == [1, 1, 1, 2, 2, 1, 1, 1, 1]
    assert np.array_equal(R.close_labels(lab, 6, 1, [1]), lab)                                       # one row: the closing erodes to nothing at the faces, nothing is removed
    rows = np.broadcast_to(lab, (3, 3, 9)).copy()
    want = rows.copy()
    want[1, 1, 7] = 1                                      # the gap at x = 7 closes in the one row that has no face next to it
    assert np.array_equal(R.close_labels(rows, 6, 1, [1]), want) and np.array_equal(R.close_labels(rows, 6, 1, [2]), rows)
    assert R.erode_labels(lab, 6, 1, [2])[0, 0].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 1]
    assert R.open_labels(lab, 6, 1, [1])[0, 0].tolist() == [0, 0, 0, 2, 2, 0, 0, 0, 0]
    assert R.erode_labels(lab, 6, 1)[0, 0].tolist() == [0] * 9 and R.open_labels(lab, 6, 1)[0, 0].tolist() == [0] * 9


# ---------------------------------------------------------------------------------------------------------------------- Postprocess
def test_postprocess_from_config_with_the_morphology_keys():
    from veloxseg_amd.utils.components import Postprocess
    p = Postprocess.from_config({"closing": 1})
    assert p.closing == 1 and p.opening is None and not p.fill_holes and p.morph_connectivity == 6 and p.labels is None and not p.identity
    p = Postprocess.from_config({"closing": 2, "opening": 3, "fill_holes": True, "morph_connectivity": 18, "labels": [2, 1], "min_voxels": 4})
    assert (p.closing, p.opening, p.fill_holes, p.morph_connectivity, p.labels, p.min_voxels, p.connectivity) == (2, 3, True, 18, [2, 1], 4, 26)
    assert not Postprocess.from_config({"fill_holes": True}).identity and not Postprocess.from_config({"opening": 1}).identity
    assert Postprocess.from_config({"fill_holes": False, "morph_connectivity": 26, "labels": [1], "closing": 0}).identity
    assert Postprocess.from_config({}).identity and Postprocess.from_config(None).identity
    x = torch.zeros((2, 2, 2), dtype=torch.uint8)
    assert Postprocess.from_config({"morph_connectivity": 18})(x) is x
    with pytest.raises(ValueError, match="unknown keys"):
        Postprocess.from_config({"closings": 1})
    with pytest.raises(ValueError, match="negative"):
        Postprocess.from_config({"closing": -1})
    with pytest.raises(ValueError, match="negative"):
        Postprocess.from_config({"opening": -2})
    with pytest.raises(ValueError, match="connectivity"):
        Postprocess.from_config({"morph_connectivity": 8})


def test_python_layer_refuses_host_tensors_and_bad_arguments():
    from veloxseg_amd.utils import morphology as M
    x = torch.zeros((2, 3, 4), dtype=torch.uint8)
    for fn in (M.binary_dilation, M.binary_erosion, M.binary_opening, M.binary_closing, M.inner_boundary, M.fill_holes, M.close_labels, M.pack):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(x)
    with pytest.raises(ValueError, match="iterations"):
        M.binary_dilation(x, iterations=0)
    with pytest.raises(ValueError, match="connectivity"):
        M.binary_erosion(x, connectivity=8)
    with pytest.raises(ValueError, match="border_value"):
        M.binary_closing(x, border_value=2)
    with pytest.raises(TypeError, match="dtype"):
        M.fill_holes(x.float())
    with pytest.raises(ValueError, match="expected"):
        M.open_labels(x[0])
