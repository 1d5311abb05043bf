"""The premise of tests/test_components_gpu.py, on the CPU: the numpy oracle (tests/components_ref.py) equals scipy.ndimage.label -- labels, numbering and count -- on
every input the GPU file uses, the hand-built inputs have the shape their tests rely on, and the Python layer refuses what it documents to refuse before touching a
GPU."""
import numpy as np
import pytest
import torch

import components_ref as R

STRUCTURE_RANK = {6: 1, 18: 2, 26: 3}


def scipy_label(vol, connectivity):
    """scipy labels a binary map; a multi-valued one is the union over its values, renumbered by smallest flat index (what `same non-zero value` means)"""
    ndi = pytest.importorskip("scipy.ndimage")
    st = ndi.generate_binary_structure(3, STRUCTURE_RANK[connectivity])
    vol = np.asarray(vol)
    values = [v for v in np.unique(vol) if v != 0]
    if len(values) <= 1:
        cc, n = ndi.label(vol != 0, structure=st)
        return cc.astype(np.int32), int(n)
    firsts, maps = [], []
    for v in values:
        cc, n = ndi.label(vol == v, structure=st)
        flat = cc.reshape(-1)
        idx = np.full(n + 1, flat.size, dtype=np.int64)
        np.minimum.at(idx, flat, np.arange(flat.size))
        firsts.append(idx[1:])
        maps.append(cc)
    order = np.argsort(np.concatenate(firsts), kind="stable")
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(1, order.size + 1)
    out, base = np.zeros(vol.shape, dtype=np.int32), 0
    for cc, f in zip(maps, firsts):
        lut = np.concatenate([[0], rank[base:base + f.size]])
        out += lut[cc].astype(np.int32)
        base += f.size
    return out, int(order.size)


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", list(R.volumes()))
def test_reference_equals_scipy(name, connectivity):
    cc, n = R.reference(name, connectivity)
    want, wn = scipy_label(R.volumes()[name], connectivity)
    assert n == wn and np.array_equal(cc, want), f"{name} / {connectivity}: {n} components against scipy's {wn}"


@pytest.mark.parametrize("name", ["multiclass_10x12x40", "blobs_gt", "blobs_pred", "lesion_gt", "lesion_one_voxel", "lesion_touching", "lesion_empty"])
def test_reference_equals_scipy_on_binarised_inputs(name):
    """what the filters with binary = True and the lesion metrics label: the map != 0 (blobs at 6 and 18, the others at every connectivity the GPU file uses)"""
    vol = (R.volumes()[name] != 0).astype(np.uint8)
    for connectivity in R.CONNECTIVITIES:
        cc, n = R.label(vol, connectivity)
        want, wn = scipy_label(vol, connectivity)
        assert n == wn and np.array_equal(cc, want), (name, connectivity)


def test_sparse_big_arithmetic_equals_scipy():
    """the expectation of the volume above 2^26 voxels is formed by arithmetic: here it is checked against scipy once, at the widest connectivity (no two of its
    components touch even there; the pair is face-adjacent)"""
    shape, idx, ids, n = R.sparse_big()
    V = int(np.prod(shape))
    assert V > 2 ** 26 and -(-V // 262144) > 256 and idx[0] == 0 and idx[-1] == V - 1 and n == idx.size - 1
    vol = np.zeros(V, dtype=np.uint8)
    vol[idx] = 1
    cc, wn = scipy_label(vol.reshape(shape), 26)          # the connectivity the GPU test runs
    assert wn == n and np.array_equal(cc.reshape(-1)[idx], ids) and int((cc != 0).sum()) == idx.size


def test_pair_cases_reference_equals_scipy_and_counts():
    cases = R.pair_cases()
    assert len(cases) == 13 + 7 and {nz for *_, nz in cases} == {1, 2, 3}          # (b at the last index has no room for an offset with a -1)
    for cid, shape, a, b, nz in cases:
        assert all(0 <= c < n for c, n in zip(a + b, shape + shape)), cid
        if cid.startswith("seam"):
            assert all((p // t != q // t) == (p != q) for p, q, t in zip(a, b, R.TILE)), f"{cid}: the pair is not astride the seam of every axis it extends on"
        else:
            assert b == tuple(n - 1 for n in shape)
        vol = np.zeros(shape, dtype=np.uint8)
        vol[a] = vol[b] = 1
        for connectivity in R.CONNECTIVITIES:
            cc, n = R.label(vol, connectivity)
            want, wn = scipy_label(vol, connectivity)
            assert n == wn == (1 if nz <= R.MAX_NONZERO[connectivity] else 2) and np.array_equal(cc, want), (cid, connectivity)


def test_premise_rows():
    """what the hand-built inputs are meant to be"""
    assert [R.reference("checker_8x9x10", c)[1] for c in R.CONNECTIVITIES] == [360, 1, 1]
    s = R.volumes()["serpentine"]
    assert all(R.reference("serpentine", c)[1] == 1 for c in R.CONNECTIVITIES)
    a, b = R._edges(s, 6)
    deg = np.bincount(np.concatenate([a, b]), minlength=s.size)[s.reshape(-1) != 0]
    assert int((deg == 1).sum()) == 2 and int((deg == 2).sum()) == deg.size - 2 and deg.size > 1500, "the serpentine is not one simple chain"
    assert all(R.reference("twin_paths", c)[1] == 2 for c in R.CONNECTIVITIES)
    t = R.volumes()["twin_paths"]
    assert np.array_equal(t[7] * 2, t[8]) and int(t[7].sum()) > 150          # face-adjacent along the whole length
    assert [R.reference("empty_5x6x7", c)[1] for c in R.CONNECTIVITIES] == [0, 0, 0] and [R.reference("full_9x10x40", c)[1] for c in R.CONNECTIVITIES] == [1, 1, 1]
    n = [R.reference(k, c)[1] for k in ("bern_19x21x37_p12", "bern_19x21x37_p30", "bern_33x17x70_p20") for c in R.CONNECTIVITIES]
    assert min(n) >= 2 and max(n) > 1000, n                                  # from a handful of large components to thousands of small ones
    assert R.reference("multiclass_48x50x52", 6)[1] > 20000
    assert len(R.forward_offsets(6)) == 3 and len(R.forward_offsets(18)) == 9 and len(R.forward_offsets(26)) == 13


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_big_volume_arithmetic_equals_scipy(connectivity):
    """the expectation of the volume above the grid caps is formed by arithmetic from the pattern's reference: here it is checked against scipy once"""
    vol, cc, n = R.big_volume(connectivity)
    assert vol.shape == (522, 64, 252) and vol[0, 0, 0] == 1 and vol[-1, -1, -1] == 1 and cc[0, 0, 0] == 1 and cc[-1, -1, -1] == n
    want, wn = scipy_label(vol, connectivity)
    assert n == wn == 58 * 4 * 7 * R.reference("pattern_4x12x28", connectivity)[1] + 2 and np.array_equal(cc, want)


def test_filters_and_lesion_reference_known_answers():
    vol = np.zeros((3, 4, 12), dtype=np.uint8)
    vol[0, 0, 0:3] = 1          # id 1, 3 voxels
    vol[1, 2, 5:8] = 2          # id 2, 3 voxels (equal size: the lower id wins)
    vol[2, 3, 10:12] = 1        # id 3, 2 voxels
    assert R.label(vol, 26)[1] == 3
    assert np.array_equal(R.keep_largest(vol, 1, 26), np.where(R.label(vol, 26)[0] == 1, vol, 0))
    assert np.array_equal(R.keep_largest(vol, 2, 26) != 0, np.isin(R.label(vol, 26)[0], (1, 2))) and np.array_equal(R.keep_largest(vol, 7, 26), vol)
    assert np.array_equal(R.remove_small(vol, 3, 26), np.where(R.label(vol, 26)[0] == 3, 0, vol))          # a component of exactly min_voxels stays
    assert not R.remove_small(vol, 4, 26).any() and np.array_equal(R.remove_small(vol, 2, 26), vol)
    gt, pred = np.zeros((4, 4, 8), dtype=np.uint8), np.zeros((4, 4, 8), dtype=np.uint8)
    gt[0, 0, 0:4] = 1           # detected through ONE shared voxel
    gt[3, 3, 0:2] = 1           # missed: 2 voxels of false-negative volume; pred touches it without overlap
    pred[0, 0, 3:6] = 1
    pred[3, 3, 2:5] = 1         # 3 voxels of false-positive volume
    m = R.lesion_metrics(gt, pred, voxel_volume=0.5)
    assert m == {"false_pos_vol": 1.5, "false_neg_vol": 1.0, "n_gt": 2, "n_pred": 2, "n_gt_detected": 1, "n_pred_matched": 1, "dice": 2.0 * 1 / 12}
    assert R.lesion_metrics(gt * 0, pred * 0)["dice"] == 1.0


def test_postprocess_from_config_refusals():
    from veloxseg_amd.utils.components import Postprocess
    assert Postprocess.from_config(None).identity and Postprocess.from_config({}).identity
    x = torch.zeros(2, 1, 3, 4, 5, dtype=torch.uint8)
    assert Postprocess.from_config(None)(x) is x
    p = Postprocess.from_config({"min_voxels": 10, "keep_largest": 2, "connectivity": 18, "binary": True})
    assert (p.min_voxels, p.keep_largest, p.connectivity, p.binary, p.identity) == (10, 2, 18, True, False)
    with pytest.raises(ValueError, match="unknown keys"):
        Postprocess.from_config({"min_voxel": 10})
    with pytest.raises(ValueError, match="connectivity"):
        Postprocess.from_config({"connectivity": 8})
    with pytest.raises(ValueError, match="negative"):
        Postprocess.from_config({"keep_largest": -1})


def test_python_layer_refusals():
    from veloxseg_amd.utils import components as C
    from veloxseg_amd.utils.metric.lesion import lesion_metrics
    lab = torch.zeros(4, 5, 6, dtype=torch.uint8)
    for call in (lambda: C.connected_components(lab), lambda: C.remove_small_components(lab, 3), lambda: C.keep_largest_components(lab), lambda: lesion_metrics(lab, lab),
                 lambda: C.component_sizes(lab.int(), [0]), lambda: C.Postprocess(min_voxels=2)(lab)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    with pytest.raises(TypeError, match="not supported"):
        C.connected_components(lab.float())
    with pytest.raises(TypeError, match="not supported"):
        lesion_metrics(lab.double(), lab)
    for bad in (4, 8, 27, 0, "26"):
        with pytest.raises(ValueError, match="connectivity"):
            C.connected_components(lab, connectivity=bad)
    with pytest.raises(ValueError, match="expected"):
        C.connected_components(torch.zeros(2, 2, 4, 5, 6, dtype=torch.uint8))          # two channels: not a label map


def test_abi_refusals_without_gpu():
    """argument checks happen on the host, before anything is launched"""
    from veloxseg_amd import _hip as H
    assert H.query("vx_cc_ws_bytes", 8, 9, 10) == 12 * 12 + 4 and H.query("vx_cc_grid_cap") == 4096
    with pytest.raises(RuntimeError, match="connectivity"):
        H.call("vx_cc_label", 8, 1, 8, 2, 2, 2, 8, 8, 8, None)
    with pytest.raises(RuntimeError, match="32-bit"):
        H.call("vx_cc_label", 8, 1, 8, 2048, 1024, 1024, 26, 8, 8, None)
    with pytest.raises(RuntimeError, match="32-bit"):
        H.query("vx_cc_ws_bytes", 2048, 1024, 1024)
    with pytest.raises(RuntimeError, match="width"):
        H.call("vx_cc_label", 8, 2, 8, 2, 2, 2, 26, 8, 8, None)
    with pytest.raises(RuntimeError, match="come together"):
        H.call("vx_cc_tally", 8, 8, 1, 8, 1, 8, None, None)
