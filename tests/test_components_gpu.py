"""The connected-component kernels (csrc/components.hip) and what is built on them against the numpy oracle of tests/components_ref.py.

Labelling is exact integer work, so every comparison in this file is `==`.  The kernel outputs of the C-ABI tests sit between 64-element canaries
(exact_ref.Guard) and are prefilled with a sentinel; the workspace is prefilled with garbage (the contract says it needs no zero-fill); a refused call raises and
leaves its prefill untouched.  tests/test_components_cpu.py holds the oracle to scipy.ndimage.label on every input used here; this file needs no scipy.

Every grid-stride loop runs above its grid cap in test_above_the_grid_caps; the carry loop of the one-block scan over the chunk sums takes more than one pass only
above 2^26 voxels and runs in test_above_256_scan_chunks."""
import numpy as np
import pytest
import torch

import components_ref as R
from exact_ref import Guard

pytestmark = pytest.mark.gpu

I32_CANARY, I32_FILL, U8_CANARY, U8_FILL, I64_CANARY, I64_FILL = 0x5A5A5A5A, -7, 0xA5, 0xEE, 0x5A5A5A5A5A5A, -7
DTYPES = {1: torch.uint8, 4: torch.int32, 8: torch.int64}


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, copy=True)).cuda()
    return t if dtype is None else t.to(dtype)


def same(got, want, what):
    g = got.detach().cpu().numpy().astype(np.int64).reshape(-1)
    w = np.asarray(want).astype(np.int64).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} elements against {w.size}"
    bad = g != w
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first flat index {i}: got {g[i]}, want {w[i]}")


def abi_label(vol, connectivity, bytes_=1):
    """vx_cc_label through the C ABI into guarded, sentinel-filled outputs -> (cc tensor, N)"""
    H = _H()
    lab = dev(vol, DTYPES[bytes_])
    D, Hh, W = lab.shape
    cc = Guard((D, Hh, W), torch.int32, fill=I32_FILL, canary=I32_CANARY)
    num = Guard((1,), torch.int32, fill=I32_FILL, canary=I32_CANARY)
    nbytes = H.query("vx_cc_ws_bytes", D, Hh, W)
    ws = Guard(((nbytes + 7) // 8,), torch.int64, fill=I64_FILL, canary=I64_CANARY)
    H.call("vx_cc_label", lab.data_ptr(), bytes_, cc.ptr, D, Hh, W, connectivity, ws.ptr, num.ptr, H.stream_ptr())
    torch.cuda.synchronize()
    for g, n in ((cc, "cc"), (num, "num"), (ws, "workspace")):
        g.check(f"vx_cc_label {n}")
    return cc.t, int(num.t.item())


def check_label(vol, connectivity, want, what, bytes_=1):
    cc, n = abi_label(vol, connectivity, bytes_)
    assert n == want[1], f"{what}: {n} components, want {want[1]}"
    same(cc, want[0], what)
    return cc, n


# ====================================================================================================================== vx_cc_label
@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
def test_adjacent_pairs(connectivity):
    for cid, shape, a, b, nz in R.pair_cases():
        vol = np.zeros(shape, dtype=np.uint8)
        vol[a] = vol[b] = 1
        joined = nz <= R.MAX_NONZERO[connectivity]
        want = np.zeros(shape, dtype=np.int32)
        first, second = sorted((a, b))                     # (tuples order as flat indices do)
        want[first], want[second] = 1, (1 if joined else 2)
        check_label(vol, connectivity, (want, 1 if joined else 2), f"pair {cid} / {connectivity}")


@pytest.mark.parametrize("connectivity", R.CONNECTIVITIES)
@pytest.mark.parametrize("name", ["bern_19x21x37_p12", "bern_19x21x37_p30", "bern_33x17x70_p20", "checker_8x9x10", "serpentine", "twin_paths", "empty_5x6x7", "full_9x10x40",
                                  "one_voxel_set", "one_voxel_clear", "line_x_70", "line_y_40"])
def test_label_equals_reference(name, connectivity):
    check_label(R.volumes()[name], connectivity, R.reference(name, connectivity), f"{name} / {connectivity}")


def test_hand_built_counts():
    assert [abi_label(R.volumes()["checker_8x9x10"], c)[1] for c in R.CONNECTIVITIES] == [360, 1, 1]
    assert [abi_label(R.volumes()["serpentine"], c)[1] for c in R.CONNECTIVITIES] == [1, 1, 1]
    assert [abi_label(R.volumes()["twin_paths"], c)[1] for c in R.CONNECTIVITIES] == [2, 2, 2]


@pytest.mark.parametrize("bytes_", [1, 4, 8])
def test_multiclass_and_label_widths(bytes_):
    vol = R.volumes()["multiclass_48x50x52"]
    check_label(vol, 6, R.reference("multiclass_48x50x52", 6), f"multi-class, {bytes_}-byte labels", bytes_)
    if bytes_ == 8:                                        # values that differ above bit 32 only are different values
        wide = vol.astype(np.int64) << 33
        cc, n = abi_label(wide, 6, 8)
        assert n == R.reference("multiclass_48x50x52", 6)[1]
        same(cc, R.reference("multiclass_48x50x52", 6)[0], "multi-class, values << 33")


def test_python_layer_batch_dtypes_and_determinism():
    from veloxseg_amd.utils import components as C
    a, b = R.volumes()["bern_19x21x37_p12"], R.volumes()["bern_19x21x37_p30"]
    batch = dev(np.stack([a, b])[:, None])
    cc, num = C.connected_components(batch, 18)
    assert cc.shape == batch.shape and cc.dtype == torch.int32 and num == [R.reference("bern_19x21x37_p12", 18)[1], R.reference("bern_19x21x37_p30", 18)[1]]
    same(cc[0], R.reference("bern_19x21x37_p12", 18)[0], "batch sample 0")
    same(cc[1], R.reference("bern_19x21x37_p30", 18)[0], "batch sample 1")          # numbered independently
    cc2, num2 = C.connected_components(batch, 18)
    assert torch.equal(cc, cc2) and num == num2
    for t in (batch[1, 0].bool(), batch[1, 0].int(), batch[1, 0].long(), batch[1, 0]):
        c1, n1 = C.connected_components(t)                 # (D, H, W), default connectivity 26
        assert c1.shape == t.shape and n1 == [R.reference("bern_19x21x37_p30", 26)[1]]
        same(c1, R.reference("bern_19x21x37_p30", 26)[0], f"{t.dtype} input")
    strided = torch.zeros((19, 21, 74), dtype=torch.uint8, device="cuda")
    strided[:, :, ::2] = batch[0, 0]
    same(C.connected_components(strided[:, :, ::2], 6)[0], R.reference("bern_19x21x37_p12", 6)[0], "non-contiguous input")


@pytest.mark.parametrize("connectivity", [6, 26])
def test_above_the_grid_caps(connectivity):
    H = _H()
    vol, want, n = R.big_volume(connectivity)
    cap = H.query("vx_cc_grid_cap")
    tiles = np.prod([-(-s // t) for s, t in zip(vol.shape, R.TILE)])
    assert tiles > cap and vol.size > 256 * cap, "the volume no longer exceeds the grid caps"
    cc, got_n = abi_label(vol, connectivity)
    assert got_n == n and int(cc[0, 0, 0]) == 1 and int(cc[-1, -1, -1]) == n
    assert torch.equal(cc, dev(want)), "component map of the tiled pattern"
    # tally and select above their caps, on the same map
    sizes = Guard((n + 1,), torch.int64, fill=0, canary=I64_CANARY)
    hits = Guard((n + 1,), torch.int64, fill=0, canary=I64_CANARY)
    other = np.zeros(vol.shape, dtype=np.uint8)
    other[::3, :, ::5] = 1
    other[0, 0, 0] = other[-1, -1, -1] = 1
    H.call("vx_cc_tally", cc.data_ptr(), dev(other).data_ptr(), 1, vol.size, n, sizes.ptr, hits.ptr, H.stream_ptr())
    keep = np.zeros(n + 1, dtype=np.uint8)
    keep[1::2] = 1                                         # every other component, the voxel at index 0 among them
    out = Guard(vol.shape, torch.uint8, fill=U8_FILL, canary=U8_CANARY)
    H.call("vx_cc_select", cc.data_ptr(), dev(keep).data_ptr(), n, dev(vol).data_ptr(), out.ptr, 1, vol.size, H.stream_ptr())
    torch.cuda.synchronize()
    for g in (sizes, hits, out):
        g.check("tally / select above the caps")
    same(sizes.t, np.bincount(want.reshape(-1), minlength=n + 1), "sizes above the cap")
    same(hits.t, np.bincount(want.reshape(-1), weights=other.reshape(-1), minlength=n + 1), "hits above the cap")
    assert torch.equal(out.t, dev(np.where(keep[want] != 0, vol, 0).astype(np.uint8))), "select above the cap"


def test_above_256_scan_chunks():
    """71 M voxels = 272 scan chunks: the one-block scan over the chunk sums carries across its 256-entry passes, and a component lies astride a chunk boundary.
    Inputs, outputs and checks stay on the device (the expectation is 75 voxels in 74 components at known flat indices, the rest background)."""
    H = _H()
    shape, idx, ids, n = R.sparse_big()
    V = int(np.prod(shape))
    lab = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    where = torch.from_numpy(idx).cuda()
    lab.view(-1)[where] = 1
    cc = Guard(shape, torch.int32, fill=I32_FILL, canary=I32_CANARY)
    num = Guard((1,), torch.int32, fill=I32_FILL, canary=I32_CANARY)
    ws = Guard(((H.query("vx_cc_ws_bytes", *shape) + 7) // 8,), torch.int64, fill=I64_FILL, canary=I64_CANARY)
    H.call("vx_cc_label", lab.data_ptr(), 1, cc.ptr, *shape, 26, ws.ptr, num.ptr, H.stream_ptr())
    torch.cuda.synchronize()
    for g, what in ((cc, "cc"), (num, "num"), (ws, "workspace")):
        g.check(f"vx_cc_label {what}")
    assert int(num.t.item()) == n
    flat = cc.t.view(-1)
    same(flat[where], ids, "ids of the sparse voxels")
    assert int((flat != 0).sum()) == idx.size and int(flat.min()) == 0, "background voxels carry an id"
    assert V > 2 ** 26


# ====================================================================================================================== tally, filters
@pytest.mark.parametrize("other_bytes", [0, 1, 4, 8])
def test_tally_equals_reference(other_bytes):
    H = _H()
    name = "bern_33x17x70_p20"
    want_cc, n = R.reference(name, 18)
    cc = dev(want_cc)
    other = np.resize(R.volumes()["bern_19x21x37_p30"], want_cc.shape) * 3
    sizes = Guard((n + 1,), torch.int64, fill=torch.arange(n + 1), canary=I64_CANARY)          # `+=`: prefilled with what the oracle adds to
    hits = Guard((n + 1,), torch.int64, fill=torch.arange(n + 1) * 2, canary=I64_CANARY)
    o = dev(other, DTYPES[other_bytes]) if other_bytes else None
    H.call("vx_cc_tally", cc.data_ptr(), None if o is None else o.data_ptr(), other_bytes, want_cc.size, n, sizes.ptr, hits.ptr if o is not None else None, H.stream_ptr())
    torch.cuda.synchronize()
    sizes.check("vx_cc_tally sizes")
    hits.check("vx_cc_tally hits")
    ws, wh = R.tally(want_cc, n, other)
    same(sizes.t, ws + np.arange(n + 1), "sizes")
    same(hits.t, (wh if o is not None else 0) + 2 * np.arange(n + 1), "hits")


def test_tally_skips_ids_outside_the_table():
    H = _H()
    cc = dev(np.array([0, 1, 1, 5, -3, 2, 2, 2, 9, 0], dtype=np.int32))
    sizes = Guard((3,), torch.int64, fill=0, canary=I64_CANARY)
    H.call("vx_cc_tally", cc.data_ptr(), None, 0, 10, 2, sizes.ptr, None, H.stream_ptr())
    torch.cuda.synchronize()
    sizes.check("vx_cc_tally with stray ids")
    assert sizes.t.tolist() == [2, 2, 3]


def test_tally_hot_and_colliding_ids():
    """one id that holds most voxels (the wave's leading id), ids that share a slot of the block's LDS table (equal modulo 256), short and long runs, more than one
    slab per block"""
    H = _H()
    rng = np.random.default_rng(11)
    n, V = 1500, 300007
    ids = rng.choice(np.array([0, 1, 1, 1, 1, 257, 513, 1025, 2, 7, 1500], dtype=np.int32), size=V)
    ids[1000:70000] = 1                                    # whole waves and blocks of one id
    ids[70000:70300] = np.arange(300, dtype=np.int32) + 600
    other = (rng.random(V) < 0.4).astype(np.uint8)
    sizes = Guard((n + 1,), torch.int64, fill=0, canary=I64_CANARY)
    hits = Guard((n + 1,), torch.int64, fill=0, canary=I64_CANARY)
    H.call("vx_cc_tally", dev(ids).data_ptr(), dev(other).data_ptr(), 1, V, n, sizes.ptr, hits.ptr, H.stream_ptr())
    torch.cuda.synchronize()
    sizes.check("vx_cc_tally sizes")
    hits.check("vx_cc_tally hits")
    same(sizes.t, np.bincount(ids, minlength=n + 1), "sizes")
    same(hits.t, np.bincount(ids, weights=other, minlength=n + 1), "hits")


def test_component_sizes_python():
    from veloxseg_amd.utils import components as C
    vol = R.volumes()["blobs_gt"]
    other = R.volumes()["blobs_pred"]
    cc, num = C.connected_components(dev(vol), 26)
    want_cc, n = R.reference("blobs_gt", 26)
    assert num == [n]
    ws, wh = R.tally(want_cc, n, other)
    s = C.component_sizes(cc, num)
    assert s.dtype == torch.int64 and s.is_cuda
    same(s, ws, "component_sizes")
    s2, h2 = C.component_sizes(cc, num[0], dev(other))
    same(s2, ws, "component_sizes with other")
    same(h2, wh, "hits")
    sb, hb = C.component_sizes(torch.stack([cc, cc])[:, None], [n, n], torch.stack([dev(other), dev(vol)])[:, None])
    same(hb[0], wh, "batched hits 0")
    same(hb[1][1:], ws[1:], "batched hits 1 (a map against itself)")
    same(sb[1], ws, "batched sizes 1")


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64])
def test_filters_equal_reference(dtype):
    from veloxseg_amd.utils import components as C
    vol = R.volumes()["ties_9x10x40"]                      # sizes 5, 5, 4, 1
    x = dev(vol, dtype)
    for k in (0, 1, 2, 3, 4, 9):                           # k = 1: one of two equal largest; k > N keeps everything
        got = C.keep_largest_components(x, k, 26)
        assert got.dtype == dtype and got.shape == x.shape
        same(got, R.keep_largest(vol, k, 26), f"keep_largest k = {k}")
    same(C.keep_largest_components(x, 1, 26), np.where(R.label(vol, 26)[0] == 1, vol, 0), "the lower id of two equal sizes")
    for m in (0, 1, 2, 4, 5, 6):                           # 4 and 5 are sizes of components: those stay
        same(C.remove_small_components(x, m, 26), R.remove_small(vol, m, 26), f"remove_small min_voxels = {m}")
    assert int((C.remove_small_components(x, 5, 26) != 0).sum()) == 10 and int((C.remove_small_components(x, 6, 26) != 0).sum()) == 0
    assert torch.equal(x, dev(vol, dtype)), "the input was modified"
    for name in ("blobs_gt", "multiclass_10x12x40"):
        v = R.volumes()[name]
        for binary in (False, True):
            same(C.remove_small_components(dev(v, dtype), 7, 6, binary=binary), R.remove_small(v, 7, 6, binary), f"{name}: remove_small binary = {binary}")
            same(C.keep_largest_components(dev(v, dtype), 3, 6, binary=binary), R.keep_largest(v, 3, 6, binary), f"{name}: keep_largest binary = {binary}")


def test_filters_bool_batch_and_postprocess():
    from veloxseg_amd.utils import components as C
    a, b = R.volumes()["blobs_gt"], R.volumes()["blobs_pred"]
    batch = dev(np.stack([a, b])[:, None]).bool()
    got = C.remove_small_components(batch, 30, 18)
    assert got.dtype == torch.bool and got.shape == batch.shape
    same(got[0, 0], R.remove_small(a, 30, 18), "bool batch sample 0")
    same(got[1, 0], R.remove_small(b, 30, 18), "bool batch sample 1")
    p = C.Postprocess.from_config({"min_voxels": 30, "keep_largest": 2, "connectivity": 18})
    same(p(batch.to(torch.uint8))[1, 0], R.keep_largest(R.remove_small(b, 30, 18), 2, 18), "Postprocess: small ones first, then the two largest")
    x = batch.to(torch.uint8)
    assert C.Postprocess.from_config(None)(x) is x


def test_select_in_place():
    H = _H()
    vol = R.volumes()["blobs_gt"].astype(np.int64) * 5
    want_cc, n = R.reference("blobs_gt", 26)
    keep = np.zeros(n + 1, dtype=np.uint8)
    keep[2:] = 1
    buf = Guard(vol.shape, torch.int64, fill=torch.from_numpy(vol.copy()), canary=I64_CANARY)
    H.call("vx_cc_select", dev(want_cc).data_ptr(), dev(keep).data_ptr(), n, buf.ptr, buf.ptr, 8, vol.size, H.stream_ptr())
    torch.cuda.synchronize()
    buf.check("vx_cc_select in place")
    same(buf.t, np.where(want_cc >= 2, vol, 0), "select in place")


# ====================================================================================================================== lesion metrics
def _lesion_cases():
    v = R.volumes()
    gt, one, touch, z = v["lesion_gt"], v["lesion_one_voxel"], v["lesion_touching"], v["lesion_empty"]
    return {"one_voxel_overlap": (gt, one), "touching_but_disjoint": (gt, touch), "empty_pred": (gt, z), "empty_gt": (z, one), "both_empty": (z, z),
            "blobs": (R.volumes()["blobs_gt"], R.volumes()["blobs_pred"])}


@pytest.mark.parametrize("case", list(_lesion_cases()))
def test_lesion_metrics_equal_reference(case):
    from veloxseg_amd.utils.metric.lesion import lesion_metrics
    gt, pred = _lesion_cases()[case]
    for connectivity in (18, 6):
        got = lesion_metrics(dev(gt), dev(pred, torch.int64), voxel_volume=2.5, connectivity=connectivity)
        assert got == R.lesion_metrics(gt, pred, 2.5, connectivity), (case, connectivity, got)
    if case == "one_voxel_overlap":
        assert got["n_gt_detected"] == 1 and got["n_pred_matched"] == 1 and got["false_pos_vol"] == 0.0 and got["false_neg_vol"] == 4 * 2.5
    if case == "touching_but_disjoint":
        assert got["n_gt_detected"] == 0 and got["false_pos_vol"] == 18 * 2.5 and got["false_neg_vol"] == (54 + 4) * 2.5 and got["dice"] == 0.0
    if case == "both_empty":
        assert got == {"false_pos_vol": 0.0, "false_neg_vol": 0.0, "n_gt": 0, "n_pred": 0, "n_gt_detected": 0, "n_pred_matched": 0, "dice": 1.0}


def test_lesion_metrics_batch():
    from veloxseg_amd.utils.metric.lesion import lesion_metrics
    cases = _lesion_cases()
    (g0, p0), (g1, p1) = cases["one_voxel_overlap"], cases["empty_pred"]
    got = lesion_metrics(dev(np.stack([g0, g1])[:, None]), dev(np.stack([p0, p1])[:, None]))
    assert got == [R.lesion_metrics(g0, p0), R.lesion_metrics(g1, p1)]


# ====================================================================================================================== refusals
def test_refused_abi_calls_leave_the_prefill():
    H = _H()
    lab = torch.ones((4, 5, 6), dtype=torch.uint8, device="cuda")
    cc = Guard((4, 5, 6), torch.int32, fill=I32_FILL, canary=I32_CANARY)
    num = Guard((1,), torch.int32, fill=I32_FILL, canary=I32_CANARY)
    ws = Guard((64,), torch.int64, fill=I64_FILL, canary=I64_CANARY)
    st = H.stream_ptr()
    for args, msg in (((lab.data_ptr(), 1, cc.ptr, 4, 5, 6, 8, ws.ptr, num.ptr, st), "connectivity"),
                      ((lab.data_ptr(), 2, cc.ptr, 4, 5, 6, 26, ws.ptr, num.ptr, st), "width"),
                      ((lab.data_ptr(), 1, cc.ptr, 2048, 1024, 1024, 26, ws.ptr, num.ptr, st), "32-bit"),
                      ((lab.data_ptr(), 1, cc.ptr, 4, 0, 6, 26, ws.ptr, num.ptr, st), "bad sizes"),
                      ((lab.data_ptr(), 1, cc.ptr, 4, 5, 6, 26, None, num.ptr, st), "null"),
                      ((lab.data_ptr(), 1, cc.ptr, 4, 5, 6, 26, ws.ptr + 4, num.ptr, st), "aligned")):
        with pytest.raises(RuntimeError, match=msg):
            H.call("vx_cc_label", *args)
    sizes = Guard((8,), torch.int64, fill=I64_FILL, canary=I64_CANARY)
    out = Guard((4, 5, 6), torch.uint8, fill=U8_FILL, canary=U8_CANARY)
    with pytest.raises(RuntimeError, match="come together"):
        H.call("vx_cc_tally", cc.ptr, lab.data_ptr(), 1, 120, 7, sizes.ptr, None, st)
    with pytest.raises(RuntimeError, match="width"):
        H.call("vx_cc_tally", cc.ptr, lab.data_ptr(), 2, 120, 7, sizes.ptr, sizes.ptr, st)
    with pytest.raises(RuntimeError, match="bad args"):
        H.call("vx_cc_tally", cc.ptr, None, 0, 120, -1, sizes.ptr, None, st)
    with pytest.raises(RuntimeError, match="width"):
        H.call("vx_cc_select", cc.ptr, lab.data_ptr(), 7, lab.data_ptr(), out.ptr, 3, 120, st)
    with pytest.raises(RuntimeError, match="bad args"):
        H.call("vx_cc_select", cc.ptr, None, 7, lab.data_ptr(), out.ptr, 1, 120, st)
    torch.cuda.synchronize()
    for g, fill, what in ((cc, I32_FILL, "cc"), (num, I32_FILL, "num"), (ws, I64_FILL, "workspace"), (sizes, I64_FILL, "sizes"), (out, U8_FILL, "select output")):
        g.check(f"refused call: {what}")
        assert bool((g.t == fill).all()), f"a refused call wrote {what}"


# ====================================================================================================================== infer_volume(postprocess=)
def test_infer_volume_postprocess():
    from recipe import CASES, fill_state_dict
    from veloxseg_amd.model.VeloxSeg import VeloxSeg
    from veloxseg_amd.utils import inference_runtime as IR
    from veloxseg_amd.utils.components import Postprocess
    cfg, _ = CASES["g2_32_m2"]
    model = VeloxSeg(**cfg)
    sd = model.state_dict()
    fill_state_dict(sd)
    model.load_state_dict(sd)
    model = model.cuda().eval()
    x = torch.randn((1, 2, 48, 40, 36), generator=torch.Generator().manual_seed(5)).cuda()
    with torch.inference_mode():
        logits, labels = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5)
        plain = labels[0, 0].cpu().numpy()
        # this model's foreground is one 18-connected mass that falls into some 250 pieces under 6-connectivity (one large, the others of a few voxels)
        cc6, n6 = R.label(plain, 6)
        assert n6 >= 3, "the plain label map has nothing to clean up"
        sizes = np.sort(np.bincount(cc6.reshape(-1))[1:])
        m = int(sizes[-2])                                 # the second largest component's size: it stays, smaller ones go
        changed = 0
        for cfg_pp in ({"min_voxels": m, "connectivity": 6}, {"keep_largest": 1, "connectivity": 6}, {"min_voxels": 10},
                       Postprocess(min_voxels=2, keep_largest=2, connectivity=6, binary=True)):
            l2, lab2 = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5, postprocess=cfg_pp)
            assert torch.equal(l2, logits), "the logits changed"
            changed += int(not torch.equal(lab2, labels))
            pp = cfg_pp if isinstance(cfg_pp, Postprocess) else Postprocess.from_config(cfg_pp)
            want = plain
            if pp.min_voxels is not None:
                want = R.remove_small(want, pp.min_voxels, pp.connectivity, pp.binary)
            if pp.keep_largest is not None:
                want = R.keep_largest(want, pp.keep_largest, pp.connectivity, pp.binary)
            assert lab2.dtype == labels.dtype and lab2.shape == labels.shape
            same(lab2, want, f"post-processed labels {cfg_pp}")
        assert changed >= 3, "the 6-connected clean-ups were expected to drop voxels"
        _, lab0 = IR.infer_volume(model, x, (32, 32, 32), 2, 0.5, postprocess=None)
        assert torch.equal(lab0, labels)
