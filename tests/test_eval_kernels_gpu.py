"""The inference, metric and input kernels (csrc/infer.hip, csrc/augment.hip) against exact oracles, straight through the C ABI.

These ten entries index, count and select.  Where they add or interpolate, the data is integer-valued (tests/eval_ref.py; tests/test_eval_ref_cpu.py proves
the premise of every row), so every comparison in this file is `==`: no tolerance appears.
  - outputs written with `=` are prefilled with NaN (float) or with a sentinel (labels, counts, indices); `+=` destinations with integers the oracle adds;
  - every output sits between 64-element canaries (exact_ref.Guard);
  - a refused call raises with a message and leaves its prefill untouched;
  - every grid-stride loop runs once at a size above its grid cap, with distinct values at the first and the last element."""
import numpy as np
import pytest
import torch

import eval_ref as R
import exact_ref as E
from exact_ref import Guard

pytestmark = pytest.mark.gpu

U8_CANARY, U8_FILL = 0xA5, 0xEE
I32_CANARY, I64_CANARY = 0x5A5A5A5A, 0x5A5A5A5A5A5A


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


def dev(a):
    """a device copy of a (read-only) numpy array"""
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def exact(got, want, what):
    """value for value (-0.0 == 0.0); a NaN is expected exactly where the oracle has one"""
    g = got.detach().cpu().numpy().reshape(-1)
    w = np.asarray(want).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} elements against {w.size}"
    if g.dtype.kind == "f" or w.dtype.kind == "f":
        if g.dtype != w.dtype:
            g, w = g.astype(np.float64), w.astype(np.float64)
        ok = (g == w) | ((g != g) & (w != w))
    else:
        ok = g.astype(np.int64) == w.astype(np.int64)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first flat index {i}: got {g[i]!r}, want {w[i]!r}")


def labels_guard(shape):
    return Guard(tuple(shape), torch.uint8, fill=U8_FILL, canary=U8_CANARY)


def done(what, *guards):
    torch.cuda.synchronize()
    for i, g in enumerate(guards):
        g.check(f"{what} (buffer {i})")


def untouched(g, what, fill=None):
    """a NaN-prefilled (fill = None) or sentinel-prefilled guard that a refused call must not have written"""
    done(what, g)
    t = g.t.reshape(-1)
    assert bool((t != t).all()) if fill is None else bool((t == fill).all()), f"{what}: the refused call wrote its output"


# ====================================================================================================================== vx_sw_extract / vx_sw_accumulate
def _win_args(r):
    return (r["C"], *r["vol"], *r["win"], *r["at"])


@pytest.mark.parametrize("row", R.WINDOW_ROWS, ids=lambda r: r["id"])
def test_sw_extract(row):
    H = _H()
    vol = R.ints(row["C"], *row["vol"], seed=R._seed(row["id"]))
    v = dev(vol)
    win = Guard((row["C"], *row["win"]))
    H.call("vx_sw_extract", H.P(v), win.ptr, *_win_args(row), H.stream_ptr())
    done(f"vx_sw_extract {row['id']}", win)
    exact(win.t, R.sw_extract(vol, *row["win"], *row["at"]), f"vx_sw_extract {row['id']}")
    exact(v, vol, "the volume itself")


@pytest.mark.parametrize("weight", [1.0, 0.5, -2.0])
@pytest.mark.parametrize("row", R.WINDOW_ROWS, ids=lambda r: r["id"])
def test_sw_accumulate(row, weight):
    H = _H()
    s = R._seed(row["id"])
    win = R.ints(row["C"], *row["win"], seed=s + 1)
    pre = E.prefill(row["C"], *row["vol"], seed=s + 2)
    acc = Guard((row["C"], *row["vol"]), fill=pre)
    w = dev(win)
    H.call("vx_sw_accumulate", H.P(w), acc.ptr, *_win_args(row), weight, H.stream_ptr())
    done(f"vx_sw_accumulate {row['id']}", acc)
    exact(acc.t, R.sw_accumulate(pre.numpy(), win, *row["at"], weight), f"vx_sw_accumulate {row['id']} weight {weight}")


def test_sw_accumulate_overlapping_windows_in_both_orders():
    H = _H()
    C, vol = 3, (5, 6, 9)
    jobs = [((3, 4, 5), (0, 0, 0), 1.0, R.ints(C, 3, 4, 5, seed=31)), ((3, 4, 5), (2, 2, 4), 0.5, R.ints(C, 3, 4, 5, seed=32)), ((2, 6, 3), (1, 0, 3), -2.0, R.ints(C, 2, 6, 3, seed=33))]
    pre = E.prefill(C, *vol, seed=34)
    want = pre.numpy()
    for shp, at, wt, win in jobs:
        want = R.sw_accumulate(want, win, *at, wt)
    for order in (jobs, jobs[::-1]):
        acc = Guard((C, *vol), fill=pre)
        keep = []
        for shp, at, wt, win in order:
            keep.append(dev(win))
            H.call("vx_sw_accumulate", H.P(keep[-1]), acc.ptr, C, *vol, *shp, *at, wt, H.stream_ptr())
        done("overlapping accumulates", acc)
        exact(acc.t, want, "three overlapping windows")


def test_sw_extract_and_accumulate_above_the_grid_cap():
    """257 x 256 x 256 = 16.84 M elements > 65536 blocks x 256 threads: the grid-stride loops loop.  (The oracle is torch slicing on the device.)"""
    H = _H()
    r = R.WINDOW_OVER_CAP
    (z0, y0, x0), (rd, rh, rw) = r["at"], r["win"]
    vol = E.ints(r["C"], *r["vol"], seed=41).cuda()
    vol[0, z0, y0, x0], vol[0, z0 + rd - 1, y0 + rh - 1, x0 + rw - 1] = 7.0, -7.0        # distinct values at the first and the last element of the window
    win = Guard((r["C"], *r["win"]))
    H.call("vx_sw_extract", H.P(vol), win.ptr, *_win_args(r), H.stream_ptr())
    done("vx_sw_extract over the cap", win)
    want = vol[:, z0:z0 + rd, y0:y0 + rh, x0:x0 + rw]
    assert torch.equal(win.t, want) and float(win.t.reshape(-1)[0]) == 7.0 and float(win.t.reshape(-1)[-1]) == -7.0
    pre = E.prefill(r["C"], *r["vol"], seed=42).cuda()
    acc = Guard((r["C"], *r["vol"]), fill=pre)
    H.call("vx_sw_accumulate", win.ptr, acc.ptr, *_win_args(r), 0.5, H.stream_ptr())
    done("vx_sw_accumulate over the cap", acc)
    pre[:, z0:z0 + rd, y0:y0 + rh, x0:x0 + rw] += 0.5 * want
    assert torch.equal(acc.t, pre)


@pytest.mark.parametrize("case", R.WINDOW_REFUSED, ids=lambda c: "_".join("x".join(map(str, t)) for t in c))
def test_sw_windows_that_leave_the_volume_are_refused(case):
    H = _H()
    vol, win, at = case
    src = torch.zeros(4096, device="cuda")
    out, acc = Guard((2048,)), Guard((2048,))
    with pytest.raises(RuntimeError, match="leaves the volume|non-positive extent"):
        H.call("vx_sw_extract", H.P(src), out.ptr, 1, *vol, *win, *at, H.stream_ptr())
    with pytest.raises(RuntimeError, match="leaves the volume|non-positive extent"):
        H.call("vx_sw_accumulate", H.P(src), acc.ptr, 1, *vol, *win, *at, 1.0, H.stream_ptr())
    untouched(out, "refused vx_sw_extract")
    untouched(acc, "refused vx_sw_accumulate")


# ====================================================================================================================== vx_sw_finalize
def _finalize(H, row, mode):
    acc, cz, cy, cx = R.finalize_case(row)
    q, lab = R.finalize_reference(row)
    C, sp, what = row["C"], tuple(row["sp"]), f"vx_sw_finalize {row['id']} {mode}"
    counts = [dev(a) for a in (cz, cy, cx)]
    src = Guard((C, *sp), fill=torch.from_numpy(np.array(acc, copy=True)))
    out = src if mode == "alias" else Guard((C, *sp)) if mode in ("separate", "out_only") else None
    labels = labels_guard(sp) if mode != "out_only" else None
    H.call("vx_sw_finalize", src.ptr, out.ptr if out else None, labels.ptr if labels else None, *(H.P(c) for c in counts), C, *sp, H.stream_ptr())
    done(what, *(g for g in (src, out, labels) if g is not None))
    if out is not None:
        exact(out.t, q, what + ": out")
    if out is not src:
        exact(src.t, acc, what + ": acc is read only")
    if labels is not None:
        exact(labels.t, lab, what + ": labels")


@pytest.mark.parametrize("mode", ["alias", "separate", "labels_only", "out_only"])
@pytest.mark.parametrize("row", R.FINALIZE_ROWS, ids=lambda r: r["id"])
def test_sw_finalize(row, mode):
    _finalize(_H(), row, mode)


def test_sw_finalize_above_the_grid_cap():
    _finalize(_H(), R.FINALIZE_OVER_CAP, "alias")


def test_sw_finalize_refusals():
    H = _H()
    acc, one = Guard((257, 8)), torch.ones(8, device="cuda")
    out, labels = Guard((257, 8)), labels_guard((8,))
    with pytest.raises(RuntimeError, match="null pointer"):
        H.call("vx_sw_finalize", acc.ptr, None, None, H.P(one), H.P(one), H.P(one), 2, 1, 1, 8, H.stream_ptr())
    for C, D in ((257, 1), (0, 1), (2, 0)):
        with pytest.raises(RuntimeError, match="bad shape"):
            H.call("vx_sw_finalize", acc.ptr, out.ptr, labels.ptr, H.P(one), H.P(one), H.P(one), C, D, 1, 8, H.stream_ptr())
    for g, fill in ((acc, None), (out, None), (labels, U8_FILL)):
        untouched(g, "refused vx_sw_finalize", fill)


# ====================================================================================================================== vx_argmax_channels
def _argmax(H, row):
    x, _ = R.argmax_case(row)
    logits = dev(x)
    labels = labels_guard((row["B"], row["V"]))
    H.call("vx_argmax_channels", H.P(logits), labels.ptr, row["B"], row["C"], row["V"], H.stream_ptr())
    done(f"vx_argmax_channels {row['id']}", labels)
    exact(labels.t, R.argmax_reference(row), f"vx_argmax_channels {row['id']}")


@pytest.mark.parametrize("row", R.ARGMAX_ROWS, ids=lambda r: r["id"])
def test_argmax_channels(row):
    _argmax(_H(), row)


def test_argmax_channels_above_the_grid_cap():
    _argmax(_H(), R.ARGMAX_OVER_CAP)


def test_argmax_channels_refusals():
    H = _H()
    labels, x = labels_guard((64,)), torch.zeros(64, device="cuda")
    for B, C, V in ((1, 257, 1), (0, 2, 8), (1, 0, 8), (1, 2, 0)):
        with pytest.raises(RuntimeError, match="bad arguments"):
            H.call("vx_argmax_channels", H.P(x), labels.ptr, B, C, V, H.stream_ptr())
    untouched(labels, "refused vx_argmax_channels", U8_FILL)


@pytest.mark.parametrize("row", [r for r in R.ARGMAX_ROWS if r["C"] >= 2], ids=lambda r: r["id"])
def test_to_label_map(row):
    from veloxseg_amd.utils.metric._counts import to_label_map
    x, _ = R.argmax_case(row)
    got = to_label_map(dev(x).view(row["B"], row["C"], 1, 1, row["V"]))
    assert got.dtype == torch.uint8 and tuple(got.shape) == (row["B"], 1, 1, 1, row["V"])
    exact(got, R.argmax_reference(row), f"to_label_map {row['id']}")


# ====================================================================================================================== vx_confusion
def _conf_prefill(row):
    return E.ints(row["B"], row["NC"], row["NC"], seed=R._seed(row["id"]), lo=0, hi=8).long()


@pytest.mark.parametrize("pair", R.CONF_PAIRS, ids=lambda p: f"pred{p[0]}_gt{p[1]}")
@pytest.mark.parametrize("row", R.CONF_ROWS, ids=lambda r: r["id"])
def test_confusion(row, pair):
    H = _H()
    pb, gb = pair
    p, g = R.labels_for(row, pb, 0), R.labels_for(row, gb, 1)
    want = R.confusion(p, g, row["NC"])
    pre = _conf_prefill(row)
    conf = Guard(tuple(pre.shape), torch.int64, fill=pre, canary=I64_CANARY)
    dp, dg = dev(p), dev(g)
    what = f"vx_confusion {row['id']} widths {pair}"
    for calls in (1, 2):                                    # a second call into the same matrix adds
        H.call("vx_confusion", dp.data_ptr(), pb, dg.data_ptr(), gb, conf.ptr, row["B"], row["V"], row["NC"], H.stream_ptr())
        done(what, conf)
        exact(conf.t, pre.numpy() + calls * want, f"{what}, call {calls}")


def test_confusion_refusals():
    H = _H()
    lab = torch.zeros(64, dtype=torch.int64, device="cuda")
    conf = Guard((81,), torch.int64, fill=-7, canary=I64_CANARY)
    for pb, gb in R.CONF_REFUSED_PAIRS:
        with pytest.raises(RuntimeError, match="unsupported label widths"):
            H.call("vx_confusion", lab.data_ptr(), pb, lab.data_ptr(), gb, conf.ptr, 1, 8, 4, H.stream_ptr())
    for NC in (1, 9):
        with pytest.raises(RuntimeError, match="2..8 classes supported"):
            H.call("vx_confusion", lab.data_ptr(), 8, lab.data_ptr(), 8, conf.ptr, 1, 8, NC, H.stream_ptr())
    untouched(conf, "refused vx_confusion", -7)


@pytest.mark.parametrize("gt_bytes", [1, 4, 8])
@pytest.mark.parametrize("pred_bytes", [1, 4, 8])
def test_confusion_wrapper_all_nine_dtype_pairs(pred_bytes, gt_bytes):
    from veloxseg_amd.utils.metric._counts import confusion
    row = next(r for r in R.CONF_ROWS if r["wild"] and r["NC"] == 4 and r["B"] == 3)
    p, g = R.labels_for(row, pred_bytes, 0), R.labels_for(row, gt_bytes, 1)
    got = confusion(dev(p), dev(g), row["NC"])
    assert got.dtype == torch.int64 and not got.is_cuda
    exact(got, R.confusion(p, g, row["NC"]), f"_counts.confusion widths ({pred_bytes}, {gt_bytes})")


# ====================================================================================================================== cal_dice / show_deep_metrics (BraTS)
def _brats_maps(seed, hi, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, hi + 1, (2, 1, 5, 6, 7), generator=g).to(dtype), torch.randint(0, hi + 1, (2, 1, 5, 6, 7), generator=g).to(dtype)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64])
@pytest.mark.parametrize("hi", [3, 4, 5, 200])
def test_cal_dice_follows_the_reference_above_label_three(hi, dtype):
    """a label above 3 is non-zero (WT) but neither ET nor TC; the expected values are the reference's formula restated on the CPU (eval_ref.brats_dice_reference)"""
    from veloxseg_amd.utils.metric import metrics_brats as MB
    out, tgt = _brats_maps(hi, min(hi, 5), dtype)
    if hi == 200:
        out[out == 5], tgt[tgt == 4] = 200, 200
    if hi == 4:                                             # a raw BraTS label map: {0, 1, 2, 4}
        out[out == 3], tgt[tgt == 3] = 4, 4
    want = R.brats_dice_reference(out, tgt)
    got = MB.cal_dice(out.cuda(), tgt.cuda())
    print(f"cal_dice hi={hi} {dtype}: got {got!r} want {want!r}")
    assert got == want


def test_show_deep_metrics_follows_the_reference_above_label_three():
    from veloxseg_amd.utils.metric import metrics_brats as MB
    g = torch.Generator().manual_seed(9)
    logits = [torch.randn(2, 6, 5, 6, 7, generator=g) for _ in range(2)]
    labels = torch.randint(0, 6, (2, 1, 5, 6, 7), generator=g)
    want_res, want = None, ""
    for o in logits:
        am = o.argmax(dim=1, keepdim=True)
        avg, et, tc, wt = R.brats_dice_reference(labels, am)
        want += f"[Avg:{avg:.4f}, ET:{et:.4f}, TC:{tc:.4f}, WT:{wt:.4f} pix:{int((am != 0).sum()):6}/{int((labels != 0).sum()):6}]\n"
        want_res = want_res or [avg, et, tc, wt]
    res, string = MB.show_deep_metrics([o.cuda() for o in logits], labels.cuda(), True)
    print(f"show_deep_metrics: got {res!r} want {want_res!r}")
    assert string == want + "\n" and res == want_res


# ====================================================================================================================== vx_min_value / vx_bbox_gt
def _bits(x):
    return int(np.array(x, dtype=np.float32).view(np.int32))


def _min(H, x, preset=float("inf")):
    d = dev(x)
    out = Guard((1,), fill=preset)
    H.call("vx_min_value", H.P(d), x.size, out.ptr, H.stream_ptr())
    done(f"vx_min_value n={x.size}", out)
    exact(d, x, "vx_min_value: the data itself")
    return int(out.t.view(torch.int32).item())


@pytest.mark.parametrize("n", R.MIN_N)
def test_min_value(n):
    H = _H()
    base = R.ints(n, seed=n % 1009)
    for at in sorted({0, n - 1, min(63, n - 1), min(64, n - 1), min(n - 1, 2048 * 256 + 63)}):      # first, last, either side of a wave boundary, past one sweep of the grid
        for low in (-7.5, -0.0 if n == 1 else -3.5):
            x = base.copy()
            x[at] = low
            assert _min(H, x) == _bits(R.min_value(x)), (n, at, low)                                  # the exact bits
    x = base.copy()
    assert _min(H, x, preset=-100.0) == _bits(-100.0)                                                 # a preset below the data stays
    x[n // 2] = np.inf
    assert _min(H, x) == _bits(R.min_value(x))
    x[n - 1] = -np.inf
    assert _min(H, x) == _bits(-np.inf)
    x = base.copy()
    x[::3] = np.nan                                                                                   # NaN voxels are ignored (the first and, for n % 3 == 1, the last among them)
    assert _min(H, x) == _bits(R.min_value(x))
    assert _min(H, np.full(n, np.nan, dtype=np.float32)) == _bits(np.inf)


PRESET = [R.INT_MAX] * 3 + [-1] * 3


def _box(H, x, thr, preset=PRESET):
    d = dev(x)
    out = Guard((6,), torch.int32, fill=torch.tensor(preset, dtype=torch.int32), canary=I32_CANARY)
    H.call("vx_bbox_gt", H.P(d), float(thr), *x.shape, out.ptr, H.stream_ptr())
    done(f"vx_bbox_gt {x.shape}", out)
    return out.t.tolist()


@pytest.mark.parametrize("shape", R.BOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bbox_gt(shape):
    H = _H()
    C, D, Hh, W = shape
    zero = np.zeros(shape, dtype=np.float32)
    for d in {0, D - 1}:
        for h in {0, Hh - 1}:
            for w in {0, W - 1}:                            # a single voxel at each corner, in the last channel only
                x = zero.copy()
                x[C - 1, d, h, w] = 1.0
                assert _box(H, x, 0.0) == [d, h, w, d, h, w] == R.bbox_gt(x, 0.0)
    x = zero.copy()
    x.reshape(-1)[-1] = 2.0                                 # the last flat element alone
    assert _box(H, x, 0.0) == [D - 1, Hh - 1, W - 1] * 2
    assert _box(H, x, 2.0) == PRESET                        # thr = the maximum: the box is empty and the presets are untouched
    x = R.ints(*shape, seed=sum(shape))
    assert _box(H, x, R.min_value(x)) == R.bbox_gt(x, R.min_value(x))
    assert _box(H, x, 2.0) == R.bbox_gt(x, 2.0)
    x[x > 2] = np.nan                                       # NaN voxels are ignored
    assert _box(H, x, 1.0) == R.bbox_gt(x, 1.0)
    assert _box(H, np.full(shape, np.nan, dtype=np.float32), -1.0) == PRESET
    inner = [D // 2, Hh // 2, W // 2] * 2                   # a preset that is already a box is merged with, not overwritten
    assert _box(H, x, 1.0, preset=inner) == R.bbox_gt(x, 1.0, preset=inner)


@pytest.mark.parametrize("shape", R.BOX_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_foreground_box_wrapper(shape):
    from oracle import augment_oracle as AO
    from veloxseg_amd.utils.augment import foreground_box
    x = R.ints(*shape, seed=sum(shape) + 1)
    x[:, :1], x[:, :, -1:] = -3.0, -3.0                     # a margin of the minimum
    assert foreground_box(dev(x)) == AO.bounding_box(x)
    y = x.copy()
    y.reshape(-1)[::5] = np.nan
    b = R.bbox_gt(y, R.min_value(y))
    assert foreground_box(dev(y)) == ((b[:3], [v + 1 for v in b[3:]]) if b[3] >= 0 else ([0, 0, 0], [0, 0, 0]))
    assert foreground_box(dev(np.full(shape, 2.0, dtype=np.float32))) == ([0, 0, 0], [0, 0, 0])


# ====================================================================================================================== vx_label_chunk_count / vx_label_kth_in_chunk
@pytest.mark.parametrize("fg", [1, 0])
@pytest.mark.parametrize("n", R.LABEL_N)
@pytest.mark.parametrize("chunk", R.CHUNKS)
@pytest.mark.parametrize("code", R.LABEL_CODES)
def test_label_chunk_count_and_kth(code, chunk, n, fg):
    H = _H()
    lab = R.labels(code, n, fg)
    d = dev(lab)
    what = f"labels code {code} chunk {chunk} n {n} fg {fg}"
    nb = -(-n // chunk)
    counts = Guard((nb,), torch.int32, fill=-7, canary=I32_CANARY)
    H.call("vx_label_chunk_count", d.data_ptr(), code, n, chunk, fg, counts.ptr, H.stream_ptr())
    done(what, counts)
    exact(counts.t, R.chunk_count(lab, chunk, fg), what + ": counts")
    queries = R.kth_queries(lab, chunk, fg)
    out = Guard((len(queries),), torch.int64, fill=-1, canary=I64_CANARY)
    for i, (c0, k, _) in enumerate(queries):
        H.call("vx_label_kth_in_chunk", d.data_ptr(), code, n, c0, chunk, fg, k, out.ptr + 8 * i, H.stream_ptr())
    done(what, out)
    exact(out.t, np.array([-1 if w is None else w for _, _, w in queries], dtype=np.int64), what + ": k-th match (-1: k is beyond the matches, nothing written)")


@pytest.mark.parametrize("code", R.LABEL_CODES)
def test_label_chunks_without_any_match(code):
    H = _H()
    n = 1000
    for fg, value in ((1, 0), (0, 1)):
        d = torch.full((n,), value, device="cuda", dtype=torch.from_numpy(np.zeros(1, R.NP_LABEL_CODE[code])).dtype)
        counts = Guard((4,), torch.int32, fill=-7, canary=I32_CANARY)
        out = Guard((1,), torch.int64, fill=-1, canary=I64_CANARY)
        H.call("vx_label_chunk_count", d.data_ptr(), code, n, 256, fg, counts.ptr, H.stream_ptr())
        H.call("vx_label_kth_in_chunk", d.data_ptr(), code, n, 768, 256, fg, 0, out.ptr, H.stream_ptr())
        done("no match", counts, out)
        assert counts.t.tolist() == [0, 0, 0, 0] and out.t.item() == -1
        H.call("vx_label_chunk_count", d.data_ptr(), code, n, 256, 1 - fg, counts.ptr, H.stream_ptr())
        H.call("vx_label_kth_in_chunk", d.data_ptr(), code, n, 768, 256, 1 - fg, n - 768 - 1, out.ptr, H.stream_ptr())
        done("every voxel matches", counts, out)
        assert counts.t.tolist() == [256, 256, 256, n - 768] and out.t.item() == n - 1


def test_label_refusals():
    H = _H()
    d = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    counts = Guard((8,), torch.int32, fill=-7, canary=I32_CANARY)
    out = Guard((1,), torch.int64, fill=-1, canary=I64_CANARY)
    with pytest.raises(RuntimeError, match="bad args"):
        H.call("vx_label_chunk_count", d.data_ptr(), 1, 1024, 255, 1, counts.ptr, H.stream_ptr())
    with pytest.raises(RuntimeError, match="not supported"):
        H.call("vx_label_chunk_count", d.data_ptr(), 2, 1024, 256, 1, counts.ptr, H.stream_ptr())
    for chunk, c0, k, code, msg in ((255, 0, 0, 1, "bad args"), (256, 1024, 0, 1, "bad args"), (256, 0, -1, 1, "bad args"), (256, 0, 0, 2, "not supported")):
        with pytest.raises(RuntimeError, match=msg):
            H.call("vx_label_kth_in_chunk", d.data_ptr(), code, 1024, c0, chunk, 0, k, out.ptr, H.stream_ptr())
    untouched(counts, "refused vx_label_chunk_count", -7)
    untouched(out, "refused vx_label_kth_in_chunk", -1)


# ====================================================================================================================== vx_rotate_z
@pytest.mark.parametrize("mode", [0, 1], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("row", R.ROT_ROWS, ids=lambda r: r["id"])
def test_rotate_z(row, mode):
    H = _H()
    x = R.rotate_input(row)
    d = dev(x)
    out = Guard(x.shape)
    H.call("vx_rotate_z", H.P(d), out.ptr, *x.shape, row["cs"], row["sn"], mode, H.stream_ptr())
    what = f"vx_rotate_z {row['id']} mode {mode}"
    done(what, out)
    exact(out.t, R.rotate_exact(x, row["cs"], row["sn"], mode), what)
    if (row["cs"], row["sn"]) == (1.0, 0.0):
        exact(out.t, x, what + ": the identity")
    exact(d, x, what + ": the input itself")


def test_rotate_z_refusals():
    H = _H()
    out = Guard((2, 3, 4, 5))
    x = torch.zeros(2, 3, 4, 5, device="cuda")
    with pytest.raises(RuntimeError, match="bad args"):
        H.call("vx_rotate_z", out.ptr, out.ptr, 2, 3, 4, 5, 1.0, 0.0, 0, H.stream_ptr())
    for mode in (2, -1):
        with pytest.raises(RuntimeError, match="bad args"):
            H.call("vx_rotate_z", H.P(x), out.ptr, 2, 3, 4, 5, 1.0, 0.0, mode, H.stream_ptr())
    with pytest.raises(RuntimeError, match="bad args"):
        H.call("vx_rotate_z", H.P(x), out.ptr, 2, 0, 4, 5, 1.0, 0.0, 0, H.stream_ptr())
    untouched(out, "refused vx_rotate_z")
