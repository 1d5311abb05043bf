"""GPU: vx_elastic_noise, vx_elastic_smooth and vx_elastic_batch (csrc/augment_elastic.hip) through utils.augment.elastic_field / elastic_sample / Rand3DElasticd
against tests/elastic_ref.py.

The noise is exact in fp32 and compared with `==`.  The smoothing is compared with `==` on dyadic weights and integer data (exact in fp32 with or without fused
multiply-adds) and held to a summation-length bound on erf weights.  The resampler is compared with `==` on the exact rows (integer data, dyadic matrices, fields
that are multiples of 1/4; tests/test_elastic_cpu.py proves the premise of every row), byte for byte against vx_affine_batch where there is no displacement, and held
to a derived bound off the dyadic rows.  Outputs are NaN- or sentinel-prefilled and sit between canaries; a record the kernel must skip leaves its prefill."""
import math
import types

import numpy as np
import pytest
import torch

import affine_ref as R
import elastic_ref as E
import eval_ref as ER
from exact_ref import Guard
from test_affine_gpu import MODES, PADS, dev, done, exact, guard, untouched

pytestmark = pytest.mark.gpu


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def _H():
    from veloxseg_amd import _hip as H
    return H


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def spy(monkeypatch):
    """the names of the C entries called from here on"""
    H = _H()
    calls, real = [], H.call
    monkeypatch.setattr(H, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    return calls


# ====================================================================================================================== 1. vx_elastic_batch: exact rows
@pytest.mark.parametrize("row", E.EXACT_ROWS, ids=lambda r: r["id"])
def test_exact_rows(row):
    """both modes x both paddings on the image, nearest x both paddings on the four label types, cval 7, one field shared by all: ONE call of twelve records, every
    output `==` its oracle"""
    A = _A()
    m, f = R.row_matrix(row), dev(E.field(row))
    entries, outs, wants = [], [], []
    x = dev(R.image(row))
    for mode in (0, 1):
        for pad in (0, 1):
            entries.append((x, m, MODES[mode], PADS[pad], E.CVAL, f, row["m"]))
            outs.append(guard(row["out"], 0))
            wants.append(E.reference(row, mode, pad))
    for code in (1, 4, 8, -4):
        lab = dev(R.label(row, code))
        for pad in (0, 1):
            entries.append((lab, m, "nearest", PADS[pad], E.CVAL, f, row["m"]))
            outs.append(guard(row["out"], code))
            wants.append(E.reference(row, 1, pad, code))
    A.elastic_sample(entries, row["out"], out=[g.t for g in outs])
    done(row["id"], *outs)
    for i, (g, w) in enumerate(zip(outs, wants)):
        exact(g.t, w, f"{row['id']} record {i} ({entries[i][2]}, {entries[i][3]}, {entries[i][0].dtype})")
    exact(x, R.image(row), "the input itself")
    exact(f, E.field(row), "the field itself")


# ====================================================================================================================== 2. no displacement: vx_affine_batch's bytes
@pytest.mark.parametrize("name", ["rot3", "big", "permute"])
def test_without_a_displacement_the_bytes_are_those_of_affine_sample(name):
    """GPU against GPU: the entries with field None, and with a zero field under magnitude 2, against affine_sample on the same entries"""
    A = _A()
    row = next(r for r in E.EXACT_ROWS if r["matrix"] == name and r["out"] == (9, 7, 5) and r["n"] == (8, 8, 8))
    m = R.row_matrix(row)
    m[:, 3] = (0.5, -0.25, 0.75)
    srcs = [dev(R.image(row))] + [dev(R.label(row, code)) for code in (1, 4, 8, -4)]
    aff = [(srcs[0], m, MODES[mode], PADS[pad], E.CVAL) for mode in (0, 1) for pad in (0, 1)] + [(s, m, "nearest", PADS[pad], E.CVAL) for s in srcs[1:] for pad in (0, 1)]
    want = A.affine_sample(aff, row["out"])
    zero = torch.zeros((3,) + row["out"], device="cuda")
    none = A.elastic_sample([e + (None, 1.0) for e in aff], row["out"])
    zeroed = A.elastic_sample([e + (zero, 2.0) for e in aff], row["out"])
    torch.cuda.synchronize()
    for i, (w, a, b) in enumerate(zip(want, none, zeroed)):
        assert same_bytes(w, a), f"record {i}: field None differs from affine_sample"
        assert same_bytes(w, b), f"record {i}: a zero field differs from affine_sample"


# ====================================================================================================================== 3. many records, shared fields
def test_many_records_in_one_call_equal_one_call_each():
    """3 samples x 3 keys (two fp32 images, one label) of mixed matrices, fields, magnitudes, modes, paddings and element types; the three keys of a sample share ONE
    field, the third sample has none: one call against one call per record, on bytes, and each `==` the oracle"""
    A = _A()
    out_size, entries = (7, 9, 10), []
    specs = [("rot3", "bilinear", "border", torch.uint8, 1.0), ("big", "bilinear", "constant", torch.int64, 0.5), ("shear", "nearest", "constant", torch.int32, 2.0)]
    fields = [dev(E._field(out_size, 100 + s)) for s in range(2)] + [None]
    for s, (name, mode, pad, lab_dtype, mag) in enumerate(specs):
        m = R.row_matrix(dict(matrix=name))
        m[:, 3] = (0.5 * s, -0.25, 0.75)
        n = (8 + s, 9, 11 - s)
        for k in range(2):
            entries.append((dev(ER.ints(*n, seed=10 * s + k, lo=-64, hi=64)), m, mode, pad, 3.0, fields[s], mag))
        entries.append((dev(ER.ints(*n, seed=10 * s + 2, lo=0, hi=64)).to(lab_dtype), m, "nearest", pad, 3.0, fields[s], mag))
    assert entries[0][5] is entries[1][5] is entries[2][5] and entries[3][5] is not entries[0][5]
    together = A.elastic_sample(entries, out_size)
    alone = [A.elastic_sample([e], out_size)[0] for e in entries]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(together, alone)):
        e = entries[i]
        assert a.dtype == e[0].dtype and tuple(a.shape) == out_size and same_bytes(a, b), f"record {i}"
        Ar, c = R.record_values(e[1], tuple(e[0].shape))
        f = None if e[5] is None else e[5].cpu().numpy()
        exact(a, E.sample(e[0].cpu().numpy(), Ar, c, out_size, 0 if e[2] == "bilinear" else 1, 0 if e[3] == "border" else 1, 3.0, f, e[6]), f"record {i}")


# ====================================================================================================================== 4. views and context
@pytest.mark.parametrize("matrix", ["rot3", "big"])
def test_views_and_context(matrix):
    """a crop view at an odd origin inside a (12, 11, 13) parent that is itself a strided view, with window bounds and with context bounds: each `==` its oracle"""
    A = _A()
    parent_np = ER.ints(12, 11, 13, seed=R._seed(matrix), lo=-64, hi=64)
    wide = torch.full((12, 11, 26), 999.0, device="cuda")
    wide[:, :, ::2] = dev(parent_np)
    start, n = (3, 1, 5), (6, 7, 5)
    view = wide[:, :, ::2][3:9, 1:8, 5:10]
    assert not view.is_contiguous()
    crop_np = parent_np[3:9, 1:8, 5:10]
    m = R.row_matrix(dict(matrix=matrix))
    Ar, c = R.record_values(m, n)
    f_np, mag = E._field(n, 5), 0.5
    f = dev(f_np)
    lo, hi = [-s for s in start], [p - 1 - s for p, s in zip(parent_np.shape, start)]
    differs = 0
    for mode in (0, 1):
        for pad in (0, 1):
            win, ctx = Guard(n), Guard(n)
            A.elastic_sample([(view, m, MODES[mode], PADS[pad], E.CVAL, f, mag), (view, m, MODES[mode], PADS[pad], E.CVAL, f, mag, (lo, hi))], n, out=[win.t, ctx.t])
            done(f"{matrix} {mode} {pad}", win, ctx)
            want_win = E.sample(crop_np, Ar, c, n, mode, pad, E.CVAL, f_np, mag)
            want_ctx = E.sample(parent_np, Ar, c, n, mode, pad, E.CVAL, f_np, mag, lo=lo, hi=hi, origin=start)
            exact(win.t, want_win, f"{matrix} mode {mode} pad {pad}: window bounds")
            exact(ctx.t, want_ctx, f"{matrix} mode {mode} pad {pad}: context bounds")
            differs += int(not np.array_equal(want_win, want_ctx))
    assert differs > 0, "the row does not show the difference between window and context bounds"
    assert bool((wide[:, :, 1::2] == 999.0).all())


# ====================================================================================================================== 5. non-finite data
@pytest.mark.parametrize("pad", [0, 1], ids=PADS)
def test_nan_and_inf_appear_where_the_oracle_has_them(pad):
    A = _A()
    row = next(r for r in E.EXACT_ROWS if r["id"] == "rot3_9x7x5_from_9x7x5")
    x = np.array(R.image(row), copy=True)
    x[4, 3, 2], x[1, 2, 2], x[2, 0, 0] = np.nan, np.inf, -np.inf
    m = R.row_matrix(row)
    Ar, c = R.record_values(m, row["n"])
    outs = [Guard(row["out"]), Guard(row["out"])]
    A.elastic_sample([(dev(x), m, MODES[mode], PADS[pad], E.CVAL, dev(E.field(row)), row["m"]) for mode in (0, 1)], row["out"], out=[g.t for g in outs])
    done("non-finite", *outs)
    for mode in (0, 1):
        want = E.sample(x, Ar, c, row["out"], mode, pad, E.CVAL, E.field(row), row["m"])
        assert np.isnan(want).any() and np.isinf(want).any()
        exact(outs[mode].t, want, f"non-finite mode {mode} pad {pad}")


# ====================================================================================================================== 6. records the kernel must skip, refusals
def test_skipped_records_and_refusals_leave_the_prefill_untouched():
    A, H = _A(), _H()
    x = dev(ER.ints(4, 5, 6, seed=1))
    lab = x.to(torch.int32)
    eye = A.affine_matrix()
    f = torch.zeros(3, 4, 5, 6, device="cuda")
    out, iout = guard((4, 5, 6), 0), guard((4, 5, 6), 4)
    ok = (x, eye, "bilinear", "border", 0.0)
    # the Python layer: affine_sample's checks reach elastic_sample unchanged, and the field's own
    for entry, exc, msg, o in ((ok[:2] + ("cubic",) + ok[3:] + (f, 1.0), ValueError, "mode", out), ((lab,) + ok[1:] + (f, 1.0), TypeError, "nearest only", iout),
                               (ok + (f, 1.0, ([0, 3, 0], [3, 2, 5])), ValueError, "lo .* > hi", out), (ok + (f, 1.0, ([0, 0, -1], [3, 4, 5])), ValueError, "reach outside", out),
                               ((out.t,) + ok[1:] + (f, 1.0), ValueError, "alias", out), (ok + (out.t.new_zeros(3, 4, 5, 6)[:, :, :, :5], 1.0), ValueError, "contiguous", out),
                               (ok + (f.cpu(), 1.0), RuntimeError, "no CPU fallback", out), (ok + (f, float("nan")), ValueError, "not finite", out)):
        with pytest.raises(exc, match=msg):
            A.elastic_sample([entry], (4, 5, 6), out=[o.t])
    both = Guard((4, 4, 5, 6))                                               # a destination inside the field's memory
    with pytest.raises(ValueError, match="field and destination alias"):
        A.elastic_sample([ok + (both.t[:3], 1.0)], (4, 5, 6), out=[both.t[2]])
    with pytest.raises(ValueError, match="field and destination alias"):     # ... also the field of ANOTHER record
        A.elastic_sample([ok + (None, 1.0), ok + (both.t[:3], 1.0)], (4, 5, 6), out=[both.t[0], both.t[3]])
    with pytest.raises(ValueError, match="`out`"):
        A.elastic_field((4, 5, 6), [1], [5.0], out=out.t)
    # the C entries: what they can see
    table = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    for name, args, msg in (("vx_elastic_batch", (None, 1, 4, 5, 6), "null pointer"), ("vx_elastic_batch", (table.data_ptr(), 0, 4, 5, 6), "no records"),
                            ("vx_elastic_batch", (table.data_ptr(), 1, 4, 5, -6), "non-positive output extent"), ("vx_elastic_noise", (table.data_ptr(), 0, 120, out.ptr), "no planes"),
                            ("vx_elastic_noise", (table.data_ptr(), 1, 0, out.ptr), "non-positive plane size"), ("vx_elastic_noise", (None, 1, 120, out.ptr), "null pointer"),
                            ("vx_elastic_smooth", (table.data_ptr(), 1, out.ptr, out.ptr, 4, 5, 6), "overlap"), ("vx_elastic_smooth", (table.data_ptr(), 1, out.ptr, None, 4, 5, 6), "null pointer"),
                            ("vx_elastic_smooth", (table.data_ptr(), 0, out.ptr, both.ptr, 4, 5, 6), "no planes"), ("vx_elastic_smooth", (table.data_ptr(), 1, out.ptr, both.ptr, 4, 0, 6), "non-positive extent")):
        with pytest.raises(RuntimeError, match=msg):
            H.call(name, *args, H.stream_ptr())
    # records that name a destination but should not have been sent write nothing: unknown mode, unknown type, unknown pad, trilinear on int32, lo > hi, a null source
    tab = np.zeros(6, dtype=A._ELA)
    aff = tab["aff"]                                                         # (a view: the first 144 bytes of every record)
    aff["src"], aff["dst"], aff["stride"], aff["n"], aff["hi"], aff["A"] = x.data_ptr(), [g.ptr for g in (out, out, out, iout, out, out)], (30, 6, 1), (4, 5, 6), (3, 4, 5), np.eye(3).reshape(-1)
    tab["field"], tab["m"] = f.data_ptr(), 1.0
    aff["mode"][0], aff["dtype"][1], aff["pad"][2], aff["dtype"][3], aff["lo"][4], aff["src"][5] = 2, 3, 2, 4, (0, 5, 0), 0
    aff["src"][3] = lab.data_ptr()
    assert tab.view(np.uint8).reshape(6, -1)[0, 80] == 2 and int(tab.view(np.uint8).reshape(6, -1)[1, 144:152].view("<u8")[0]) == f.data_ptr()
    H.call("vx_elastic_batch", torch.from_numpy(tab.view(np.uint8).reshape(-1)).cuda().data_ptr(), 6, 4, 5, 6, H.stream_ptr())
    # a weight record whose tail is out of range writes nothing either
    wt = np.zeros(1, dtype=A._ELW)
    wt["tail"], wt["w"][0, 0] = A.ELASTIC_MAX_TAIL + 1, 1.0
    H.call("vx_elastic_smooth", torch.from_numpy(wt.view(np.uint8).reshape(-1)).cuda().data_ptr(), 1, x.data_ptr(), out.ptr, 4, 5, 6, H.stream_ptr())
    untouched(out, 0, "refused calls / skipped records")
    untouched(iout, 4, "refused calls / skipped records")
    both.check("refused calls")
    assert bool((both.t != both.t).all()) and not f.any()


# ====================================================================================================================== 7. vx_elastic_batch off the dyadic rows
def test_off_dyadic_rows():
    """24^3, three random angles at once, scale 0.8 .. 1.2 (affine_ref's case), a DEVICE-made field (sigma 5) whose magnitude gives displacements of up to 3 voxels.
    The record (A, c in fp32), the fp32 field and the fp32 magnitude are the inputs of both the kernel and the fp64 oracle, so the bound covers the kernel's arithmetic
    alone: section 28.4's bound with the coordinate term extended by the displacement, eps = gamma(5) max_a (sum_i |A[a][i]| |p'_i|max + |c_a|)
    (elastic_ref.coord_bound), trilinear within 3 eps G + gamma(9) max|x|; nearest `==` outside eps of a .5 tie, at most 1 % of the voxels left out (the seed is
    checked against that cap on the CPU restatement of the field in tests/test_elastic_cpu.py, and here on the device's field).
    Measured on an MI355X (printed below): DESIGN.md section 37."""
    A = _A()
    x, m = R.off_dyadic_case(E.OFF_SEED)
    Ar, c = R.record_values(m, E.OFF_N)
    field = A.elastic_field(E.OFF_N, [E.OFF_FIELD_SEED], [E.OFF_SIGMA])[0]
    f = field.cpu().numpy()
    mag = E.off_magnitude(f)
    eps = E.coord_bound(Ar, c, E.OFF_N, f, mag)
    vmax, cval = float(np.abs(x).max()), 2.0
    d = dev(x)
    outs = {(mode, pad): Guard(E.OFF_N) for mode in (0, 1) for pad in (0, 1)}
    A.elastic_sample([(d, m, MODES[mode], PADS[pad], cval, field, mag) for mode, pad in outs], E.OFF_N, out=[g.t for g in outs.values()])
    done("off-dyadic", *outs.values())
    print(f"off-dyadic: magnitude {mag:.2f}, largest displacement {mag * float(np.abs(f).max()):.3f} voxels, eps {eps:.3e}")
    hi = [v - 1 for v in E.OFF_N]
    for pad in (0, 1):
        G = R.neighbour_difference(x, cval if pad else None)
        bound = 3 * eps * G + R.gamma(9) * vmax
        got = outs[0, pad].t.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - E.sample(x, Ar, c, E.OFF_N, 0, pad, cval, f, mag)).max())
        print(f"off-dyadic trilinear {PADS[pad]}: max |error| {err:.3e}, bound {bound:.3e} (eps {eps:.3e}, G {G:.3f}, max|x| {vmax:.2f})")
        assert err <= bound, f"trilinear {PADS[pad]}: max |error| {err:.3e} above the derived bound {bound:.3e}"
        skip = E.near_tie(Ar, c, E.OFF_N, f, mag, [0, 0, 0], hi, pad, eps)
        assert float(skip.mean()) <= 0.01
        got, want = outs[1, pad].t.cpu().numpy(), E.sample(x, Ar, c, E.OFF_N, 1, pad, cval, f, mag)
        bad = (got != want) & ~skip
        print(f"off-dyadic nearest {PADS[pad]}: {int(skip.sum())} of {skip.size} voxels left out, {int(bad.sum())} differ")
        assert not bad.any(), f"nearest {PADS[pad]}: {int(bad.sum())} voxels differ away from ties"
    assert float(np.abs(outs[0, 0].t.cpu().numpy() - R.sample(x, Ar, c, E.OFF_N, 0, 0, cval)).max()) > 0.1          # the field moved the patch


# ====================================================================================================================== 8. vx_elastic_noise
def raw_noise(keys, n_planes, V, shift=0):
    H = _H()
    table = torch.from_numpy(np.array(keys, dtype=np.uint64).view(np.int64)).cuda()
    g = Guard((n_planes, V), shift=shift)
    H.call("vx_elastic_noise", table.data_ptr(), n_planes, V, g.ptr, H.stream_ptr())
    done(f"noise V {V}", g)
    return g.t


@pytest.mark.parametrize("V", [1, 3, 4, 5, 257, 4099])
def test_noise_equals_the_restatement(V):
    """two fields with different keys in ONE call, `==` the restatement: Philox quads straddle the plane boundaries wherever V is no multiple of 4, and the last quad
    of a field is ragged; a third field with the first key again gives the first field's bits; a call that ends inside a field fills the planes it was asked for"""
    keys = [0x0123456789ABCDEF, 7, 0x0123456789ABCDEF]
    got = raw_noise(keys, 9, V)
    exact(got, E.noise_planes(keys, 9, V), f"noise V {V}")
    assert torch.equal(got[:3], got[6:]) and not torch.equal(got[:3], got[3:6])
    exact(raw_noise(keys, 4, V), E.noise_planes(keys, 4, V), f"noise V {V}, four planes")
    exact(raw_noise(keys, 9, V, shift=1), E.noise_planes(keys, 9, V), f"noise V {V}, output 4 bytes off a 16-byte boundary")
    assert float(got.min()) >= -1.0 and float(got.max()) < 1.0


# ====================================================================================================================== 9. vx_elastic_smooth
def raw_smooth(x, halves):
    """x: (n_planes, D, H, W) fp32 numpy, halves: one half weight vector per FIELD -> the smoothed planes (device), between canaries; the source planes are scratch"""
    A, H = _A(), _H()
    wt = np.zeros(len(halves), dtype=A._ELW)
    for r, h in zip(wt, halves):
        r["tail"], r["w"][:len(h)] = len(h) - 1, h
    table = torch.from_numpy(wt.view(np.uint8).reshape(-1)).cuda()
    src, g = Guard(x.shape, fill=torch.from_numpy(np.array(x, copy=True))), Guard(x.shape)
    H.call("vx_elastic_smooth", table.data_ptr(), x.shape[0], src.ptr, g.ptr, *x.shape[1:], H.stream_ptr())
    done(f"smooth {x.shape}", src, g)
    return g.t


def raw_passes(x, halves):
    """the three passes one by one through vx_elastic_smooth_pass (W, H, D) -> the smoothed planes"""
    A, H = _A(), _H()
    wt = np.zeros(len(halves), dtype=A._ELW)
    for r, h in zip(wt, halves):
        r["tail"], r["w"][:len(h)] = len(h) - 1, h
    table = torch.from_numpy(wt.view(np.uint8).reshape(-1)).cuda()
    a, b = Guard(x.shape, fill=torch.from_numpy(np.array(x, copy=True))), Guard(x.shape)
    for axis, (src, dst) in zip((2, 1, 0), ((a, b), (b, a), (a, b))):
        H.call("vx_elastic_smooth_pass", table.data_ptr(), x.shape[0], src.ptr, dst.ptr, axis, *x.shape[1:], H.stream_ptr())
    done(f"passes {x.shape}", a, b)
    return b.t


def smooth_shapes():
    A = _A()
    return E.smooth_shapes(A.ELASTIC_ROWS, A.ELASTIC_TILE_W, A.ELASTIC_STRIP, A.ELASTIC_TILE_LINE)


@pytest.mark.parametrize("case", range(5))
def test_smooth_is_exact_on_dyadic_weights(case):
    """tails 0, 1, 16, 17 and 48 as five fields (fifteen planes) of ONE call, `==` the fp64 restatement, and byte for byte what one call per field gives.  Shapes: one
    voxel; shorter than the tail (5 against 17 and 48); one row past a W-pass block and one output past its chunk; one output past the H / D pass's tile along the axis
    and one column past its strip (the widths come from the constants the module exports).  Zero padding: the data is non-zero up to both ends of every axis."""
    A = _A()
    shape = smooth_shapes()[case]
    tails = E.SMOOTH_TAILS
    halves = [E.dyadic_half(t, 10 * case + i) for i, t in enumerate(tails)]
    x = E.dyadic_data(shape, 15, 100 * case)
    got = raw_smooth(x, halves)
    assert same_bytes(got, raw_passes(x, halves)), f"shape {shape}: vx_elastic_smooth_pass x 3 differs from vx_elastic_smooth"
    for i, h in enumerate(halves):
        alone = raw_smooth(x[3 * i:3 * i + 3], [h])
        assert same_bytes(got[3 * i:3 * i + 3], alone), f"shape {shape}, tail {tails[i]}: one call for five fields differs from a call of its own"
        for j in range(3):
            exact(got[3 * i + j], E.smooth64(x[3 * i + j], h), f"shape {shape}, tail {tails[i]}, plane {j}")


@pytest.mark.parametrize("sigma", [5.0, 13.0])
def test_smooth_erf_weights_within_the_summation_bound(sigma):
    """erf weights on standard normal data, 20 x 18 x 22: |got - fp64| <= 4 (tail + 3) 2^-24 times the fp64 smoothing of |x| (elastic_ref.smooth_bound: a pass is a
    (tail + 2)-rounding dot product plus the pair add, three passes, weights that sum to at most 1)"""
    A = _A()
    h = A.elastic_weights(sigma)
    x = np.random.RandomState(int(sigma)).standard_normal((3, 20, 18, 22)).astype(np.float32)
    got = raw_smooth(x, [h]).cpu().numpy().astype(np.float64)
    worst = 0.0
    for j in range(3):
        worst = max(worst, float((np.abs(got[j] - E.smooth64(x[j], h)) / E.smooth_bound(x[j], h)).max()))
    print(f"erf smoothing sigma {sigma} (tail {h.size - 1}): largest |error| / bound {worst:.3f}")
    assert worst <= 1.0


def test_elastic_field(monkeypatch):
    A = _A()
    calls = spy(monkeypatch)
    shape, seeds, sigmas = (9, 6, 11), [5, 2 ** 40 + 1, 5], [1.5, 5.0, 1.5]
    f = A.elastic_field(shape, seeds, sigmas)
    assert calls == ["vx_elastic_noise", "vx_elastic_smooth"] and f.shape == (3, 3) + shape and f.dtype == torch.float32 and f.is_cuda
    assert torch.equal(f[0], f[2]) and not torch.equal(f[0], f[1])          # the same seed and sigma: the same bits
    g = Guard((3, 3) + shape)
    assert A.elastic_field(shape, seeds, sigmas, out=g.t) is g.t
    done("elastic_field", g)
    assert torch.equal(g.t, f)
    got = f.cpu().numpy().astype(np.float64)
    V = int(np.prod(shape))
    for i, (s, sg) in enumerate(zip(seeds, sigmas)):
        h = A.elastic_weights(sg)
        for j, plane in enumerate(E.noise_planes([s], 3, V)):
            ref, bound = E.smooth64(plane.reshape(shape), h), E.smooth_bound(plane.reshape(shape), h)
            assert bool((np.abs(got[i, j] - ref) <= bound).all()), f"field {i} plane {j}"


# ====================================================================================================================== 10. Rand3DElasticd
def _sample(seed, shape=(10, 9, 8), lab_dtype=torch.uint8):
    return {"a": dev(ER.ints(2, *shape, seed=seed, lo=-64, hi=64)), "seg": dev(ER.ints(1, *shape, seed=seed + 1, lo=0, hi=3)).to(lab_dtype), "name": f"case{seed}"}


def test_rand_3d_elasticd(monkeypatch):
    A = _A()
    kw = dict(rotate_range=(0.4, 0.3, 0.2), scale_range=(0.1, 0.1, 0.2), translate_range=(1.0, 2.0, 0.5), mode=("bilinear", "nearest"))
    samples = [_sample(40 + 2 * i) for i in range(4)]
    calls = spy(monkeypatch)
    t = A.Rand3DElasticd(["a", "seg"], (1.0, 2.0), (20.0, 40.0), prob=1.0, padding_mode="constant", cval=1.0, **kw).set_random_state(5)
    four = t(samples)
    assert calls == ["vx_elastic_noise", "vx_elastic_smooth", "vx_elastic_batch"], f"a list of four samples made the calls {calls}"
    want = E.draws(5, 1.0, (1.0, 2.0), (20.0, 40.0), kw["rotate_range"], kw["scale_range"], kw["translate_range"], 4)
    assert t.last_draws == [tuple(w) for w in want] and len({w[0] for w in want}) == 4
    # the outputs are elastic_sample on elastic_field, rebuilt from the recorded draws
    shape = (10, 9, 8)
    fields = A.elastic_field(shape, [w[0] for w in want], [w[2] for w in want])
    entries = []
    for d, f, w in zip(samples, fields, want):
        m = A.affine_matrix(w[3], w[5], w[4])
        entries += [(d["a"][0], m, "bilinear", "constant", 1.0, f, w[1]), (d["a"][1], m, "bilinear", "constant", 1.0, f, w[1]), (d["seg"][0], m, "nearest", "constant", 1.0, f, w[1])]
    rebuilt = A.elastic_sample(entries, shape)
    for i, (d, o) in enumerate(zip(samples, four)):
        assert o is not d and o["name"] == d["name"] and o["a"].dtype == torch.float32 and o["seg"].dtype == torch.uint8 and o["a"].shape == d["a"].shape
        assert same_bytes(o["a"][0], rebuilt[3 * i]) and same_bytes(o["a"][1], rebuilt[3 * i + 1]) and same_bytes(o["seg"][0], rebuilt[3 * i + 2]), f"sample {i}"
        assert set(o["seg"].unique().tolist()) <= set(d["seg"].unique().tolist()) | {1}                    # labels stay inside their set (and cval)
        assert not torch.equal(o["a"], d["a"])
    # reproducible from its seed; a dict in gives a dict out, equal to the first of the list
    calls.clear()
    again = A.Rand3DElasticd(["a", "seg"], (1.0, 2.0), (20.0, 40.0), prob=1.0, padding_mode="constant", cval=1.0, **kw).set_random_state(5)(samples)
    assert all(same_bytes(a["a"], b["a"]) and same_bytes(a["seg"], b["seg"]) for a, b in zip(again, four))
    calls.clear()
    one = A.Rand3DElasticd(["a", "seg"], (1.0, 2.0), (20.0, 40.0), prob=1.0, padding_mode="constant", cval=1.0, **kw).set_random_state(5)(samples[0])
    assert calls == ["vx_elastic_noise", "vx_elastic_smooth", "vx_elastic_batch"] and isinstance(one, dict)
    assert same_bytes(one["a"], four[0]["a"]) and same_bytes(one["seg"], four[0]["seg"])
    # Compose hands the list over whole
    calls.clear()
    A.Compose([A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=1.0, **kw)]).set_random_state(3)(samples)
    assert calls == ["vx_elastic_noise", "vx_elastic_smooth", "vx_elastic_batch"]
    # prob = 0: the tensors themselves, no call; some fire, some do not
    calls.clear()
    same = A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=0.0, **kw)(samples)
    assert calls == [] and all(o["a"] is d["a"] and o["seg"] is d["seg"] for o, d in zip(same, samples))
    t = A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=0.5, **kw).set_random_state(21)
    mixed = t([_sample(60 + 2 * i) for i in range(8)])
    fired = [w is not None for w in t.last_draws]
    assert any(fired) and not all(fired) and calls == ["vx_elastic_noise", "vx_elastic_smooth", "vx_elastic_batch"]
    # magnitude 0: affine_sample with the matrices of the recorded draws, byte for byte
    t = A.Rand3DElasticd(["a", "seg"], (1.0, 2.0), (0.0, 0.0), prob=1.0, **kw).set_random_state(9)
    flat = t(samples)
    aff = []
    for d, w in zip(samples, t.last_draws):
        m = A.affine_matrix(w[3], w[5], w[4])
        aff += [(d["a"][0], m, "bilinear", "border", 0.0), (d["a"][1], m, "bilinear", "border", 0.0), (d["seg"][0], m, "nearest", "border", 0.0)]
    want = A.affine_sample(aff, shape)
    for i, o in enumerate(flat):
        assert same_bytes(o["a"][0], want[3 * i]) and same_bytes(o["a"][1], want[3 * i + 1]) and same_bytes(o["seg"][0], want[3 * i + 2]), f"magnitude 0, sample {i}"
    # spatial_size: samples that do not fire are resampled with the identity, without a field
    calls.clear()
    sized = A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=0.0, spatial_size=(6, 5, 4), mode=("bilinear", "nearest"))(samples[:2])
    assert calls == ["vx_elastic_batch"]
    for o, d in zip(sized, samples):
        assert torch.equal(o["a"], d["a"][:, 2:8, 2:7, 2:6]) and torch.equal(o["seg"], d["seg"][:, 2:8, 2:7, 2:6])
    with pytest.raises(ValueError, match="crop_start"):
        A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=1.0, mode=("bilinear", "nearest"), context=True)(samples[:2])
    with pytest.raises(TypeError, match="nearest only"):
        A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=1.0)(samples[0])


def test_crop_views_and_context():
    """RandCropByPosNegLabeld(copy=False) hands views over; with context=True the displaced, rotated patch reads the volume around its window"""
    A = _A()
    vol = {"a": dev(ER.ints(2, 20, 18, 16, seed=3, lo=-64, hi=64)), "seg": (dev(ER.ints(1, 20, 18, 16, seed=4, lo=-3, hi=1)) > 0).to(torch.uint8)}
    kw = dict(keys=["a", "seg"], label_key="seg", spatial_size=(8, 7, 6), pos=1, neg=1, num_samples=4)
    copies = A.RandCropByPosNegLabeld(**kw).set_random_state(9)(vol)
    views = A.RandCropByPosNegLabeld(copy=False, **kw).set_random_state(9)(vol)
    mk = lambda **k2: A.Rand3DElasticd(["a", "seg"], 1.5, 30.0, prob=1.0, rotate_range=(0.5, 0.5, 0.5), mode=("bilinear", "nearest"), **k2).set_random_state(2)
    on_views, on_copies = mk()(views), mk()(copies)
    t = mk(context=True)
    ctx = t(views)
    some_differ = False
    fields = A.elastic_field((8, 7, 6), [w[0] for w in t.last_draws], [w[2] for w in t.last_draws]).cpu().numpy()
    for vw, a, b, c4, w, f in zip(views, on_views, on_copies, ctx, t.last_draws, fields):
        for k in ("a", "seg"):
            assert torch.equal(a[k], b[k])                                       # a view is read like its copy
        Ar, c = R.record_values(A.affine_matrix(w[3], w[5], w[4]), (8, 7, 6))
        s = vw["crop_start"]
        lo, hi = [-v for v in s], [p - 1 - v for p, v in zip((20, 18, 16), s)]
        eps = E.coord_bound(Ar, c, (8, 7, 6), f, w[1])
        skip = E.near_tie(Ar, c, (8, 7, 6), f, w[1], lo, hi, 0, eps)
        ref = E.sample(vol["seg"][0].cpu().numpy(), Ar, c, (8, 7, 6), 1, 0, 0.0, f, w[1], lo=lo, hi=hi, origin=s)
        assert not ((c4["seg"][0].cpu().numpy() != ref) & ~skip).any()
        for ch in range(2):
            xs = vol["a"][ch].cpu().numpy()
            bound = 3 * eps * R.neighbour_difference(xs) + R.gamma(9) * float(np.abs(xs).max())
            assert float(np.abs(c4["a"][ch].cpu().numpy() - E.sample(xs, Ar, c, (8, 7, 6), 0, 0, 0.0, f, w[1], lo=lo, hi=hi, origin=s)).max()) <= bound
        some_differ |= not torch.equal(c4["a"], a["a"])
    assert some_differ, "context made no difference: the patches never looked past their window"


# ====================================================================================================================== 11. loader, training step
AFFINE_CFG = {"rotate_degrees": 20.0, "scale": 0.15, "translate": 2.0, "prob": 0.75, "padding_mode": "border", "context": True}
ELASTIC_CFG = dict(AFFINE_CFG, elastic_sigma=(5.0, 8.0), elastic_magnitude=(100.0, 200.0))


def _same(a, b):
    return same_bytes(a.cpu(), b.cpu())


def test_loader_with_and_without_the_elastic_keys(monkeypatch):
    from recipe import CASES
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    A = _A()
    cfg, _ = CASES["g2_32_m2"]
    mk = lambda **kw: SyntheticVolumes(cfg, 2, 2, torch.device("cuda", 0), volume=(72, 64, 56), **kw)
    plain = list(mk())
    # without the new keys: today's loaders, the same transform objects and not one elastic call
    calls = spy(monkeypatch)
    affine_loader = mk(spatial=AFFINE_CFG)
    assert type(affine_loader.pipe.transforms[2]) is A.RandAffined
    affine = list(affine_loader)
    assert not [c for c in calls if c.startswith("vx_elastic")] and "vx_affine_batch" in calls
    for a, b in zip(affine, list(mk(spatial=AFFINE_CFG))):
        assert _same(a[0], b[0]) and _same(a[1], b[1])
    for a, p in zip(list(mk(spatial=None)), plain):
        assert _same(a[0], p[0]) and _same(a[1], p[1])
    # with them
    for cfg_s in (ELASTIC_CFG, dict(ELASTIC_CFG, context=False, padding_mode="constant")):
        calls.clear()
        loader = mk(spatial=cfg_s)
        assert type(loader.pipe.transforms[2]) is A.Rand3DElasticd and loader.pipe.transforms[1].copy is not cfg_s["context"]
        aug, again = list(loader), list(mk(spatial=cfg_s))
        assert len(aug) == 2 and "vx_elastic_batch" in calls and "vx_affine_batch" not in calls
        for (x, y), (x2, y2), (px, py) in zip(aug, again, plain):
            assert x.shape == px.shape and y.shape == py.shape and x.dtype == px.dtype and y.dtype == py.dtype and x.device == px.device
            assert _same(x, x2) and _same(y, y2)                                 # reproducible from its seed
            assert set(y.unique().tolist()) <= {0, 1} and bool(torch.isfinite(x).all())
        assert any(not _same(a[0], p[0]) for a, p in zip(aug, plain)) and any(not _same(a[0], p[0]) for a, p in zip(aug, affine))
    both = list(mk(spatial=ELASTIC_CFG, augment={"flip_axes": [0, 1, 2], "flip_prob": 0.5}))
    assert len(both) == 2 and all(x.shape == px.shape and set(y.unique().tolist()) <= {0, 1} for (x, y), (px, py) in zip(both, plain))
    with pytest.raises(ValueError, match="unknown keys"):
        mk(spatial=dict(ELASTIC_CFG, shear=0.1))


def test_two_training_steps_with_the_elastic_keys():
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    from veloxseg_amd.utils.train_loop import run_train
    cfg, _ = CASES["g2_32_m2"]
    args = types.SimpleNamespace(model_name="VeloxSeg", dataset_name="AutoPETII", checkpoint_path=None, synthetic_steps=2, augment=True)
    h = run_train(args, dict(TRAIN_CFG, epochs=1, spatial_augment=ELASTIC_CFG), {"VeloxSeg": cfg})
    assert len(h["loss"]) == 1 and math.isfinite(h["loss"][0])
    with pytest.raises(ValueError, match="unknown keys"):
        run_train(args, dict(TRAIN_CFG, epochs=1, spatial_augment=dict(ELASTIC_CFG, zoom=1.0)), {"VeloxSeg": cfg})
