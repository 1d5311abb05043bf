"""GPU: vx_affine_batch (csrc/augment_affine.hip) through utils.augment.affine_sample / RandAffined against tests/affine_ref.py.

On the exact rows (integer data, dyadic matrices; tests/test_affine_cpu.py proves the premise of every row) every comparison is `==`.  Outputs are NaN- or
sentinel-prefilled and sit between canaries (exact_ref.Guard); a refused call raises with a message and leaves its prefill untouched.  Off the dyadic rows
trilinear is held to a bound derived in that test's docstring, nearest to `==` away from ties."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

import affine_ref as R
import eval_ref as ER
from exact_ref import Guard

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

TORCH_DTYPE = {0: torch.float32, 1: torch.uint8, 4: torch.int32, 8: torch.int64, -4: torch.float32}
SENTINEL = {1: (0xEE, 0xA5), 4: (-77777, 0x5A5A5A5A), 8: (-77777, 0x5A5A5A5A5A5A)}           # (prefill, canary) of the integer types
MODES, PADS = ("bilinear", "nearest"), ("border", "constant")


def _A():
    from veloxseg_amd.utils import augment as A
    return A


def dev(a):
    """a device copy of a (read-only) numpy array"""
    return torch.from_numpy(np.array(a, copy=True)).cuda()


def guard(shape, code):
    if code in (0, -4):
        return Guard(tuple(shape))
    fill, canary = SENTINEL[code]
    return Guard(tuple(shape), TORCH_DTYPE[code], fill=fill, canary=canary)


def exact(got, want, what):
    """value for value (-0.0 == 0.0); a NaN is expected exactly where the oracle has one"""
    g = got.detach().cpu().numpy().reshape(-1)
    w = np.asarray(want).reshape(-1)
    assert g.size == w.size, f"{what}: {g.size} elements against {w.size}"
    if g.dtype.kind == "f" or w.dtype.kind == "f":
        g, w = g.astype(np.float64), w.astype(np.float64)
        ok = (g == w) | ((g != g) & (w != w))
    else:
        ok = g.astype(np.int64) == w.astype(np.int64)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements differ; first flat index {i}: got {g[i]!r}, want {w[i]!r}")


def done(what, *guards):
    torch.cuda.synchronize()
    for i, g in enumerate(guards):
        g.check(f"{what} (buffer {i})")


def untouched(g, code, what):
    done(what, g)
    t = g.t.reshape(-1)
    assert bool((t != t).all()) if code in (0, -4) else bool((t == SENTINEL[code][0]).all()), f"{what}: the refused call wrote its output"


# ====================================================================================================================== 1. exact rows
@pytest.mark.parametrize("row", R.EXACT_ROWS, ids=lambda r: r["id"])
def test_exact_rows(row):
    """both modes x both paddings on the image, nearest x both paddings on the four label types: ONE call of twelve records, every output `==` its oracle"""
    A = _A()
    m = R.row_matrix(row)
    entries, outs, wants = [], [], []
    x = dev(R.image(row))
    for mode in (0, 1):
        for pad in (0, 1):
            entries.append((x, m, MODES[mode], PADS[pad], R.CVAL))
            outs.append(guard(row["out"], 0))
            wants.append(R.reference(row, mode, pad))
    labs = {code: dev(R.label(row, code)) for code in (1, 4, 8, -4)}
    for code, lab in labs.items():
        for pad in (0, 1):
            entries.append((lab, m, "nearest", PADS[pad], R.CVAL))
            outs.append(guard(row["out"], code))
            wants.append(R.reference(row, 1, pad, code))
    A.affine_sample(entries, row["out"], out=[g.t for g in outs])
    done(row["id"], *outs)
    for i, (g, w) in enumerate(zip(outs, wants)):
        exact(g.t, w, f"{row['id']} record {i} ({entries[i][2]}, {entries[i][3]}, {entries[i][0].dtype})")
    exact(x, R.image(row), "the input itself")
    if row["matrix"] == "identity" and row["out"] == row["n"]:
        exact(outs[0].t, R.image(row), "the identity")


# ====================================================================================================================== 2. vx_rotate_z's oracle
@pytest.mark.parametrize("row", ER.ROT_ROWS, ids=lambda r: r["id"])
def test_z_rotation_agrees_with_the_rotate_z_oracle(row):
    A = _A()
    x = ER.rotate_input(row)
    d = dev(x)
    m = np.array([[row["cs"], -row["sn"], 0, 0], [row["sn"], row["cs"], 0, 0], [0, 0, 1, 0]], dtype=np.float64)
    outs = {mode: Guard(x.shape) for mode in (0, 1)}
    A.affine_sample([(d[ch], m, MODES[mode], "border", 0.0) for mode in (0, 1) for ch in range(x.shape[0])], x.shape[1:],
                    out=[outs[mode].t[ch] for mode in (0, 1) for ch in range(x.shape[0])])
    done(row["id"], *outs.values())
    for mode in (0, 1):
        exact(outs[mode].t, ER.rotate_exact(x, row["cs"], row["sn"], mode), f"{row['id']} mode {mode}")


# ====================================================================================================================== 3. views and context
@pytest.mark.parametrize("matrix", ["rot3", "big", "permute"])
def test_views_and_context(matrix):
    """the source is a crop view at an odd origin inside a (12, 11, 13) parent that is itself a strided view (every second element of a wider buffer along W)"""
    A = _A()
    parent_np = ER.ints(12, 11, 13, seed=R._seed(matrix), lo=-64, hi=64)
    wide = torch.full((12, 11, 26), 999.0, device="cuda")
    wide[:, :, ::2] = dev(parent_np)
    parent = wide[:, :, ::2]
    start, n = (3, 1, 5), (6, 7, 5)
    view = parent[3:9, 1:8, 5:10]
    assert not view.is_contiguous() and view.stride() == (11 * 26, 26, 2)
    crop_np = parent_np[3:9, 1:8, 5:10]
    m = R.row_matrix(dict(matrix=matrix))
    Ar, c = R.record_values(m, n)
    lo, hi = [-s for s in start], [p - 1 - s for p, s in zip(parent_np.shape, start)]
    differs = 0
    for mode in (0, 1):
        for pad in (0, 1):
            win, ctx = Guard(n), Guard(n)
            A.affine_sample([(view, m, MODES[mode], PADS[pad], R.CVAL), (view, m, MODES[mode], PADS[pad], R.CVAL, (lo, hi))], n, out=[win.t, ctx.t])
            done(f"{matrix} {mode} {pad}", win, ctx)
            want_win = R.sample(crop_np, Ar, c, n, mode, pad, R.CVAL)
            want_ctx = R.sample(parent_np, Ar, c, n, mode, pad, R.CVAL, lo=lo, hi=hi, origin=start)
            exact(win.t, want_win, f"{matrix} mode {mode} pad {pad}: window bounds against the oracle on the copied crop")
            exact(ctx.t, want_ctx, f"{matrix} mode {mode} pad {pad}: context bounds")
            differs += int(not np.array_equal(want_win, want_ctx))
            assert not torch.equal(win.t, ctx.t) or np.array_equal(want_win, want_ctx)
    assert differs > 0, "the row does not show the difference between window and context bounds"
    assert bool((wide[:, :, 1::2] == 999.0).all())


# ====================================================================================================================== 4. many records
def test_many_records_in_one_call_equal_one_call_each():
    """3 samples x 3 keys (two fp32 images, one label) with different matrices, modes, paddings and element types: one call against one call per record, on bytes"""
    A = _A()
    out_size, entries = (7, 9, 10), []
    specs = [("rot3", "bilinear", "border", torch.uint8), ("big", "bilinear", "constant", torch.int64), ("shear", "nearest", "constant", torch.int32)]
    for s, (name, mode, pad, lab_dtype) in enumerate(specs):
        m = R.row_matrix(dict(matrix=name))
        m[:, 3] = (0.5 * s, -0.25, 0.75)
        n = (8 + s, 9, 11 - s)
        for k in range(2):
            entries.append((dev(ER.ints(*n, seed=10 * s + k, lo=-64, hi=64)), m, mode, pad, 3.0))
        entries.append((dev(ER.ints(*n, seed=10 * s + 2, lo=0, hi=64)).to(lab_dtype), m, "nearest", pad, 3.0))
    together = A.affine_sample(entries, out_size)
    alone = [A.affine_sample([e], out_size)[0] for e in entries]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(together, alone)):
        assert a.dtype == b.dtype == entries[i][0].dtype and a.shape == b.shape == out_size
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) if a.dtype != torch.float32 else torch.equal(a.view(torch.int32), b.view(torch.int32)), f"record {i}"
        Ar, c = R.record_values(entries[i][1], tuple(entries[i][0].shape))
        exact(a, R.sample(entries[i][0].cpu().numpy(), Ar, c, out_size, 0 if entries[i][2] == "bilinear" else 1, 0 if entries[i][3] == "border" else 1, 3.0), f"record {i}")
    # (the kernel takes one block per brick of one record, grid = records x bricks, and has no grid-stride loop: there is no cap to run above)


# ====================================================================================================================== 5. non-finite values
@pytest.mark.parametrize("pad", [0, 1], ids=PADS)
def test_nan_and_inf_appear_where_the_oracle_has_them(pad):
    A = _A()
    row = next(r for r in R.EXACT_ROWS if r["id"] == "rot3_9x7x5_from_9x7x5")
    x = np.array(R.image(row), copy=True)
    x[4, 3, 2], x[1, 2, 2], x[2, 0, 0] = np.nan, np.inf, -np.inf                      # voxels that both modes sample under both paddings
    m = R.row_matrix(row)
    Ar, c = R.record_values(m, row["n"])
    outs = [Guard(row["out"]), Guard(row["out"])]
    A.affine_sample([(dev(x), m, MODES[mode], PADS[pad], R.CVAL) for mode in (0, 1)], row["out"], out=[g.t for g in outs])
    done("non-finite", *outs)
    for mode in (0, 1):
        want = R.sample(x, Ar, c, row["out"], mode, pad, R.CVAL)
        assert np.isnan(want).any() and np.isinf(want).any()
        exact(outs[mode].t, want, f"non-finite mode {mode} pad {pad}")


# ====================================================================================================================== 6. off the dyadic rows
def test_off_dyadic_rows():
    """Three random angles about x, y and z at once, scale 0.8 .. 1.2, 24^3, data = a linear ramp plus small integers; the record (A, c in fp32) is the input of both
    the kernel and the fp64 oracle, so the bound covers the kernel's arithmetic alone.

    Coordinate: s_a = ((A0 p0 + A1 p1) + A2 p2) + c_a with exact p (half-integers).  Every term A_i p_i passes through at most four fp32 roundings (its product and
    three additions), c_a through one, so |s_fp32 - s_exact| <= eps = gamma(4) max_a (sum_i |A[a][i]| |p_i|max + |c_a|), gamma(k) = k u / (1 - k u), u = 2^-24
    (affine_ref.coord_bound).  The clamps are exact and do not increase a difference; l = s - floor(s) is exact in fp32.
    Trilinear: the interpolant is continuous and piecewise linear with slope at most G = the largest neighbour difference along each axis, so moving the three
    coordinates by eps moves it by at most 3 eps G (this also covers a coordinate that crosses into the next cell; under constant padding G is taken over the volume
    with its one-voxel frame of cval, where the interpolant runs from the outermost voxels down to cval).  The three nested lerps
    (1 - l) u + l v round 1 - l, two products and a sum: every data value passes through at most 9 roundings with weights that sum to 1, adding at most
    gamma(9) max|x| (cval is below max|x| here).  bound = 3 eps G + gamma(9) max|x|; the oracle's own fp64 roundings are 2^-29 of that and are not counted.
    Nearest: `==` except where the fp64 coordinate lies within eps of a .5 tie on some axis (the only places where the two precisions may round differently); at
    most 1 % of the voxels may be left out (tests/test_affine_cpu.py checks the seed against that cap on the oracle alone).
    Measured on an MI355X (printed below): DESIGN.md section 28."""
    A = _A()
    x, m = R.off_dyadic_case()
    Ar, c = R.record_values(m, R.OFF_N)
    eps = R.coord_bound(Ar, c, R.OFF_N)
    vmax, cval = float(np.abs(x).max()), 2.0
    assert cval <= vmax
    d = dev(x)
    outs = {(mode, pad): Guard(R.OFF_N) for mode in (0, 1) for pad in (0, 1)}
    A.affine_sample([(d, m, MODES[mode], PADS[pad], cval) for mode, pad in outs], R.OFF_N, out=[g.t for g in outs.values()])
    done("off-dyadic", *outs.values())
    hi = [v - 1 for v in R.OFF_N]
    for pad in (0, 1):
        G = R.neighbour_difference(x, cval if pad else None)
        bound = 3 * eps * G + R.gamma(9) * vmax
        got = outs[0, pad].t.cpu().numpy().astype(np.float64)
        err = float(np.abs(got - R.sample(x, Ar, c, R.OFF_N, 0, pad, cval)).max())
        print(f"off-dyadic trilinear {PADS[pad]}: max |error| {err:.3e}, bound {bound:.3e} (eps {eps:.3e}, G {G:.3f}, max|x| {vmax:.2f})")
        assert err <= bound, f"trilinear {PADS[pad]}: max |error| {err:.3e} above the derived bound {bound:.3e}"
        skip = R.near_tie(Ar, c, R.OFF_N, [0, 0, 0], hi, pad, eps)
        assert float(skip.mean()) <= 0.01
        got, want = outs[1, pad].t.cpu().numpy(), R.sample(x, Ar, c, R.OFF_N, 1, pad, cval)
        bad = (got != want) & ~skip
        print(f"off-dyadic nearest {PADS[pad]}: {int(skip.sum())} of {skip.size} voxels left out, {int(bad.sum())} differ")
        assert not bad.any(), f"nearest {PADS[pad]}: {int(bad.sum())} voxels differ away from ties"


# ====================================================================================================================== 7. refusals
def test_refusals_leave_the_prefill_untouched():
    A = _A()
    from veloxseg_amd import _hip as H
    x = dev(ER.ints(4, 5, 6, seed=1))
    lab = x.to(torch.int32)
    eye = A.affine_matrix()
    out, iout = guard((4, 5, 6), 0), guard((4, 5, 6), 4)
    ok = (x, eye, "bilinear", "border", 0.0)
    with pytest.raises(ValueError, match="mode"):
        A.affine_sample([ok, (x, eye, "cubic", "border", 0.0)], (4, 5, 6), out=[out.t, out.t])
    with pytest.raises(ValueError, match="padding_mode"):
        A.affine_sample([(x, eye, "nearest", "reflection", 0.0)], (4, 5, 6), out=[out.t])
    with pytest.raises(TypeError, match="nearest only"):
        A.affine_sample([(lab, eye, "bilinear", "border", 0.0)], (4, 5, 6), out=[iout.t])
    with pytest.raises(ValueError, match="lo .* > hi"):
        A.affine_sample([(x, eye, "nearest", "border", 0.0, ([0, 3, 0], [3, 2, 5]))], (4, 5, 6), out=[out.t])
    with pytest.raises(ValueError, match="reach outside"):
        A.affine_sample([(x, eye, "nearest", "border", 0.0, ([0, 0, -1], [3, 4, 5]))], (4, 5, 6), out=[out.t])
    with pytest.raises(ValueError, match="reach outside"):
        A.affine_sample([(x, eye, "nearest", "border", 0.0, ([0, 0, 0], [4, 4, 5]))], (4, 5, 6), out=[out.t])
    with pytest.raises(ValueError, match="out_size"):
        A.affine_sample([ok], (4, 0, 6), out=[out.t])
    with pytest.raises(ValueError, match="empty source"):
        A.affine_sample([(x[:, :0], eye, "nearest", "border", 0.0)], (4, 5, 6), out=[out.t])
    with pytest.raises(ValueError, match="no entries"):
        A.affine_sample([], (4, 5, 6), out=[])
    with pytest.raises(ValueError, match="finite"):
        A.affine_sample([(x, eye * float("nan"), "nearest", "border", 0.0)], (4, 5, 6), out=[out.t])
    with pytest.raises(ValueError, match="alias"):                               # the destination is the source
        A.affine_sample([(out.t, eye, "nearest", "border", 0.0)], (4, 5, 6), out=[out.t])
    with pytest.raises(ValueError, match="alias"):                               # ... or overlaps what ANOTHER record reads
        A.affine_sample([ok, (out.t, eye, "nearest", "border", 0.0)], (4, 5, 6), out=[out.t, torch.empty(4, 5, 6, device="cuda")])
    with pytest.raises(ValueError, match="contiguous"):
        A.affine_sample([ok], (4, 5, 6), out=[torch.empty(4, 5, 12, device="cuda")[:, :, ::2]])
    # the C entry: what it can see
    table = torch.zeros(A.AFFINE_RECORD_BYTES, dtype=torch.uint8, device="cuda")
    for args, msg in (((None, 1, 4, 5, 6), "null pointer"), ((table.data_ptr(), 0, 4, 5, 6), "no records"), ((table.data_ptr(), -3, 4, 5, 6), "no records"),
                      ((table.data_ptr(), 1, 0, 5, 6), "non-positive output extent"), ((table.data_ptr(), 1, 4, 5, -6), "non-positive output extent")):
        with pytest.raises(RuntimeError, match=msg):
            H.call("vx_affine_batch", *args, H.stream_ptr())
    # records that name a destination but should not have been sent write nothing: unknown mode, unknown type, trilinear on int32, lo > hi, a null source
    tab = np.zeros(5, dtype=A._AFF)
    for r, g in zip(tab, (out, out, iout, out, out)):
        r["src"], r["dst"], r["stride"], r["n"], r["hi"], r["A"] = x.data_ptr(), g.ptr, (30, 6, 1), (4, 5, 6), (3, 4, 5), np.eye(3).reshape(-1)
    tab[0]["mode"], tab[1]["dtype"], tab[2]["dtype"], tab[3]["lo"], tab[4]["src"] = 2, 3, 4, (0, 5, 0), 0
    tab[2]["src"] = lab.data_ptr()
    H.call("vx_affine_batch", torch.from_numpy(tab.view(np.uint8).reshape(-1)).cuda().data_ptr(), 5, 4, 5, 6, H.stream_ptr())
    untouched(out, 0, "refused calls / records")
    untouched(iout, 4, "refused calls / records")


# ====================================================================================================================== 8. RandAffined
def _sample(seed, shape=(10, 9, 8), lab_dtype=torch.uint8):
    return {"a": dev(ER.ints(2, *shape, seed=seed, lo=-64, hi=64)), "seg": dev(ER.ints(1, *shape, seed=seed + 1, lo=0, hi=3)).to(lab_dtype), "name": f"case{seed}"}


def test_rand_affined_draws_matrices_and_one_call(monkeypatch):
    A = _A()
    from veloxseg_amd import _hip as H
    kw = dict(rotate_range=(0.4, 0.3, 0.2), scale_range=(0.1, 0.1, 0.2), translate_range=(1.0, 2.0, 0.5))
    t = A.RandAffined(["a", "seg"], prob=0.5, mode=("bilinear", "nearest"), padding_mode="constant", cval=1.0, **kw).set_random_state(21)
    samples = [_sample(40 + 2 * i) for i in range(8)]
    calls = []
    real = H.call
    monkeypatch.setattr(H, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    outs = t(samples)
    assert calls == ["vx_affine_batch"], f"a list of {len(samples)} samples made the calls {calls}"
    want = R.draws(21, 0.5, kw["rotate_range"], kw["scale_range"], kw["translate_range"], len(samples))
    assert any(w is None for w in want) and sum(w is not None for w in want) >= 2
    for d, o, w in zip(samples, outs, want):
        assert o["name"] == d["name"] and o is not d
        if w is None:
            assert o["a"] is d["a"] and o["seg"] is d["seg"]                     # not fired: the tensors themselves
            continue
        rot, tra, sca = w
        m = R.matrix(rot, sca, tra)
        assert np.allclose(A.affine_matrix(rot, sca, tra), m, rtol=0, atol=1e-13)
        Ar, c = R.record_values(A.affine_matrix(rot, sca, tra), d["a"].shape[1:])
        assert o["a"].dtype == torch.float32 and o["seg"].dtype == torch.uint8 and o["a"].shape == d["a"].shape and o["seg"].shape == d["seg"].shape
        eps = R.coord_bound(Ar, c, d["a"].shape[1:])
        hi = [v - 1 for v in d["a"].shape[1:]]
        skip = R.near_tie(Ar, c, d["a"].shape[1:], [0, 0, 0], hi, 1, eps)
        got, ref = o["seg"][0].cpu().numpy(), R.sample(d["seg"][0].cpu().numpy(), Ar, c, d["seg"].shape[1:], 1, 1, 1.0)
        assert not ((got != ref) & ~skip).any()
        for ch in range(2):
            xs = d["a"][ch].cpu().numpy()
            bound = 3 * eps * R.neighbour_difference(xs, 1.0) + R.gamma(9) * float(np.abs(xs).max())          # (the bound of test_off_dyadic_rows)
            assert float(np.abs(o["a"][ch].cpu().numpy() - R.sample(xs, Ar, c, xs.shape, 0, 1, 1.0)).max()) <= bound
    # a single dict goes the same way; four fired samples are still one call
    calls.clear()
    t1 = A.RandAffined(["a", "seg"], prob=1.0, mode=("bilinear", "nearest"), **kw).set_random_state(5)
    four = t1(samples[:4])
    assert calls == ["vx_affine_batch"] and all(o["a"] is not d["a"] for o, d in zip(four, samples))
    calls.clear()
    one = A.RandAffined(["a", "seg"], prob=1.0, mode=("bilinear", "nearest"), **kw).set_random_state(5)(samples[0])
    assert calls == ["vx_affine_batch"] and isinstance(one, dict) and torch.equal(one["a"], four[0]["a"]) and torch.equal(one["seg"], four[0]["seg"])
    # Compose hands the list over whole
    calls.clear()
    A.Compose([A.RandAffined(["a", "seg"], prob=1.0, mode=("bilinear", "nearest"), **kw)]).set_random_state(3)(samples[:4])
    assert calls == ["vx_affine_batch"]
    # prob = 0: the input tensors themselves, no call
    calls.clear()
    same = A.RandAffined(["a", "seg"], prob=0.0, mode=("bilinear", "nearest"), **kw)(samples[:3])
    assert calls == [] and all(o["a"] is d["a"] and o["seg"] is d["seg"] for o, d in zip(same, samples))
    # spatial_size: every sample comes out at that size, fired or not (the identity for those that did not fire)
    calls.clear()
    sized = A.RandAffined(["a", "seg"], prob=0.0, spatial_size=(6, 5, 4), mode=("bilinear", "nearest"))(samples[:2])
    assert calls == ["vx_affine_batch"]
    for o, d in zip(sized, samples):
        assert torch.equal(o["a"], d["a"][:, 2:8, 2:7, 2:6]) and torch.equal(o["seg"], d["seg"][:, 2:8, 2:7, 2:6])           # centred: (10 - 6) / 2, (9 - 5) / 2, (8 - 4) / 2
    with pytest.raises(ValueError, match="crop_start"):
        A.RandAffined(["a", "seg"], prob=1.0, mode=("bilinear", "nearest"), context=True)(samples[:2])
    with pytest.raises(TypeError, match="nearest only"):
        A.RandAffined(["a", "seg"], prob=1.0)(samples[0])


def test_crop_views_and_context():
    A = _A()
    vol = {"a": dev(ER.ints(2, 20, 18, 16, seed=3, lo=-64, hi=64)), "seg": (dev(ER.ints(1, 20, 18, 16, seed=4, lo=-3, hi=1)) > 0).to(torch.uint8)}
    kw = dict(keys=["a", "seg"], label_key="seg", spatial_size=(8, 7, 6), pos=1, neg=1, num_samples=4)
    copies = A.RandCropByPosNegLabeld(**kw).set_random_state(9)(vol)
    views = A.RandCropByPosNegLabeld(copy=False, **kw).set_random_state(9)(vol)
    assert len(copies) == len(views) == 4
    for cp, vw in zip(copies, views):
        assert "crop_start" not in cp and "crop_source_shape" not in cp and cp["crop_center"] == vw["crop_center"]
        assert vw["crop_source_shape"] == [20, 18, 16] and len(vw["crop_start"]) == 3
        for k in ("a", "seg"):
            assert cp[k].is_contiguous() and vw[k].untyped_storage().data_ptr() == vol[k].untyped_storage().data_ptr()
            assert torch.equal(vw[k].contiguous(), cp[k])
            s = vw["crop_start"]
            assert torch.equal(vw[k], vol[k][:, s[0]:s[0] + 8, s[1]:s[1] + 7, s[2]:s[2] + 6])
    mk = lambda **k2: A.RandAffined(["a", "seg"], prob=1.0, rotate_range=(0.5, 0.5, 0.5), scale_range=(0.1, 0.1, 0.1), mode=("bilinear", "nearest"), **k2).set_random_state(2)
    on_views, on_copies, ctx = mk()(views), mk()(copies), mk(context=True)(views)
    params = R.draws(2, 1.0, (0.5, 0.5, 0.5), (0.1, 0.1, 0.1), None, 4)
    some_differ = False
    for vw, a, b, c4, (rot, tra, sca) in zip(views, on_views, on_copies, ctx, params):
        for k in ("a", "seg"):
            assert torch.equal(a[k], b[k])                                       # a view is read like its copy
        Ar, c = R.record_values(A.affine_matrix(rot, sca, tra), (8, 7, 6))
        s = vw["crop_start"]
        lo, hi = [-v for v in s], [p - 1 - v for p, v in zip((20, 18, 16), s)]
        eps = R.coord_bound(Ar, c, (8, 7, 6))
        skip = R.near_tie(Ar, c, (8, 7, 6), lo, hi, 0, eps)
        ref = R.sample(vol["seg"][0].cpu().numpy(), Ar, c, (8, 7, 6), 1, 0, lo=lo, hi=hi, origin=s)
        assert not ((c4["seg"][0].cpu().numpy() != ref) & ~skip).any()
        for ch in range(2):
            xs = vol["a"][ch].cpu().numpy()
            bound = 3 * eps * R.neighbour_difference(xs) + R.gamma(9) * float(np.abs(xs).max())
            assert float(np.abs(c4["a"][ch].cpu().numpy() - R.sample(xs, Ar, c, (8, 7, 6), 0, 0, lo=lo, hi=hi, origin=s)).max()) <= bound
        some_differ |= not torch.equal(c4["a"], a["a"])
    assert some_differ, "context made no difference: the patches never looked past their window"


# ====================================================================================================================== 9. loader
SPATIAL_CFG = {"rotate_degrees": 20.0, "scale": 0.15, "translate": 2.0, "prob": 0.75, "padding_mode": "border", "context": True}


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else t.dtype)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a.cpu()), _bits(b.cpu()))


def test_loader_with_and_without_the_spatial_config():
    from recipe import CASES
    from veloxseg_amd.utils.train_loop import SyntheticVolumes
    cfg, _ = CASES["g2_32_m2"]
    mk = lambda **kw: SyntheticVolumes(cfg, 2, 2, torch.device("cuda", 0), volume=(72, 64, 56), **kw)
    plain = list(mk())
    for a, p in zip(list(mk(spatial=None)), plain):
        assert _same(a[0], p[0]) and _same(a[1], p[1])
    with pytest.raises(ValueError, match="unknown keys"):
        mk(spatial={"shear": 0.1})
    for cfg_s in (SPATIAL_CFG, dict(SPATIAL_CFG, context=False, padding_mode="constant")):
        aug, again = list(mk(spatial=cfg_s)), list(mk(spatial=cfg_s))
        assert len(aug) == 2
        for (x, y), (x2, y2), (px, py) in zip(aug, again, plain):
            assert x.shape == px.shape and y.shape == py.shape and x.dtype == px.dtype and y.dtype == py.dtype and x.device == px.device
            assert _same(x, x2) and _same(y, y2)                                 # reproducible from its seed
            assert set(y.unique().tolist()) <= {0, 1} and bool(torch.isfinite(x).all())
        assert any(not _same(a[0], p[0]) for a, p in zip(aug, plain))
    # together with the batch assembler, which reads the views directly
    both = list(mk(spatial=SPATIAL_CFG, augment={"flip_axes": [0, 1, 2], "flip_prob": 0.5}))
    assert len(both) == 2 and all(x.shape == px.shape and y.dtype == py.dtype and set(y.unique().tolist()) <= {0, 1} for (x, y), (px, py) in zip(both, plain))


def test_two_training_steps_with_the_spatial_config():
    from recipe import CASES
    from test_train_harness_cpu import TRAIN_CFG
    from veloxseg_amd.utils.train_loop import run_train
    cfg, _ = CASES["g2_32_m2"]
    args = types.SimpleNamespace(model_name="VeloxSeg", dataset_name="AutoPETII", checkpoint_path=None, synthetic_steps=2, augment=True)
    h = run_train(args, dict(TRAIN_CFG, epochs=1, spatial_augment=SPATIAL_CFG), {"VeloxSeg": cfg})
    assert len(h["loss"]) == 1 and math.isfinite(h["loss"][0])
    with pytest.raises(ValueError, match="unknown keys"):
        run_train(args, dict(TRAIN_CFG, epochs=1, spatial_augment={"gamma": 1.0}), {"VeloxSeg": cfg})
