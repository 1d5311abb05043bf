"""The linear kernels against bit-exact fp64 oracles on integer-valued data, straight through the C ABI.

Operands are integers in [-3, 3] (tests/exact_ref.py; tests/test_exact_ref_cpu.py proves for every row of the table that all sums stay below 2^24 and that
fp32 reproduces fp64), so every kernel here -- fp32 FMAs in any order, float atomics, fp32 MFMA, products from 16-bit pieces with power-of-two scales -- must
return the oracle VALUE FOR VALUE: `(got.double() == ref).all()`.  No tolerance appears in this file.
  - outputs written with `=` are prefilled with NaN, `+=` destinations (and accumulate = 1) with integers in [-8, 8] that the reference adds;
  - every output and every workspace sits between 64-element canaries (exact_ref.Guard); workspaces have exactly the size the entry reports or the header
    states and are filled with NaN -- unless the header says the caller zeroes them;
  - entries with an `accumulate` flag run with 0 and with 1; a declined call (return value 1) must leave its NaN prefill untouched;
  - `*_set_*` knobs are restored in `finally`."""
import contextlib
import ctypes

import pytest
import torch

import exact_ref as E
from exact_ref import Guard

pytestmark = pytest.mark.gpu


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


@contextlib.contextmanager
def knob(H, name, value, default, getter=None):
    """set a `*_set_*` knob for the body and put it back in `finally`: to the value its getter reports where the header has one, else to the documented default"""
    if getter is not None:
        default = H.query(getter)
    H.call(name, value)
    try:
        yield
    finally:
        H.call(name, default)


class Run:
    """the guards of one test: out() = NaN-prefilled, acc() = integer-prefilled (returns the prefill in fp64 too); done() checks every canary"""

    def __init__(self, H, what):
        self.H, self.what, self.guards, self.keep, self.seed = H, what, [], [], 1000
        self.st = H.stream_ptr()

    def out(self, shape, dtype=torch.float32):
        g = Guard(tuple(shape), dtype)
        self.guards.append(g)
        return g

    def acc(self, shape, dtype=torch.float32):
        self.seed += 1
        p = E.prefill(*shape, seed=self.seed)
        g = Guard(tuple(shape), dtype, fill=p)
        self.guards.append(g)
        return g, p.double()

    def dst(self, shape, accumulate):
        """destination of an entry with an accumulate flag: (guard, what the reference adds)"""
        if accumulate:
            return self.acc(shape)
        return self.out(shape), 0.0

    def dev(self, t):
        """a device copy of a CPU operand that lives as long as the test (a temporary's memory would be handed to the next allocation before the launch)"""
        self.keep.append(t.contiguous().cuda())
        return self.keep[-1]

    def done(self):
        torch.cuda.synchronize()
        for i, g in enumerate(self.guards):
            g.check(f"{self.what} (buffer {i})")


def cu(t):
    return None if t is None else t.contiguous().cuda()


def split(t, C1):
    """(first C1 channels, the rest) of a channel concat; C1 == 0: (t, None)"""
    if not C1:
        return t, None
    return t[:, :C1].contiguous(), t[:, C1:].contiguous()


def conv_args(r):
    return (r["B"], r["Cin"], *r["sp"], r["Cout"], r["K"], r["S"], r["P"], r["G"], r["ps"])


# ====================================================================================================================== A. direct kernels
@pytest.mark.parametrize("row", E.rows("direct"), ids=E.ids("direct"))
def test_direct_forward_and_input_gradient(row):
    """vx_conv3d_fwd (concat source, pixel-shuffled store) and vx_conv3d_bwd_data (split destination, with and without bias_like, accumulate 0 and 1)"""
    H = _H()
    t, ref, C1 = E.inputs("direct", row), E.reference("direct", row), row["C1"]
    R = Run(H, f"direct {row['id']}")
    x1, x2 = (cu(v) for v in split(t["x"], C1))
    w, b, dy = cu(t["w"]), cu(t["b"]), cu(t["dy"])
    y = R.out(ref["y"].shape)
    H.call("vx_conv3d_fwd", H.P(x1), H.P(x2), C1, H.P(w), H.P(b), y.ptr, *conv_args(row), R.st)
    y0 = R.out(ref["y"].shape)
    H.call("vx_conv3d_fwd", H.P(x1), H.P(x2), C1, H.P(w), None, y0.ptr, *conv_args(row), R.st)
    bl = E.ints(row["Cin"], seed=77)
    checks = [(y.t, ref["y"], "y"), (y0.t, ref["y"] - _bias_plane(row, t["b"], ref["y"].shape), "y without bias")]
    for with_bl in (False, True):
        for accumulate in (0, 1):
            shp = t["x"].shape
            c1 = C1 or shp[1]
            d1, p1 = R.dst((shp[0], c1, *shp[2:]), accumulate)
            d2, p2 = R.dst((shp[0], shp[1] - c1, *shp[2:]), accumulate) if C1 else (None, None)
            H.call("vx_conv3d_bwd_data", H.P(dy), H.P(w), H.P(R.dev(bl)) if with_bl else None, d1.ptr, d2.ptr if d2 else None, C1, *conv_args(row), accumulate, R.st)
            want = ref["dx"] + (bl.double().view(1, -1, 1, 1, 1) if with_bl else 0.0)
            tag = f"dx bias_like={with_bl} accumulate={accumulate}"
            checks.append((d1.t, want[:, :c1] + p1, tag))
            if d2:
                checks.append((d2.t, want[:, c1:] + p2, tag + " (second tensor)"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


def _bias_plane(row, b, yshape):
    """the bias as it sits in the (possibly pixel-shuffled) output of one sample"""
    from oracle import veloxseg_oracle as O
    ps = row["ps"]
    p = b.double().view(1, -1, 1, 1, 1).expand(1, -1, *(n // ps for n in yshape[2:])).contiguous()
    return O.pixel_shuffle3d(p, ps) if ps > 1 else p


@pytest.mark.parametrize("rows_knob", [0, 1], ids=["pairs", "rows"])
@pytest.mark.parametrize("row", E.rows("direct"), ids=E.ids("direct"))
def test_direct_weight_gradients(row, rows_knob):
    """vx_conv3d_bwd_weight, vx_conv3d_bwd_weight_tiled and, where vx_conv3d_bwd_weight_ws_floats > 0, vx_conv3d_bwd_weight_tiled_ws with a NaN workspace of
    exactly that size; db given and NULL; vx_wgrad_set_rows 0 and 1"""
    H = _H()
    t, ref, C1 = E.inputs("direct", row), E.reference("direct", row), row["C1"]
    R = Run(H, f"direct wgrad {row['id']} rows={rows_knob}")
    x1, x2 = (cu(v) for v in split(t["x"], C1))
    dy = cu(t["dy"])
    checks = []
    with knob(H, "vx_wgrad_set_rows", rows_knob, 1):
        nws = H.query("vx_conv3d_bwd_weight_ws_floats", *conv_args(row))
        for entry in ("vx_conv3d_bwd_weight", "vx_conv3d_bwd_weight_tiled", "vx_conv3d_bwd_weight_tiled_ws"):
            if entry.endswith("_ws") and nws == 0:
                continue
            for with_db in (True, False):
                dw, pw = R.acc(ref["dw"].shape)
                db, pb = R.acc(ref["db"].shape) if with_db else (None, None)
                extra = ()
                if entry.endswith("_ws"):
                    ws = R.out((nws,))
                    extra = (ws.ptr, nws)
                H.call(entry, H.P(x1), H.P(x2), C1, H.P(dy), dw.ptr, db.ptr if db else None, *extra, *conv_args(row), R.st)
                checks.append((dw.t, ref["dw"] + pw, f"{entry} dw (db {'given' if with_db else 'NULL'})"))
                if db:
                    checks.append((db.t, ref["db"] + pb, f"{entry} db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


# ====================================================================================================================== B. vx_conv_s1
@pytest.mark.parametrize("row", E.rows("s1"), ids=E.ids("s1"))
def test_conv_s1(row):
    """wmode 0 (forward, out_ps) and wmode 1 (input gradient from the pixel-shuffled dy, in_ps), accumulate 0 and 1"""
    H = _H()
    t, ref = E.inputs("s1", row), E.reference("s1", row)
    R = Run(H, f"s1 {row['id']}")
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    B, Cin, Cout, (D, Hh, W), K, G, ps = row["B"], row["Cin"], row["Cout"], row["sp"], row["K"], row["G"], row["ps"]
    checks = []
    for accumulate in (0, 1):
        y, p = R.dst(ref["y"].shape, accumulate)
        H.call("vx_conv_s1", H.P(x), H.P(w), H.P(b), y.ptr, B, Cin, Cout, D, Hh, W, K, G, 0, 1, ps, accumulate, R.st)
        checks.append((y.t, ref["y"] + p, f"forward accumulate={accumulate}"))
        dx, p = R.dst(ref["dx"].shape, accumulate)
        H.call("vx_conv_s1", H.P(dy), H.P(w), None, dx.ptr, B, Cout, Cin, D, Hh, W, K, G, 1, ps, 1, accumulate, R.st)
        checks.append((dx.t, ref["dx"] + p, f"input gradient accumulate={accumulate}"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


# ====================================================================================================================== C. dense strided convs on MFMA
def _mfma_case(H, fam, row):
    t, ref = E.inputs(fam, row), E.reference(fam, row)
    R = Run(H, f"{fam} {row['id']}")
    B, Cin, Cout, (D, Hh, W), K, S, P = row["B"], row["Cin"], row["Cout"], row["sp"], row["K"], row["S"], row["P"]
    assert H.query("vx_conv_mfma_ok", Cin, Cout, D, Hh, W, K, S, P, 1, 1) == 1
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    checks = []
    nf, nb = H.query("vx_conv_mfma_ws_floats", Cin, Cout, K, 0), H.query("vx_conv_mfma_ws_floats", Cin, Cout, K, 1)
    y, ws = R.out(ref["y"].shape), R.out((nf,))
    H.call("vx_conv_mfma_fwd", H.P(x), H.P(w), H.P(b), y.ptr, ws.ptr, B, Cin, D, Hh, W, Cout, K, S, P, R.st)
    checks.append((y.t, ref["y"], "forward"))
    y, ws, mx = R.out(ref["y"].shape), R.out((nf,)), R.out((1,))
    H.call("vx_conv_mfma_fwd_mx", H.P(x), H.P(w), H.P(b), y.ptr, ws.ptr, mx.ptr, B, Cin, D, Hh, W, Cout, K, S, P, R.st)
    checks.append((y.t, ref["y"], "forward (_mx)"))
    writes = H.query("vx_conv_mfma_fwd_writes_absmax", Cin, Cout, D, Hh, W, K, S, P)
    for accumulate in (0, 1):
        dx, p = R.dst(ref["dx"].shape, accumulate)
        ws = R.out((nb,))
        H.call("vx_conv_mfma_bwd_data", H.P(dy), H.P(w), dx.ptr, ws.ptr, B, Cin, D, Hh, W, Cout, K, S, P, accumulate, R.st)
        checks.append((dx.t, ref["dx"] + p, f"input gradient accumulate={accumulate}"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")
    if writes:
        bits, want = int(mx.t.view(torch.int32)[0]), int(t["x"].abs().max().view(torch.int32))
        assert bits == want, f"{R.what}: x_absmax holds {bits:#x}, the bits of max |x| are {want:#x}"
    return writes


@pytest.mark.parametrize("row", E.rows("mfma"), ids=E.ids("mfma"))
def test_conv_mfma(row):
    """vx_conv_mfma_fwd, _fwd_mx and _bwd_data (accumulate 0 and 1) with NaN workspaces of exactly vx_conv_mfma_ws_floats"""
    _mfma_case(_H(), "mfma", row)


@pytest.mark.parametrize("row", E.rows("stem"), ids=E.ids("stem"))
def test_conv_mfma_stem_on_the_f16_pipe(row):
    """the k7 s4 stem: two scaled fp16 pieces, one piece (which also brings 4 input channels in), and the fp32 gather kernel behind vx_conv_mfma_set_stem_f16(0);
    where vx_conv_mfma_fwd_writes_absmax answers 1 the word left at x_absmax is the bits of max |x|"""
    H = _H()
    f16, pieces = row["knobs"]
    with knob(H, "vx_conv_mfma_set_stem_f16", f16, 1), knob(H, "vx_conv_mfma_set_stem_pieces", pieces, 2, getter="vx_conv_mfma_stem_pieces"):
        writes = _mfma_case(H, "stem", row)
    assert writes == (1 if f16 else 0)


# ====================================================================================================================== D. weight gradients on MFMA
@pytest.mark.parametrize("row", E.rows("gather"), ids=E.ids("gather"))
def test_conv_wgrad_gather_mfma(row):
    H = _H()
    t, ref = E.inputs("gather", row), E.reference("gather", row)
    R = Run(H, f"gather {row['id']}")
    B, Cin, Cout, (D, Hh, W), K, S, P = row["B"], row["Cin"], row["Cout"], row["sp"], row["K"], row["S"], row["P"]
    assert H.query("vx_conv_wgrad_gather_ok", B, Cin, D, Hh, W, Cout, K, S, P) == 1
    x, dy = cu(t["x"]), cu(t["dy"])
    checks = []
    for with_db in (True, False):
        dw, pw = R.acc(ref["dw"].shape)
        db, pb = R.acc(ref["db"].shape) if with_db else (None, None)
        H.call("vx_conv_wgrad_gather_mfma", H.P(x), H.P(dy), dw.ptr, db.ptr if db else None, B, Cin, D, Hh, W, Cout, K, S, P, R.st)
        checks.append((dw.t, ref["dw"] + pw, f"dw (db {'given' if with_db else 'NULL'})"))
        if db:
            checks.append((db.t, ref["db"] + pb, "db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", E.rows("down_wgrad"), ids=E.ids("down_wgrad"))
def test_down_wgrad_mfma(row):
    """the stem weight gradient: vx_down_wgrad_mfma (x_absmax found here) and vx_down_wgrad_mfma_mx with max |x| handed over from vx_conv_mfma_fwd_mx where the
    forward writes it; the workspace has exactly vx_down_wgrad_ws_floats floats, NaN-filled"""
    H = _H()
    t, ref = E.inputs("down_wgrad", row), E.reference("down_wgrad", row)
    R = Run(H, f"down_wgrad {row['id']}")
    B, Cin, Cout, (D, Hh, W) = row["B"], row["Cin"], row["Cout"], row["sp"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    checks = []
    with knob(H, "vx_down_wgrad_set_f16", row["f16"], 1):
        nws = H.query("vx_down_wgrad_ws_floats", B, Cin, D, Hh, W, Cout)
        assert nws > 0
        for with_db in (True, False):
            dw, pw = R.acc(ref["dw"].shape)
            db, pb = R.acc(ref["db"].shape) if with_db else (None, None)
            ws = R.out((nws,))
            rc = H.query("vx_down_wgrad_mfma", H.P(x), H.P(dy), dw.ptr, db.ptr if db else None, ws.ptr, nws, B, Cin, D, Hh, W, Cout, R.st)
            assert rc == 0
            checks.append((dw.t, ref["dw"] + pw, f"dw (db {'given' if with_db else 'NULL'})"))
            if db:
                checks.append((db.t, ref["db"] + pb, "db"))
        if H.query("vx_conv_mfma_fwd_writes_absmax", Cin, Cout, D, Hh, W, 7, 4, 3):
            y, wsf, mx = R.out(ref["y"].shape), R.out((H.query("vx_conv_mfma_ws_floats", Cin, Cout, 7, 0),)), R.out((1,))
            H.call("vx_conv_mfma_fwd_mx", H.P(x), H.P(w), H.P(b), y.ptr, wsf.ptr, mx.ptr, B, Cin, D, Hh, W, Cout, 7, 4, 3, R.st)
            dw, pw = R.acc(ref["dw"].shape)
            db, pb = R.acc(ref["db"].shape)
            ws = R.out((nws,))
            rc = H.query("vx_down_wgrad_mfma_mx", H.P(x), H.P(dy), dw.ptr, db.ptr, ws.ptr, nws, mx.ptr, B, Cin, D, Hh, W, Cout, R.st)
            assert rc == 0
            checks += [(dw.t, ref["dw"] + pw, "dw (_mx, max |x| from the forward)"), (db.t, ref["db"] + pb, "db (_mx)")]
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", E.rows("jlc_gather"), ids=E.ids("jlc_gather"))
def test_jlc_wgrad_gather(row):
    """the three grouped weight gradients (k = 1, 3, 5) of a JLC block in one launch, += into integer prefills"""
    H = _H()
    t, ref = E.inputs("jlc_gather", row), E.reference("jlc_gather", row)
    R = Run(H, f"jlc_gather {row['id']}")
    B, C, G, (D, Hh, W) = row["B"], row["C"], row["G"], row["sp"]
    assert H.query("vx_jlc_wgrad_gather_ok", C, G, D, Hh, W) == 1
    d = {n: cu(v) for n, v in t.items()}
    dws = {k: R.acc(ref[f"dw{k}"].shape) for k in (1, 3, 5)}
    H.call("vx_jlc_wgrad_gather", H.P(d["x"]), H.P(d["g1"]), H.P(d["g3"]), H.P(d["g5"]), dws[1][0].ptr, dws[3][0].ptr, dws[5][0].ptr, B, C, G, D, Hh, W, R.st)
    R.done()
    for k in (1, 3, 5):
        E.exact(dws[k][0].t, ref[f"dw{k}"] + dws[k][1], f"{R.what} dw{k}")


@pytest.mark.parametrize("row", E.rows("gconv1"), ids=E.ids("gconv1"))
def test_gconv1_bwd_weight(row):
    H = _H()
    t, ref = E.inputs("gconv1", row), E.reference("gconv1", row)
    R = Run(H, f"gconv1 {row['id']}")
    B, C, G, V = row["B"], row["Cin"], row["G"], row["sp"][2]
    x, dy = cu(t["x"]), cu(t["dy"])
    checks = []
    for with_db in (True, False):
        dw, pw = R.acc((C, C // G))
        db, pb = R.acc((C,)) if with_db else (None, None)
        H.call("vx_gconv1_bwd_weight", H.P(x), H.P(dy), dw.ptr, db.ptr if db else None, B, C, G, V, R.st)
        checks.append((dw.t, ref["dw"].reshape(C, C // G) + pw, f"dw (db {'given' if with_db else 'NULL'})"))
        if db:
            checks.append((db.t, ref["db"] + pb, "db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


# ====================================================================================================================== E. 1x1 products
def _pw(fam, row):
    t, ref = E.inputs(fam, row), E.reference(fam, row)
    B, Cin, Cout, V, C1 = row["B"], row["Cin"], row["Cout"], row["sp"][2], row["C1"]
    flat = lambda v: v.reshape(v.shape[0], v.shape[1], V)
    x, dy = flat(t["x"]), flat(t["dy"])
    r = dict(y=flat(ref["y"]), dx=flat(ref["dx"]), dw=ref["dw"].reshape(Cout, Cin), db=ref["db"])
    return x, dy, t["w"].reshape(Cout, Cin), t["b"], r, (B, Cin, Cout, V, C1)


def _pw_rows(entry):
    rows = [r for r in E.rows("pw") if entry in r["on"]]
    return dict(argvalues=rows, ids=[r["id"] for r in rows])


@pytest.mark.parametrize("v4", [1, 0], ids=["v4_on", "v4_off"])
@pytest.mark.parametrize("row", **_pw_rows("fwd"))
def test_pw_conv_fwd(row, v4):
    H = _H()
    x, dy, w, b, ref, (B, Cin, Cout, V, C1) = _pw("pw", row)
    R = Run(H, f"pw fwd {row['id']} v4={v4}")
    x1, x2 = (cu(v) for v in split(x, C1))
    y = R.out((B, Cout, V))
    with knob(H, "vx_pw_conv_set_v4", v4, 1):
        H.call("vx_pw_conv_fwd", H.P(x1), H.P(x2), C1, H.P(R.dev(w)), H.P(R.dev(b)), y.ptr, B, Cin, Cout, V, R.st)
    R.done()
    E.exact(y.t, ref["y"], R.what)


@pytest.mark.parametrize("row", **_pw_rows("bwd_data"))
def test_pw_conv_bwd_data(row):
    H = _H()
    x, dy, w, b, ref, (B, Cin, Cout, V, C1) = _pw("pw", row)
    R = Run(H, f"pw bwd_data {row['id']}")
    c1 = C1 or Cin
    checks = []
    for accumulate in (0, 1):
        d1, p1 = R.dst((B, c1, V), accumulate)
        d2, p2 = R.dst((B, Cin - c1, V), accumulate) if C1 else (None, None)
        H.call("vx_pw_conv_bwd_data", H.P(R.dev(dy)), H.P(R.dev(w)), d1.ptr, d2.ptr if d2 else None, C1, B, Cin, Cout, V, accumulate, R.st)
        checks.append((d1.t, ref["dx"][:, :c1] + p1, f"dx accumulate={accumulate}"))
        if d2:
            checks.append((d2.t, ref["dx"][:, c1:] + p2, f"dx2 accumulate={accumulate}"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", **_pw_rows("bwd_weight"))
def test_pw_conv_bwd_weight(row):
    H = _H()
    x, dy, w, b, ref, (B, Cin, Cout, V, C1) = _pw("pw", row)
    R = Run(H, f"pw bwd_weight {row['id']}")
    x1, x2 = (cu(v) for v in split(x, C1))
    checks = []
    for with_db in (True, False):
        dw, pw = R.acc((Cout, Cin))
        db, pb = R.acc((Cout,)) if with_db else (None, None)
        H.call("vx_pw_conv_bwd_weight", H.P(x1), H.P(x2), C1, H.P(R.dev(dy)), dw.ptr, db.ptr if db else None, B, Cin, Cout, V, R.st)
        checks.append((dw.t, ref["dw"] + pw, f"dw (db {'given' if with_db else 'NULL'})"))
        if db:
            checks.append((db.t, ref["db"] + pb, "db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("wide", [1, 0], ids=["wide", "narrow"])
@pytest.mark.parametrize("row", **_pw_rows("mfma"))
def test_pw_conv_mfma(row, wide):
    """transpose_w 0 (forward from a concat source, bias) and 1 (input gradient into a split destination), accumulate 0 and 1, vx_pw_mfma_set_wide 0 and 1"""
    H = _H()
    x, dy, w, b, ref, (B, Cin, Cout, V, C1) = _pw("pw", row)
    R = Run(H, f"pw mfma {row['id']} wide={wide}")
    x1, x2 = (cu(v) for v in split(x, C1))
    c1 = C1 or Cin
    wd, bd, dyd = cu(w), cu(b), cu(dy)
    checks = []
    with knob(H, "vx_pw_mfma_set_wide", wide, 1):
        for accumulate in (0, 1):
            y, p = R.dst((B, Cout, V), accumulate)
            H.call("vx_pw_conv_mfma", H.P(x1), H.P(x2), C1, H.P(wd), 0, H.P(bd), y.ptr, None, 0, B, Cout, Cin, Cin, V, accumulate, R.st)
            checks.append((y.t, ref["y"] + p, f"forward accumulate={accumulate}"))
            d1, p1 = R.dst((B, c1, V), accumulate)
            d2, p2 = R.dst((B, Cin - c1, V), accumulate) if C1 else (None, None)
            H.call("vx_pw_conv_mfma", H.P(dyd), None, 0, H.P(wd), 1, None, d1.ptr, d2.ptr if d2 else None, C1, B, Cin, Cout, Cin, V, accumulate, R.st)
            checks.append((d1.t, ref["dx"][:, :c1] + p1, f"input gradient accumulate={accumulate}"))
            if d2:
                checks.append((d2.t, ref["dx"][:, c1:] + p2, f"input gradient (second tensor) accumulate={accumulate}"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


def _pw_fused(entry, row):
    H = _H()
    x, dy, w, b, ref, (B, Cin, Cout, V, C1) = _pw("pw", row)
    R = Run(H, f"{entry} {row['id']}")
    x1, x2 = (cu(v) for v in split(x, C1))
    c1 = C1 or Cin
    checks = []
    for accumulate in (0, 1):
        d1, p1 = R.dst((B, c1, V), accumulate)
        d2, p2 = R.dst((B, Cin - c1, V), accumulate) if C1 else (None, None)
        dw, pw = R.acc((Cout, Cin))
        db, pb = R.acc((Cout,)) if accumulate == 0 else (None, None)          # (db given once, NULL once)
        H.call(entry, H.P(R.dev(dy)), H.P(R.dev(w)), H.P(x1), H.P(x2), C1, d1.ptr, d2.ptr if d2 else None, dw.ptr, db.ptr if db else None, B, Cin, Cout, V, accumulate, R.st)
        checks.append((d1.t, ref["dx"][:, :c1] + p1, f"dx accumulate={accumulate}"))
        if d2:
            checks.append((d2.t, ref["dx"][:, c1:] + p2, f"dx2 accumulate={accumulate}"))
        checks.append((dw.t, ref["dw"] + pw, f"dw accumulate={accumulate}"))
        if db:
            checks.append((db.t, ref["db"] + pb, "db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", **_pw_rows("fused"))
def test_pw_conv_bwd_fused(row):
    _pw_fused("vx_pw_conv_bwd_fused", row)


@pytest.mark.parametrize("row", **_pw_rows("fused_big"))
def test_pw_conv_bwd_fused_big(row):
    _pw_fused("vx_pw_conv_bwd_fused_big", row)


@pytest.mark.parametrize("row", E.rows("pw_group"), ids=E.ids("pw_group"))
def test_pw_wgrad_group(row):
    """three weight-gradient jobs of different (Cin, Cout, V, B) (one with db NULL) and one fold of integer partial rows in ONE launch"""
    H = _H()
    t, ref = E.inputs("pw_group", row), E.reference("pw_group", row)
    R = Run(H, f"pw_group {row['id']}")
    d = {n: cu(v) for n, v in t.items()}
    ptrs, dims, outs = [], [], []
    for j, (ci, co, V, B) in enumerate(row["jobs"]):
        dw, pw = R.acc((co, ci))
        db, pb = R.acc((co,)) if j != 1 else (None, None)
        ptrs += [H.P(d[f"x{j}"]), H.P(d[f"dy{j}"]), dw.ptr, db.ptr if db else None]
        dims += [ci, co, V, B]
        outs.append((dw.t, ref[f"dw{j}"] + pw, f"dw of job {j}"))
        if db:
            outs.append((db.t, ref[f"db{j}"] + pb, f"db of job {j}"))
    C, nrows = row["fold"]
    dg, pg = R.acc((C,))
    dbt, pbt = R.acc((C,))
    outs += [(dg.t, ref["dgamma"] + pg, "dgamma"), (dbt.t, ref["dbeta"] + pbt, "dbeta")]
    P_ = (ctypes.c_void_p * len(ptrs))(*ptrs)
    D_ = (ctypes.c_long * len(dims))(*dims)
    FP = (ctypes.c_void_p * 3)(H.P(d["part"]), dg.ptr, dbt.ptr)
    FD = (ctypes.c_int * 2)(C, nrows)
    H.call("vx_pw_wgrad_group", ctypes.addressof(P_), ctypes.addressof(D_), len(row["jobs"]), ctypes.addressof(FP), ctypes.addressof(FD), 1, R.st)
    R.done()
    for got, want, tag in outs:
        E.exact(got, want, f"{R.what} {tag}")


# ====================================================================================================================== F. ConvTranspose3d k2 s2
@pytest.mark.parametrize("mfma4", [1, 0], ids=["mfma4_on", "mfma4_off"])
@pytest.mark.parametrize("row", E.rows("upconv"), ids=E.ids("upconv"))
def test_upconv_k2s2(row, mfma4):
    """forward, input gradient, and (Ci, Co multiples of 16) the weight gradient; vx_channel_sum gives db"""
    H = _H()
    t, ref = E.inputs("upconv", row), E.reference("upconv", row)
    R = Run(H, f"upconv {row['id']} mfma4={mfma4}")
    B, Ci, Co, (d_, h_, w_) = row["B"], row["Ci"], row["Co"], row["sp"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    checks = []
    with knob(H, "vx_upconv_set_mfma4", mfma4, 1):
        y = R.out(ref["y"].shape)
        H.call("vx_upconv_k2s2_fwd", H.P(x), H.P(w), H.P(b), y.ptr, B, Ci, Co, d_, h_, w_, R.st)
        checks.append((y.t, ref["y"], "forward"))
        dx = R.out(ref["dx"].shape)
        H.call("vx_upconv_k2s2_bwd_data", H.P(dy), H.P(w), dx.ptr, B, Ci, Co, d_, h_, w_, R.st)
        checks.append((dx.t, ref["dx"], "input gradient"))
        if row["wgrad"]:
            assert H.query("vx_upconv_k2s2_wgrad_ok", Ci, Co) == 1
            dw, pw = R.acc(ref["dw"].shape)
            H.call("vx_upconv_k2s2_wgrad", H.P(x), H.P(dy), dw.ptr, B, Ci, Co, d_, h_, w_, R.st)
            checks.append((dw.t, ref["dw"] + pw, "dw"))
        db, pb = R.acc((Co,))
        H.call("vx_channel_sum", H.P(dy), db.ptr, B, Co, 8 * d_ * h_ * w_, R.st)
        checks.append((db.t, ref["db"] + pb, "db (vx_channel_sum)"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


# ====================================================================================================================== G. patch-expand
def _expand_rows(declined):
    rows = [r for r in E.rows("expand") if r["id"].endswith("declined") == declined]
    return dict(argvalues=rows, ids=[r["id"] for r in rows])


@pytest.mark.parametrize("wlds", [1, 0], ids=["wlds_on", "wlds_off"])
@pytest.mark.parametrize("row", **_expand_rows(False))
def test_expand_fwd_mfma(row, wlds):
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand fwd {row['id']} wlds={wlds}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    y, ws = R.out(ref["y"].shape), R.out((64 * Cc * 16 * 27,))
    with knob(H, "vx_expand_set_fwd_wlds", wlds, 1):
        rc = H.query("vx_expand_fwd_mfma", H.P(R.dev(t["x"])), H.P(R.dev(t["w"])), H.P(R.dev(t["b"])), ws.ptr, y.ptr, B, Cc, D, Hh, W, R.st)
    R.done()
    assert rc == 0
    E.exact(y.t, ref["y"], R.what)


@pytest.mark.parametrize("lds", [1, 2, 0], ids=["lds_halo_and_weights", "lds_halo", "lds_off"])
@pytest.mark.parametrize("row", E.rows("expand"), ids=E.ids("expand"))
def test_expand_bwd_data_mfma(row, lds):
    """accumulate 0 and 1 under every vx_expand_set_lds mode; at 3 x 5 x 6 every mode takes the general kernel, which must be exact there"""
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand bwd_data {row['id']} lds={lds}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    dy, w = cu(t["dy"]), cu(t["w"])
    checks = []
    with knob(H, "vx_expand_set_lds", lds, 1):
        for accumulate in (0, 1):
            dx, p = R.dst(ref["dx"].shape, accumulate)
            ws = R.out((64 * Cc * 16 * 27,))
            H.call("vx_expand_bwd_data_mfma", H.P(dy), H.P(w), ws.ptr, dx.ptr, B, Cc, D, Hh, W, accumulate, R.st)
            checks.append((dx.t, ref["dx"] + p, f"accumulate={accumulate}"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", E.rows("expand"), ids=E.ids("expand"))
def test_expand_wgrad_mfma(row):
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand wgrad {row['id']}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    x, dy = cu(t["x"]), cu(t["dy"])
    checks = []
    for with_db in (True, False):
        dw, pw = R.acc(ref["dw"].shape)
        db, pb = R.acc(ref["db"].shape) if with_db else (None, None)
        xcl = R.out((B * D * Hh * W * 16,))
        H.call("vx_expand_wgrad_mfma", H.P(x), xcl.ptr, H.P(dy), dw.ptr, db.ptr if db else None, B, Cc, D, Hh, W, R.st)
        checks.append((dw.t, ref["dw"] + pw, f"dw (db {'given' if with_db else 'NULL'})"))
        if db:
            checks.append((db.t, ref["db"] + pb, "db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("ns", [2, 3, 22])
@pytest.mark.parametrize("row", **_expand_rows(False))
def test_expand_split_forward_and_input_gradient(row, ns):
    """vx_expand_fwd_mfma_split / vx_expand_bwd_data_mfma_split: ns bf16 pieces (2, 3) or two scaled fp16 pieces (22) per operand -- a small integer is its own
    first piece and the scales are powers of two, so the products are exact; workspace of exactly vx_expand_split_ws_floats, NaN-filled; accumulate 0 and 1"""
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand split {row['id']} ns={ns}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    nws = H.query("vx_expand_split_ws_floats", Cc, ns)
    y, ws = R.out(ref["y"].shape), R.out((nws,))
    rcs = [H.query("vx_expand_fwd_mfma_split", H.P(x), H.P(w), H.P(b), ws.ptr, y.ptr, B, Cc, D, Hh, W, ns, R.st)]
    checks = [(y.t, ref["y"], "forward")]
    for accumulate in (0, 1):
        dx, p = R.dst(ref["dx"].shape, accumulate)
        ws = R.out((nws,))
        rcs.append(H.query("vx_expand_bwd_data_mfma_split", H.P(dy), H.P(w), ws.ptr, dx.ptr, B, Cc, D, Hh, W, accumulate, ns, R.st))
        checks.append((dx.t, ref["dx"] + p, f"input gradient accumulate={accumulate}"))
    R.done()
    assert rcs == [0, 0, 0]
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", **_expand_rows(False))
def test_expand_split22_prepared_chain(row):
    """vx_expand_prep_split22, then the matrix kernels alone on the prepared images (forward, input gradient with accumulate 0 and 1), then
    vx_expand_bwd_data_mfma_split_ew taking the weight scale word the forward left"""
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand prepared {row['id']}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    nws, ewo = H.query("vx_expand_split_ws_floats", Cc, 22), H.query("vx_expand_split_ew_offset", Cc)
    wf, wb = R.out((nws,)), R.out((nws,))
    H.call("vx_expand_prep_split22", H.P(w), wf.ptr, wb.ptr, Cc, R.st)
    y = R.out(ref["y"].shape)
    rcs = [H.query("vx_expand_fwd_mfma_split_prepared", H.P(x), H.P(b), wf.ptr, y.ptr, B, Cc, D, Hh, W, R.st)]
    checks = [(y.t, ref["y"], "forward on prepared images")]
    for accumulate in (0, 1):
        dx, p = R.dst(ref["dx"].shape, accumulate)
        rcs.append(H.query("vx_expand_bwd_data_mfma_split_prepared", H.P(dy), wb.ptr, wf.ptr + 4 * ewo, dx.ptr, B, Cc, D, Hh, W, accumulate, R.st))
        checks.append((dx.t, ref["dx"] + p, f"input gradient on prepared images accumulate={accumulate}"))
    dx, ws = R.out(ref["dx"].shape), R.out((nws,))
    rcs.append(H.query("vx_expand_bwd_data_mfma_split_ew", H.P(dy), H.P(w), ws.ptr, dx.ptr, B, Cc, D, Hh, W, 0, 22, wf.ptr + 4 * ewo, R.st))
    checks.append((dx.t, ref["dx"], "input gradient (_ew)"))
    R.done()
    assert rcs == [0, 0, 0, 0]
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("ns", [1, 2, 3])
@pytest.mark.parametrize("row", **_expand_rows(False))
def test_expand_wgrad_mfma_split(row, ns):
    """partial-sum workspace of exactly vx_expand_wgrad_split_ws_floats floats, NaN-filled: every row that is folded must have been written"""
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand wgrad split {row['id']} ns={ns}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    nws = H.query("vx_expand_wgrad_split_ws_floats", B, Cc, D, Hh, W)
    dw, pw = R.acc(ref["dw"].shape)
    db, pb = R.acc(ref["db"].shape)
    ws = R.out((nws,))
    rc = H.query("vx_expand_wgrad_mfma_split", H.P(R.dev(t["x"])), H.P(R.dev(t["dy"])), dw.ptr, db.ptr, ws.ptr, nws, B, Cc, D, Hh, W, ns, R.st)
    R.done()
    assert rc == 0
    E.exact(dw.t, ref["dw"] + pw, f"{R.what} dw")
    E.exact(db.t, ref["db"] + pb, f"{R.what} db")


@pytest.mark.parametrize("row", **_expand_rows(False))
def test_expand_bf16_operands(row):
    """vx_expand_fwd_mfma_bf16 / vx_expand_bwd_data_mfma_bf16: operands rounded to bf16 -- small integers are unchanged --, fp32 accumulation"""
    H = _H()
    t, ref = E.inputs("expand", row), E.reference("expand", row)
    R = Run(H, f"expand bf16 {row['id']}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    nws = 64 * Cc * 16 * 27
    y, ws = R.out(ref["y"].shape), R.out((nws,))
    rcs = [H.query("vx_expand_fwd_mfma_bf16", H.P(x), H.P(w), H.P(b), ws.ptr, y.ptr, B, Cc, D, Hh, W, R.st)]
    checks = [(y.t, ref["y"], "forward")]
    for accumulate in (0, 1):
        dx, p = R.dst(ref["dx"].shape, accumulate)
        ws = R.out((nws,))
        rcs.append(H.query("vx_expand_bwd_data_mfma_bf16", H.P(dy), H.P(w), ws.ptr, dx.ptr, B, Cc, D, Hh, W, accumulate, R.st))
        checks.append((dx.t, ref["dx"] + p, f"input gradient accumulate={accumulate}"))
    R.done()
    assert rcs == [0, 0, 0]
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


@pytest.mark.parametrize("row", **_expand_rows(True))
def test_expand_entries_decline_and_write_nothing(row):
    """D, H or W no multiple of 4: the MFMA forward, the bf16 pair, the split pair and (W % 4 != 0) the split weight gradient return 1 and leave every buffer as it was"""
    H = _H()
    t = E.inputs("expand", row)
    R = Run(H, f"expand declined {row['id']}")
    B, Cc, (D, Hh, W) = row["B"], row["Cc"], row["sp"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    nws = max(64 * Cc * 16 * 27, H.query("vx_expand_split_ws_floats", Cc, 22))
    rcs = {}
    for name in ("vx_expand_fwd_mfma", "vx_expand_fwd_mfma_bf16"):
        y, ws = R.out(t["dy"].shape), R.out((nws,))
        rcs[name] = H.query(name, H.P(x), H.P(w), H.P(b), ws.ptr, y.ptr, B, Cc, D, Hh, W, R.st)
    dx, ws = R.out(t["x"].shape), R.out((nws,))
    rcs["vx_expand_bwd_data_mfma_bf16"] = H.query("vx_expand_bwd_data_mfma_bf16", H.P(dy), H.P(w), ws.ptr, dx.ptr, B, Cc, D, Hh, W, 0, R.st)
    for ns in (2, 3, 22):
        y, ws = R.out(t["dy"].shape), R.out((nws,))
        rcs[f"vx_expand_fwd_mfma_split ns={ns}"] = H.query("vx_expand_fwd_mfma_split", H.P(x), H.P(w), H.P(b), ws.ptr, y.ptr, B, Cc, D, Hh, W, ns, R.st)
        dx, ws = R.out(t["x"].shape), R.out((nws,))
        rcs[f"vx_expand_bwd_data_mfma_split ns={ns}"] = H.query("vx_expand_bwd_data_mfma_split", H.P(dy), H.P(w), ws.ptr, dx.ptr, B, Cc, D, Hh, W, 0, ns, R.st)
    dw, db, ws = R.out(t["w"].shape), R.out(t["b"].shape), R.out((64,))
    rcs["vx_expand_wgrad_mfma_split"] = H.query("vx_expand_wgrad_mfma_split", H.P(x), H.P(dy), dw.ptr, db.ptr, ws.ptr, 64, B, Cc, D, Hh, W, 3, R.st)
    R.done()
    assert all(rc == 1 for rc in rcs.values()), rcs
    for i, g in enumerate(R.guards):
        assert bool(torch.isnan(g.t).all()), f"{R.what}: a declined call wrote into buffer {i}"


# ====================================================================================================================== H. patch embedding
@pytest.mark.parametrize("row", E.rows("patchify"), ids=E.ids("patchify"))
def test_patchify(row):
    """K = 2, 3, 4; a whole tensor through vx_patchify, a channel slice of a wider one through vx_patchify_bs"""
    H = _H()
    t, ref = E.inputs("patchify", row), E.reference("patchify", row)
    R = Run(H, f"patchify {row['id']}")
    B, C, Ct, co, (d_, h_, w_), K = row["B"], row["C"], row["Ctot"], row["c_off"], row["grid"], row["K"]
    x = cu(t["x"])
    Vin = d_ * h_ * w_ * K ** 3
    o = R.out(ref["out"].shape)
    if Ct == C:
        H.call("vx_patchify", H.P(x), o.ptr, B, C, d_, h_, w_, K, R.st)
    else:
        H.call("vx_patchify_bs", x.data_ptr() + 4 * co * Vin, Ct * Vin, o.ptr, B, C, d_, h_, w_, K, R.st)
    R.done()
    E.exact(o.t, ref["out"], R.what)


@pytest.mark.parametrize("row", E.rows("patch_embed"), ids=E.ids("patch_embed"))
def test_patch_embed(row):
    """vx_patch_embed_fwd / _bwd_weight reading a channel slice in place (batch stride larger than the slice)"""
    H = _H()
    t, ref = E.inputs("patch_embed", row), E.reference("patch_embed", row)
    R = Run(H, f"patch_embed {row['id']}")
    B, Cin, Ct, co, Cout, (d_, h_, w_) = row["B"], row["Cin"], row["Ctot"], row["c_off"], row["Cout"], row["grid"]
    x, w, b, dy = cu(t["x"]), cu(t["w"]), cu(t["b"]), cu(t["dy"])
    Vin = 64 * d_ * h_ * w_
    xp, bstride = x.data_ptr() + 4 * co * Vin, Ct * Vin
    y = R.out(ref["y"].shape)
    H.call("vx_patch_embed_fwd", xp, bstride, H.P(w), H.P(b), y.ptr, B, Cin, Cout, d_, h_, w_, R.st)
    checks = [(y.t, ref["y"], "forward")]
    for with_db in (True, False):
        dw, pw = R.acc(ref["dw"].shape)
        db, pb = R.acc(ref["db"].shape) if with_db else (None, None)
        H.call("vx_patch_embed_bwd_weight", xp, bstride, H.P(dy), dw.ptr, db.ptr if db else None, B, Cin, Cout, d_, h_, w_, R.st)
        checks.append((dw.t, ref["dw"] + pw, f"dw (db {'given' if with_db else 'NULL'})"))
        if db:
            checks.append((db.t, ref["db"] + pb, "db"))
    R.done()
    for got, want, tag in checks:
        E.exact(got, want, f"{R.what} {tag}")


# ====================================================================================================================== I. small linear pieces
@pytest.mark.parametrize("row", E.rows("add"), ids=E.ids("add"))
def test_add_and_add_many(row):
    """16 tensors of 1, 5, 1023, ... floats in one vx_add_many launch, some without a third operand; the same sums one by one through vx_add"""
    H = _H()
    t, ref = E.inputs("add", row), E.reference("add", row)
    R = Run(H, f"add {row['id']}")
    d = {n: cu(v) for n, v in t.items()}
    k = len(row["n"])
    many, single = [R.out((n,)) for n in row["n"]], [R.out((n,)) for n in row["n"]]
    arr = lambda vals: (ctypes.c_void_p * k)(*vals)
    a, b = arr([H.P(d[f"a{j}"]) for j in range(k)]), arr([H.P(d[f"b{j}"]) for j in range(k)])
    c = arr([H.P(d.get(f"c{j}")) for j in range(k)])
    o = arr([g.ptr for g in many])
    n = (ctypes.c_long * k)(*row["n"])
    H.call("vx_add_many", ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c), ctypes.addressof(o), ctypes.addressof(n), k, R.st)
    for j in range(k):
        H.call("vx_add", H.P(d[f"a{j}"]), H.P(d[f"b{j}"]), H.P(d.get(f"c{j}")), single[j].ptr, row["n"][j], R.st)
    R.done()
    for j in range(k):
        E.exact(many[j].t, ref[f"out{j}"], f"{R.what} vx_add_many tensor {j}")
        E.exact(single[j].t, ref[f"out{j}"], f"{R.what} vx_add tensor {j}")


@pytest.mark.parametrize("row", E.rows("channel_sum"), ids=E.ids("channel_sum"))
def test_channel_sum(row):
    H = _H()
    t, ref = E.inputs("channel_sum", row), E.reference("channel_sum", row)
    R = Run(H, f"channel_sum {row['id']}")
    db, p = R.acc((row["C"],))
    H.call("vx_channel_sum", H.P(R.dev(t["dy"])), db.ptr, row["B"], row["C"], row["V"], R.st)
    R.done()
    E.exact(db.t, ref["db"] + p, R.what)


@pytest.mark.parametrize("row", E.rows("s2d"), ids=E.ids("s2d"))
def test_space_to_depth2_both_directions(row):
    H = _H()
    t, ref = E.inputs("s2d", row), E.reference("s2d", row)
    R = Run(H, f"s2d {row['id']}")
    B, C, (d_, h_, w_) = row["B"], row["C"], row["sp"]
    out, inv = R.out(ref["out"].shape), R.out(ref["inv"].shape)
    H.call("vx_space_to_depth2", H.P(R.dev(t["x"])), out.ptr, B, C, d_, h_, w_, 0, R.st)
    H.call("vx_space_to_depth2", H.P(R.dev(t["z"])), inv.ptr, B, C, d_, h_, w_, 1, R.st)
    R.done()
    E.exact(out.t, ref["out"], f"{R.what} forward")
    E.exact(inv.t, ref["inv"], f"{R.what} inverse")


@pytest.mark.parametrize("row", E.rows("gram"), ids=E.ids("gram"))
def test_gram(row):
    """C V a power of two: the normalisation 1 / (C V) is exact"""
    H = _H()
    t, ref = E.inputs("gram", row), E.reference("gram", row)
    R = Run(H, f"gram {row['id']}")
    B, C, V = row["B"], row["C"], row["sp"][0] * row["sp"][1] * row["sp"][2]
    x = cu(t["x"])
    G_, dx = R.out(ref["G"].shape), R.out(ref["dx"].shape)
    H.call("vx_gram_fwd", H.P(x), G_.ptr, B, C, V, R.st)
    H.call("vx_gram_bwd", H.P(x), H.P(R.dev(t["dG"])), dx.ptr, B, C, V, R.st)
    R.done()
    E.exact(G_.t, ref["G"], f"{R.what} G")
    E.exact(dx.t, ref["dx"], f"{R.what} dx")


@pytest.mark.parametrize("row", E.rows("trilinear"), ids=E.ids("trilinear"))
def test_upsample_trilinear(row):
    """dyadic ratios: the align_corners weights are exact; the adjoint's workspace has exactly BC d (H W + h W) floats, NaN-filled"""
    H = _H()
    t, ref = E.inputs("trilinear", row), E.reference("trilinear", row)
    R = Run(H, f"trilinear {row['id']}")
    BC, (d_, h_, w_), (D, Hh, W) = row["BC"], row["lo"], row["hi"]
    out, dx, ws = R.out(ref["out"].shape), R.out(ref["dx"].shape), R.out((BC * d_ * (Hh * W + h_ * W),))
    H.call("vx_upsample_trilinear_fwd", H.P(R.dev(t["x"])), out.ptr, BC, d_, h_, w_, D, Hh, W, R.st)
    H.call("vx_upsample_trilinear_bwd", H.P(R.dev(t["dout"])), dx.ptr, ws.ptr, BC, d_, h_, w_, D, Hh, W, R.st)
    R.done()
    E.exact(out.t, ref["out"], f"{R.what} forward")
    E.exact(dx.t, ref["dx"], f"{R.what} adjoint")


@pytest.mark.parametrize("row", E.rows("sqdiff"), ids=E.ids("sqdiff"))
def test_sqdiff_sum(row):
    """vx_sqdiff_sum zeroes its accumulator (NaN prefill); vx_sqdiff_sum_bs adds into it (integer prefill: the contract says it is not zeroed)"""
    H = _H()
    t, ref = E.inputs("sqdiff", row), E.reference("sqdiff", row)
    R = Run(H, f"sqdiff {row['id']}")
    B, n = row["B"], row["n"]
    a, b = cu(t["a"]), cu(t["b"])
    acc0 = R.out((1,), torch.float64)
    H.call("vx_sqdiff_sum", H.P(a), H.P(R.dev(t["b"][:, :n])), B * n, acc0.ptr, R.st)
    acc1, p = R.acc((1,), torch.float64)
    H.call("vx_sqdiff_sum_bs", H.P(a), H.P(b), n, n + row["pad"], B, acc1.ptr, R.st)
    R.done()
    E.exact(acc0.t, ref["acc"], f"{R.what} vx_sqdiff_sum")
    E.exact(acc1.t, ref["acc"] + p, f"{R.what} vx_sqdiff_sum_bs")


@pytest.mark.parametrize("row", E.rows("axpy"), ids=E.ids("axpy"))
def test_axpy_drop_without_dropout(row):
    H = _H()
    t, ref = E.inputs("axpy", row), E.reference("axpy", row)
    R = Run(H, f"axpy {row['id']}")
    n, alpha = row["n"], row["alpha"]
    out, dx, dz = R.out((n,)), R.out((n,)), R.out((n,))
    H.call("vx_axpy_drop_fwd", H.P(R.dev(t["x"])), H.P(R.dev(t["z"])), out.ptr, alpha, n, None, 0, 0.0, R.st)
    H.call("vx_axpy_drop_bwd", H.P(R.dev(t["dout"])), dx.ptr, dz.ptr, alpha, n, None, 0, 0.0, R.st)
    R.done()
    for got, name in ((out, "out"), (dx, "dx"), (dz, "dz")):
        E.exact(got.t, ref[name], f"{R.what} {name}")
