"""The paired-window attention core against fp64 on sharp and shifted soft-max rows, straight through the C ABI (oracle, families, case table and
restatements: tests/attn_ref.py; their premises: tests/test_attn_ref_cpu.py).

Every case runs vx_pwa_attn_fwd (vx_pwa_attn_fwd_mb with dropout) and then vx_pwa_attn_bwd (_bwd_mb) on the O and LSE that forward just wrote, as the model does,
under the knobs of its row, and FIRST asserts through vx_pwa_attn_mfma_ok / vx_pwa_attn_bwd1_ok / vx_pwa_attn_bwd1h_ok that the row takes the forward and backward
path it names.  O, LSE, dQ, dK, dV and dtable (minus its prefill) are each held to

    max |got - ref64|  <=  FACTOR * max |ref32 - ref64|  +  FLOOR * max |ref64|          (tests/stable_ref.py: FACTOR 8 unless FACTORS names the path, FLOOR 16 * 2^-24)

Every destination and workspace is an exact_ref.Guard: O, LSE, dQ, dK, dV and the workspace start as NaN, dtable as integers in [-8, 8] that the reference adds
(the entry is `+=`: its one fp32 rounding at the size of the sum is added to the bound of dtable, see _round_slack), the keep-bit words between integer canaries.  Rows marked `nofold` run vx_pwa_attn_bwd_nofold(_mb) + vx_pwa_attn_bwd_fold as well: a return
of 1 must leave every prefill untouched, otherwise the folded dtable meets the same bound.  Knobs are restored in `finally`."""
import contextlib
import ctypes

import pytest
import torch

import attn_ref as A
import exact_ref as E
from exact_ref import Guard

pytestmark = pytest.mark.gpu

BITS_CANARY = 0x5A5A


def _H():
    from veloxseg_amd import _hip as H
    H.LIB.load()
    return H


@contextlib.contextmanager
def knobs(H, values):
    try:
        for name, v in values.items():
            H.call(A.KNOBS[name][0], v)
        yield
    finally:
        for name in values:
            H.call(A.KNOBS[name][0], A.KNOBS[name][1])


class Run:
    """the guards and device operands of one case; done() synchronises and checks every canary"""

    def __init__(self, H, row, d):
        self.H, self.guards, self.keep, self.seed = H, [], [], A._seed(row["id"], 900)
        pl = d["pl"]
        self.plan = H.make_plan(row["grid"], pl["n"], row["heads"], pl["small"], pl["nwin"])
        self.pp, self.st = ctypes.addressof(self.plan), H.stream_ptr()

    def out(self, shape):
        self.guards.append(Guard(tuple(shape)))
        return self.guards[-1]

    def bits(self, n):
        self.guards.append(Guard((n,), torch.int16, fill=0, canary=BITS_CANARY))
        return self.guards[-1]

    def acc(self, shape):
        self.seed += 1
        p = E.prefill(*shape, seed=self.seed)
        self.guards.append(Guard(tuple(shape), fill=p))
        return self.guards[-1], p.double()

    def dev(self, t):
        self.keep.append(t.contiguous().cuda())
        return self.keep[-1]

    def done(self, what):
        torch.cuda.synchronize()
        for i, g in enumerate(self.guards):
            g.check(f"{what} (buffer {i})")


def _assert_paths(H, row, a):
    """the row takes the forward and the backward path it names, by the library's own answers"""
    mf = H.query("vx_pwa_attn_mfma_ok", *a)
    got = (H.query("vx_pwa_attn_bwd1h_ok", *a), H.query("vx_pwa_attn_bwd1_ok", *a), mf & 2)
    want = A.BWD_PATHS[row["path"]]
    assert all(w is None or w == g for w, g in zip(want, got)), f"{row['id']}: backward path {row['path']} wants (bwd1h_ok, bwd1_ok, mfma_ok & 2) = {want}, the library answers {got}"
    assert (mf & 1) == A.FWD_PATHS[row["fwd"]], f"{row['id']}: forward path {row['fwd']}, vx_pwa_attn_mfma_ok answers {mf}"
    l = row["big"][0] * row["big"][1] * row["big"][2]
    assert (row["path"] == "f16_aligned") == (got[0] == 1 and l % 64 == 0 and row["M"] == 2)
    assert (row["path"] == "f16_ragged") == (got[0] == 1 and l % 64 != 0)
    assert (row["path"] == "f16_m1") == (got[0] == 1 and row["M"] == 1)


def _hold(row, family, p, got, c, tag="", slack=0.0):
    """every tensor to the bound; the figures are printed (pytest -s) before anything is asserted.  `slack`: added to the bound of dtable (see ROUNDING OF `+=`)"""
    bad = []
    for name, g in got.items():
        op = f"attn_fwd_{row['fwd']}" if name in ("O", "LSE") else f"attn_bwd_{row['path']}"
        r64, r32 = c["r64"][name], c["r32"][name]
        assert not bool(torch.isnan(g).any()), f"{row['id']} {family}{tag} {name}: {int(torch.isnan(g).sum())} elements were never written (NaN prefill left)"
        e, e32, M = A.figures(g, r64, r32)
        lim = A.limit(e32, M, op) + (slack if name == "dtable" else 0.0)
        print(f"[fp64] {op} {row['id']} {family} p={p:g}{tag} {name}: err {e:.3e} ref32 {e32:.3e} M {M:.3e} ratio {e / e32 if e32 > 0 else float('nan'):.2f} "
              f"floor-units {e / (A.S.FLOOR * M) if M > 0 else float('nan'):.2f} bound-use {e / lim if lim > 0 else float('nan'):.3f}")
        if not e <= lim:
            bad.append(f"{row['id']} {family} p={p:g}{tag} {name} [{row['branch']}]: max|got-ref64| = {e:.3e} > bound {lim:.3e} (max|ref32-ref64| = {e32:.3e}, M = {M:.3e}, "
                       f"ratio {e / e32 if e32 > 0 else float('inf'):.1f})")
    assert not bad, "\n".join(bad)


def _round_slack(pre, r64):
    """ROUNDING OF `+=`: dtable leaves the kernels as fl(prefill + g) in fp32, one rounding at the size of the SUM: |err| <= 2^-24 max |prefill + g|.  With a prefill
    of up to 8 that is up to 4.8e-7 whatever the size of g, so it is added to the bound of `dtable minus its prefill`; where it exceeds the floor term of the plain
    bound (M below about 0.5: the `dO_small` family) the case repeats the backward into a ZERO prefill, where the addition is exact, and holds that to the plain bound"""
    return 2.0 ** -24 * float((pre + r64).abs().max())


@pytest.mark.parametrize("rid,family,p", A.CASES, ids=A.CASE_IDS)
def test_attention_core_against_fp64(rid, family, p):
    H = _H()
    row = A.ROW[rid]
    c = A.row_case(rid, family, p)
    d, inp = c["d"], c["inp"]
    B, M, h, Nt, ML, cq, cv = row["B"], row["M"], d["heads"], d["Nt"], d["ML"], d["cq"], d["cv"]
    run = Run(H, row, d)
    a = (run.pp, B, M, cq, cv)
    q, k, v, table, dO = (run.dev(inp[x]) for x in ("q", "k", "v", "table", "dO"))
    seed = run.dev(torch.tensor([A.SEED, A.STEP], dtype=torch.int64))
    sp = H.P(seed, torch.int64)
    with knobs(H, row["knobs"]):
        _assert_paths(H, row, a)
        mb = None
        if p > 0 and H.query("vx_pwa_attn_mbits_useful", *a) == 1:                   # (the model keeps the forward's bits exactly where this answers 1)
            mb = run.bits(H.query("vx_pwa_attn_mbits_words", run.pp, B, M))
        assert not (p > 0 and (row["path"].startswith("f16") or row["knobs"].get("valu_bits"))) or mb is not None, f"{rid}: this path reads the forward's keep bits"
        o, lse = run.out((B, h, Nt, ML, cv)), run.out((B, h, Nt, ML))
        if p > 0:
            H.call("vx_pwa_attn_fwd_mb", H.P(q), H.P(k), H.P(v), H.P(table), o.ptr, lse.ptr, *a, sp, A.SITE, p, mb.ptr if mb else None, run.st)
        else:
            H.call("vx_pwa_attn_fwd", H.P(q), H.P(k), H.P(v), H.P(table), o.ptr, lse.ptr, *a, sp, A.SITE, 0.0, run.st)
        nws = H.query("vx_pwa_attn_bwd_ws_floats", run.pp, B, M)

        def backward(entry, with_table, zero=False):
            dq, dk, dv, ws = run.out(q.shape), run.out(k.shape), run.out(v.shape), run.out((nws,))
            dt, pre = run.acc(table.shape)
            if zero:
                dt.t.zero_()
                pre = torch.zeros_like(pre)
            args = [H.P(q), H.P(k), H.P(v), H.P(table), o.ptr, lse.ptr, H.P(dO), dq.ptr, dk.ptr, dv.ptr] + ([dt.ptr] if with_table else []) + [ws.ptr, *a, sp, A.SITE, p]
            rc = H.query(entry + ("_mb" if p > 0 else ""), *args, *([mb.ptr if mb else None] if p > 0 else []), run.st)
            return rc, dq, dk, dv, dt, pre, ws

        rc, dq, dk, dv, dt, pre, _ = backward("vx_pwa_attn_bwd", True)
        assert rc == 0
        slack = _round_slack(pre, c["r64"]["dtable"])
        exact_add = None
        if slack > A.S.FLOOR * float(c["r64"]["dtable"].abs().max()):
            exact_add = backward("vx_pwa_attn_bwd", True, zero=True)
            assert exact_add[0] == 0
        nf = None
        if row["nofold"] and family == "plain":
            nf = backward("vx_pwa_attn_bwd_nofold", False)
            assert nf[0] in (0, 1)
            if nf[0] == 0:
                H.call("vx_pwa_attn_bwd_fold", nf[6].ptr, nf[4].ptr, run.pp, B, M, run.st)
    run.done(f"attention {rid} {family} p={p:g}")
    _hold(row, family, p, dict(O=o.t, LSE=lse.t, dQ=dq.t, dK=dk.t, dV=dv.t, dtable=dt.t.double().cpu() - pre), c, slack=slack)
    if exact_add is not None:
        _, dq0, dk0, dv0, dt0, _, _ = exact_add
        _hold(row, family, p, dict(dQ=dq0.t, dK=dk0.t, dV=dv0.t, dtable=dt0.t), c, tag=" (zero prefill)")
    if nf is not None:
        rc, dq2, dk2, dv2, dt2, pre2, ws2 = nf
        print(f"[fp64] {rid} {family} p={p:g}: vx_pwa_attn_bwd_nofold returned {rc}")
        if rc == 1:                                            # declined: nothing may have been written
            for name, g in (("dQ", dq2), ("dK", dk2), ("dV", dv2), ("workspace", ws2)):
                assert bool(torch.isnan(g.t).all()), f"{rid}: vx_pwa_attn_bwd_nofold declined, but wrote {name}"
            assert torch.equal(dt2.t.double().cpu(), pre2), f"{rid}: vx_pwa_attn_bwd_nofold declined, but the table gradient changed"
        else:
            _hold(row, family, p, dict(dQ=dq2.t, dK=dk2.t, dV=dv2.t, dtable=dt2.t.double().cpu() - pre2), c, tag=" (nofold + fold)", slack=_round_slack(pre2, c["r64"]["dtable"]))
