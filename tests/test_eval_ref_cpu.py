"""The premises of tests/test_eval_kernels_gpu.py, proved on the CPU for every row of the case tables in tests/eval_ref.py.  Each bound below is a condition on the
INPUTS (a badly chosen row fails here, not a kernel): rotation coordinates that fp32 evaluates exactly whatever the contraction, interpolated values that fp32
holds, nearest rows rich in .5 ties, border rows rich in clamped samples, confusion rows that fill every cell, arg-max rows rich in ties / NaNs / infinities /
signed zeros, and over-cap cases that really exceed the grid cap of the kernel they are for."""
import numpy as np
import pytest

import eval_ref as R


# ---------------------------------------------------------------------------------------------------------------------- arg-max
def test_argmax_rule_is_the_written_one():
    nan, inf = float("nan"), float("inf")
    cols = np.array([[1, 3, 3, 2], [nan, 5, nan, 1], [inf, nan, 0, 0], [-0.0, 0.0, -1, -1], [0.0, -0.0, -1, -1], [-inf, -inf, -inf, -inf], [2, 2, 2, 2], [inf, inf, 1, nan]], dtype=np.float32).T
    assert R.argmax_first(cols, axis=0).tolist() == [1, 0, 1, 0, 0, 0, 0, 3]
    assert R.argmax_first(np.array([[nan], [1.0]], dtype=np.float32).T, axis=0).tolist() == [0, 0]         # C = 1


def test_argmax_table_covers_the_stated_sizes():
    assert {r["B"] for r in R.ARGMAX_ROWS} == {1, 3} and {r["C"] for r in R.ARGMAX_ROWS} == {1, 2, 4, 256}
    assert {r["V"] for r in R.ARGMAX_ROWS} == {1, 255, 256, 257, 4099}
    assert len({r["id"] for r in R.ARGMAX_ROWS}) == len(R.ARGMAX_ROWS)
    r = R.ARGMAX_OVER_CAP
    assert r["V"] > R.GRID_CAP[r["cap"]] and r["V"] % 256 != 0


@pytest.mark.parametrize("row", [r for r in R.ARGMAX_ROWS if r["C"] >= 2 and r["V"] >= 255], ids=lambda r: r["id"])
def test_argmax_rows_hold_every_planted_case(row):
    x, kind = R.argmax_case(row)
    for b in range(row["B"]):
        share = R.column_shares(x[b])
        for name in R.ARGMAX_KINDS:
            assert share[name] >= 0.05, (row["id"], b, name, share)
    assert kind[-1, -1] == 2 and np.isnan(x[-1, -2:, -1]).all()                                             # the last voxel of the last batch item
    assert R.argmax_reference(row)[-1, -1] == row["C"] - 2


def test_argmax_rows_with_one_channel_hold_nan_and_inf():
    for row in (r for r in R.ARGMAX_ROWS if r["C"] == 1 and r["V"] >= 255):
        x, _ = R.argmax_case(row)
        assert np.isnan(x).mean() >= 0.05 and np.isinf(x).mean() >= 0.05
        assert not R.argmax_reference(row).any()


def test_finalize_table():
    assert {r["C"] for r in R.FINALIZE_ROWS} == {1, 2, 5, 256}
    r = R.FINALIZE_OVER_CAP
    assert np.prod(r["sp"]) == R.OVER_CAP_V > R.GRID_CAP[r["cap"]] and r["C"] == 2
    for row in R.FINALIZE_ROWS:
        acc, cz, cy, cx = R.finalize_case(row)
        assert set(np.concatenate([cz, cy, cx]).tolist()) <= set(R.COUNTS)
        q, lab = R.finalize_reference(row)
        assert q.dtype == np.float32 and lab.max() < row["C"]
        if row["C"] >= 2 and acc[0].size >= 255:
            share = R.column_shares(q.reshape(row["C"], -1))                                               # ties and NaNs survive the division: they are ties of the QUOTIENT
            assert all(share[k] >= 0.05 for k in R.ARGMAX_KINDS), (row["id"], share)
    used = set()
    for row in R.FINALIZE_ROWS:
        for a in R.finalize_case(row)[1:]:
            used |= set(a.tolist())
    assert used == set(R.COUNTS)


def test_window_table():
    rows = R.WINDOW_ROWS
    assert {r["win"][2] for r in rows} >= {1, 3, 4, 5, 8} and {r["C"] for r in rows} == {1, 3}
    assert any(r["at"] == (0, 0, 0) and r["win"] != r["vol"] for r in rows) and any(r["win"] == r["vol"] for r in rows) and any(r["win"] == (1, 1, 1) for r in rows)
    assert any(tuple(a + w for a, w in zip(r["at"], r["win"])) == r["vol"] and r["at"] != (0, 0, 0) for r in rows)      # the far corner
    assert any(r["at"][2] % 2 == 1 for r in rows)
    for r in rows + [R.WINDOW_OVER_CAP]:
        assert all(a >= 0 and w > 0 and a + w <= v for a, w, v in zip(r["at"], r["win"], r["vol"])), r["id"]
    for vol, win, at in R.WINDOW_REFUSED:
        assert any(v <= 0 or w <= 0 or a < 0 or a + w > v for a, w, v in zip(at, win, vol))
    r = R.WINDOW_OVER_CAP
    assert r["win"] == (257, 256, 256) and r["vol"] == (258, 257, 257) and r["C"] * np.prod(r["win"]) > R.GRID_CAP[r["cap"]]


# ---------------------------------------------------------------------------------------------------------------------- confusion
def test_confusion_clamps_in_the_source_width():
    big = np.array([[(1 << 32) + 1, -(1 << 32) - 1, -1, 4, 255, 2]], dtype=np.int64)
    c = R.confusion(big, np.zeros_like(big), 4)[0]
    assert c[0].tolist() == [2, 0, 1, 3]                    # 2^32 + 1 -> 3 (not 1), -2^32 - 1 -> 0 (not 3), -1 -> 0, 4 -> 3, 255 -> 3, 2 -> 2
    u8 = np.array([[255, 4, 3, 0]], dtype=np.uint8)
    assert R.confusion(u8, u8, 4)[0].diagonal().tolist() == [1, 0, 0, 3]


def test_confusion_table():
    rows = R.CONF_ROWS
    assert {r["NC"] for r in rows} == {2, 4, 5, 8} and {r["B"] for r in rows} == {1, 3} and {r["V"] for r in rows} == {1, 257, 4099, 262144 + 4099}
    assert set(R.CONF_PAIRS) | set(R.CONF_REFUSED_PAIRS) == {(p, g) for p in (1, 4, 8) for g in (1, 4, 8)}
    for r in rows:
        if "cap" in r:
            assert r["V"] > R.GRID_CAP[r["cap"]]
    assert any("cap" in r for r in rows)


@pytest.mark.parametrize("row", R.CONF_ROWS, ids=lambda r: r["id"])
def test_confusion_rows_fill_every_cell(row):
    for pb, gb in R.CONF_PAIRS:
        p, g = R.labels_for(row, pb, 0), R.labels_for(row, gb, 1)
        assert p.dtype == R.NP_LABEL[pb] and g.dtype == R.NP_LABEL[gb]
        conf = R.confusion(p, g, row["NC"])
        assert conf.sum() == row["B"] * row["V"]
        if row["cover"]:
            assert (conf > 0).all(), (row["id"], pb, gb)
        if row["wild"]:
            for a, nb in ((p, pb), (g, gb)):
                assert (a.astype(np.int64) >= row["NC"]).any() and (nb == 1 or (a < 0).any())
                assert set(R.WILD[nb]) <= set(a.ravel().tolist())
    assert row["cover"] or row["V"] < row["NC"] ** 2          # only a row too small to hold NC*NC voxels is excused


def test_some_confusion_row_is_wild_at_every_class_count():
    assert {r["NC"] for r in R.CONF_ROWS if r["wild"]} == {2, 4, 5, 8}
    assert any(r["wild"] and "cap" in r for r in R.CONF_ROWS)


# ---------------------------------------------------------------------------------------------------------------------- box, rank-select
def test_box_and_min_oracles_agree_with_the_augment_oracle_and_ignore_nan():
    from oracle import augment_oracle as AO
    x = R.ints(3, 5, 6, 7, seed=2)
    start, end = AO.bounding_box(x)
    b = R.bbox_gt(x, R.min_value(x))
    assert b[:3] == start and [v + 1 for v in b[3:]] == end and R.min_value(x) == x.min()
    y = x.copy()
    y[0, 0, 0, 0] = np.nan
    y[2, 4, 5, 6] = np.nan
    assert R.min_value(y) == -3.0 and np.isnan(y.min())
    assert R.bbox_gt(np.full((1, 2, 2, 2), np.nan, dtype=np.float32), -1.0) == [R.INT_MAX] * 3 + [-1] * 3
    assert R.bbox_gt(x, 3.0) == [R.INT_MAX] * 3 + [-1] * 3                                                  # thr = the maximum: empty
    assert R.MIN_N[-1] > R.GRID_CAP["vx_min_value"] and np.prod(R.BOX_SHAPES[-1]) > R.GRID_CAP["vx_bbox_gt"]


@pytest.mark.parametrize("code", R.LABEL_CODES)
def test_label_oracles_are_np_nonzero(code):
    for n in R.LABEL_N:
        assert n % 256 != 0 and all(n % c != 0 for c in R.CHUNKS)
        for fg in (0, 1):
            lab = R.labels(code, n, fg)
            with np.errstate(invalid="ignore"):
                idx = np.nonzero(lab > 0)[0] if fg else np.nonzero(~(lab > 0))[0]
            for chunk in R.CHUNKS:
                cnt = R.chunk_count(lab, chunk, fg)
                assert cnt.sum() == idx.size and cnt.size == -(-n // chunk)
                assert chunk == 65536 or (cnt == 0).any()                                                   # a chunk with no match
                q = R.kth_queries(lab, chunk, fg)
                last = (n - 1) // chunk * chunk
                last += (n - 1 - last) // 256 * 256                                                         # where the ragged last strip of the last chunk starts
                assert any(want is None for _, _, want in q) and any(want is not None and want >= last for _, _, want in q)
                lanes = {(want - c0) % 256 for c0, _, want in q if want is not None}
                assert {0, 255} <= lanes
                for c0, k, want in q[:: max(1, len(q) // 50)]:
                    inside = idx[(idx >= c0) & (idx < c0 + chunk)]
                    assert want == (int(inside[k]) if k < inside.size else None)
    if code == -4:
        lab = R.labels(code, R.LABEL_N[0], 1)
        assert np.isnan(lab).any() and (lab == 0.5).any() and (lab == -1).any()


# ---------------------------------------------------------------------------------------------------------------------- rotation
def test_rotation_table_is_the_45_combinations():
    assert len(R.ROT_ROWS) == 45 == len({r["id"] for r in R.ROT_ROWS})
    assert {r["W"] for r in R.ROT_ROWS} == {1, 3, 5} and {r["C"] for r in R.ROT_ROWS} == {1, 2}
    assert any(r["ties"] for r in R.ROT_ROWS) and any(r["border"] for r in R.ROT_ROWS)
    assert any((r["cs"], r["sn"]) in ((0.0, 1.0), (0.0, -1.0)) and r["D"] != r["H"] for r in R.ROT_ROWS)


@pytest.mark.parametrize("row", R.ROT_ROWS, ids=lambda r: r["id"])
def test_rotation_row_is_exact_in_fp32(row):
    D, H, cs, sn = row["D"], row["H"], row["cs"], row["sn"]
    assert float(np.float32(cs)) == cs and float(np.float32(sn)) == sn
    c64, c32 = R.rotate_coords(D, H, cs, sn, np.float64), R.rotate_coords(D, H, cs, sn, np.float32)
    cd, ch = (D - 1) / 2, (H - 1) / 2
    pd, ph = (np.arange(D) - cd)[:, None], (np.arange(H) - ch)[None, :]
    for got32, got64, (p, q) in zip(c32, c64, ((cs * pd, -sn * ph), (sn * pd, cs * ph))):
        assert got32.dtype == np.float32 and (got32.astype(np.float64) == got64).all()                     # fp32 == fp64, bit for bit
        assert (got64 * 16 == np.rint(got64 * 16)).all()                                                   # multiples of 1/16
        # every product and every partial sum is a multiple of 1/16 far below 2^24 / 16: each is exact in fp32, so a fused multiply-add (which skips the rounding of
        # the product) rounds nothing either
        for t in (p + 0 * q, q + 0 * p, p + q):
            assert (t * 16 == np.rint(t * 16)).all() and np.abs(t).max() < 2 ** 20
    x = R.rotate_input(row)
    for mode in (0, 1):
        r64, r32 = R.rotate_exact(x, cs, sn, mode, np.float64), R.rotate_exact(x, cs, sn, mode, np.float32)
        assert r32.dtype == np.float32 and r64.shape == x.shape and (r32.astype(np.float64) == r64).all()  # the interpolated values are representable
        assert (r64 * 256 == np.rint(r64 * 256)).all()
    sd, sh = c64
    inside = (sd >= 0) & (sd <= D - 1) & (sh >= 0) & (sh <= H - 1)
    tie = inside & ((np.abs(sd - np.floor(sd) - 0.5) == 0) | (np.abs(sh - np.floor(sh) - 0.5) == 0))
    if row["ties"]:
        assert tie.sum() >= 0.10 * inside.sum(), (row["id"], tie.sum(), inside.sum())
    if row["border"]:
        assert (~inside).mean() >= 0.10, (row["id"], (~inside).mean())
    if (cs, sn) == (1.0, 0.0):
        assert (R.rotate_exact(x, cs, sn, 0) == x).all() and (R.rotate_exact(x, cs, sn, 1) == x).all()
    if (cs, sn) in ((0.0, 1.0), (0.0, -1.0)) and D != H:
        assert (~inside).any()


def test_nearest_is_half_to_even_not_half_up():
    row = next(r for r in R.ROT_ROWS if r["ties"])
    x = R.rotate_input(row)
    sd, sh = (np.clip(c, 0, n - 1) for c, n in zip(R.rotate_coords(row["D"], row["H"], row["cs"], row["sn"]), (row["D"], row["H"])))
    up = x[:, np.floor(sd + 0.5).astype(int), np.floor(sh + 0.5).astype(int), :]
    assert (up != R.rotate_exact(x, row["cs"], row["sn"], 1)).any()           # the row tells the two rounding rules apart


# ---------------------------------------------------------------------------------------------------------------------- BraTS
def test_brats_reference_counts_labels_above_three_in_wt_only():
    o = np.array([0, 4, 3, 1, 5, 0], dtype=np.int64).reshape(1, 1, 1, 6, 1)
    t = np.array([4, 4, 3, 3, 0, 0], dtype=np.int64).reshape(1, 1, 1, 6, 1)
    avg, et, tc, wt = R.brats_dice_reference(o, t)
    assert abs(et - 2 * 1 / (1 + 2)) < 1e-6 and abs(tc - 2 * 2 / (2 + 2)) < 1e-6 and abs(wt - 2 * 3 / (4 + 4)) < 1e-6
