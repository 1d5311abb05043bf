"""CPU side of mirror test-time augmentation: the mirror schedule, and the argument checks of the new C-ABI entry points (csrc/infer.hip), which
answer with error codes before anything is launched -- so also on a machine without a GPU."""
import ctypes
import itertools

import pytest

import tta_ref as TR


def test_mirror_schedule_is_nnunets_order_for_every_subset():
    from veloxseg_amd.utils.inference_runtime import mirror_schedule
    assert mirror_schedule(()) == [0]
    assert mirror_schedule((0, 1, 2)) == [0, 1, 2, 4, 3, 5, 6, 7]
    for n in range(4):
        for sub in itertools.combinations((0, 1, 2), n):
            want = [0] + [sum(1 << a for a in c) for i in range(1, n + 1) for c in itertools.combinations(sub, i)]
            assert TR.masks(sub) == want
            for perm in itertools.permutations(sub):                       # the order of the axes is irrelevant
                got = mirror_schedule(perm)
                assert got == want and len(got) == 2 ** n and len(set(got)) == len(got)
                assert mirror_schedule(list(perm)) == want
    for bad in ((0, 0), (2, 1, 2), (3,), (-1,), (0, 4), (1.5,), ("0",)):
        with pytest.raises(ValueError):
            mirror_schedule(bad)


def test_window_table_capacity_is_the_headers():
    """SW_MAX_WINDOWS (how many windows the driver hands to one vx_sw_extract_mirror call) restates VX_SW_MAX_WINDOWS of the public header"""
    import re
    from veloxseg_amd import _hip
    from veloxseg_amd.utils.inference_runtime import SW_MAX_WINDOWS
    m = re.search(r"^#define\s+VX_SW_MAX_WINDOWS\s+(\d+)\s*$", open(_hip.HEADER).read(), re.M)
    assert m and int(m.group(1)) == SW_MAX_WINDOWS


def _table(*rows):
    t = (ctypes.c_int * (4 * len(rows)))(*[v for r in rows for v in r])
    return t, ctypes.addressof(t)


def test_new_entry_points_return_error_codes_without_gpu():
    import __graft_entry__ as G
    G.build()
    from veloxseg_amd import _hip
    from veloxseg_amd.utils.inference_runtime import SW_MAX_WINDOWS
    keep, tab = _table((0, 0, 0, 0))
    # (vol, win, table, nwin, mask, B, C, D, H, W, rd, rh, rw, stream): pointers that are never dereferenced -- every call fails its checks first
    with pytest.raises(RuntimeError, match="mask 8 outside 0..7"):
        _hip.call("vx_sw_extract_mirror", 16, 16, tab, 1, 8, 1, 1, 4, 4, 4, 2, 2, 2, None)
    with pytest.raises(RuntimeError, match="mask -1 outside 0..7"):
        _hip.call("vx_sw_extract_mirror", 16, 16, tab, 1, -1, 1, 1, 4, 4, 4, 2, 2, 2, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("vx_sw_extract_mirror", None, 16, tab, 1, 0, 1, 1, 4, 4, 4, 2, 2, 2, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("vx_sw_extract_mirror", 16, 16, None, 1, 0, 1, 1, 4, 4, 4, 2, 2, 2, None)
    for nwin in (0, SW_MAX_WINDOWS + 1):
        with pytest.raises(RuntimeError, match="the table holds"):
            _hip.call("vx_sw_extract_mirror", 16, 16, tab, nwin, 0, 1, 1, 4, 4, 4, 2, 2, 2, None)
    keep2, tab2 = _table((0, 0, 0, 0), (0, 0, 3, 0))                        # the second window: y0 + rh = 5 > H = 4
    with pytest.raises(RuntimeError, match="leaves the volume"):
        _hip.call("vx_sw_extract_mirror", 16, 16, tab2, 2, 5, 1, 1, 4, 4, 4, 2, 2, 2, None)
    keep3, tab3 = _table((1, 0, 0, 0))                                      # batch item 1 of a batch of 1
    with pytest.raises(RuntimeError, match="batch item"):
        _hip.call("vx_sw_extract_mirror", 16, 16, tab3, 1, 0, 1, 1, 4, 4, 4, 2, 2, 2, None)
    # (pred, wsum, rows, rd, rh, rw, mask, first, stream)
    with pytest.raises(RuntimeError, match="mask 8 outside 0..7"):
        _hip.call("vx_sw_mirror_sum", 16, 32, 1, 2, 2, 2, 8, 1, None)
    with pytest.raises(RuntimeError, match="null or aliased"):
        _hip.call("vx_sw_mirror_sum", None, 32, 1, 2, 2, 2, 0, 1, None)
    with pytest.raises(RuntimeError, match="null or aliased"):
        _hip.call("vx_sw_mirror_sum", 32, 32, 1, 2, 2, 2, 0, 0, None)
    with pytest.raises(RuntimeError, match="non-positive"):
        _hip.call("vx_sw_mirror_sum", 16, 32, 0, 2, 2, 2, 0, 1, None)
    # (pred, wsum, acc, C, D, H, W, rd, rh, rw, z0, y0, x0, mask, weight, stream)
    with pytest.raises(RuntimeError, match="mask 8 outside 0..7"):
        _hip.call("vx_sw_mirror_accumulate", 16, 32, 48, 1, 4, 4, 4, 2, 2, 2, 0, 0, 0, 8, 0.5, None)
    with pytest.raises(RuntimeError, match="leaves the volume"):
        _hip.call("vx_sw_mirror_accumulate", 16, 32, 48, 1, 4, 4, 4, 2, 2, 2, 0, 0, 3, 4, 0.5, None)
    with pytest.raises(RuntimeError, match="leaves the volume"):
        _hip.call("vx_sw_mirror_accumulate", 16, 32, 48, 1, 4, 4, 4, 2, 2, 2, -1, 0, 0, 4, 0.5, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _hip.call("vx_sw_mirror_accumulate", 16, None, 48, 1, 4, 4, 4, 2, 2, 2, 0, 0, 0, 4, 0.5, None)
    del keep, keep2, keep3


def test_keywords_are_checked_before_any_gpu_work():
    """sliding_window_inference on CPU inputs keeps raising RuntimeError (there is no CPU path), unknown keywords NotImplementedError"""
    import torch
    from veloxseg_amd.utils import inference_runtime as IR
    x = torch.zeros((1, 1, 4, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X only"):
        IR.sliding_window_inference(x, (2, 2, 2), 1, TR.flat_predictor, mirror_axes=(2,), sw_device="cpu", device="cpu")
    with pytest.raises(NotImplementedError, match="progress"):
        IR.sliding_window_inference(x, (2, 2, 2), 1, TR.flat_predictor, mirror_axes=(2,), progress=True)
