"""numpy restatement of the way back from the network grid to the image's own grid (utils/preprocess.py inverse_tables / labels_on_native_grid, csrc/preprocess.hip
vx_native_argmax), for tests/test_native_grid_cpu.py and tests/test_native_grid_gpu.py.  CPU-only at import: plain numpy, the rules written out.

The interpolation is preprocess_ref.resample_linear: fp64 lerps a + w (b - a) along x, then y, then z, with the fp32 weights as given.  The arg-max rule is the
project's (include/veloxseg_hip.h, vx_sw_finalize): a column that holds a NaN gives the index of its first NaN, any other the index of its first maximum."""
import numpy as np

import preprocess_ref as R


def tables(net_shape, native_shape, net_spacing, native_spacing):
    """per axis (i0, i1, fp32 weight) of the GIVEN native extent: native index j samples the network coordinate clamp(j * net / native, 0, n_net - 1)"""
    out = []
    for n, no, s, d in zip(net_shape, native_shape, net_spacing, native_spacing):
        i0, i1, w = R.table(int(n), int(no), float(s), float(d))
        out.append((i0, i1, w.astype(np.float32)))
    return out


def first_nan_else_first_max(v):
    """v (K, ...) -> uint8 (...): written out class by class -- a later class wins only when it is strictly greater (so -0.0 does not beat +0.0 and the first of
    equal maxima stays); a column with a NaN gives its first NaN"""
    v = np.asarray(v)
    best = v[0].copy()
    arg = np.zeros(v.shape[1:], dtype=np.int64)
    for c in range(1, v.shape[0]):
        with np.errstate(invalid="ignore"):
            better = v[c] > best
        arg[better] = c
        best[better] = v[c][better]
    nan = np.isnan(v)
    first_nan = np.zeros(v.shape[1:], dtype=np.int64)
    seen = np.zeros(v.shape[1:], dtype=bool)
    for c in range(v.shape[0]):
        new = nan[c] & ~seen
        first_nan[new] = c
        seen |= nan[c]
    return np.where(seen, first_nan, arg).astype(np.uint8)


def values_on_native_grid(logits, native_shape, net_spacing, native_spacing):
    """(K, d, h, w) -> fp64 (K, D, H, W) trilinear values on the native grid"""
    logits = np.asarray(logits)
    with np.errstate(invalid="ignore"):
        return R.resample_linear(logits, tables(logits.shape[1:], native_shape, net_spacing, native_spacing))


def labels_on_native_grid(logits, native_shape, net_spacing, native_spacing):
    return first_nan_else_first_max(values_on_native_grid(logits, native_shape, net_spacing, native_spacing))


def top_two_margin(v):
    """v (K, ...) without NaN, K >= 2 -> the largest value minus the second largest (0 for a tie), per column"""
    s = np.sort(np.asarray(v, dtype=np.float64), axis=0)
    return s[-1] - s[-2]
