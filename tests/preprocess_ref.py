"""fp64 restatements of the reference's volume preprocessing, for tests/test_preprocess_cpu.py (against tests/golden/preprocess.pt, recorded from the reference
itself) and tests/test_preprocess_gpu.py (against the kernels of csrc/preprocess.hip).  CPU-only at import: plain numpy, the rules written out.

The resampling restates MONAI's Spacing for axis-aligned affines; MONAI is not available, so that part is unpinned against MONAI itself."""
import numpy as np


# ====================================================================================================================== normalisation
def zscore(image, seg):
    """preprocess/normalization_MRI.py:7-12 = preprocess/normalization_CT_PET.py:6-11.  `seg >= 0` is formed from whatever seg holds: the reference passes the
    BOOLEAN array `data > data.min()` (normalization_MRI.py:52, normalization_CT_PET.py:67), for which it is true everywhere -- every voxel is normalised with the
    statistics of the whole volume.  Works on a copy (the reference writes into its argument)."""
    image = np.array(image, dtype=np.float64)
    mask = np.asarray(seg) >= 0
    sel = image[mask]
    mean, std = sel.mean(), sel.std()
    image[mask] = (sel - mean) / max(std, 1e-8)
    return image


def zscore_reference_call(image):
    """the call the reference makes: zscore(data, data > data.min())"""
    image = np.asarray(image, dtype=np.float64)
    return zscore(image, image > image.min())


def foreground_moments(image):
    """count, mean, population std (two-pass, numpy's) over {x > x.min()}"""
    image = np.asarray(image, dtype=np.float64)
    sel = image[image > image.min()]
    if sel.size == 0:
        return 0, 0.0, 0.0
    return sel.size, float(sel.mean()), float(sel.std())


def zscore_foreground(image):
    """what the call spells out: statistics over {x > x.min()}, written to those voxels only (`image[mask] = ...`, normalization_MRI.py:11); the voxels at the minimum
    keep their raw value, a constant volume has an empty mask and stays as it is"""
    image = np.array(image, dtype=np.float64)
    mask = image > image.min()
    if not mask.any():
        return image
    sel = image[mask]
    image[mask] = (sel - sel.mean()) / max(sel.std(), 1e-8)
    return image


def ct_norm(image, props):
    """preprocess/normalization_CT_PET.py:23-31"""
    image = np.clip(np.asarray(image, dtype=np.float64), props["percentile_00_5"], props["percentile_99_5"])
    return (image - props["mean"]) / max(props["std"], 1e-8)


def normalize_intensity(x, channel_wise):
    """MONAI NormalizeIntensity (utils/inference_extern_mri.py:95): (x - mean) / std over all voxels, of each channel or of the whole array; std == 0 divides by 1"""
    x = np.asarray(x, dtype=np.float64)
    if channel_wise:
        return np.stack([normalize_intensity(c, False) for c in x])
    std = x.std()
    return (x - x.mean()) / (std if std != 0.0 else 1.0)


def intensity_statistics(voxels):
    """preprocess/normalization_CT_PET.py:72-81 on the gathered foreground voxels (fp64)"""
    v = np.asarray(voxels, dtype=np.float64)
    return {"mean": float(np.mean(v)), "median": float(np.median(v)), "std": float(np.std(v)), "min": float(np.min(v)), "max": float(np.max(v)),
            "percentile_99_5": float(np.percentile(v, 99.5)), "percentile_00_5": float(np.percentile(v, 0.5))}


# ====================================================================================================================== resampling
def out_size(n, src, dst):
    """round half to even of (n - 1) src / dst + 1, written out"""
    v = (n - 1) * src / dst + 1.0
    f = np.floor(v)
    r = v - f
    if r > 0.5 or (r == 0.5 and int(f) % 2 == 1):
        f += 1
    return int(f)


def coords(n, n_out, src, dst):
    """clamped continuous input index of every output index, fp64"""
    return np.array([min(max(j * src / dst, 0.0), float(n - 1)) for j in range(n_out)], dtype=np.float64)


def table(n, n_out, src, dst):
    c = coords(n, n_out, src, dst)
    i0 = np.floor(c).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), c - i0


def nearest_index(n, n_out, src, dst):
    """ties go to the even index"""
    c = coords(n, n_out, src, dst)
    f = np.floor(c)
    r = c - f
    up = (r > 0.5) | ((r == 0.5) & (f % 2 == 1))
    return (f + up).astype(np.int64)


def resample_linear(x, tables):
    """x (C, D, H, W) fp64; tables = [(i0, i1, w)] for z, y, x; lerps a + w (b - a) along x, then y, then z, in fp64 with the weights as given"""
    x = np.asarray(x, dtype=np.float64)
    (z0, z1, wz), (y0, y1, wy), (x0, x1, wx) = [(np.asarray(a), np.asarray(b), np.asarray(w, dtype=np.float64)) for a, b, w in tables]
    a, b = x[..., x0], x[..., x1]
    x = a + wx * (b - a)
    a, b = x[:, :, y0, :], x[:, :, y1, :]
    x = a + wy[:, None] * (b - a)
    a, b = x[:, z0], x[:, z1]
    return a + wz[:, None, None] * (b - a)


def resample_nearest(x, idx):
    x = np.asarray(x)
    return x[:, idx[0]][:, :, idx[1]][:, :, :, idx[2]]
