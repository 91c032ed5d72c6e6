"""numpy evaluation of the contracts of csrc/volume_prep.hip (include/synthsr_hip.h: "inference volumes"), in float64 as the
reference of the tests and in float32 as the yardstick printed next to the device's error.  Positions are always float64, as on
the device; `dtype` is the type of the weights and of the arithmetic on voxel values."""
import numpy as np


def reflect(i, n):
    m = np.mod(i, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def blur_axis(vol, axis, taps, dtype=np.float64):
    """out[i] = sum_t taps[t + r] vol[reflect(i + t)] along axis, accumulated in tap order in `dtype`"""
    vol = np.asarray(vol, dtype=dtype)
    taps = np.asarray(taps, dtype=dtype)
    r = (len(taps) - 1) // 2
    n = vol.shape[axis]
    out = np.zeros(vol.shape, dtype=dtype)
    for t in range(-r, r + 1):
        out = out + taps[t + r] * np.take(vol, reflect(np.arange(n) + t, n), axis=axis)
    return out


def positions(M, out_shape):
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing='ij'), 0)
    M = np.asarray(M, dtype=np.float64)
    return np.einsum('ab,b...->a...', M[:3, :3], g) + M[:3, 3].reshape(3, 1, 1, 1)


def near_a_face(M, out_shape, src_shape, tol=1e-9):
    """voxels whose position lies within tol of a face of the source grid on some axis: which side of it a position falls on may
    differ between two ways of adding up the same matrix product"""
    pos = positions(M, out_shape)
    n = np.array(src_shape).reshape(3, 1, 1, 1)
    return np.any((np.abs(pos) < tol) | (np.abs(pos - (n - 1)) < tol), axis=0)


def sample(vol, M, out_shape, zero_outside=False, dtype=np.float64):
    """positions M (i, j, k, 1); clamp, or zero outside the grid; i0 = min(floor(pos), max(n - 2, 0)), i1 = min(i0 + 1, n - 1),
    w = pos - i0 rounded to dtype; a (1 - w) + b w along axis 2, then 1, then 0"""
    vol = np.asarray(vol, dtype=dtype)
    pos = positions(M, out_shape)
    n = np.array(vol.shape).reshape(3, 1, 1, 1)
    inside = np.all((pos >= 0) & (pos <= n - 1), axis=0)
    p = np.clip(pos, 0, n - 1)
    i0 = np.minimum(np.floor(p).astype(np.int64), np.maximum(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    w = (p - i0).astype(dtype)
    u = (1 - w).astype(dtype)
    corner = lambda a, b, c: vol[(i1 if a else i0)[0], (i1 if b else i0)[1], (i1 if c else i0)[2]]
    c00, c01 = corner(0, 0, 0) * u[2] + corner(0, 0, 1) * w[2], corner(0, 1, 0) * u[2] + corner(0, 1, 1) * w[2]
    c10, c11 = corner(1, 0, 0) * u[2] + corner(1, 0, 1) * w[2], corner(1, 1, 0) * u[2] + corner(1, 1, 1) * w[2]
    out = (c00 * u[1] + c01 * w[1]) * u[0] + (c10 * u[1] + c11 * w[1]) * w[0]
    if zero_outside:
        out = np.where(inside, out, 0).astype(dtype)
    assert out.dtype == dtype
    return out


def normalise(vol, gain=1.0, dtype=np.float64):
    vol = np.asarray(vol, dtype=dtype)
    lo, hi = vol.min(), vol.max()
    return (dtype(gain) * ((vol - lo) / (hi - lo))).astype(dtype)
