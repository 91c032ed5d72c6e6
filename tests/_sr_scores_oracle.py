"""numpy statement of the image scores of include/synthsr_hip.h (synthsr_sr_moments / _errors / _ssim3d) and
synthsr_amd/evaluate.py, shared by tests/test_sr_scores_cpu.py and tests/test_sr_scores_gpu.py.  Every formula is evaluated in
the dtype asked for: float64 is the reference, float32 measures what single precision itself costs on the same input (the `o`
of the accuracy rule  d <= 6 o + floor).  The Gaussian window is applied by explicit 1-D tap sums, axis after axis."""
import numpy as np

WINDOW, SIGMA, C1, C2 = 11, 1.5, 0.01 ** 2, 0.03 ** 2
K, FLOOR = 6.0, 2e-5   # the accuracy rule (the floor is GRAD_FLOOR of tests/conftest.py)


def taps(dtype=np.float64):
    k = np.arange(WINDOW, dtype=np.float64) - WINDOW // 2
    g = np.exp(-k * k / (2.0 * SIGMA * SIGMA))
    return (g / g.sum()).astype(dtype)


def window3(v):
    """w * v at the 'valid' positions, in v's dtype: explicit tap sums along axis 0, then 1, then 2"""
    w = taps(v.dtype)
    for axis in range(3):
        n = v.shape[axis] - WINDOW + 1
        acc = np.zeros(v.shape[:axis] + (n,) + v.shape[axis + 1:], dtype=v.dtype)
        for k in range(WINDOW):
            acc = acc + w[k] * np.take(v, np.arange(k, k + n), axis=axis)
        v = acc
    return v


def ssim_map(pred, truth, a=1.0, b=0.0, data_range=1.0, dtype=np.float64):
    """S [d0 - 10, d1 - 10, d2 - 10] of x = (a pred + b) / L against y = truth / L"""
    f = dtype
    inv = f(1.0) / f(data_range)
    x = (f(a) * np.asarray(pred, dtype=f) + f(b)) * inv
    y = np.asarray(truth, dtype=f) * inv
    mx, my = window3(x), window3(y)
    vx = window3(x * x) - mx * mx
    vy = window3(y * y) - my * my
    vxy = window3(x * y) - mx * my
    return ((f(2) * mx * my + f(C1)) * (f(2) * vxy + f(C2))) / ((mx * mx + my * my + f(C1)) * (vx + vy + f(C2)))


def ssim_map_correlate1d(pred, truth, a=1.0, b=0.0, data_range=1.0):
    """the same map from scipy.ndimage.correlate1d (float64), cropped to the 'valid' positions: an independent check"""
    from scipy.ndimage import correlate1d
    w = taps()

    def win(v):
        for axis in range(3):
            v = correlate1d(v, w, axis=axis, mode='constant', cval=0.0)
        h = WINDOW // 2
        return v[h:-h, h:-h, h:-h]
    x = (a * np.asarray(pred, dtype=np.float64) + b) / data_range
    y = np.asarray(truth, dtype=np.float64) / data_range
    mx, my = win(x), win(y)
    vx, vy, vxy = win(x * x) - mx * mx, win(y * y) - my * my, win(x * y) - mx * my
    return ((2 * mx * my + C1) * (2 * vxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))


def centre_mask(mask, shape):
    """bool [d0 - 10, d1 - 10, d2 - 10]: the window's centre voxel is in the mask"""
    h = WINDOW // 2
    if mask is None:
        return np.ones(tuple(s - WINDOW + 1 for s in shape), dtype=bool)
    return np.asarray(mask)[h:-h, h:-h, h:-h] != 0


def scores(pred, truth, mask=None, normalise='none', data_range=None, dtype=np.float64, ssim=True):
    """every score of evaluate.image_scores in `dtype`, plus 'mse' and 'ssim_map'.  The moments are sums of values shifted by the
    first masked voxel, as the kernel's are, so float32 stays meaningful on an offset-dominated volume."""
    f = dtype
    nan = float('nan')
    sel = np.ones(np.shape(pred), dtype=bool) if mask is None else np.asarray(mask) != 0
    p, t = np.asarray(pred, dtype=f)[sel], np.asarray(truth, dtype=f)[sel]
    n = int(p.size)
    out = dict(n_voxels=n, mae=nan, rmse=nan, max_abs=nan, psnr=nan, ncc=nan, scale=nan, offset=nan, ssim=nan, n_ssim=0,
               data_range=nan, mse=nan, ssim_map=None)
    if n == 0:
        return out
    L = f(data_range) if data_range is not None else f(t.max() - t.min())
    out['data_range'] = float(L)
    sp, st = p[0], t[0]
    dp, dt = p - sp, t - st
    ep, et = dp.sum(dtype=f) / f(n), dt.sum(dtype=f) / f(n)
    vp = (dp * dp).sum(dtype=f) / f(n) - ep * ep
    vt = (dt * dt).sum(dtype=f) / f(n) - et * et
    cov = (dp * dt).sum(dtype=f) / f(n) - ep * et
    if vp > 0 and vt > 0:
        out['ncc'] = float(cov / np.sqrt(vp * vt))
    if vp > 0:
        out['scale'] = float(cov / vp)
        out['offset'] = float((st + et) - f(out['scale']) * (sp + ep))
    a, b = (out['scale'], out['offset']) if normalise == 'affine' else (1.0, 0.0)
    if not (np.isfinite(a) and np.isfinite(b)):
        return out
    d = f(a) * p + f(b) - t
    mse = (d * d).sum(dtype=f) / f(n)
    out.update(mae=float(np.abs(d).sum(dtype=f) / f(n)), rmse=float(np.sqrt(mse)), max_abs=float(np.abs(d).max()), mse=float(mse))
    if L > 0:
        out['psnr'] = float('inf') if mse == 0 else float(10.0 * np.log10(L * L / mse))
        if ssim:
            S = ssim_map(pred, truth, a, b, L, dtype=f)
            c = centre_mask(mask, np.shape(pred))
            out['ssim_map'] = S
            out['n_ssim'] = int(c.sum())
            if out['n_ssim']:
                out['ssim'] = float(S[c].sum(dtype=f) / f(out['n_ssim']))
    return out


def textured(shape, seed, ramp=(0.011, -0.007, 0.004), base=0.3):
    """float32 pair (pred, truth) in about [0, 1]: smoothed noise plus an anisotropic ramp (an axis mix-up cannot cancel), the
    prediction a perturbed copy of the truth"""
    from scipy.ndimage import gaussian_filter
    rng = np.random.default_rng(seed)
    g = gaussian_filter(rng.standard_normal(shape), 1.2)
    g = 0.25 * g / g.std()
    i, j, k = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij')
    truth = base + g + ramp[0] * i + ramp[1] * j + ramp[2] * k
    pred = truth + 0.05 * gaussian_filter(rng.standard_normal(shape), 0.7) + 0.02 * rng.standard_normal(shape)
    return pred.astype(np.float32), truth.astype(np.float32)
