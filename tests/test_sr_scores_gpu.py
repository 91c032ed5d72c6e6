"""The image-score kernels of csrc/sr_scores.hip (synthsr_sr_moments / _errors / _ssim3d) against the float64 oracle of
tests/_sr_scores_oracle.py, through the C ABI (ops.sr_* and evaluate.image_scores are ctypes callers of it).

Accuracy rule of every numeric comparison:  d <= 6 o + 2e-5,  d = |device - float64 oracle|, o = |float32 oracle - float64 oracle|
on the same input, both range-normalised: SSIM (mean and map, the map by its largest deviation), NCC and scale as they are; MAE,
RMSE, max_abs and offset divided by data_range; PSNR through its MSE divided by data_range^2.

Measured on one MI355X (tag, quantity, d, o; printed again by every run with -s):
  textured (11, 11, 11)              ssim      d 1.390e-07  o 2.582e-07
  textured (11, 11, 11)              ncc       d 1.186e-09  o 1.178e-07
  textured (11, 11, 11)              scale     d 3.973e-09  o 2.124e-07
  textured (11, 11, 11)              offset    d 4.745e-10  o 2.887e-08
  textured (11, 11, 11)              mae       d 6.053e-14  o 1.791e-10
  textured (11, 11, 11)              rmse      d 6.483e-12  o 2.026e-10
  textured (11, 11, 11)              max_abs   d 0.000e+00  o 0.000e+00
  textured (11, 11, 11)              mse       d 1.530e-13  o 9.828e-13
  textured (11, 11, 11)              ssim_map  d 1.390e-07  o 2.582e-07
  textured (12, 11, 13)              ssim      d 6.970e-08  o 1.687e-07
  textured (12, 11, 13)              ncc       d 4.134e-10  o 5.399e-08
  textured (12, 11, 13)              scale     d 8.326e-09  o 1.611e-07
  textured (12, 11, 13)              offset    d 1.582e-09  o 3.322e-08
  textured (12, 11, 13)              mae       d 4.483e-12  o 8.492e-11
  textured (12, 11, 13)              rmse      d 1.019e-11  o 9.786e-10
  textured (12, 11, 13)              max_abs   d 0.000e+00  o 0.000e+00
  textured (12, 11, 13)              mse       d 2.769e-13  o 1.409e-11
  textured (12, 11, 13)              ssim_map  d 3.137e-07  o 2.823e-07
  textured (19, 23, 37)              ssim      d 3.492e-08  o 4.795e-08
  textured (19, 23, 37)              ncc       d 8.295e-10  o 2.087e-07
  textured (19, 23, 37)              scale     d 8.560e-10  o 2.425e-07
  textured (19, 23, 37)              offset    d 2.165e-10  o 3.782e-08
  textured (19, 23, 37)              mae       d 5.678e-13  o 9.343e-11
  textured (19, 23, 37)              rmse      d 1.554e-12  o 6.571e-10
  textured (19, 23, 37)              max_abs   d 0.000e+00  o 0.000e+00
  textured (19, 23, 37)              mse       d 3.041e-14  o 9.603e-12
  textured (19, 23, 37)              ssim_map  d 2.175e-06  o 2.287e-06
  textured (68, 47, 80)              ssim      d 2.521e-08  o 3.030e-08
  textured (68, 47, 80)              ncc       d 7.562e-11  o 2.102e-06
  textured (68, 47, 80)              scale     d 1.146e-10  o 2.485e-06
  textured (68, 47, 80)              offset    d 2.285e-11  o 4.903e-07
  textured (68, 47, 80)              mae       d 3.235e-14  o 8.145e-10
  textured (68, 47, 80)              rmse      d 4.906e-13  o 4.872e-10
  textured (68, 47, 80)              max_abs   d 0.000e+00  o 0.000e+00
  textured (68, 47, 80)              mse       d 7.050e-15  o 6.121e-12
  textured (68, 47, 80)              ssim_map  d 1.300e-05  o 1.454e-05
  planted centre max |1 - S| away from the voxel = 2.384e-07
  planted centre                     ssim      d 7.807e-09  o 9.875e-09
  planted centre                     mae       d 1.885e-13  o 6.447e-14
  planted centre                     rmse      d 4.697e-12  o 1.757e-11
  planted centre                     max_abs   d 2.926e-09  o 2.926e-09
  planted centre                     ssim_map  d 1.444e-06  o 1.444e-06
  planted origin max |1 - S| away from the voxel = 2.384e-07
  planted origin                     ssim      d 3.209e-13  o 3.209e-13
  planted origin                     mae       d 0.000e+00  o 1.240e-13
  planted origin                     rmse      d 1.879e-11  o 4.106e-11
  planted origin                     max_abs   d 0.000e+00  o 0.000e+00
  planted origin                     ssim_map  d 1.064e-09  o 1.064e-09
  planted far_corner max |1 - S| away from the voxel = 2.384e-07
  planted far_corner                 ssim      d 5.785e-13  o 5.785e-13
  planted far_corner                 mae       d 0.000e+00  o 2.031e-13
  planted far_corner                 rmse      d 1.096e-11  o 4.539e-11
  planted far_corner                 max_abs   d 0.000e+00  o 0.000e+00
  planted far_corner                 ssim_map  d 1.918e-09  o 1.769e-07
  identical                          ncc       d 0.000e+00  o 0.000e+00
  identical                          scale     d 0.000e+00  o 0.000e+00
  identical                          offset    d 0.000e+00  o 0.000e+00
  identical                          ssim      d 1.811e-09  o 0.000e+00
  offset-dominated none              ncc       d 2.792e-11  o 4.655e-09
  offset-dominated none              scale     d 6.573e-10  o 2.101e-08
  offset-dominated none              offset    d 9.737e-08  o 2.084e-06
  offset-dominated none              mae       d 0.000e+00  o 3.154e-09
  offset-dominated none              rmse      d 2.573e-10  o 1.053e-09
  offset-dominated none              max_abs   d 0.000e+00  o 0.000e+00
  offset-dominated half              ncc       d 1.090e-09  o 2.553e-08
  offset-dominated half              scale     d 1.502e-12  o 1.884e-07
  offset-dominated half              offset    d 2.273e-10  o 3.038e-05
  offset-dominated half              mae       d 0.000e+00  o 3.241e-09
  offset-dominated half              rmse      d 2.512e-10  o 1.270e-09
  offset-dominated half              max_abs   d 0.000e+00  o 0.000e+00
  mask none (19, 23, 37)             ncc       d 8.295e-10  o 2.087e-07
  mask none (19, 23, 37)             scale     d 8.560e-10  o 2.425e-07
  mask none (19, 23, 37)             offset    d 2.165e-10  o 3.782e-08
  mask none (19, 23, 37)             mae       d 5.678e-13  o 9.343e-11
  mask none (19, 23, 37)             rmse      d 1.554e-12  o 6.571e-10
  mask none (19, 23, 37)             max_abs   d 0.000e+00  o 0.000e+00
  mask none (19, 23, 37)             mse       d 3.041e-14  o 9.603e-12
  mask none (19, 23, 37)             ssim      d 3.492e-08  o 4.795e-08
  mask none (19, 23, 37)             ssim_map  d 2.175e-06  o 2.287e-06
  mask half (19, 23, 37)             ncc       d 8.585e-10  o 1.131e-07
  mask half (19, 23, 37)             scale     d 1.206e-09  o 2.342e-07
  mask half (19, 23, 37)             offset    d 2.567e-10  o 5.889e-08
  mask half (19, 23, 37)             mae       d 1.064e-12  o 1.078e-10
  mask half (19, 23, 37)             rmse      d 1.290e-12  o 4.570e-10
  mask half (19, 23, 37)             max_abs   d 0.000e+00  o 0.000e+00
  mask half (19, 23, 37)             mse       d 2.860e-14  o 3.221e-12
  mask half (19, 23, 37)             ssim      d 3.261e-08  o 3.850e-08
  mask half (19, 23, 37)             ssim_map  d 3.543e-06  o 2.364e-06
  mask border (19, 23, 37)           ncc       d 4.121e-10  o 1.054e-07
  mask border (19, 23, 37)           scale     d 6.645e-10  o 4.389e-07
  mask border (19, 23, 37)           offset    d 1.986e-10  o 5.229e-08
  mask border (19, 23, 37)           mae       d 6.410e-13  o 4.250e-10
  mask border (19, 23, 37)           rmse      d 1.437e-12  o 6.249e-10
  mask border (19, 23, 37)           max_abs   d 0.000e+00  o 0.000e+00
  mask border (19, 23, 37)           mse       d 2.817e-14  o 7.635e-12
  mask border (19, 23, 37)           ssim_map  d 2.175e-06  o 2.287e-06
  mask none (68, 47, 80)             ncc       d 7.562e-11  o 2.102e-06
  mask none (68, 47, 80)             scale     d 1.146e-10  o 2.485e-06
  mask none (68, 47, 80)             offset    d 2.285e-11  o 4.903e-07
  mask none (68, 47, 80)             mae       d 3.235e-14  o 8.145e-10
  mask none (68, 47, 80)             rmse      d 4.906e-13  o 4.872e-10
  mask none (68, 47, 80)             max_abs   d 0.000e+00  o 0.000e+00
  mask none (68, 47, 80)             mse       d 7.050e-15  o 6.121e-12
  mask none (68, 47, 80)             ssim      d 2.521e-08  o 3.030e-08
  mask none (68, 47, 80)             ssim_map  d 1.300e-05  o 1.454e-05
  mask half (68, 47, 80)             ncc       d 6.339e-11  o 4.589e-07
  mask half (68, 47, 80)             scale     d 8.837e-11  o 4.427e-07
  mask half (68, 47, 80)             offset    d 3.181e-11  o 8.612e-08
  mask half (68, 47, 80)             mae       d 1.905e-14  o 1.027e-09
  mask half (68, 47, 80)             rmse      d 5.514e-13  o 7.881e-11
  mask half (68, 47, 80)             max_abs   d 0.000e+00  o 0.000e+00
  mask half (68, 47, 80)             mse       d 8.106e-15  o 1.389e-12
  mask half (68, 47, 80)             ssim      d 1.883e-08  o 9.117e-08
  mask half (68, 47, 80)             ssim_map  d 1.705e-05  o 1.390e-05
  mask border (68, 47, 80)           ncc       d 5.959e-12  o 1.189e-06
  mask border (68, 47, 80)           scale     d 5.079e-10  o 2.125e-07
  mask border (68, 47, 80)           offset    d 2.774e-11  o 2.214e-08
  mask border (68, 47, 80)           mae       d 4.044e-14  o 2.048e-11
  mask border (68, 47, 80)           rmse      d 2.849e-13  o 2.262e-10
  mask border (68, 47, 80)           max_abs   d 0.000e+00  o 0.000e+00
  mask border (68, 47, 80)           mse       d 4.149e-15  o 6.000e-12
  mask border (68, 47, 80)           ssim_map  d 1.300e-05  o 1.454e-05
  affine                             ssim      d 4.297e-08  o 3.557e-08
  affine                             ncc       d 2.583e-10  o 3.028e-08
  affine                             scale     d 4.180e-10  o 5.451e-07
  affine                             offset    d 1.140e-09  o 1.486e-06
  affine                             mae       d 1.279e-10  o 5.441e-10
  affine                             rmse      d 1.148e-11  o 4.352e-10
  affine                             max_abs   d 1.034e-07  o 1.711e-07
  affine                             mse       d 3.695e-14  o 1.482e-12
  affine                             ssim_map  d 2.386e-06  o 2.251e-06
"""
import functools
import math
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sr_scores_oracle as O  # noqa: E402

# the kernel's tiling: 16 x 32 output positions in axes 1 and 2, chunks of >= 24 output planes along axis 0.  (68, 47, 80) has
# 58 x 37 x 70 positions: chunks of 20, 20, 18 planes (30 steps of the march each), 2 tiles + 5 rows, 2 tiles + 6 columns
SHAPES = [(11, 11, 11), (12, 11, 13), (19, 23, 37), (68, 47, 80)]
PLANT_SHAPE = (23, 25, 27)
SENTINEL = -777.25


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def volumes(shape, seed=0):
    p, t = O.textured(shape, seed=1000 + seed + sum(shape))
    p.setflags(write=False)
    t.setflags(write=False)
    return p, t


@functools.lru_cache(maxsize=None)
def mask_of(shape, kind):
    if kind == 'none':
        return None
    if kind == 'half':
        m = (np.random.default_rng(7).random(shape) < 0.5).astype(np.int32) * 3
    elif kind == 'border':
        m = np.ones(shape, np.int32)
        m[5:-5, 5:-5, 5:-5] = 0
    else:
        m = np.zeros(shape, np.int32)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle(shape, kind='none', seed=0):
    p, t = volumes(shape, seed)
    return O.scores(p, t, mask_of(shape, kind)), O.scores(p, t, mask_of(shape, kind), dtype=np.float32)


def scores_on_device(pred, truth, mask=None, normalise='none', data_range=None, ssim=True):
    from synthsr_amd.evaluate import image_scores
    return image_scores(pred, truth, mask, normalise=normalise, data_range=data_range, ssim=ssim, return_ssim_map=ssim)


def rule_rows(dev, o64, o32, keys=('ssim', 'ncc', 'scale', 'offset', 'mae', 'rmse', 'max_abs', 'mse', 'ssim_map'), sel=None):
    """[(name, d, o)] under the normalisation of the module docstring"""
    L = o64['data_range']
    rows = []
    for key in keys:
        if key == 'ssim_map':
            s = slice(None) if sel is None else sel
            d = float(np.max(np.abs(dev['ssim_map'].astype(np.float64)[s] - o64['ssim_map'][s])))
            o = float(np.max(np.abs(o32['ssim_map'].astype(np.float64)[s] - o64['ssim_map'][s])))
        else:
            div = {'mae': L, 'rmse': L, 'max_abs': L, 'offset': L, 'mse': L * L}.get(key, 1.0)
            dv = dev['rmse'] ** 2 if key == 'mse' else dev[key]
            d, o = abs(dv - o64[key]) / div, abs(o32[key] - o64[key]) / div
        rows.append((key, d, o))
    return rows


def assert_rule(tag, rows):
    bad = []
    for name, d, o in rows:
        print('sr_scores %-34s %-9s d = %.3e  o = %.3e  bound = %.3e' % (tag, name, d, o, O.K * o + O.FLOOR))
        if not d <= O.K * o + O.FLOOR:
            bad.append((name, d, o))
    assert not bad, (tag, bad)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sr_scores_textured_volumes_match_the_oracle(T, shape):
    p, t = volumes(shape)
    o64, o32 = oracle(shape)
    dev = scores_on_device(p, t)
    assert dev['n_voxels'] == o64['n_voxels'] == int(np.prod(shape))
    assert dev['n_ssim'] == o64['n_ssim'] == int(np.prod([s - 10 for s in shape]))
    assert dev['ssim_map'].shape == o64['ssim_map'].shape
    assert abs(dev['data_range'] - o64['data_range']) == 0    # min and max are exact
    assert_rule('textured %s' % (shape,), rule_rows(dev, o64, o32))
    assert abs(dev['psnr'] - o64['psnr']) < 1e-3


@pytest.mark.parametrize('where', ['centre', 'origin', 'far_corner'])
def test_sr_scores_planted_voxel(T, where):
    _, t = volumes(PLANT_SHAPE)
    v = {'centre': (11, 12, 13), 'origin': (0, 0, 0), 'far_corner': (22, 24, 26)}[where]
    p = t.copy()
    p[v] += 0.3
    dev = scores_on_device(p, t)
    o64, o32 = O.scores(p, t), O.scores(p, t, dtype=np.float32)
    S = dev['ssim_map'].astype(np.float64)
    idx = np.meshgrid(*[np.arange(n) for n in S.shape], indexing='ij')
    touched = np.ones(S.shape, bool)
    for a in range(3):
        touched &= (idx[a] >= v[a] - 10) & (idx[a] <= v[a])    # the window of position c covers voxels c .. c + 10
    assert touched.sum() == {'centre': 11 ** 3, 'origin': 1, 'far_corner': 1}[where]
    away = np.abs(1.0 - S[~touched])
    print('sr_scores planted %-10s max |1 - S| away from the voxel = %.3e' % (where, away.max()))
    assert away.max() <= 1e-6                                   # every untouched position, none left out
    assert np.all(o64['ssim_map'][~touched] == 1) and np.all(o64['ssim_map'][touched] < 1)
    assert_rule('planted %s' % where, rule_rows(dev, o64, o32, keys=('ssim', 'mae', 'rmse', 'max_abs', 'ssim_map'), sel=touched))
    assert dev['n_ssim'] == o64['n_ssim']


def test_sr_scores_identical_volumes(T):
    _, t = volumes((19, 23, 37))
    dev = scores_on_device(t, t)
    o64, o32 = O.scores(t, t), O.scores(t, t, dtype=np.float32)
    assert abs(dev['ssim'] - 1) <= 1e-6 and np.max(np.abs(dev['ssim_map'] - 1)) <= 1e-6
    assert dev['mae'] == 0 and dev['rmse'] == 0 and dev['max_abs'] == 0 and dev['psnr'] == math.inf
    assert_rule('identical', rule_rows(dev, o64, o32, keys=('ncc', 'scale', 'offset', 'ssim')))


def test_sr_scores_offset_dominated_moments(T):
    """1000 + unit noise: plain fp32 sums of p^2 lose the variance (p^2 = 1e6 carries 0.06 of rounding per term)"""
    rng = np.random.default_rng(21)
    shape = (19, 23, 37)
    noise = rng.standard_normal(shape)
    p = (1000.0 + noise).astype(np.float32)
    t = (1000.0 + 0.8 * noise + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    for kind in ('none', 'half'):
        m = mask_of(shape, kind)
        dev = scores_on_device(p, t, m, ssim=False)
        o64, o32 = O.scores(p, t, m, ssim=False), O.scores(p, t, m, dtype=np.float32, ssim=False)
        assert dev['n_voxels'] == o64['n_voxels']
        assert 0.9 < o64['ncc'] < 0.96 and 0.75 < o64['scale'] < 0.85
        assert_rule('offset-dominated %s' % kind, rule_rows(dev, o64, o32, keys=('ncc', 'scale', 'offset', 'mae', 'rmse', 'max_abs')))


@pytest.mark.parametrize('kind', ['none', 'half', 'border', 'zero'])
@pytest.mark.parametrize('shape', [(19, 23, 37), (68, 47, 80)], ids=lambda s: 'x'.join(map(str, s)))
def test_sr_scores_masks(T, shape, kind):
    p, t = volumes(shape)
    m = mask_of(shape, kind)
    o64, o32 = oracle(shape, kind)
    dev = scores_on_device(p, t, m)
    assert dev['n_voxels'] == o64['n_voxels'] and dev['n_ssim'] == o64['n_ssim']    # counts: exactly
    if kind == 'zero':
        assert dev['n_voxels'] == 0 and dev['n_ssim'] == 0
        assert all(math.isnan(dev[k]) for k in ('mae', 'rmse', 'max_abs', 'psnr', 'ncc', 'scale', 'offset', 'ssim'))
        return
    keys = ('ncc', 'scale', 'offset', 'mae', 'rmse', 'max_abs', 'mse')
    if kind == 'border':
        assert dev['n_voxels'] > 0 and dev['n_ssim'] == 0 and math.isnan(dev['ssim'])
        assert_rule('mask border %s' % (shape,), rule_rows(dev, o64, o32, keys=keys + ('ssim_map',)))   # the map ignores the mask
    else:
        assert_rule('mask %s %s' % (kind, shape), rule_rows(dev, o64, o32, keys=keys + ('ssim', 'ssim_map')))


def test_sr_scores_affine_normalisation(T):
    shape = (19, 23, 37)
    _, t = volumes(shape)
    p = (0.5 * t.astype(np.float64) + 7.0 + 0.002 * np.random.default_rng(31).standard_normal(shape)).astype(np.float32)
    dev = scores_on_device(p, t, normalise='affine')
    o64, o32 = O.scores(p, t, normalise='affine'), O.scores(p, t, normalise='affine', dtype=np.float32)
    assert abs(dev['scale'] - 2.0) < 0.02 and abs(dev['offset'] + 14.0) < 0.15
    assert dev['ssim'] > 0.95 and dev['mae'] < 0.01
    assert_rule('affine', rule_rows(dev, o64, o32))
    plain = scores_on_device(p, t)
    assert plain['mae'] > 6 and plain['ssim'] < dev['ssim']     # without the map the prediction is far off


def test_sr_scores_run_to_run_bits(T):
    from synthsr_amd import ops
    shape = (68, 47, 80)
    p, t = (T.from_numpy(v.copy()).cuda() for v in volumes(shape))
    m = T.from_numpy(mask_of(shape, 'half').copy()).cuda()
    runs = []
    for _ in range(2):
        ws = T.empty(ops.sr_scores_workspace_bytes(shape), dtype=T.uint8, device='cuda').random_(0, 256)   # no initialisation needed
        s, smap = ops.sr_ssim3d(p, t, m, 0.9, 0.01, 0.7, want_map=True, workspace=ws)
        runs.append((ops.sr_moments(p, t, m, workspace=ws).clone(), ops.sr_errors(p, t, m, 0.9, 0.01, workspace=ws).clone(),
                     s.clone(), smap.clone()))
    for a, b in zip(*runs):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert float(runs[0][2][1]) > 0


def test_sr_scores_refusals_write_nothing(T):
    from synthsr_amd import _lib, ops
    lib = _lib.load()
    shape = (12, 13, 14)
    p = T.rand(shape, device='cuda')
    t = T.rand(shape, device='cuda')
    need = ops.sr_scores_workspace_bytes(shape)
    assert need == int(lib.synthsr_sr_scores_workspace_bytes(_lib.i3(shape))) > 0
    assert int(lib.synthsr_sr_scores_workspace_bytes(_lib.i3((12, 0, 14)))) == -1
    ws = T.full((need,), 0xA5, dtype=T.uint8, device='cuda')
    out = T.full((12,), SENTINEL, dtype=T.float64, device='cuda')
    smap = T.full((2, 3, 4), SENTINEL, dtype=T.float32, device='cuda')
    P = _lib.ptr
    calls = {
        'ssim side 10': lambda: lib.synthsr_sr_ssim3d(P(p), P(t), None, _lib.i3((10, 13, 14)), 1.0, 0.0, 1.0, P(out), P(smap), P(ws),
                                                      need, _lib.stream()),
        'ssim workspace': lambda: lib.synthsr_sr_ssim3d(P(p), P(t), None, _lib.i3(shape), 1.0, 0.0, 1.0, P(out), P(smap), P(ws),
                                                        need - 8, _lib.stream()),
        'moments workspace': lambda: lib.synthsr_sr_moments(P(p), P(t), None, _lib.i3(shape), P(out), P(ws), need - 8, _lib.stream()),
        'errors workspace': lambda: lib.synthsr_sr_errors(P(p), P(t), None, _lib.i3(shape), 1.0, 0.0, P(out), P(ws), need - 8,
                                                          _lib.stream()),
        'moments side 0': lambda: lib.synthsr_sr_moments(P(p), P(t), None, _lib.i3((12, 0, 14)), P(out), P(ws), need, _lib.stream()),
        'errors null volume': lambda: lib.synthsr_sr_errors(None, P(t), None, _lib.i3(shape), 1.0, 0.0, P(out), P(ws), need,
                                                            _lib.stream()),
    }
    for name, call in calls.items():
        assert call() == -1, name
        T.cuda.synchronize()
        assert bool((out == SENTINEL).all()) and bool((smap == SENTINEL).all()) and bool((ws == 0xA5).all()), name
    with pytest.raises(ValueError):
        ops.sr_ssim3d(p[:10].contiguous(), t[:10].contiguous())
    # and the accepted call does write
    assert lib.synthsr_sr_moments(P(p), P(t), None, _lib.i3(shape), P(out), P(ws), need, _lib.stream()) == 0
    T.cuda.synchronize()
    assert float(out[0]) == p.numel()


def test_sr_scores_score_predictions_end_to_end(T, tmp_path):
    """two NIfTI pairs, the second truth on a 2 mm grid (resliced onto its prediction's grid), masks given as label maps"""
    from synthsr_amd import volumes as V
    from synthsr_amd.evaluate import score_predictions, image_scores, COLUMNS
    shape = (14, 16, 18)
    aff = np.diag([1.0, 1.0, 1.0, 1.0])
    aff[:3, 3] = (-3.0, 5.0, 2.0)
    aff2 = aff.copy()
    aff2[:3, :3] *= 2.0
    aff2[:3, 3] += 0.5          # voxel centres of the 2 mm grid sit between those of the 1 mm grid
    for sub in ('pred', 'truth', 'mask'):
        os.makedirs(str(tmp_path / sub))
    for i in range(2):
        p, t = O.textured(shape, seed=50 + i)
        lab = np.random.default_rng(60 + i).integers(0, 4, size=shape).astype(np.float64)
        V.save_volume(100.0 * p, aff, None, str(tmp_path / 'pred' / ('s%d.nii.gz' % i)))
        if i == 0:
            V.save_volume(100.0 * t, aff, None, str(tmp_path / 'truth' / ('s%d.nii.gz' % i)))
        else:
            V.save_volume(100.0 * t[::2, ::2, ::2], aff2, None, str(tmp_path / 'truth' / ('s%d.nii.gz' % i)))
        V.save_volume(lab, aff, None, str(tmp_path / 'mask' / ('s%d.nii.gz' % i)))
    table = score_predictions(str(tmp_path / 'pred'), str(tmp_path / 'truth'), str(tmp_path / 'scores.csv'),
                              path_masks=str(tmp_path / 'mask'), mask_labels=[2, 3], normalise='affine', verbose=False)
    assert table['names'] == ['s0.nii.gz', 's1.nii.gz', 'mean'] and table['values'].shape == (3, len(COLUMNS))
    for i in range(2):
        pred, a_p, _ = V.load_volume(str(tmp_path / 'pred' / ('s%d.nii.gz' % i)), im_only=False)
        truth, a_t, _ = V.load_volume(str(tmp_path / 'truth' / ('s%d.nii.gz' % i)), im_only=False)
        if i == 1:
            assert truth.shape == (7, 8, 9)
            truth = V.resample_volume_like(pred, a_p, truth, a_t)
        lab = V.load_volume(str(tmp_path / 'mask' / ('s%d.nii.gz' % i)))
        want = image_scores(pred, truth, np.isin(lab, [2, 3]), normalise='affine')
        np.testing.assert_array_equal(table['values'][i], np.array([float(want[c]) for c in COLUMNS]))
        assert 0 < want['n_ssim'] < want['n_voxels'] < pred.size and want['ssim'] < 1
    np.testing.assert_allclose(table['values'][2], table['values'][:2].mean(axis=0), rtol=1e-12)
    assert table['values'][0, COLUMNS.index('ssim')] > table['values'][1, COLUMNS.index('ssim')]   # the resliced truth is blurrier
    lines = open(str(tmp_path / 'scores.csv')).read().splitlines()
    assert len(lines) == 4 and lines[3].startswith('mean,')
    one = score_predictions(str(tmp_path / 'pred' / 's0.nii.gz'), str(tmp_path / 'truth' / 's0.nii.gz'),
                            str(tmp_path / 'one.npy'), verbose=False)
    np.testing.assert_array_equal(np.load(str(tmp_path / 'one.npy')), one['values'])
    assert one['values'].shape == (2, len(COLUMNS)) and one['values'][0, 0] == pred.size
