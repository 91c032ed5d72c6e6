"""Host side of the image scores (synthsr_amd/evaluate.py, scripts/score_predictions.py) and the numpy oracle the GPU tests
use (tests/_sr_scores_oracle.py).  No GPU."""
import importlib.util
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _sr_scores_oracle as O  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sums_of(pred, truth, mask=None, a=1.0, b=0.0, data_range=None, shift=(0.0, 0.0)):
    """the kernels' sums, made by hand in float64: (moments [12], errors [4], ssim [2])"""
    sel = np.ones(pred.shape, bool) if mask is None else mask != 0
    p, t = pred[sel].astype(np.float64), truth[sel].astype(np.float64)
    n = p.size
    if n == 0:
        return [0, 0, 0, 0, 0, 0, 0, 0, np.inf, -np.inf, np.inf, -np.inf], [0, 0, 0, 0], [0, 0]
    dp, dt = p - shift[0], t - shift[1]
    mom = [n, shift[0], shift[1], dp.sum(), dt.sum(), (dp * dp).sum(), (dt * dt).sum(), (dp * dt).sum(), p.min(), p.max(),
           t.min(), t.max()]
    d = a * p + b - t
    err = [n, np.abs(d).sum(), (d * d).sum(), np.abs(d).max()]
    L = data_range if data_range is not None else t.max() - t.min()
    ss = [0, 0]
    if L > 0 and min(pred.shape) >= 11:
        S = O.ssim_map(pred, truth, a, b, L)
        c = O.centre_mask(mask, pred.shape)
        ss = [S[c].sum(), c.sum()]
    return mom, err, ss


def close(a, b, tol=1e-10):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= tol * max(1.0, abs(b))


@pytest.mark.parametrize('shift', [(0.0, 0.0), (0.37, -1.2)])
@pytest.mark.parametrize('masked', [False, True])
def test_sr_scores_from_sums_match_the_oracle(shift, masked):
    from synthsr_amd.evaluate import scores_from_sums, COLUMNS
    pred, truth = O.textured((13, 12, 15), seed=3)
    mask = (np.random.default_rng(4).random(pred.shape) < 0.5).astype(np.int32) if masked else None
    want = O.scores(pred, truth, mask)
    got = scores_from_sums(*sums_of(pred, truth, mask, shift=shift))
    assert set(got) == set(COLUMNS)
    for key in COLUMNS:
        assert close(got[key], want[key]), (key, got[key], want[key])
    assert got['n_voxels'] == want['n_voxels'] and got['n_ssim'] == want['n_ssim'] > 0


def test_sr_scores_from_sums_degenerate_inputs():
    from synthsr_amd.evaluate import scores_from_sums, affine_from_moments
    pred, truth = O.textured((12, 11, 13), seed=5)
    # n = 0: every score NaN, the counts 0, nothing raises
    got = scores_from_sums(*sums_of(pred, truth, np.zeros(pred.shape, np.int32)))
    assert got['n_voxels'] == 0 and got['n_ssim'] == 0
    assert all(math.isnan(got[k]) for k in ('mae', 'rmse', 'max_abs', 'psnr', 'ncc', 'scale', 'offset', 'ssim', 'data_range'))
    # mse = 0: psnr +inf, mae 0, ncc 1, the identity map
    got = scores_from_sums(*sums_of(truth, truth))
    assert got['psnr'] == math.inf and got['mae'] == 0 and got['rmse'] == 0 and got['max_abs'] == 0
    assert abs(got['ncc'] - 1) < 1e-12 and abs(got['scale'] - 1) < 1e-12 and abs(got['offset']) < 1e-12
    assert abs(got['ssim'] - 1) < 1e-12
    # constant truth: NCC NaN, data range 0 -> no PSNR; the errors still stand
    const = np.full(pred.shape, 0.5, np.float32)
    got = scores_from_sums(*sums_of(pred, const))
    assert math.isnan(got['ncc']) and math.isnan(got['psnr']) and got['data_range'] == 0 and got['mae'] > 0
    # constant prediction: no least-squares map
    assert all(math.isnan(v) for v in affine_from_moments(sums_of(const, truth)[0]))
    # border-only mask: voxels but no SSIM centre
    border = np.ones(pred.shape, np.int32)
    border[5:-5, 5:-5, 5:-5] = 0
    got = scores_from_sums(*sums_of(pred, truth, border))
    assert got['n_voxels'] > 0 and got['n_ssim'] == 0 and math.isnan(got['ssim']) and got['mae'] > 0


def test_sr_scores_argument_checks():
    from synthsr_amd.evaluate import check_arguments, image_scores
    check_arguments((11, 12, 13), (11, 12, 13), (11, 12, 13), 'affine', 2.0, True)
    check_arguments((5, 12, 13), (5, 12, 13), None, 'none', None, False)
    for bad in (dict(shape_truth=(11, 12, 14)), dict(shape_mask=(11, 12, 12)), dict(normalise='zscore'), dict(data_range=0.0),
                dict(data_range=-1.0), dict(data_range=float('inf')), dict(data_range=float('nan')),
                dict(shape_pred=(10, 12, 13), shape_truth=(10, 12, 13))):
        kw = dict(shape_pred=(11, 12, 13), shape_truth=(11, 12, 13), shape_mask=None, normalise='none', data_range=None, ssim=True)
        kw.update(bad)
        with pytest.raises(ValueError):
            check_arguments(**kw)
    # image_scores refuses before it touches a device
    z = np.zeros((11, 12, 13), np.float32)
    with pytest.raises(ValueError):
        image_scores(z, np.zeros((11, 12, 14), np.float32))
    with pytest.raises(ValueError):
        image_scores(z, z, data_range=float('nan'))
    with pytest.raises(ValueError):
        image_scores(z[:10], z[:10])


def test_sr_scores_writer_csv_and_npy(tmp_path):
    from synthsr_amd.evaluate import write_scores, COLUMNS
    values = np.arange(2 * len(COLUMNS), dtype=np.float64).reshape(2, -1) / 7.0
    values[1, 4] = np.inf
    values[0, 5] = np.nan
    write_scores(str(tmp_path / 'sub' / 's.npy'), ['a.nii.gz', 'mean'], values)
    np.testing.assert_array_equal(np.load(str(tmp_path / 'sub' / 's.npy')), values)
    write_scores(str(tmp_path / 's.csv'), ['a.nii.gz', 'mean'], values)
    lines = open(str(tmp_path / 's.csv')).read().splitlines()
    assert lines[0].split(',') == ['name'] + list(COLUMNS) and len(lines) == 3
    for line, name, row in zip(lines[1:], ['a.nii.gz', 'mean'], values):
        cells = line.split(',')
        assert cells[0] == name
        np.testing.assert_array_equal(np.array([float(c) for c in cells[1:]]), row)   # repr round-trips, nan and inf included


def test_sr_scores_script_parser():
    spec = importlib.util.spec_from_file_location('score_predictions_script', os.path.join(REPO, 'scripts', 'score_predictions.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    a = p.parse_args(['P', 'T'])
    assert (a.path_predictions, a.path_truth, a.scores, a.masks, a.mask_labels, a.normalise, a.data_range) == \
        ('P', 'T', None, None, None, 'none', None)
    a = p.parse_args(['P', 'T', '--scores', 'S.csv', '--masks', 'M', '--mask_labels', '2', '41', '--normalise', 'affine',
                      '--data_range', '128'])
    assert (a.scores, a.masks, a.mask_labels, a.normalise, a.data_range) == ('S.csv', 'M', [2.0, 41.0], 'affine', 128.0)
    with pytest.raises(SystemExit):
        p.parse_args(['P', 'T', '--normalise', 'zscore'])
    with pytest.raises(SystemExit):
        mod.main(['P', 'T', '--mask_labels', '3'])
    with pytest.raises(SystemExit):
        mod.main(['P', 'T', '--data_range', '0'])


def test_sr_scores_oracle_ssim_matches_correlate1d():
    pred, truth = O.textured((14, 17, 13), seed=11)
    a, b, L = 0.9, 0.03, 1.7
    S = O.ssim_map(pred, truth, a, b, L)
    assert S.shape == (4, 7, 3)
    np.testing.assert_allclose(S, O.ssim_map_correlate1d(pred, truth, a, b, L), rtol=0, atol=1e-12)
    assert abs(O.taps().sum() - 1) < 1e-15 and O.taps().argmax() == 5


def test_sr_scores_oracle_identical_volumes_give_exactly_one():
    _, truth = O.textured((12, 13, 11), seed=12)
    for dtype in (np.float64, np.float32):
        S = O.ssim_map(truth, truth, dtype=dtype)
        assert S.dtype == dtype and np.all(S == 1)


def test_sr_scores_oracle_inverted_volume_scores_negative():
    _, x = O.textured((15, 15, 15), seed=13)
    x = ((x - x.min()) / (x.max() - x.min())).astype(np.float32)
    s = O.scores(1.0 - x, x, data_range=1.0)
    assert s['ssim'] < 0 and s['ncc'] < -0.999
