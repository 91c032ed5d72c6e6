"""Image-quality scores of super-resolved volumes against their ground truth: MAE, RMSE, maximum error, PSNR, normalised
cross-correlation, the least-squares intensity map and the 3-D SSIM, optionally inside a mask.

The sums come from the HIP kernels of csrc/sr_scores.hip (`ops.sr_moments`, `ops.sr_errors`, `ops.sr_ssim3d`);
`scores_from_sums` turns them into the scores in float64 on the host.  There is no CPU path for the sums.
"""
import math
import os

import numpy as np

from . import volumes as V

COLUMNS = ('n_voxels', 'mae', 'rmse', 'max_abs', 'psnr', 'ncc', 'scale', 'offset', 'ssim', 'n_ssim', 'data_range')
NAN = float('nan')


def fit_from_moments(moments):
    """(n, mean_p, mean_t, var_p, var_t, cov) in float64 from the 12 values of `ops.sr_moments`"""
    m = [float(v) for v in moments]
    n = m[0]
    if n <= 0:
        return 0.0, NAN, NAN, NAN, NAN, NAN
    ep, et = m[3] / n, m[4] / n
    return n, m[1] + ep, m[2] + et, m[5] / n - ep * ep, m[6] / n - et * et, m[7] / n - ep * et


def affine_from_moments(moments):
    """least-squares (a, b) of truth ~ a pred + b over the masked voxels; NaN where the prediction is constant or n = 0"""
    n, mp, mt, vp, vt, cov = fit_from_moments(moments)
    if n <= 0 or not vp > 0:
        return NAN, NAN
    a = cov / vp
    return a, mt - a * mp


def scores_from_sums(moments, errors=None, ssim=None, data_range=None):
    """The scores, from the kernels' sums alone (pure host float64).

    moments [12]: n, shift_p, shift_t, S p', S t', S p'^2, S t'^2, S p't', min p, max p, min t, max t (shifted sums);
    errors [4] or None: n, S |d|, S d^2, max |d| of d = (mapped prediction) - truth;  ssim [2] or None: S ssim, count.
    data_range: L of the PSNR; None = max t - min t of the moments.
    Returns a dict with the keys of COLUMNS.  With n = 0 (or no valid SSIM centre) the affected scores are NaN and the
    counts 0; nothing raises.  psnr is +inf for a zero mean squared error; ncc is NaN when either volume is constant."""
    m = [float(v) for v in moments]
    n, mp, mt, vp, vt, cov = fit_from_moments(m)
    out = dict.fromkeys(COLUMNS, NAN)
    out['n_voxels'] = int(n)
    out['n_ssim'] = 0
    if data_range is None:
        data_range = m[11] - m[10] if n > 0 else NAN
    out['data_range'] = float(data_range)
    if n > 0:
        if vp > 0 and vt > 0:
            out['ncc'] = cov / math.sqrt(vp * vt)
        out['scale'], out['offset'] = affine_from_moments(m)
    if errors is not None and float(errors[0]) > 0:
        ne, sabs, ssq, mx = [float(v) for v in errors]
        mse = ssq / ne
        out['mae'], out['rmse'], out['max_abs'] = sabs / ne, math.sqrt(mse), mx
        if data_range > 0 and math.isfinite(data_range):
            out['psnr'] = math.inf if mse == 0 else 10.0 * math.log10(data_range * data_range / mse)
    if ssim is not None and float(ssim[1]) > 0:
        out['ssim'] = float(ssim[0]) / float(ssim[1])
        out['n_ssim'] = int(ssim[1])
    return out


def check_arguments(shape_pred, shape_truth, shape_mask=None, normalise='none', data_range=None, ssim=True):
    """the argument checks of image_scores (no device needed)"""
    if tuple(shape_pred) != tuple(shape_truth) or len(shape_pred) != 3:
        raise ValueError('image_scores takes two 3-D volumes of one shape (got %s and %s)' % (tuple(shape_pred), tuple(shape_truth)))
    if shape_mask is not None and tuple(shape_mask) != tuple(shape_pred):
        raise ValueError('image_scores: the mask has shape %s, the volumes %s' % (tuple(shape_mask), tuple(shape_pred)))
    if normalise not in ('none', 'affine'):
        raise ValueError("normalise should be 'none' or 'affine', had %r" % (normalise,))
    if data_range is not None and not (math.isfinite(float(data_range)) and float(data_range) > 0):
        raise ValueError('data_range should be a finite positive number, had %r' % (data_range,))
    if ssim and min(shape_pred) < 11:
        raise ValueError('the 3-D SSIM needs every side >= 11 (got %s); pass ssim=False for the other scores' % (tuple(shape_pred),))


def image_scores(pred, truth, mask=None, normalise='none', data_range=None, ssim=True, return_ssim_map=False, device=None):
    """Scores of `pred` against `truth` (numpy arrays or torch tensors [d0, d1, d2]) over the voxels where `mask` is non-zero
    (None: everywhere).  normalise='affine' maps the prediction with the least-squares a pred + b before the errors and the
    SSIM.  data_range (L of PSNR and SSIM): None = the truth's max - min over the mask.  Returns the dict of
    scores_from_sums (plus 'ssim_map', float32 numpy [d0 - 10, d1 - 10, d2 - 10], if asked for)."""
    import torch
    from . import ops
    check_arguments(np.shape(pred), np.shape(truth), None if mask is None else np.shape(mask), normalise, data_range, ssim)
    device = device or 'cuda'

    def dev(v, dtype):
        if not torch.is_tensor(v):
            v = np.ascontiguousarray(v)
            v = torch.from_numpy(v if v.flags.writeable else v.copy())
        return v.to(device=device, dtype=dtype).contiguous()

    p, t = dev(pred, torch.float32), dev(truth, torch.float32)
    m = None
    if mask is not None:
        m = (dev(mask, None) != 0).to(torch.int32).contiguous()
    ws = torch.empty(ops.sr_scores_workspace_bytes(p.shape), dtype=torch.uint8, device=p.device)
    moments = ops.sr_moments(p, t, m, workspace=ws).cpu().numpy()
    a, b = affine_from_moments(moments) if normalise == 'affine' else (1.0, 0.0)
    L = float(data_range) if data_range is not None else (float(moments[11] - moments[10]) if moments[0] > 0 else NAN)
    errors = ssim_sums = ssim_map = None
    if moments[0] > 0 and math.isfinite(a) and math.isfinite(b):
        errors = ops.sr_errors(p, t, m, a, b, workspace=ws).cpu().numpy()
        if ssim and L > 0 and math.isfinite(L):
            s, smap = ops.sr_ssim3d(p, t, m, a, b, 1.0 / L, want_map=return_ssim_map, workspace=ws)
            ssim_sums = s.cpu().numpy()
            ssim_map = None if smap is None else smap.cpu().numpy()
    out = scores_from_sums(moments, errors, ssim_sums, data_range=L)
    if return_ssim_map:
        out['ssim_map'] = ssim_map
    return out


def _list(path):
    """a file -> [file]; a folder -> its volumes, sorted (the extension handling of predict())"""
    path = os.path.abspath(path)
    if not any(ext in os.path.basename(path) for ext in ('.nii.gz', '.nii', '.mgz', '.npz')):
        if os.path.isfile(path):
            raise Exception('extension not supported for %s, only use: nii.gz, .nii, .mgz, or .npz' % path)
        return V.list_images_in_folder(path)
    assert os.path.isfile(path), 'files does not exist: %s \nplease make sure the path and the extension are correct' % path
    return [path]


def _on_grid(ref, aff_ref, vol, aff, interpolation):
    if vol.shape == ref.shape and np.allclose(aff, aff_ref, atol=1e-5):
        return vol
    return V.resample_volume_like(ref, aff_ref, vol, aff, interpolation=interpolation)


def write_scores(path, names, values):
    """.npy: the float64 table [rows, len(COLUMNS)]; anything else: CSV with a header line and the row names first"""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    values = np.asarray(values, dtype=np.float64)
    if path.endswith('.npy'):
        np.save(path, values)
        return
    with open(path, 'w') as f:
        f.write(','.join(('name',) + COLUMNS) + '\n')
        for name, row in zip(names, values):
            f.write(','.join([name] + [repr(float(v)) for v in row]) + '\n')


def score_predictions(path_predictions, path_truth, path_scores=None, path_masks=None, mask_labels=None, normalise='none',
                      data_range=None, verbose=True, device=None):
    """Scores every prediction against its ground truth.  The paths are files, or folders sorted alike.  A truth (or mask) on
    another voxel grid is resliced onto the prediction's grid (volumes.resample_volume_like; masks with nearest neighbour).
    mask_labels: the mask is where the mask volume holds one of these values (None: where it is non-zero).
    Returns {'names': [..., 'mean'], 'columns': COLUMNS, 'values': float64 [n + 1, len(COLUMNS)]}: one row per volume and
    the mean row (non-finite entries left out of the mean); written to path_scores (.npy, or CSV for any other name) if given."""
    preds, truths = _list(path_predictions), _list(path_truth)
    masks = _list(path_masks) if path_masks is not None else [None] * len(preds)
    if len(truths) != len(preds) or len(masks) != len(preds):
        raise ValueError('%d predictions, %d ground truths and %d masks' % (len(preds), len(truths), len(masks)))
    if verbose:
        print('Found %d images' % len(preds))
    rows = []
    for i, (pp, pt, pm) in enumerate(zip(preds, truths, masks)):
        if verbose:
            print('  Scoring image %d ' % (i + 1))
            print('  ' + pp + ' against ' + pt)
        pred, aff, _ = V.load_volume(pp, im_only=False, dtype='float')
        truth, aff_t, _ = V.load_volume(pt, im_only=False, dtype='float')
        truth = _on_grid(pred, aff, truth, aff_t, 'linear')
        mask = None
        if pm is not None:
            mv, aff_m, _ = V.load_volume(pm, im_only=False, dtype='float')
            mv = np.round(_on_grid(pred, aff, mv, aff_m, 'nearest'))
            mask = (mv != 0) if mask_labels is None else np.isin(mv, np.asarray(list(mask_labels), dtype=np.float64))
        s = image_scores(pred, truth, mask, normalise=normalise, data_range=data_range, ssim=min(pred.shape) >= 11, device=device)
        rows.append([float(s[c]) for c in COLUMNS])
    values = np.asarray(rows, dtype=np.float64).reshape(len(rows), len(COLUMNS))
    with np.errstate(all='ignore'):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            mean = np.nanmean(np.where(np.isfinite(values), values, np.nan), axis=0)
    values = np.concatenate([values, mean[None]], axis=0)
    names = [os.path.basename(p) for p in preds] + ['mean']
    if path_scores is not None:
        write_scores(path_scores, names, values)
    return {'names': names, 'columns': COLUMNS, 'values': values}
