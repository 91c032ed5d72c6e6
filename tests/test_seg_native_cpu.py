"""Host side of label maps on the input image's own voxel grid (no GPU): the float64 oracle of synthsr_seg_resample_argmax
(tests/_seg_native_oracle.py) against volumes.resample_volume_like, predict_segmentation.native_grid_affine against the host
resampler of predict.prepare_volume, the declaration and the argument checks of the C entry point (csrc/seg_resample.hip), which
returns before any HIP call, the checks of ops.seg_resample_argmax, and the command line of scripts/predict_segmentation.py."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_native_oracle as O  # noqa: E402


def _script():
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------- the oracle
def test_oracle_follows_resample_volume_like():
    """with the whole source as the box, every channel of the oracle is volumes.resample_volume_like of that channel wherever
    that function calls a voxel inside (0 <= pos <= n - 1; the oracle's half-voxel rim lies outside it and is clamped)"""
    from synthsr_amd import volumes as V
    probs = O.softmax_posteriors((6, 7, 9), 3, seed=1)
    c, s = np.cos(0.3), np.sin(0.3)
    aff_flo = np.eye(4)
    aff_ref = np.array([[0.37 * c, -0.9 * s, 0, 1.3], [0.37 * s, 0.9 * c, 0, 0.2], [0, 0, 1.7, -0.4], [0, 0, 0, 1]])
    out_shape = (14, 9, 7)
    got = O.resample_argmax(probs, [0, 0, 0, 5, 6, 8], aff_ref[:3], out_shape, [4, 5, 6], 9)
    assert got['near_boundary'] == 0
    pos = np.einsum('ab,b...->a...', aff_ref[:3, :3], np.stack(np.meshgrid(*[np.arange(n) for n in out_shape], indexing='ij'))) \
        + aff_ref[:3, 3].reshape(3, 1, 1, 1)
    strict = np.all((pos >= 0) & (pos <= np.array([5, 6, 8]).reshape(3, 1, 1, 1)), axis=0)
    assert 0 < strict.sum() < got['inside'].sum() < strict.size
    for n in range(3):
        want = V.resample_volume_like(np.zeros(out_shape), aff_ref, probs[..., n].astype(np.float64), aff_flo)
        assert np.abs(got['probs'][..., n] - want)[strict].max() < 1e-7      # the oracle rounds its weights to float32
    assert np.all(got['label'][~got['inside']] == 9) and np.all(got['probs'][~got['inside']] == 0)
    assert np.array_equal(got['label'][got['inside']], (4 + np.argmax(got['probs'], -1))[got['inside']])
    assert np.all(got['margin'][got['inside']] >= 0) and np.all(np.isinf(got['margin'][~got['inside']]))


# ---------------------------------------------------------------------------------------------------- the matrix
def test_native_grid_affine_against_the_host_resampler():
    """A volume that is a linear ramp in world coordinates, voxels of 2 x 1.5 x 1 mm, LIA-like orientation, pushed through
    resample_volume, align_volume_to_ref and the padding of prepare_volume, then interpolated back at every native voxel with
    the oracle and the composed matrix.  resample_volume clamps its sampling positions to the native grid (_axis_samples), so
    the 1 mm array holds the ramp at the clamped positions; interpolated back, native voxel v reproduces the ramp at
    np.interp(position of v in the 1 mm array, 1 mm index, clamped native position): v itself everywhere but in the first and
    last voxel of an up-sampled axis (and the 1 mm axis, which resample_volume smooths, keeps the smoothed end values).  Every
    native voxel is held to 1e-9 of the ramp's range against that, and every voxel away from the ends to 1e-9 against the ramp
    itself; a half-voxel shift, an axis permutation or a wrong idx in the matrix moves every voxel by far more."""
    from synthsr_amd import volumes as V
    from synthsr_amd.predict import prepare_volume
    from synthsr_amd.predict_segmentation import native_grid_affine
    shape = (9, 12, 14)
    aff = np.array([[-2.0, 0, 0, 31.5], [0, 0, 1.0, -20.25], [0, -1.5, 0, 12.75], [0, 0, 0, 1]])     # L, I, A
    g = np.array([0.013, -0.021, 0.017])                                                              # per mm of world x, y, z
    ijk = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing='ij'), -1)
    ramp_at = lambda p: (p @ aff[:3, :3].T + aff[:3, 3]) @ g + 5.0                                    # p: native voxel positions
    ramp = ramp_at(ijk)
    span = ramp.max() - ramp.min()
    im, aff1 = V.resample_volume(ramp, aff, [1.0, 1.0, 1.0])
    im, aff2 = V.align_volume_to_ref(im, aff1, aff_ref=np.eye(4), return_aff=True, n_dims=3)
    shape1 = np.array(im.shape)
    W = (np.ceil(shape1 / 32.0) * 32).astype('int')
    idx = np.floor((W - shape1) / 2).astype('int')
    S = np.zeros(W)
    S[idx[0]:idx[0] + shape1[0], idx[1]:idx[1] + shape1[1], idx[2]:idx[2] + shape1[2]] = im
    _, p_idx, p_shape, p_aff = prepare_volume(ramp, aff)        # the same frame (prepare_volume also normalises intensities)
    assert np.array_equal(p_idx, idx) and np.array_equal(p_shape, shape1) and np.allclose(p_aff, aff2, atol=0, rtol=0)
    assert np.any(idx > 0) and tuple(shape1) != tuple(W)

    M = native_grid_affine(aff, aff2, idx)
    assert M.shape == (3, 4) and M.dtype == np.float64
    box = list(idx) + list(idx + shape1 - 1)
    got = O.resample_argmax(np.stack([S, -S], -1), box, M, shape, [0, 1], 7)
    assert got['inside'].all() and got['near_boundary'] == 0
    # where the host resampler took its samples: per native axis the clamped positions, in the order of its 1 mm samples
    expect_pos = np.empty(shape + (3,))
    vox = np.array([2.0, 1.5, 1.0])
    for a in range(3):
        samples = V._axis_samples(shape[a], vox[a])                       # native positions of the 1 mm samples of native axis a
        ras_axis = int(np.argmax(np.abs(M[:, a])))                         # the axis of S that native axis a runs along
        u = (M[ras_axis, a] * np.arange(shape[a]) + M[ras_axis, 3]) - idx[ras_axis]     # 1 mm index of native voxel 0 .. n-1
        flipped = M[ras_axis, a] < 0
        u = (len(samples) - 1 - u) if flipped else u                       # in the order resample_volume produced them
        assert u.min() >= -1e-9 and u.max() <= len(samples) - 1 + 1e-9 and len(samples) == shape1[ras_axis]
        at = np.interp(u, np.arange(len(samples)), samples)
        interior = slice(1, -1) if vox[a] != 1.0 else slice(None)
        assert np.abs(at - np.arange(shape[a]))[interior].max() < 1e-12, 'interior voxels come back at their own index'
        view = [None] * 3
        view[a] = slice(None)
        expect_pos[..., a] = np.broadcast_to(at[tuple(view)], shape)
    # the 1 mm axis is not up-sampled: resample_volume smooths it with sigma 0.25 voxels, which leaves a ramp alone except in
    # its first and last voxel (the filter reflects there); its positions are whole numbers, so those two values come back as
    # they are
    from scipy.ndimage import gaussian_filter
    smoothing = gaussian_filter(ramp, [0, 0, 0.25]) - ramp
    assert np.abs(smoothing[:, :, 1:-1]).max() < 1e-12 * span and np.abs(smoothing).max() > 1e-7 * span
    err = np.abs(got['probs'][..., 0] - (ramp_at(expect_pos) + smoothing)).max() / span
    inner = np.abs(got['probs'][1:-1, 1:-1, 1:-1, 0] - ramp[1:-1, 1:-1, 1:-1]).max() / span
    print('ramp through the host resampler and back: %.3g of its range at every voxel, %.3g against the ramp itself inside'
          % (err, inner))
    assert err <= 1e-9 and inner <= 1e-9
    # what the check is worth: the obvious mistakes are far outside the bound
    for wrong in (native_grid_affine(aff, aff2, idx * 0), native_grid_affine(aff, aff2, idx) + np.array([[0, 0, 0, .5]] * 3),
                  native_grid_affine(aff[:, [1, 0, 2, 3]], aff2, idx)):
        bad = O.resample_argmax(np.stack([S, -S], -1), box, wrong, shape, [0, 1], 7)
        assert np.abs(bad['probs'][1:-1, 1:-1, 1:-1, 0] - ramp[1:-1, 1:-1, 1:-1]).max() / span > 1e-3
    with pytest.raises(ValueError, match='4 x 4'):
        native_grid_affine(aff[:3], aff2, idx)


# ---------------------------------------------------------------------------------------------------- the C interface
def test_symbol_is_declared_and_bound():
    from synthsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'synthsr_hip.h')).read()
    lib = _lib.load()
    name = 'synthsr_seg_resample_argmax'
    decl = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M)
    assert decl, name
    assert len(decl.group(1).split(',')) == 11
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 11
    assert getattr(lib, name) is not None
    assert lib.synthsr_abi_version() == 2


def test_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()
    p = 4096                                                    # a non-NULL address; never followed
    I6, D12 = ctypes.c_int * 6, ctypes.c_double * 12
    ident = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]

    def call(probs=p, src=(16, 24, 40), N=5, box=(2, 1, 3, 13, 22, 36), M=ident, out_shape=(8, 9, 10), labels=p, out=p,
             probs_out=None):
        return lib.synthsr_seg_resample_argmax(probs, None if src is None else _lib.i3(src), N, None if box is None else I6(*box),
                                               None if M is None else D12(*M), None if out_shape is None else _lib.i3(out_shape),
                                               labels, 0, out, probs_out, None)
    for name in ('probs', 'src', 'box', 'M', 'out_shape', 'labels', 'out'):
        assert call(**{name: None}) == -1, name
    for bad in (1, 65, 0, -3):
        assert call(N=bad) == -1
    for a in range(3):
        for side in (0, 1025, -1):
            shape = [16, 24, 40]
            shape[a] = side
            assert call(src=shape, box=(0, 0, 0, 0, 0, 0)) == -1
            shape = [8, 9, 10]
            shape[a] = side
            assert call(out_shape=shape) == -1
        box = [2, 1, 3, 13, 22, 36]
        box[3 + a] = (16, 24, 40)[a]                            # hi one past the source
        assert call(box=box) == -1
        box = [2, 1, 3, 13, 22, 36]
        box[a] = -1
        assert call(box=box) == -1
        box = [2, 1, 3, 13, 22, 36]
        box[a] = box[3 + a] + 1                                 # lo > hi
        assert call(box=box) == -1
    for e in range(12):
        for bad in (float('nan'), float('inf'), -float('inf')):
            M = list(ident)
            M[e] = bad
            assert call(M=M) == -1


def test_ops_wrapper_checks_before_the_library():
    import torch
    from synthsr_amd import ops
    probs = torch.zeros(4, 5, 6, 3)
    labels = torch.zeros(3, dtype=torch.int32)
    ok = dict(box=[0, 0, 0, 3, 4, 5], M=np.eye(4)[:3], out_shape=(4, 5, 6), labels=labels, fill_value=0)

    def call(probs=probs, **kw):
        return ops.seg_resample_argmax(probs, **{**ok, **kw})
    with pytest.raises(ValueError, match='float32'):
        call(probs=probs.double())
    with pytest.raises(ValueError, match='int32'):
        call(labels=labels.long())
    with pytest.raises(ValueError, match=r'\[s0, s1, s2, N\]'):
        call(probs=probs[0])
    with pytest.raises(ValueError, match='2 <= N <= 64'):
        call(probs=torch.zeros(4, 5, 6, 1), labels=labels[:1])
    with pytest.raises(ValueError, match='2 <= N <= 64'):
        call(probs=torch.zeros(2, 2, 2, 65), labels=torch.zeros(65, dtype=torch.int32))
    with pytest.raises(ValueError, match='one label value per channel'):
        call(labels=labels[:2])
    with pytest.raises(ValueError, match='out_shape'):
        call(out_shape=(4, 5, 1025))
    with pytest.raises(ValueError, match='out_shape'):
        call(out_shape=(4, 5))
    for box in ([0, 0, 0, 4, 4, 5], [1, 0, 0, 0, 4, 5], [-1, 0, 0, 3, 4, 5], [0, 0, 0, 3, 4]):
        with pytest.raises(ValueError, match='box'):
            call(box=box)
    bad = np.eye(4)[:3].copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError, match='finite'):
        call(M=bad)
    with pytest.raises(ValueError, match='finite'):
        call(M=np.eye(3))
    with pytest.raises(ValueError, match='fill_value'):
        call(fill_value=2 ** 31)
    with pytest.raises(ValueError, match='one value per output voxel'):
        call(out=torch.zeros(4, 5, 5, dtype=torch.int32))
    with pytest.raises(ValueError, match='probs_out'):
        call(probs_out=torch.zeros(4, 5, 6, 2))


# ---------------------------------------------------------------------------------------------------- the command line
def test_script_arguments_and_the_voxel_checks():
    S = _script()
    p = S.build_parser()
    base = ['in', 'out', '--model', 'm.npz', '--labels', 'l.npy']
    assert p.parse_args(base).native_space is False
    a = p.parse_args(base + ['--native_space', '--truth', 't', '--surface_scores', 'd.csv', '--volumes', 'v.npy'])
    assert a.native_space is True and (a.truth, a.surface_scores, a.volumes) == ('t', 'd.csv', 'v.npy')
    with pytest.raises(SystemExit):
        p.parse_args(base + ['--native_space', 'yes', 'more'])
    assert '--native_space' in S.__doc__
    # voxel sizes of an affine, orientation and shear-free rotation included
    c, s = np.cos(0.4), np.sin(0.4)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    aff = np.eye(4)
    aff[:3, :3] = rot @ np.diag([0.7, 0.7, 0.7])[:, [2, 0, 1]] * np.array([1, -1, 1])
    assert np.allclose(S.voxel_sizes(aff), 0.7) and abs(S.isotropic_voxel_size(aff) - 0.7) < 1e-12
    assert abs(S.voxel_volume(aff) - 0.7 ** 3) < 1e-12
    aff[:3, :3] = rot @ np.diag([1.0, 1.0, 5.0])
    assert abs(S.voxel_volume(aff) - 5.0) < 1e-12
    with pytest.raises(ValueError, match='isotropic'):
        S.isotropic_voxel_size(aff, 'scan.nii.gz')
    with pytest.raises(ValueError, match=r'scan.nii.gz has voxels of 1 x 1 x 5 mm'):
        S.isotropic_voxel_size(aff, 'scan.nii.gz')
    # the threshold: a spread of 1e-3 relative passes, more does not
    assert S.ISOTROPY_TOLERANCE == 1e-3
    S.isotropic_voxel_size(np.diag([1.0, 1.0005, 1.0009, 1.0]))
    with pytest.raises(ValueError, match='isotropic'):
        S.isotropic_voxel_size(np.diag([1.0, 1.0, 1.0011, 1.0]))
    with pytest.raises(ValueError, match='isotropic'):
        S.isotropic_voxel_size(np.diag([1.5, 1.5, 3.0, 1.0]))


def test_predict_segmentation_takes_native_space():
    import inspect
    from synthsr_amd.predict_segmentation import predict_segmentation, SegmentationPredictor
    sig = inspect.signature(predict_segmentation)
    assert list(sig.parameters)[-1] == 'native_space' and sig.parameters['native_space'].default is False
    assert inspect.signature(SegmentationPredictor.segment_volume).parameters['native'].default is None
