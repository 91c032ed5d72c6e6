"""Host side of segmentation inference and Dice scoring (no GPU): the left/right channel permutation, Dice from counts, the
command line of scripts/predict_segmentation.py, the C ABI's new names and their argument checks, and the head-width check of
SegmentationPredictor."""
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('synthsr_seg_head_argmax', 'synthsr_seg_head_tta_argmax', 'synthsr_seg_label_counts')


def _script():
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_lr_pairs_give_the_channel_permutation():
    from synthsr_amd.predict_segmentation import lr_permutation
    labels = np.array([0, 14, 2, 41, 17, 53, 3, 42])
    assert np.array_equal(lr_permutation(labels), np.arange(8))
    assert np.array_equal(lr_permutation(labels, []), np.arange(8))
    perm = lr_permutation(labels, [(2, 41), (17, 53), (3, 42)])
    assert perm.dtype == np.int32
    assert np.array_equal(perm, [0, 1, 3, 2, 5, 4, 7, 6])
    assert np.array_equal(perm[perm], np.arange(8))                       # swapping twice is the identity
    assert np.array_equal(lr_permutation(labels, np.array([[53, 17]])), [0, 1, 2, 3, 5, 4, 6, 7])


@pytest.mark.parametrize('pairs,msg', [
    ([(2, 41), (2, 42)], 'twice'),            # a value in two pairs
    ([(2, 2)], 'twice'),                      # a value paired with itself
    ([(2, 99)], 'not in the segmentation label list'),
    ([(2, 41, 3)], 'pairs'),
    ([2, 41], 'pairs'),
    ([(2.5, 41)], 'integer'),
])
def test_lr_pairs_refusals(pairs, msg):
    from synthsr_amd.predict_segmentation import lr_permutation
    with pytest.raises(ValueError, match=msg):
        lr_permutation(np.array([0, 14, 2, 41, 17, 53, 3, 42]), pairs)


def test_dice_from_counts_and_its_nan():
    from synthsr_amd.predict_segmentation import dice_from_counts, mean_dice
    counts = np.array([[5, 0, 0, 2 ** 40], [5, 3, 0, 2 ** 40], [10, 0, 0, 2 ** 40 + 2]], dtype=np.int64)
    d = dice_from_counts(counts)
    assert d.dtype == np.float64 and d.shape == (4,)
    assert d[0] == 2 * 5 / 15 and d[1] == 0.0 and np.isnan(d[2])
    assert d[3] == 2.0 * 2 ** 40 / (2.0 ** 41 + 2)
    assert mean_dice(d) == (d[0] + d[1] + d[3]) / 3                      # the absent label is left out of the mean
    assert np.isnan(mean_dice(np.array([np.nan, np.nan])))
    assert np.array_equal(dice_from_counts(counts.astype(np.uint64)), d, equal_nan=True)
    with pytest.raises(ValueError):
        dice_from_counts(np.zeros((2, 4)))


def test_script_arguments(tmp_path):
    S = _script()
    p = S.build_parser()
    a = p.parse_args(['in', 'out', '--model', 'm.npz', '--labels', 'l.npy'])
    assert (a.path_images, a.path_segmentations, a.model, a.labels) == ('in', 'out', 'm.npz', 'l.npy')
    assert a.lr_pairs is None and a.posteriors is None and a.truth is None and a.scores is None and not a.disable_flipping
    assert (a.n_levels, a.nb_conv_per_level, a.unet_feat_count, a.feat_multiplier, a.activation) == (5, 2, 24, 2, 'elu')
    a = p.parse_args(['in', 'out', '--model', 'm.h5', '--labels', 'l.npy', '--lr_pairs', 'p.npy', '--posteriors', 'post',
                      '--disable_flipping', '--n_levels', '3', '--conv_per_level', '1', '--unet_feat', '8', '--feat_mult', '1',
                      '--activation', 'relu', '--truth', 'gt', '--scores', 's.csv'])
    assert (a.lr_pairs, a.posteriors, a.truth, a.scores, a.disable_flipping) == ('p.npy', 'post', 'gt', 's.csv', True)
    assert (a.n_levels, a.nb_conv_per_level, a.unet_feat_count, a.feat_multiplier, a.activation) == (3, 1, 8, 1, 'relu')
    for bad in (['in', 'out', '--labels', 'l.npy'], ['in', 'out', '--model', 'm.npz'], ['in', '--model', 'm', '--labels', 'l']):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    for bad in (['--scores', 's.npy'], ['--truth', 'gt', '--scores', 's.txt']):   # --scores needs --truth, .npy or .csv
        with pytest.raises(SystemExit):
            S.main(['in', 'out', '--model', 'm.npz', '--labels', 'l.npy'] + bad)
    table = np.array([[1.0, np.nan, 0.25]])
    S.write_scores(str(tmp_path / 's.npy'), [0, 14, 2], table)
    assert np.array_equal(np.load(tmp_path / 's.npy'), table, equal_nan=True)
    S.write_scores(str(tmp_path / 's.csv'), [0, 14, 2], table)
    assert open(tmp_path / 's.csv').read().split('\n')[:2] == ['0,14,2', '1.0,nan,0.25']


def test_the_three_entry_points_are_declared_and_bound():
    from synthsr_amd import _lib
    with open(os.path.join(ROOT, 'include', 'synthsr_hip.h')) as f:
        header = f.read()
    for name in NAMES:
        assert name in _lib.SIGNATURES
        assert re.search(r'\bint\s+%s\s*\(' % name, header), name


def test_limits_are_refused_before_any_launch():
    """C = 68 (> 64), C = 6 (not whole channel quads), N = 65 and N = 1 return SYNTHSR_EINVAL; the arguments are checked before
    any HIP call, so this runs without a device (the pointers are never followed)"""
    from synthsr_amd import _lib
    lib = _lib.load()
    assert lib.synthsr_abi_version() == 2
    p = 4096      # a non-NULL, 16-byte aligned address
    shape = _lib.i3([5, 7, 9])
    for C, N in ((68, 5), (6, 5), (24, 65), (24, 1)):
        assert lib.synthsr_seg_head_argmax(p, 315, C, p, p, p, 1e-3, p, p, N, p, p, None) == -1
        assert lib.synthsr_seg_head_tta_argmax(p, shape, C, p, p, p, 1e-3, p, p, N, p, p, p, p, None, None) == -1
    assert lib.synthsr_seg_head_argmax(p + 4, 315, 24, p, p, p, 1e-3, p, p, 5, p, p, None) == -1      # x not 16-byte aligned
    assert lib.synthsr_seg_head_argmax(p, 0, 24, p, p, p, 1e-3, p, p, 5, p, p, None) == -1
    assert lib.synthsr_seg_head_argmax(p, 315, 24, p, p, p, 1e-3, p, p, 5, None, p, None) == -1
    assert lib.synthsr_seg_head_tta_argmax(p, _lib.i3([5, 0, 9]), 24, p, p, p, 1e-3, p, p, 5, p, p, p, p, None, None) == -1
    assert lib.synthsr_seg_head_tta_argmax(p, shape, 24, p, p, p, 1e-3, p, p, 5, p, p, None, p, None, None) == -1   # no perm
    q = 1 << 20                                                                       # posteriors written over prev
    assert lib.synthsr_seg_head_tta_argmax(p, shape, 24, p, p, p, 1e-3, p, p, 5, p, q, p, p, q + 315 * 5 * 4 - 4, None) == -1
    for N in (65, 0):
        assert lib.synthsr_seg_label_counts(p, p, 315, p, 8, N, p, None) == -1
    assert lib.synthsr_seg_label_counts(p, p, 315, p, 0, 5, p, None) == -1
    assert lib.synthsr_seg_label_counts(p, p, 315, p, 8, 5, None, None) == -1


def test_predictor_refuses_a_head_of_another_width():
    """table_only networks give the head's name and shape: no device is needed to see that a weight file does not fit"""
    from synthsr_amd.predict_segmentation import SegmentationPredictor, check_head_width
    from synthsr_amd.unet import UNet3D
    table = UNet3D(8, [4, 4, 4, 1], 3, 3, 5, feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax',
                   table_only=True)
    state = {nm: np.zeros(shp, dtype=np.float32) for nm, shp, _ in table.specs}
    arch = dict(n_levels=3, unet_feat_count=8)
    with pytest.raises(ValueError, match='5 channels, the segmentation label list 4 labels'):
        SegmentationPredictor(None, np.array([0, 14, 2, 41]), state_dict=state, **arch)
    with pytest.raises(ValueError, match='5 channels'):
        SegmentationPredictor(None, np.array([0, 14, 2, 41, 17, 3]), state_dict=state, **arch)
    head5 = dict(state)
    head5['unet_likelihood/kernel'] = np.zeros((1, 1, 1, 8, 5), dtype=np.float32)     # the 5-D kernel of a Keras file
    check_head_width(head5, table, np.arange(5))
    ok = SegmentationPredictor(None, np.array([0, 14, 2, 41, 17]), state_dict=state, **arch)   # fits: nothing is built yet
    assert ok.nets == {} and ok.labels.dtype == np.int32 and ok.lut[41] == 3
    with pytest.raises(FileNotFoundError):
        SegmentationPredictor('/nowhere/model.npz', np.array([0, 14]))
    with pytest.raises(ValueError):
        SegmentationPredictor(None, np.array([0, 14, 14]), state_dict=state, **arch)


def test_predict_labels_is_refused_on_a_linear_head():
    from synthsr_amd.unet import UNet3D
    lin = UNet3D(8, [4, 4, 4, 1], 3, 3, 1, feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='linear',
                 table_only=True)
    with pytest.raises(ValueError, match='softmax'):
        lin.predict_labels(None, None)


def test_predict_segmentation_needs_levels_that_divide_the_padding():
    from synthsr_amd.predict_segmentation import predict_segmentation
    with pytest.raises(ValueError, match='multiples of 32'):
        predict_segmentation('/nowhere/a.nii.gz', '/nowhere/b.nii.gz', None, np.array([0, 2]), n_levels=7)
