#!/usr/bin/env python
"""Command-line launcher of `synthsr_amd.segmentation_training.training_segmentation`: trains the softmax-headed segmentation
U-Net that `scripts/training.py --seg_reg_model_file` later freezes, with the generator flags of scripts/training.py.

    python scripts/training_segmentation.py <labels_dir> <model_dir> <prior_means.npy> <prior_stds.npy> <generation_labels.npy>
                                            <segmentation_labels.npy> [flags]"""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd.segmentation_training import training_segmentation  # noqa: E402
import training as _t  # noqa: E402  (scripts/training.py: the flag tables)

POSITIONAL = _t.POSITIONAL + ('segmentation_label_list',)
# the flags of scripts/training.py that training_segmentation() has a parameter for
DROPPED = ('images_dir', 'regression_metric', 'work_with_residual_channel', 'loss_cropping', 'segmentation_model_file',
           'segmentation_label_list', 'segmentation_label_equivalency', 'relative_weight_segmentation', 'segnet_dtype')
VALUED = [row for row in _t.VALUED + _t.EXTRA_VALUED if (row[1] or row[0]) not in DROPPED]
SWITCHES = [row for row in _t.SWITCHES + _t.EXTRA_SWITCHES if row[1] != 'fs_header_segnet']


def build_parser():
    parser = ArgumentParser(description=__doc__.split('\n')[0])
    for name in POSITIONAL:
        parser.add_argument(name, type=str)
    for flag, keyword, kind, default in VALUED:
        parser.add_argument('--' + flag, dest=keyword or flag, type=kind, default=0 if flag == 'output_channel' else default)
    for flag, keyword, stored in SWITCHES:
        parser.add_argument('--' + flag, dest=keyword, action='store_true' if stored else 'store_false')
    parser.add_argument('--deterministic', dest='deterministic', action='store_true')
    # the weights of the soft Dice (DiceLoss): class weights -1 = dynamic, or the path of a .npy with one value per label
    parser.add_argument('--dice_class_weights', dest='dice_class_weights', type=str, default=None)
    parser.add_argument('--dice_boundary_weights', dest='dice_boundary_weights', type=float, default=0.)
    parser.add_argument('--dice_boundary_dist', dest='dice_boundary_dist', type=int, default=3)
    parser.add_argument('--dice_no_skip_background', dest='dice_skip_background', action='store_false')
    # the other losses: WeightedL2Loss on the logits for the first epochs (the warm-up), then the Dice or the cross-entropy
    parser.add_argument('--wl2_epochs', dest='wl2_epochs', type=int, default=0)
    parser.add_argument('--wl2_target_value', dest='wl2_target_value', type=float, default=5.)
    parser.add_argument('--segmentation_loss', dest='segmentation_loss', type=str, default='dice',
                        choices=('dice', 'cross_entropy'))
    return parser


if __name__ == '__main__':
    training_segmentation(**vars(build_parser().parse_args()))
