#!/usr/bin/env python
"""Scores super-resolved volumes against their ground truth: MAE, RMSE, maximum error, PSNR, normalised cross-correlation, the
least-squares intensity map and the 3-D SSIM (11^3 Gaussian window), optionally inside a mask.

    python scripts/score_predictions.py <path_predictions> <path_truth> [--scores S.csv|S.npy]
                                        [--masks <path> [--mask_labels V ...]] [--normalise none|affine] [--data_range L]

<path_predictions>, <path_truth> (and --masks) are all single files or all folders, sorted alike.  A ground truth or mask on
another voxel grid is resliced onto the prediction's grid.  --mask_labels: score where the mask volume holds one of these
values (default: where it is non-zero).  --normalise affine: map every prediction with the least-squares a * prediction + b
before the errors and the SSIM.  --data_range: the L of PSNR and SSIM (default: the ground truth's max - min over the mask).
--scores: one row per volume and a mean row; .npy holds the numbers alone, any other name is written as CSV."""
import os
import sys
from argparse import ArgumentParser

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    p = ArgumentParser(description='image-quality scores of super-resolved volumes (MI355X build)')
    p.add_argument('path_predictions', help='prediction, or folder of predictions')
    p.add_argument('path_truth', help='ground truth (or folder, sorted like the predictions)')
    p.add_argument('--scores', default=None, help='write the table here (.csv or .npy)')
    p.add_argument('--masks', default=None, help='mask or label map (or folder, sorted like the predictions)')
    p.add_argument('--mask_labels', type=float, nargs='+', default=None, help='values of the mask volume that count')
    p.add_argument('--normalise', choices=('none', 'affine'), default='none')
    p.add_argument('--data_range', type=float, default=None, help='L of PSNR and SSIM')
    return p


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.mask_labels is not None and args.masks is None:
        parser.error('--mask_labels needs --masks')
    if args.data_range is not None and not args.data_range > 0:
        parser.error('--data_range is positive')
    from synthsr_amd.evaluate import score_predictions
    table = score_predictions(args.path_predictions, args.path_truth, path_scores=args.scores, path_masks=args.masks,
                              mask_labels=args.mask_labels, normalise=args.normalise, data_range=args.data_range)
    for name, row in zip(table['names'], table['values']):
        print(name + '  ' + '  '.join('%s %.6g' % (c, v) for c, v in zip(table['columns'], row)))
    return table


if __name__ == '__main__':
    main()
