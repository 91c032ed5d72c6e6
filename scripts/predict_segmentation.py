#!/usr/bin/env python
"""Segments volumes with a network trained by scripts/training_segmentation.py and, given ground-truth label maps, scores
the result with the per-label Dice coefficient and the distances between the surfaces of the two label maps.

    python scripts/predict_segmentation.py <path_images> <path_segmentations> --model M.npz|M.h5 --labels L.npy
                                           [--lr_pairs P.npy] [--posteriors <path>] [--disable_flipping]
                                           [--n_levels 5 --conv_per_level 2 --unet_feat 24 --feat_mult 2 --activation elu]
                                           [--dtype f32|bf16]
                                           [--keep_largest per_label|foreground|G.npy [--connectivity 6|18|26] [--fill_label V]]
                                           [--volumes V.npy|V.csv] [--native_space]
                                           [--truth <path> [--scores S.npy|S.csv]
                                                            [--surface_scores D.npy|D.csv [--surface_percentile 95]]]

<path_images>, <path_segmentations> (and --posteriors, --truth) are all single files or all folders; label maps written
into a folder carry the suffix _seg.  --labels: the label values in head-channel order (what training_segmentation took as
segmentation_label_list); --lr_pairs: a [K, 2] array of (left value, right value) pairs whose channels are swapped in the
flipped pass of the test-time augmentation.  --surface_scores: per label the Hausdorff distance, the --surface_percentile-th
percentile distance and the mean distance between the surfaces of segmentation and ground truth, in mm (label maps are written
at 1 mm): .npy [n_volumes, 3, N] in that order; .csv a header of label values, then three rows per volume in that order.
--keep_largest: write only the largest connected component of every group of labels (per_label: every label but the fill label
is a group; foreground: they form one group; G.npy: a group id per head channel, -1 = untouched), under --connectivity; the
removed voxels become --fill_label (default: the first label of --labels).  Dice and surface scores are then those of the
filtered maps.  --volumes: the volume of every label in every written map, in mm^3: .npy [n_volumes, N]; .csv as --scores.
--native_space: label maps (and --posteriors) are written on each image's own voxel grid, with its shape and affine, instead of
the 1 mm RAS frame: the 1 mm posteriors are interpolated onto that grid and the argmax is taken there.  --truth label maps are
then expected on each image's own grid, --volumes counts voxels of the image's own volume |det(affine[:3, :3])|, and
--surface_scores measures in the image's voxel size, which has to be the same along the three axes (to 1e-3 relative): surface
distances are computed in isotropic voxel units, so images with anisotropic voxels are refused before anything is segmented."""
import os
import sys
from argparse import ArgumentParser

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_parser():
    p = ArgumentParser(description='segmentation with a trained segmentation U-Net (MI355X build)')
    p.add_argument('path_images', help='scan, or folder of scans, to segment')
    p.add_argument('path_segmentations', help='output label map (or folder, if path_images is a folder)')
    p.add_argument('--model', required=True, help='weights: the .npz or .h5 checkpoint of training_segmentation')
    p.add_argument('--labels', required=True, help='.npy with the label values in head-channel order')
    p.add_argument('--lr_pairs', default=None, help='.npy [K, 2] of (left value, right value) label pairs')
    p.add_argument('--posteriors', default=None, help='also write the posteriors: file (or folder)')
    p.add_argument('--disable_flipping', action='store_true', help='no left-right flip averaging at test time')
    p.add_argument('--n_levels', type=int, default=5)
    p.add_argument('--conv_per_level', dest='nb_conv_per_level', type=int, default=2)
    p.add_argument('--unet_feat', dest='unet_feat_count', type=int, default=24)
    p.add_argument('--feat_mult', dest='feat_multiplier', type=int, default=2)
    p.add_argument('--activation', type=str, default='elu')
    p.add_argument('--dtype', choices=('f32', 'bf16'), default='f32',
                   help='arithmetic of the network: bf16 = bf16 activations and packed weights, fp32 head and posteriors')
    p.add_argument('--keep_largest', default=None,
                   help='keep the largest connected component per group: per_label, foreground, or a .npy of group ids per label')
    p.add_argument('--connectivity', type=int, choices=(6, 18, 26), default=6,
                   help='voxels are connected through faces (6), faces and edges (18) or faces, edges and corners (26)')
    p.add_argument('--fill_label', type=int, default=None,
                   help='the label value removed voxels take (default: the first label of --labels)')
    p.add_argument('--volumes', default=None, help='write the per-label volumes in mm^3 here (.npy or .csv)')
    p.add_argument('--native_space', action='store_true',
                   help="write on each image's own voxel grid (its shape and affine) instead of the 1 mm RAS frame")
    p.add_argument('--truth', default=None, help='ground-truth label map (or folder, sorted like the images): score with Dice')
    p.add_argument('--scores', default=None, help='write the per-label Dice table here (.npy or .csv); needs --truth')
    p.add_argument('--surface_scores', default=None,
                   help='write the per-label surface distances (Hausdorff, percentile, mean) here (.npy or .csv); needs --truth')
    p.add_argument('--surface_percentile', type=float, default=95, help='the percentile of the percentile distance')
    return p


def write_surface_scores(path, labels, table):
    """table [n_volumes, 3, N] (hausdorff, percentile, mean) -> .npy (the table), or .csv (a header of label values, then
    three rows per volume: hausdorff, percentile, mean)"""
    if path.endswith('.npy'):
        np.save(path, table)
    elif path.endswith('.csv'):
        with open(path, 'w') as f:
            f.write(','.join(str(int(v)) for v in labels) + '\n')
            for volume in table:
                for row in volume:
                    f.write(','.join(repr(float(v)) for v in row) + '\n')
    else:
        raise ValueError('--surface_scores takes a .npy or a .csv path, got %s' % path)


def write_scores(path, labels, table, flag='--scores'):
    """table [n_volumes, N] -> .npy (the table), or .csv (a header of label values, one row per volume)"""
    if path.endswith('.npy'):
        np.save(path, table)
    elif path.endswith('.csv'):
        with open(path, 'w') as f:
            f.write(','.join(str(int(v)) for v in labels) + '\n')
            for row in table:
                f.write(','.join(repr(float(v)) for v in row) + '\n')
    else:
        raise ValueError('%s takes a .npy or a .csv path, got %s' % (flag, path))


def write_volumes(path, labels, table):
    """table [n_volumes, N] of volumes in mm^3 -> the layout of write_scores"""
    write_scores(path, labels, table, flag='--volumes')


ISOTROPY_TOLERANCE = 1e-3   # relative spread of the three voxel sizes


def voxel_sizes(aff):
    """the three voxel sizes (mm) of an affine: the lengths of the columns of its 3 x 3 part"""
    return np.sqrt(np.sum(np.asarray(aff, dtype=np.float64)[:3, :3] ** 2, axis=0))


def isotropic_voxel_size(aff, what='the image'):
    """the voxel size of an affine whose three voxel sizes agree to ISOTROPY_TOLERANCE (relative spread); anything else is
    refused: surface distances are measured in isotropic voxel units"""
    vox = voxel_sizes(aff)
    if not np.all(np.isfinite(vox)) or vox.min() <= 0 or (vox.max() - vox.min()) > ISOTROPY_TOLERANCE * vox.mean():
        raise ValueError('--surface_scores with --native_space needs isotropic voxels: %s has voxels of %s mm; surface distances '
                         'are measured in isotropic voxel units (score without --native_space, at 1 mm, instead)'
                         % (what, ' x '.join('%g' % v for v in vox)))
    return float(vox.mean())


def voxel_volume(aff):
    """mm^3 per voxel: |det| of the affine's 3 x 3 part"""
    return float(abs(np.linalg.det(np.asarray(aff, dtype=np.float64)[:3, :3])))


def main(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.scores is not None and args.truth is None:
        parser.error('--scores needs --truth')
    if args.scores is not None and not args.scores.endswith(('.npy', '.csv')):
        parser.error('--scores takes a .npy or a .csv path')
    if args.surface_scores is not None and args.truth is None:
        parser.error('--surface_scores needs --truth')
    if args.surface_scores is not None and not args.surface_scores.endswith(('.npy', '.csv')):
        parser.error('--surface_scores takes a .npy or a .csv path')
    if not 0 <= args.surface_percentile <= 100:
        parser.error('--surface_percentile lies in 0 .. 100')
    if args.volumes is not None and not args.volumes.endswith(('.npy', '.csv')):
        parser.error('--volumes takes a .npy or a .csv path')
    keep_largest = args.keep_largest
    if keep_largest is not None and keep_largest not in ('per_label', 'foreground'):
        if not keep_largest.endswith('.npy'):
            parser.error('--keep_largest takes per_label, foreground or a .npy path')
        keep_largest = np.load(keep_largest)
    from synthsr_amd import volumes as V
    from synthsr_amd.predict_segmentation import predict_segmentation, dice_scores, label_values, mean_dice
    labels = label_values(args.labels)
    lr_pairs = None if args.lr_pairs is None else np.load(args.lr_pairs)
    affines = None
    if args.native_space and (args.volumes is not None or args.surface_scores is not None):
        images = V.list_images_in_folder(os.path.abspath(args.path_images))     # the order predict_segmentation works in
        affines = [V.load_volume(p, im_only=False)[1] for p in images]
    sizes = None
    if args.native_space and args.surface_scores is not None:
        sizes = [isotropic_voxel_size(a, p) for a, p in zip(affines, images)]
    outs = predict_segmentation(args.path_images, args.path_segmentations, args.model, labels,
                                path_posteriors=args.posteriors, lr_pairs=lr_pairs, disable_flipping=args.disable_flipping,
                                n_levels=args.n_levels, nb_conv_per_level=args.nb_conv_per_level,
                                unet_feat_count=args.unet_feat_count, feat_multiplier=args.feat_multiplier,
                                activation=args.activation, dtype=args.dtype, keep_largest=keep_largest,
                                connectivity=args.connectivity, fill_label=args.fill_label, native_space=args.native_space)
    if args.volumes is not None:
        from synthsr_amd.predict_segmentation import label_volumes
        per_voxel = [1.0] * len(outs) if affines is None else [voxel_volume(a) for a in affines]   # 1.0: written at 1 mm
        write_volumes(args.volumes, labels, np.stack([label_volumes(o, labels, v) for o, v in zip(outs, per_voxel)]))
    if args.truth is None:
        return None
    truths = V.list_images_in_folder(os.path.abspath(args.truth))
    if len(truths) != len(outs):
        raise ValueError('%d ground-truth label maps for %d segmentations' % (len(truths), len(outs)))
    table = np.stack([dice_scores(o, t, labels) for o, t in zip(outs, truths)])
    surface = None
    if args.surface_scores is not None:
        from synthsr_amd.predict_segmentation import surface_distances, mean_surface_scores, SURFACE_KEYS
        per_volume = [surface_distances(o, t, labels, percentile=args.surface_percentile, voxel_size=v)
                      for o, t, v in zip(outs, truths, sizes or [1.0] * len(outs))]
        surface = np.stack([np.stack([s[key] for key in SURFACE_KEYS]) for s in per_volume])
    for i, (o, row) in enumerate(zip(outs, table)):
        print(o)
        for v, d in zip(labels, row):
            print('  label %5d  Dice %s' % (v, 'absent' if np.isnan(d) else '%.4f' % d))
        print('  mean Dice %.4f' % mean_dice(row))
        if surface is not None:
            print('  mean Hausdorff %.4f  mean HD%g %.4f  mean surface distance %.4f'
                  % ((mean_surface_scores(per_volume[i])[0], args.surface_percentile) + mean_surface_scores(per_volume[i])[1:]))
    if args.scores is not None:
        write_scores(args.scores, labels, table)
    if surface is not None:
        write_surface_scores(args.surface_scores, labels, surface)
    return table


if __name__ == '__main__':
    main()
