"""Segmenting volumes with a network trained by `synthsr_amd.segmentation_training.training_segmentation`, and scoring label
maps with the Dice coefficient.

    per volume:  resample to 1 mm, re-orient to RAS, min-max normalise, zero-pad to a multiple of 32 (predict.prepare_volume:
                 the image the segmentation network saw in training is a clean one-channel image) -> U-Net forward with the
                 moving statistics -> head + argmax in one kernel (UNet3D.predict_labels) -> crop -> int32 label map.

With flip averaging the first pass keeps its posteriors (UNet3D.predict_probs); the second pass, on the volume flipped along
its first (left-right) axis, averages them with its own mirrored ones -- channels of left and right structures swapped --
inside the head kernel and writes the label map of the average.  Without it no posterior is ever formed.

Asked to (keep_largest), the label map is cleaned on the device before it is written: of every group of labels only the
largest connected component stays (ops.seg_components, ops.seg_keep_largest), the rest takes the fill label.

Asked to (native_space), the label map is written on the input image's own voxel grid instead of the 1 mm RAS frame: the
1 mm posteriors are interpolated onto that grid and the argmax is taken there, in one kernel that keeps the interpolated
posteriors in registers (ops.seg_resample_argmax; native_grid_affine composes the matrix).  The filter then runs on that map.

The head's channel order is `segmentation_label_list`, as in training_segmentation().  fp32 only."""
import os
import numpy as np

from . import host_math as hm
from . import volumes as V
from .predict import prepare_volume
from .segmentation_training import segmentation_lut


def label_values(segmentation_label_list):
    """the label values in head-channel order as int32 (the checks of segmentation_lut: non-negative integers, none twice)"""
    segmentation_lut(segmentation_label_list)
    return np.asarray(hm.load_array_if_path(segmentation_label_list)).reshape(-1).astype(np.int32)


def lr_permutation(segmentation_label_list, lr_pairs=None):
    """int32 [N]: head channel -> the channel of the same structure on the other side.  lr_pairs: (left value, right value)
    pairs of listed label values, no value in more than one place; channels of unpaired labels map to themselves."""
    labels = label_values(segmentation_label_list)
    perm = np.arange(len(labels), dtype=np.int32)
    if lr_pairs is None:
        return perm
    pairs = np.asarray(lr_pairs)
    if pairs.size == 0:
        return perm
    if pairs.ndim != 2 or pairs.shape[1] != 2:
        raise ValueError('lr_pairs should be a list of (left value, right value) pairs, got an array of shape %s'
                         % (pairs.shape,))
    if np.any(pairs != np.round(pairs)):
        raise ValueError('lr_pairs should hold integer label values')
    pairs = pairs.astype(np.int64)
    flat = pairs.reshape(-1)
    if len(np.unique(flat)) != len(flat):
        raise ValueError('lr_pairs names a label value twice')
    channel = {int(v): i for i, v in enumerate(labels)}
    unlisted = [int(v) for v in flat if int(v) not in channel]
    if unlisted:
        raise ValueError('lr_pairs names label values that are not in the segmentation label list: %s' % unlisted)
    for left, right in pairs:
        perm[channel[int(left)]], perm[channel[int(right)]] = channel[int(right)], channel[int(left)]
    return perm


def dice_from_counts(counts):
    """per-label Dice 2 |a = k and b = k| / (|a = k| + |b = k|) as float64 from counts [3, N] (overlap, |a|, |b|); a label
    absent from both maps scores NaN"""
    counts = np.asarray(counts)
    if counts.ndim != 2 or counts.shape[0] != 3:
        raise ValueError('counts should be [3, N], got %s' % (counts.shape,))
    top = 2.0 * counts[0].astype(np.float64)
    bottom = counts[1].astype(np.float64) + counts[2].astype(np.float64)
    out = np.full(counts.shape[1], np.nan, dtype=np.float64)
    np.divide(top, bottom, out=out, where=bottom > 0)
    return out


def mean_dice(scores):
    """mean over the labels present in at least one of the two maps (NaN when there is none)"""
    scores = np.asarray(scores, dtype=np.float64)
    present = ~np.isnan(scores)
    return float(scores[present].mean()) if present.any() else float('nan')


GROUPINGS = ('per_label', 'foreground')
MAX_GROUPS = 64   # include/synthsr_hip.h: synthsr_seg_components


def component_groups(label_list, groups='per_label', fill_label=None):
    """(lut, G, fill_value) for connected_components / keep_largest_components: lut, int32, maps a label value to its group
    0 .. G-1 or to -1 (left untouched); fill_value is what removed voxels become: `fill_label`, by default the first listed
    label (conventionally background).  groups:
      'per_label'   every listed label except the fill label is a group of its own, in the order of the list
      'foreground'  all listed labels except the fill label form one group
      int array [N] the group of every head channel, -1: left untouched (SynthSeg's topology classes); the ids used are
                    0 .. G-1 without gaps.  The fill label is not treated specially here.
    At most 64 groups."""
    labels = label_values(label_list)
    if fill_label is None:
        fill_value = int(labels[0])
    else:
        if fill_label != np.round(fill_label) or not -2 ** 31 <= int(fill_label) < 2 ** 31:
            raise ValueError('fill_label should be an integer label value, got %r' % (fill_label,))
        fill_value = int(fill_label)
    if isinstance(groups, str):
        if groups not in GROUPINGS:
            raise ValueError("groups should be 'per_label', 'foreground' or an array of group ids per label, got %r" % (groups,))
        ids = np.full(len(labels), -1, dtype=np.int64)
        others = labels != fill_value
        ids[others] = np.arange(int(others.sum())) if groups == 'per_label' else 0
    else:
        ids = np.asarray(hm.load_array_if_path(groups))
        if ids.ndim != 1 or ids.size != len(labels):
            raise ValueError('groups should hold one group id per listed label (%d), got an array of shape %s'
                             % (len(labels), ids.shape))
        if np.any(ids != np.round(ids)) or np.any(ids < -1):
            raise ValueError('groups should hold integer group ids, -1 for a label that is left untouched')
        ids = ids.astype(np.int64)
    used = np.unique(ids[ids >= 0])
    G = len(used)
    if G < 1:
        raise ValueError('the grouping leaves no label in any group')
    if G > MAX_GROUPS:
        raise ValueError('%d groups: connected components take at most %d groups' % (G, MAX_GROUPS))
    if not np.array_equal(used, np.arange(G)):
        raise ValueError('group ids should be 0 .. %d without gaps, got %s' % (G - 1, used.tolist()))
    lut = np.full(int(labels.max()) + 1, -1, dtype=np.int32)
    lut[labels] = ids.astype(np.int32)
    return lut, G, fill_value


def _filter_on_device(seg, lut, G, fill_value, connectivity):
    """(out, stats) on the device for a contiguous int32 device label map [d0, d1, d2]"""
    import torch
    from . import ops
    lut_d = torch.from_numpy(lut).to(seg.device)
    workspace = torch.empty(ops.seg_components_workspace_bytes(seg.shape), dtype=torch.uint8, device=seg.device)
    comp = ops.seg_components(seg, lut_d, G, connectivity, workspace=workspace)
    return ops.seg_keep_largest(seg, comp, lut_d, G, fill_value, workspace=workspace)


def native_grid_affine(aff_native, aff_ras, idx):
    """float64 [3, 4]: voxel index of the image as it was loaded (affine `aff_native`) -> voxel coordinates of the padded 1 mm
    RAS array predict.prepare_volume built from it (`aff_ras`: the affine it returned, `idx`: its padding offsets).  Both affines
    map the centre of voxel (0, 0, 0) to the translation column, the convention volumes.resample_volume and align_volume_to_ref
    keep, so the matrix is inv(aff_ras) @ aff_native with idx added to its translation."""
    aff_native, aff_ras = np.asarray(aff_native, dtype=np.float64), np.asarray(aff_ras, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.float64).reshape(-1)
    if aff_native.shape != (4, 4) or aff_ras.shape != (4, 4) or idx.shape != (3,):
        raise ValueError('native_grid_affine takes two 4 x 4 affines and three padding offsets')
    M = (np.linalg.inv(aff_ras) @ aff_native)[:3].copy()
    M[:, 3] += idx
    return M


def check_head_width(state, table, labels):
    """the weight file's head should have one channel per listed label"""
    name = table.head['w']
    if name in state:
        width = int(np.shape(state[name])[-1])
        if width != len(labels):
            raise ValueError('the network\'s head has %d channels, the segmentation label list %d labels' % (width, len(labels)))


class SegmentationPredictor:
    """The softmax-headed U-Net of training_segmentation() (one input channel), rebuilt per padded volume shape like
    predict.Predictor; one resident network.  dtype 'bf16': bf16 activations and packed conv weights (the head, its
    posteriors and the flip average stay fp32)."""

    def __init__(self, path_model, segmentation_label_list, n_levels=5, nb_conv_per_level=2, unet_feat_count=24,
                 feat_multiplier=2, activation='elu', device=None, state_dict=None, dtype='f32'):
        if dtype not in ('f32', 'bf16'):
            raise ValueError("dtype should be 'f32' or 'bf16', got %r" % (dtype,))
        self.dtype = dtype
        self.labels = label_values(segmentation_label_list)
        self.lut = segmentation_lut(self.labels)
        self.arch = dict(nb_features=unet_feat_count, nb_levels=n_levels, conv_size=3, nb_labels=len(self.labels),
                         feat_mult=feat_multiplier, nb_conv_per_level=nb_conv_per_level, batch_norm=-1,
                         final_pred_activation='softmax', activation=activation)
        self.device = device or 'cuda'
        self.state = state_dict
        if state_dict is None:
            if path_model is None or not os.path.isfile(path_model):
                raise FileNotFoundError('model file %s not found (the .npz or .h5 checkpoint written by '
                                        'training_segmentation)' % path_model)
            from .training import read_weights
            self.state = {k: v for k, v in read_weights(path_model).items() if not k.startswith('optimizer/')}
        from .unet import UNet3D
        side = 2 ** (int(n_levels) - 1)
        check_head_width(self.state, UNet3D(input_shape=[side] * 3 + [1], table_only=True, **self.arch), self.labels)
        self.nets = {}
        self._labels_dev = None

    def net_for(self, shape):
        import torch
        from .unet import unet
        key = tuple(int(s) for s in shape)
        if key not in self.nets:
            self.nets.clear()  # one resident network: volumes of a folder usually share their shape
            net = unet(input_shape=list(key) + [1], conv_dropout=0, input_model=None, device=self.device, dtype=self.dtype,
                       **self.arch)
            # a weight file with another layer prefix / missing layers must not leave random weights in place silently
            missing = [nm for nm, _, _ in net.specs if nm not in self.state]
            missing += [b['name'] + '/moving_mean' for b in net.bn_layers if b['name'] + '/moving_mean' not in self.state]
            if missing:
                raise KeyError('the weight file lacks %d of the network\'s tensors (first: %s): wrong model file or layer '
                               'prefix?' % (len(missing), missing[0]))
            net.load_state_dict({k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in self.state.items()}, strict=True)
            net.repack()
            self.nets[key] = net
        return self.nets[key]

    def segment_volume(self, S, flipping=True, lr_pairs=None, return_posteriors=False, keep_largest=None, connectivity=6,
                       fill_label=None, crop=None, native=None):
        """S [W0,W1,W2] (numpy, padded: every side a multiple of 2**(n_levels-1)) -> int32 label map [W0,W1,W2] of label
        values (numpy); with return_posteriors also the posteriors [W0,W1,W2,N] float32 the map is the argmax of.
        flipping: average with the pass on the volume flipped along the first (left-right) axis, the channels of each
        (left value, right value) pair of lr_pairs swapped.
        crop: three slices; what is returned is cut to them, on the device.
        keep_largest: None, or a grouping of component_groups() ('per_label', 'foreground', group ids per channel): the
        returned (cropped) map keeps only the largest connected component of every group under `connectivity` (6, 18, 26), the
        other voxels of the group become `fill_label` (default: the first listed label).  The filter runs on the device.  The
        posteriors are returned unchanged: they are those of the unfiltered map.
        native: None, or (M, out_shape): the map is returned on another voxel grid of shape out_shape, M (3 x 4, float64) taking
        a voxel index of that grid to voxel coordinates of S (native_grid_affine).  The posteriors of S are always formed then;
        they are interpolated at every voxel of the grid and the map is their argmax there (ops.seg_resample_argmax), `crop`
        being the box that is interpolated in: voxels that fall more than half a voxel outside it get `fill_label` (default: the
        first listed label) and zero posteriors.  The returned posteriors are the interpolated ones [*out_shape, N], and the
        filter runs on the grid's map."""
        import torch
        perm = lr_permutation(self.labels, lr_pairs)
        grouping = None if keep_largest is None else component_groups(self.labels, keep_largest, fill_label)
        if connectivity not in (6, 18, 26):
            raise ValueError('connectivity is 6, 18 or 26, got %r' % (connectivity,))
        S = np.asarray(S)
        if S.ndim != 3:
            raise ValueError('segment_volume takes one 3-D volume, got an array of shape %s' % (S.shape,))
        net = self.net_for(S.shape)
        N = len(self.labels)
        if self._labels_dev is None:
            self._labels_dev = torch.from_numpy(self.labels).to(net.device)
        x = torch.from_numpy(np.ascontiguousarray(S, dtype=np.float32)).to(net.device)[..., None].contiguous()
        probs = None
        if native is not None:
            from . import ops
            M, out_shape = native
            fill_value = component_groups(self.labels, 'foreground', fill_label)[2]
            box = [0, 0, 0] + [int(n) - 1 for n in S.shape]
            if crop is not None:
                spans = [sl.indices(int(n)) for sl, n in zip(crop, S.shape)]
                if any(step != 1 or stop <= start for start, stop, step in spans):
                    raise ValueError('crop should be three non-empty slices of step 1, got %r' % (crop,))
                box = [sp[0] for sp in spans] + [sp[1] - 1 for sp in spans]
            probs = net.predict_probs(x)
            if flipping:
                probs = net.predict_labels(torch.flip(x, dims=[0]).contiguous(), self._labels_dev, prev=probs,
                                           perm=torch.from_numpy(perm).to(net.device), want_probs=True)[1]
            res = ops.seg_resample_argmax(probs.view(*S.shape, N), box, M, out_shape, self._labels_dev, fill_value,
                                          want_probs=return_posteriors)
            out, probs = res if return_posteriors else (res, None)
            if grouping is not None:
                out = _filter_on_device(out, grouping[0], grouping[1], grouping[2], connectivity)[0]
            seg = out.cpu().numpy().astype(np.int32, copy=False)
            return (seg, probs.cpu().numpy()) if return_posteriors else seg
        if flipping:
            prev = net.predict_probs(x)
            out = net.predict_labels(torch.flip(x, dims=[0]).contiguous(), self._labels_dev, prev=prev,
                                     perm=torch.from_numpy(perm).to(net.device), want_probs=return_posteriors)
            if return_posteriors:
                out, probs = out
        elif return_posteriors:   # the posteriors are asked for: the label map is their argmax (first of equal values)
            probs = net.predict_probs(x)
            out = self._labels_dev[torch.argmax(probs, dim=1)]
        else:
            out = net.predict_labels(x, self._labels_dev)
        out = out.reshape(S.shape)
        if crop is not None:
            out = out[tuple(crop)]
        if grouping is not None:
            out = _filter_on_device(out.to(torch.int32).contiguous(), grouping[0], grouping[1], grouping[2], connectivity)[0]
        seg = out.cpu().numpy().astype(np.int32, copy=False)
        if return_posteriors:
            probs = probs.reshape(*S.shape, N)
            return seg, (probs if crop is None else probs[tuple(crop)]).cpu().numpy()
        return seg


def _suffixed(path, suffix):
    for ext in ('.nii.gz', '.nii', '.mgz', '.npz'):
        if path.endswith(ext):
            return path[:-len(ext)] + suffix + ext
    return path + suffix


def predict_segmentation(path_images, path_segmentations, path_model, segmentation_label_list, path_posteriors=None,
                         lr_pairs=None, disable_flipping=False, n_levels=5, nb_conv_per_level=2, unet_feat_count=24,
                         feat_multiplier=2, activation='elu', device=None, verbose=True, predictor=None, dtype='f32',
                         keep_largest=None, connectivity=6, fill_label=None, native_space=False):
    """The file / folder contract of predict.predict(): `path_images` / `path_segmentations` (and `path_posteriors`, if
    given) are all single files (.nii, .nii.gz, .mgz, .npz) or all folders; in folders the outputs carry the suffixes
    `_seg` and `_posteriors`.  Label maps are saved as int32 in the 1 mm RAS frame predict() writes in.  Returns the paths
    of the label maps.  dtype: 'f32' or 'bf16', the arithmetic of the network (SegmentationPredictor); posteriors are
    written as float32 either way.
    keep_largest: None (the raw argmax), or a grouping of component_groups(): the label map that is written keeps only the largest
    connected component of every group under `connectivity`, the other voxels of the group become `fill_label` (default: the first
    listed label).  The filter runs on the device on the cropped map, so the file equals keep_largest_components() of the file
    written without it.  Posteriors, when asked for, are written unchanged.
    native_space: label maps and posteriors are written with the input image's own shape and affine instead: the 1 mm posteriors
    are interpolated onto the input's voxel grid and the argmax is taken there (SegmentationPredictor.segment_volume: native);
    voxels of the input that lie outside the resampled volume get `fill_label`.  The filter then runs on that map.  For 3-D
    images."""
    if dtype not in ('f32', 'bf16'):
        raise ValueError("dtype should be 'f32' or 'bf16', got %r" % (dtype,))
    if 32 % (2 ** (int(n_levels) - 1)) != 0:
        raise ValueError('volumes are padded to multiples of 32: n_levels = %d needs sides divisible by %d'
                         % (n_levels, 2 ** (int(n_levels) - 1)))
    path_images = os.path.abspath(path_images)
    basename = os.path.basename(path_images)
    path_segmentations = os.path.abspath(path_segmentations)
    if not any(ext in basename for ext in ('.nii.gz', '.nii', '.mgz', '.npz')):
        if os.path.isfile(path_images):
            raise Exception('extension not supported for %s, only use: nii.gz, .nii, .mgz, or .npz' % path_images)
        images = V.list_images_in_folder(path_images)
        os.makedirs(path_segmentations, exist_ok=True)
        outs = [_suffixed(os.path.join(path_segmentations, os.path.basename(p)), '_seg') for p in images]
        posts = [None] * len(images)
        if path_posteriors is not None:
            os.makedirs(path_posteriors, exist_ok=True)
            posts = [_suffixed(os.path.join(os.path.abspath(path_posteriors), os.path.basename(p)), '_posteriors')
                     for p in images]
    else:
        assert os.path.isfile(path_images), "files does not exist: %s " \
                                            "\nplease make sure the path and the extension are correct" % path_images
        images, outs = [path_images], [path_segmentations]
        posts = [None if path_posteriors is None else os.path.abspath(path_posteriors)]
    predictor = predictor or SegmentationPredictor(path_model, segmentation_label_list, n_levels, nb_conv_per_level,
                                                   unet_feat_count, feat_multiplier, activation, device, dtype=dtype)
    if verbose:
        print('Found %d images' % len(images))
    for i, (pin, pout, ppost) in enumerate(zip(images, outs, posts)):
        if verbose:
            print('  Working on image %d ' % (i + 1))
            print('  ' + pin)
        im, aff, _ = V.load_volume(pin, im_only=False, dtype='float')
        S, idx, shape, aff2 = prepare_volume(im, aff)
        crop = tuple(slice(int(o), int(o) + int(n)) for o, n in zip(idx, shape))
        native, aff_out = None, aff2
        if native_space:
            if np.ndim(im) != 3:
                raise ValueError('native_space takes 3-D images, %s has shape %s' % (pin, np.shape(im)))
            native, aff_out = (native_grid_affine(aff, aff2, idx), np.shape(im)), aff
        res = predictor.segment_volume(S, flipping=not disable_flipping, lr_pairs=lr_pairs,
                                       return_posteriors=ppost is not None, keep_largest=keep_largest,
                                       connectivity=connectivity, fill_label=fill_label, crop=crop, native=native)
        seg = res[0] if ppost is not None else res
        V.save_volume(np.ascontiguousarray(seg), aff_out, None, pout, dtype='int32')
        if ppost is not None:
            V.save_volume(np.ascontiguousarray(res[1]), aff_out, None, ppost, dtype='float32', n_dims=3)
    return outs


def _label_map(m):
    if isinstance(m, str):
        m = V.load_volume(m, im_only=True, dtype='int')
    m = np.asarray(m)
    if not np.issubdtype(m.dtype, np.integer):
        m = np.round(m)
    return np.ascontiguousarray(m, dtype=np.int32)


def dice_scores(seg, truth, label_list, device=None):
    """per-label Dice (float64 [N], in the order of `label_list`) of two label maps of equal shape, given as arrays or
    paths; the voxels are counted on the GPU (ops.seg_label_counts).  A label absent from both maps scores NaN."""
    import torch
    from . import ops
    lut = segmentation_lut(label_list)
    a, b = _label_map(seg), _label_map(truth)
    if a.shape != b.shape:
        raise ValueError('dice_scores: label maps of shapes %s and %s' % (a.shape, b.shape))
    dev = device or 'cuda'
    counts = ops.seg_label_counts(torch.from_numpy(a).to(dev).reshape(-1), torch.from_numpy(b).to(dev).reshape(-1),
                                  torch.from_numpy(lut).to(dev), int((lut >= 0).sum()))
    return dice_from_counts(counts.cpu().numpy())


def label_volumes(seg, label_list, voxel_volume=1.0):
    """per-label volumes (float64 [N], in the order of `label_list`, background included) of a label map given as an array or
    a path: voxel_volume times the voxels of each label, counted on the GPU (ops.seg_label_counts of the map against itself)"""
    import torch
    from . import ops
    lut = segmentation_lut(label_list)
    a = torch.from_numpy(_label_map(seg)).to('cuda').reshape(-1)
    counts = ops.seg_label_counts(a, a, torch.from_numpy(lut).to('cuda'), int((lut >= 0).sum()))
    return counts[1].cpu().numpy().astype(np.float64) * float(voxel_volume)


def connected_components(label_map, label_list, groups='per_label', connectivity=6, device=None):
    """the component map of a 3-D label map (an array or a path) as int32 numpy: at every voxel the smallest linear index (C
    order) of any voxel of its connected component, -1 at voxels in no group.  groups: component_groups(); connectivity: 6
    (faces), 18 (faces and edges) or 26 (faces, edges and corners).  Labelled on the GPU (ops.seg_components)."""
    import torch
    from . import ops
    lut, G, _ = component_groups(label_list, groups)
    m = _label_map(label_map)
    if m.ndim != 3:
        raise ValueError('connected_components takes a 3-D label map, got shape %s' % (m.shape,))
    dev = device or 'cuda'
    return ops.seg_components(torch.from_numpy(m).to(dev), torch.from_numpy(lut).to(dev), G, connectivity).cpu().numpy()


def keep_largest_components(seg, label_list, groups='per_label', connectivity=6, fill_label=None, device=None,
                            return_stats=False):
    """the 3-D label map `seg` (an array or a path) with only the largest connected component of every group kept (of several
    of that size: the one that holds the smallest linear index); the other voxels of the group become `fill_label` (default: the
    first listed label), voxels in no group stay.  int32 numpy; with return_stats also int64 [G, 4]: per group the root of the
    kept component (-1: empty group), its size, the components and the voxels of the group.  Runs on the GPU."""
    import torch
    lut, G, fill_value = component_groups(label_list, groups, fill_label)
    m = _label_map(seg)
    if m.ndim != 3:
        raise ValueError('keep_largest_components takes a 3-D label map, got shape %s' % (m.shape,))
    out, stats = _filter_on_device(torch.from_numpy(m).to(device or 'cuda'), lut, G, fill_value, connectivity)
    if return_stats:
        return out.cpu().numpy(), stats.cpu().numpy()
    return out.cpu().numpy()


SURFACE_KEYS = ('hausdorff', 'hd_percentile', 'mean')


def surface_scores_from_d2(cls_a, d2_ab, cls_b, d2_ba, N, percentile=95, voxel_size=1.0):
    """The host half of surface_distances(): float64 scores per head channel from exact squared distances.

    cls_a, d2_ab: arrays of equal shape, the head channel of each voxel of map a and its squared distance to the surface of the
    same class in map b (ops.seg_surface_dist2: < 0 at voxels that are no surface voxels, which are left out, INT32_MAX when b
    has no surface of the class); whole volumes or only the gathered surface voxels.  cls_b, d2_ba: the same for map b.
    With D = voxel_size * sqrt of the distances of class k from both directions: hausdorff = max(D), hd_percentile =
    numpy.percentile(D, percentile), mean = D.mean(); a class without a surface voxel in one of the maps (or both) scores NaN.
    Returns a dict of float64 [N] arrays under SURFACE_KEYS and the int64 [N] surface voxel counts 'n_seg' (map a) and
    'n_truth' (map b)."""
    N = int(N)
    if not 0 <= float(percentile) <= 100:
        raise ValueError('percentile should lie in 0 .. 100, got %r' % (percentile,))
    sides = []
    for what, cls, d2 in (('a', cls_a, d2_ab), ('b', cls_b, d2_ba)):
        cls, d2 = np.asarray(cls).reshape(-1), np.asarray(d2).reshape(-1)
        if cls.shape != d2.shape:
            raise ValueError('surface_scores_from_d2: %d classes for %d distances of map %s' % (cls.size, d2.size, what))
        keep = d2 >= 0
        cls, d2 = cls[keep].astype(np.int64), d2[keep].astype(np.int64)
        if cls.size and (cls.min() < 0 or cls.max() >= N):
            raise ValueError('surface_scores_from_d2: a surface voxel of map %s has no class in 0 .. %d' % (what, N - 1))
        order = np.argsort(cls, kind='stable')
        counts = np.bincount(cls, minlength=N).astype(np.int64)
        sides.append((d2[order], np.concatenate([[0], np.cumsum(counts)]), counts))
    out = {key: np.full(N, np.nan, dtype=np.float64) for key in SURFACE_KEYS}
    far = np.iinfo(np.int32).max
    for k in range(N):
        parts = [d2[start[k]:start[k + 1]] for d2, start, _ in sides]
        if parts[0].size == 0 or parts[1].size == 0:
            continue
        d2 = np.concatenate(parts)
        if d2.max() >= far:     # the other map has no surface of the class: cannot happen with both present
            continue
        D = np.sqrt(d2.astype(np.float64)) * float(voxel_size)
        out['hausdorff'][k] = D.max()
        out['hd_percentile'][k] = np.percentile(D, percentile)
        out['mean'][k] = D.mean()
    out['n_seg'], out['n_truth'] = sides[0][2], sides[1][2]
    return out


def mean_surface_scores(scores):
    """the three means over the labels present in both maps (NaN when there is none), in the order of SURFACE_KEYS"""
    return tuple(mean_dice(scores[key]) for key in SURFACE_KEYS)


def surface_distances(seg, truth, label_list, percentile=95, voxel_size=1.0, device=None):
    """Hausdorff distance, `percentile`-th percentile distance and mean distance between the surfaces of two label maps of equal
    shape (arrays or paths), per label in the order of `label_list`, in units of `voxel_size`: surface_scores_from_d2 of the
    exact squared distance maps of ops.seg_surface_dist2.  Only the surface voxels leave the device."""
    import torch
    from . import ops
    lut = segmentation_lut(label_list)
    a, b = _label_map(seg), _label_map(truth)
    if a.ndim != 3 or a.shape != b.shape:
        raise ValueError('surface_distances: 3-D label maps of equal shape, got %s and %s' % (a.shape, b.shape))
    dev = device or 'cuda'
    N = int((lut >= 0).sum())
    lut_d = torch.from_numpy(lut).to(dev)
    a_d, b_d = torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev)
    d2_ab, d2_ba = ops.seg_surface_dist2(a_d, b_d, lut_d, N)
    sides = []
    for m, d2 in ((a_d, d2_ab), (b_d, d2_ba)):
        at = d2 >= 0                      # surface voxels: their label values are inside the table
        sides += [lut_d[m[at].long()].cpu().numpy(), d2[at].cpu().numpy()]
    return surface_scores_from_d2(*sides, N=N, percentile=percentile, voxel_size=voxel_size)
