"""`training_segmentation()` — trains the softmax-headed segmentation U-Net that `training(segmentation_model_file=...)`
freezes behind its prediction (SynthSR/training.py:371-409), with the soft Dice of `DiceLoss` (ext/lab2im/layers.py:1343-1376,
enable_checks=False) against the generator's own label map -- or with the two other losses the reference defines for such a
network: `WeightedL2Loss` on the logits (:1408-1412) for the first `wl2_epochs` epochs, the warm-up that gets a random head past
the flat start of the Dice, and `CrossEntropyLoss` (:1498-1526, unweighted) in place of the Dice.

    per step:  host input sampler -> generator kernels -> U-Net forward on the generator's regression TARGET (what the frozen
               regulariser will later be fed: a clean one-channel image) -> fused head + loss (UNet3D.loss_dice, or
               loss_wl2 / loss_cross_entropy, which keep no posteriors)
               -> backward -> Keras-semantics Adam.

The head's channel order is `segmentation_label_list`, the array `training(segmentation_label_list=...)` takes: a checkpoint
written here plugs straight in.  Generator, step, optimizer, logs and checkpoints are those of synthsr_amd.training.
Scope: fp32, one process, batchsize 1, losses dice | cross_entropy (unweighted) after an optional weighted-L2 warm-up;
everything else raises.
"""
import os
import numpy as np

from . import host_math as hm
from . import volumes
from .brain_generator import BrainGenerator
from .training import Trainer, fit_loop, load_checkpoint
from .unet import unet as build_unet


def segmentation_lut(segmentation_label_list):
    """int32 table label value -> head channel (the position of the value in `segmentation_label_list`), -1 for every value
    that is not listed; as long as the largest listed value + 1.  Values beyond the table have no class either."""
    labels = np.asarray(hm.load_array_if_path(segmentation_label_list)).reshape(-1)
    if labels.size < 2:
        raise ValueError('segmentation_label_list should hold at least two labels, holds %d' % labels.size)
    if np.any(labels != np.round(labels)) or np.any(labels < 0):
        raise ValueError('segmentation_label_list should hold non-negative integer label values')
    labels = labels.astype(np.int64)
    if len(np.unique(labels)) != len(labels):
        raise ValueError('segmentation_label_list holds a label twice')
    lut = np.full(int(labels.max()) + 1, -1, dtype=np.int32)
    lut[labels] = np.arange(len(labels), dtype=np.int32)
    return lut


SEGMENTATION_LOSSES = ('dice', 'cross_entropy')


def phase_loss(epoch, wl2_epochs=0, segmentation_loss='dice'):
    """the loss of the epoch with 0-based index `epoch`: 'wl2' during the warm-up, then `segmentation_loss`"""
    return 'wl2' if epoch < wl2_epochs else segmentation_loss


def phase_resets_optimizer(epoch, wl2_epochs=0):
    """whether the optimizer starts afresh (Adam moments and iteration count zeroed) in front of the first step of the epoch
    with 0-based index `epoch`: at the first epoch behind a warm-up, reached by training through it or by resuming there.  The
    weighted-L2 gradients are orders of magnitude larger than the Dice's and stale second moments would throttle the first
    Dice steps (the workflow this mirrors compiles the model anew between the phases)"""
    return wl2_epochs > 0 and epoch == wl2_epochs


def loss_settings(wl2_epochs=0, wl2_target_value=5., segmentation_loss='dice', dice_class_weights=None,
                  dice_boundary_weights=0., dice_boundary_dist=3, dice_skip_background=True):
    """the three loss keywords of training_segmentation, checked: (wl2_epochs, wl2_target_value) as (int, float)"""
    if isinstance(wl2_epochs, bool) or not isinstance(wl2_epochs, (int, np.integer)) or wl2_epochs < 0:
        raise ValueError('wl2_epochs should be an integer >= 0 (got %r)' % (wl2_epochs,))
    if isinstance(wl2_target_value, bool) or not isinstance(wl2_target_value, (int, float, np.integer, np.floating)) \
            or not np.isfinite(wl2_target_value) or not wl2_target_value > 0:
        raise ValueError('wl2_target_value should be a finite number > 0 (got %r)' % (wl2_target_value,))
    if segmentation_loss not in SEGMENTATION_LOSSES:
        raise ValueError('segmentation_loss should be one of %s (got %r)' % (', '.join(map(repr, SEGMENTATION_LOSSES)),
                                                                            segmentation_loss))
    if segmentation_loss == 'cross_entropy':
        at_default = dict(dice_class_weights=dice_class_weights is None,
                          dice_boundary_weights=np.ndim(dice_boundary_weights) == 0 and dice_boundary_weights == 0,
                          dice_boundary_dist=np.ndim(dice_boundary_dist) == 0 and dice_boundary_dist == 3,
                          dice_skip_background=dice_skip_background is True)
        values = dict(dice_class_weights=dice_class_weights, dice_boundary_weights=dice_boundary_weights,
                      dice_boundary_dist=dice_boundary_dist, dice_skip_background=dice_skip_background)
        for name, value in values.items():
            if not at_default[name]:
                raise ValueError('segmentation_loss=\'cross_entropy\' is the unweighted cross-entropy: %s=%r is a setting of '
                                 'the Dice (the reference\'s class-weighted cross-entropy sums over the wrong axis and is not '
                                 'restated)' % (name, value))
    return int(wl2_epochs), float(wl2_target_value)


class SegmentationTrainer(Trainer):
    """generator + softmax-headed U-Net + soft Dice (or cross-entropy, behind an optional weighted-L2 warm-up) + Adam; the
    sample, the optimizer step and the moving statistics are Trainer's"""

    def __init__(self, brain_generator, net, lut, lr=1e-4, lr_decay=0.0, fixed_sample=False, dice=None, wl2_epochs=0,
                 wl2_target_value=5., segmentation_loss='dice', init_epoch=0, steps_per_epoch=1):
        import torch
        Trainer.__init__(self, brain_generator, net, lr, lr_decay)
        self.lut = torch.as_tensor(np.asarray(lut, dtype=np.int32)).to(net.device)
        self.fixed_sample = bool(fixed_sample)
        self.dice = dict(dice or {})   # the weights of UNet3D.loss_dice (dice_settings); empty: the plain soft Dice
        self._fixed = None
        self.wl2_epochs, self.wl2_target_value, self.segmentation_loss = int(wl2_epochs), float(wl2_target_value), segmentation_loss
        self.init_epoch, self.steps_per_epoch = int(init_epoch), int(steps_per_epoch)
        self.steps_done = 0   # steps of this trainer: with init_epoch and steps_per_epoch, the epoch a step belongs to

    def _loss(self, x, seg):
        """forward + the loss of the epoch this step belongs to; in front of the first step behind the warm-up the optimizer
        starts afresh (phase_resets_optimizer)"""
        net = self.net
        epoch = self.init_epoch + self.steps_done // self.steps_per_epoch
        if self.steps_done % self.steps_per_epoch == 0 and phase_resets_optimizer(epoch, self.wl2_epochs):
            net.adam_m.zero_()
            net.adam_v.zero_()
            net.iterations = 0
        kind = phase_loss(epoch, self.wl2_epochs, self.segmentation_loss)
        if kind == 'wl2':
            return net.loss_wl2(x, seg, self.lut, self.wl2_target_value)
        if kind == 'cross_entropy':
            return net.loss_cross_entropy(x, seg, self.lut)
        return net.loss_dice(x, seg, self.lut, **self.dice)

    def step(self, model_inputs=None, draws=None, label_index=None):
        """one training step; returns the loss as a 1-element device tensor (no host sync)"""
        from . import ops
        net = self.net
        if self._fixed is not None:
            x, seg = self._fixed
        else:
            _, target, seg, B = self._generate(model_inputs, draws, label_index)
            if B != 1:
                raise NotImplementedError('training_segmentation takes batchsize=1 (got a batch of %d)' % B)
            if target.shape[-1] != 1 or list(seg.shape) != list(target.shape[:3]):
                raise ValueError('the segmentation network reads ONE regression target on the label maps\' grid (target %s, '
                                 'label map %s)' % (list(target.shape), list(seg.shape)))
            x = target
            if self.fixed_sample:   # the first sample, kept: every step trains on it
                self._fixed = x, seg = target.clone(), seg.clone()
        net.set_batch(1)
        with ops.trace_range('forward + loss'):
            loss = self._loss(x, seg)
        with ops.trace_range('backward'):
            net.backward()
        with ops.trace_range('optimizer'):
            net.adam_step(self.lr, self.lr_decay)
            net.update_moving_stats()
        self.steps_done += 1
        return loss


def check_scope(batchsize=1, dtype='f32', images_dir=None, fs_header_segnet=False, world_size=1):
    """the follow-ups of training_segmentation: refused, not silently different"""
    if dtype != 'f32':
        raise NotImplementedError('training_segmentation is fp32 only (dtype=%r): the soft-Dice head kernels have no bf16 form'
                                  % (dtype,))
    if batchsize != 1:
        raise NotImplementedError('training_segmentation takes batchsize=1 (got %r)' % (batchsize,))
    if world_size > 1:
        raise NotImplementedError('training_segmentation runs in one process (WORLD_SIZE=%d)' % world_size)
    if images_dir is not None:
        raise NotImplementedError('training_segmentation synthesises its images from the label maps: images_dir is not '
                                  'supported')
    if fs_header_segnet:
        raise NotImplementedError('training_segmentation trains in the generator\'s frame: fs_header_segnet is not supported')


def dice_settings(n_labels, dice_class_weights=None, dice_boundary_weights=0., dice_boundary_dist=3,
                  dice_skip_background=True):
    """the four Dice settings of training_segmentation as keywords of UNet3D.loss_dice, checked: class weights None, -1
    (dynamic; '-1' from a command line), a sequence or the path of a .npy of n_labels finite values >= 0 that are not all zero;
    boundary weights a finite number >= 0; a boundary distance of 1 .. 5"""
    from .ops import check_boundary_dist
    from .unet import dice_class_weights as normalised
    cw = dice_class_weights
    if isinstance(cw, str):
        cw = None if cw in ('', 'None') else (-1 if cw.strip() == '-1' else np.load(cw))
    if cw is not None and not (np.ndim(cw) == 0 and cw == -1):
        if np.ndim(cw) == 0:
            raise ValueError('dice_class_weights: None, -1 (dynamic), a sequence or a .npy path (got %r)' % (dice_class_weights,))
        cw = normalised(cw, n_labels)
    elif cw is not None:
        cw = -1
    bw = float(dice_boundary_weights)
    if not bw >= 0. or not np.isfinite(bw):
        raise ValueError('dice_boundary_weights should be a finite number >= 0 (got %r)' % (dice_boundary_weights,))
    return dict(class_weights=cw, boundary_weights=bw, boundary_dist=check_boundary_dist(dice_boundary_dist),
                skip_background=bool(dice_skip_background))


def training_segmentation(labels_dir, model_dir, prior_means, prior_stds, path_generation_labels, segmentation_label_list,
                          prior_distributions='normal', images_dir=None, path_generation_classes=None, FS_sort=True,
                          batchsize=1, input_channels=True, output_channel=0, target_res=None, output_shape=None,
                          flipping=True, padding_margin=None, scaling_bounds=0.15, rotation_bounds=15, shearing_bounds=0.02,
                          translation_bounds=5, nonlin_std=4., nonlin_shape_factor=0.03125,
                          simulate_registration_error=True, data_res=None, thickness=None, randomise_res=None,
                          downsample=True, blur_range=1.15, build_reliability_maps=True, bias_field_std=.3,
                          bias_shape_factor=0.03125, n_levels=5, nb_conv_per_level=2, conv_size=3, unet_feat_count=24,
                          feat_multiplier=2, dropout=0, activation='elu', lr=1e-4, lr_decay=0, epochs=100,
                          steps_per_epoch=1000, checkpoint=None, seed=0, verbose=True, dtype='f32', deterministic=False,
                          fs_header_segnet=False, fixed_sample=False, step_losses=None, dice_class_weights=None,
                          dice_boundary_weights=0., dice_boundary_dist=3, dice_skip_background=True, wl2_epochs=0,
                          wl2_target_value=5., segmentation_loss='dice'):
    """Generator arguments: those of synthsr_amd.training.training, same names and defaults.  `segmentation_label_list`
    (array or path): the label values the network predicts, in head-channel order; label values of the maps that are not
    listed have no class (an all-zero ground-truth row).  `output_channel`: ONE index, the synthetic channel the network is
    trained on (the generator's regression target, as is).  `fixed_sample`: every step trains on the first sample drawn
    (overfitting tests).  `step_losses` (optional list): receives every step's loss as a float, at the cost of a host
    synchronisation per step.
    The weights of the reference's DiceLoss (UNet3D.loss_dice), all off by default: `dice_class_weights` None, -1 (dynamic:
    the inverse of each label's volume in the sample; a label that the sample does not hold gets weight 0 where the reference
    divides by zero), a sequence or the path of a .npy with one value >= 0 per entry of segmentation_label_list;
    `dice_boundary_weights` (bonus weight of voxels within `dice_boundary_dist`, 1 .. 5, of a label's boundary) and
    `dice_skip_background` (no bonus for the first label of the list).
    `wl2_epochs`: the epochs with 0-based index < wl2_epochs (counted from the start of the whole run, not from a resumed
    checkpoint) train with WeightedL2Loss on the logits (UNet3D.loss_wl2, `wl2_target_value`), the others with
    `segmentation_loss`: 'dice' or 'cross_entropy' (UNet3D.loss_cross_entropy: unweighted, every dice_* setting at its
    default).  In front of the first step of epoch index wl2_epochs, trained up to or resumed at, the Adam moments and the
    iteration count are zeroed; resuming at a later epoch resets nothing.  Returns the network."""
    check_scope(batchsize, dtype, images_dir, fs_header_segnet, int(os.environ.get('WORLD_SIZE', '1')))
    wl2_epochs, wl2_target_value = loss_settings(wl2_epochs, wl2_target_value, segmentation_loss, dice_class_weights,
                                                 dice_boundary_weights, dice_boundary_dist, dice_skip_background)
    if deterministic:  # process-wide switch: on for the duration of this call, previous setting restored on the way out
        from . import ops as _ops
        kw = dict(locals())
        kw.pop('_ops', None)
        kw['deterministic'] = False
        previous = _ops.set_deterministic(True)
        try:
            return training_segmentation(**kw)
        finally:
            _ops.set_deterministic(previous)
    input_channels = [{'True': True, 'False': False}.get(c, c) if isinstance(c, str) else c
                      for c in hm.reformat_to_list(input_channels)]
    output_channel = None if output_channel is None else list(hm.reformat_to_list(output_channel))
    if output_channel is None or len(output_channel) != 1:
        raise ValueError('training_segmentation needs ONE output_channel: the segmentation network takes a single-channel '
                         'image (SynthSR/training.py:375), got %r' % (output_channel,))
    if output_channel[0] >= len(input_channels):
        raise Exception('indices in output_channel cannot be greater than the total number of channels')
    lut = segmentation_lut(segmentation_label_list)
    n_seg = int((lut >= 0).sum())
    dice = dice_settings(n_seg, dice_class_weights, dice_boundary_weights, dice_boundary_dist, dice_skip_background)

    generation_labels, n_neutral_labels = volumes.get_list_labels(label_list=path_generation_labels, labels_dir=labels_dir,
                                                                  FS_sort=FS_sort)
    os.makedirs(model_dir, exist_ok=True)
    rng = np.random.Generator(np.random.Philox(key=(int(seed) << 20)))
    brain_generator = BrainGenerator(labels_dir=labels_dir, images_dir=None, generation_labels=generation_labels,
                                     n_neutral_labels=n_neutral_labels, padding_margin=padding_margin, batchsize=1,
                                     input_channels=input_channels, output_channel=output_channel, target_res=target_res,
                                     output_shape=output_shape, output_div_by_n=2 ** n_levels,
                                     generation_classes=path_generation_classes, prior_means=prior_means,
                                     prior_stds=prior_stds, prior_distributions=prior_distributions, flipping=flipping,
                                     scaling_bounds=scaling_bounds, rotation_bounds=rotation_bounds,
                                     shearing_bounds=shearing_bounds, translation_bounds=translation_bounds,
                                     nonlin_std=nonlin_std, nonlin_shape_factor=nonlin_shape_factor,
                                     simulate_registration_error=simulate_registration_error, randomise_res=randomise_res,
                                     data_res=data_res, thickness=thickness, downsample=downsample, blur_range=blur_range,
                                     build_reliability_maps=build_reliability_maps, bias_field_std=bias_field_std,
                                     bias_shape_factor=bias_shape_factor, rng=rng)
    brain_generator.labels_to_image_model.seed(seed, 0)
    shape = list(brain_generator.model_output_shape[:-1])
    net = build_unet(nb_features=unet_feat_count, input_shape=shape + [1], nb_levels=n_levels, conv_size=conv_size,
                     nb_labels=n_seg, feat_mult=feat_multiplier, nb_conv_per_level=nb_conv_per_level, conv_dropout=dropout,
                     final_pred_activation='softmax', batch_norm=-1, activation=activation, input_model=None, seed=seed)
    init_epoch = 0
    if checkpoint is not None:
        if verbose:
            print('loading', checkpoint)
        load_checkpoint(checkpoint, net)
        try:
            init_epoch = int(os.path.basename(checkpoint)[:3])
        except ValueError:
            init_epoch = 0
    trainer = SegmentationTrainer(brain_generator, net, lut, lr, lr_decay, fixed_sample=fixed_sample, dice=dice,
                                  wl2_epochs=wl2_epochs, wl2_target_value=wl2_target_value, segmentation_loss=segmentation_loss,
                                  init_epoch=init_epoch, steps_per_epoch=steps_per_epoch)
    step = trainer.step
    if step_losses is not None:
        def step():
            loss = trainer.step()
            step_losses.append(float(loss.item()))
            return loss
    fit_loop(step, net, model_dir, init_epoch, epochs, steps_per_epoch, verbose=verbose)
    return net
