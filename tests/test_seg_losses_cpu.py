"""Host side of the weighted-L2 warm-up and the cross-entropy of training_segmentation() (no GPU): the float64 formulas that
tests/test_seg_losses_gpu.py holds the kernels to, checked against the reference's own WeightedL2Loss.call / CrossEntropyLoss.call
(tests/golden/seg_losses.npz, written by tests/golden/gen/make_seg_losses_golden.py); the argument checks of
training_segmentation, UNet3D.loss_wl2 and UNet3D.loss_cross_entropy; the launcher's flags; the phase schedule."""
import inspect
import os
import sys

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'seg_losses.npz')


# ------------------------------------------------------------------------- the reference mathematics, on logits, any dtype
def wl2_loss(gt, z, target_value=5.):
    """WeightedL2Loss.call (ext/lab2im/layers.py:1408-1412) of logits z [..., N] against the one-hot gt [..., N] (rows may be
    all zero).  The voxel weights are the float32 values of `1 - gt[..., 0] + 1e-8` (:1411: 1e-8 on the background, exactly 1
    elsewhere), whatever the dtype of the rest"""
    weights = (1 - gt[..., 0].float() + 1e-8).to(z.dtype).unsqueeze(-1)                              # :1411
    return (weights * (z - target_value * (2 * gt.to(z.dtype) - 1)) ** 2).sum() / (weights.sum() * gt.shape[-1])   # :1412


def ce_loss_of_probs(gt, p):
    """CrossEntropyLoss.call (ext/lab2im/layers.py:1498-1526) with enable_checks=False and no weights, as the reference
    writes it: on posteriors"""
    import torch
    ce = -gt.to(p.dtype) * torch.log(p)          # :1499
    return ce.sum(-1).mean()                     # :1524: the sum along the labels, the mean over ALL voxels


def ce_loss(gt, z):
    """the same loss on logits: log softmax(z) in place of log(p) -- the same number wherever no posterior underflows"""
    import torch
    return -(gt.to(z.dtype) * torch.log_softmax(z, -1)).sum(-1).mean()


def test_float64_formulas_against_the_reference_layers():
    import torch
    g = np.load(GOLDEN)
    gt, z, p = (torch.from_numpy(g[k]) for k in ('gt', 'logits', 'probs'))
    assert list(gt.shape) == [1, 4, 5, 6, 5] and int((gt.sum(-1) == 0).sum()) >= 1 and int(gt[..., 0].sum()) >= 3
    # the golden scalars are float32 results of 600-term sums: 1e-6 relative
    for name, tv in (('wl2_t5', 5.), ('wl2_t3', 3.)):
        got = wl2_loss(gt.double(), z.double(), tv).item()
        assert abs(got - float(g[name])) < 1e-6 * abs(float(g[name])), (name, got, float(g[name]))
    got = ce_loss_of_probs(gt.double(), p.double()).item()
    assert abs(got - float(g['ce'])) < 1e-6 * abs(float(g['ce'])), (got, float(g['ce']))
    # and the logit form equals the posterior form (log softmax(log p) = log p for rows that sum to 1)
    pz = torch.softmax(z.double(), -1)
    assert abs(ce_loss(gt.double(), z.double()).item() - ce_loss_of_probs(gt.double(), pz).item()) < 1e-12
    # the background weight matters: without it the loss is another number
    w1 = ((z.double() - 5. * (2 * gt.double() - 1)) ** 2).mean().item()
    assert abs(w1 - float(g['wl2_t5'])) > 1e-3 * float(g['wl2_t5'])


# ------------------------------------------------------------------------- argument checks
@pytest.mark.parametrize('kw,msg', [
    (dict(wl2_epochs=-1), 'wl2_epochs should be an integer >= 0'),
    (dict(wl2_epochs=1.5), 'wl2_epochs should be an integer >= 0'),
    (dict(wl2_epochs='2'), 'wl2_epochs should be an integer >= 0'),
    (dict(wl2_epochs=True), 'wl2_epochs should be an integer >= 0'),
    (dict(wl2_target_value=0.), 'wl2_target_value should be a finite number > 0'),
    (dict(wl2_target_value=-5.), 'wl2_target_value should be a finite number > 0'),
    (dict(wl2_target_value=float('inf')), 'wl2_target_value should be a finite number > 0'),
    (dict(wl2_target_value=float('nan')), 'wl2_target_value should be a finite number > 0'),
    (dict(wl2_target_value='5'), 'wl2_target_value should be a finite number > 0'),
    (dict(segmentation_loss='l2'), 'segmentation_loss should be one of \'dice\', \'cross_entropy\''),
    (dict(segmentation_loss='wl2'), 'segmentation_loss should be one of'),
    (dict(segmentation_loss='cross_entropy', dice_class_weights=-1), 'unweighted cross-entropy: dice_class_weights'),
    (dict(segmentation_loss='cross_entropy', dice_class_weights=[1., 1., 1.]), 'unweighted cross-entropy: dice_class_weights'),
    (dict(segmentation_loss='cross_entropy', dice_boundary_weights=.5), 'unweighted cross-entropy: dice_boundary_weights'),
    (dict(segmentation_loss='cross_entropy', dice_boundary_dist=2), 'unweighted cross-entropy: dice_boundary_dist'),
    (dict(segmentation_loss='cross_entropy', dice_skip_background=False), 'unweighted cross-entropy: dice_skip_background'),
])
def test_loss_keywords_are_checked_before_anything_is_read(kw, msg):
    from synthsr_amd.segmentation_training import training_segmentation
    with pytest.raises(ValueError, match=msg):
        training_segmentation('/nowhere/labels', '/nowhere/models', None, None, None, np.array([0, 2, 3]), **kw)


def test_valid_loss_keywords_pass_the_checks():
    """the checks let every valid combination through: the call then fails on the label directory that does not exist"""
    from synthsr_amd.segmentation_training import training_segmentation, loss_settings
    assert loss_settings() == (0, 5.)
    assert loss_settings(np.int64(3), 2, 'cross_entropy') == (3, 2.)
    assert loss_settings(1, 5., 'dice', dice_class_weights=-1, dice_boundary_weights=.5, dice_boundary_dist=2) == (1, 5.)
    with pytest.raises(Exception) as e:
        training_segmentation('/nowhere/labels', '/nowhere/models', None, None, None, np.array([0, 2, 3]), wl2_epochs=2,
                              wl2_target_value=3., segmentation_loss='cross_entropy')
    assert 'wl2' not in str(e.value) and 'segmentation_loss' not in str(e.value)
    params = inspect.signature(training_segmentation).parameters
    assert (params['wl2_epochs'].default, params['wl2_target_value'].default, params['segmentation_loss'].default) == \
        (0, 5., 'dice')


def test_scope_messages_are_unchanged():
    from synthsr_amd.segmentation_training import check_scope
    with pytest.raises(NotImplementedError, match='fp32 only .*: the soft-Dice head kernels have no bf16 form'):
        check_scope(dtype='bf16')
    with pytest.raises(NotImplementedError, match='takes batchsize=1'):
        check_scope(batchsize=2)


def test_logit_losses_refuse_what_they_cannot_do():
    """on table_only nets (nothing allocated, no GPU): a linear head, a bf16 network and a bad target_value"""
    from synthsr_amd.unet import UNet3D
    kw = dict(feat_mult=2, nb_conv_per_level=2, batch_norm=-1, table_only=True)
    soft = UNet3D(24, [16, 16, 16, 1], 3, 3, 5, final_pred_activation='softmax', **kw)
    linear = UNet3D(24, [16, 16, 16, 1], 3, 3, 1, final_pred_activation='linear', **kw)
    bf16 = UNet3D(24, [16, 16, 16, 1], 3, 3, 5, final_pred_activation='softmax', dtype='bf16', **kw)
    p = inspect.signature(soft.loss_wl2).parameters
    assert list(p) == ['x', 'seg', 'lut', 'target_value'] and p['target_value'].default == 5.
    assert list(inspect.signature(soft.loss_cross_entropy).parameters) == ['x', 'seg', 'lut']
    with pytest.raises(ValueError, match=r'loss_wl2\(\) is for softmax heads'):
        linear.loss_wl2(None, None, None)
    with pytest.raises(ValueError, match=r'loss_cross_entropy\(\) is for softmax heads'):
        linear.loss_cross_entropy(None, None, None)
    with pytest.raises(NotImplementedError, match='fp32 only'):
        bf16.loss_wl2(None, None, None)
    with pytest.raises(NotImplementedError, match='fp32 only'):
        bf16.loss_cross_entropy(None, None, None)
    for bad in (0., -1., float('inf'), float('nan'), '5', None, True):
        with pytest.raises(ValueError, match='target_value should be a finite number > 0'):
            soft.loss_wl2(None, None, None, target_value=bad)


def test_ops_refuse_an_unknown_kind_before_they_touch_a_tensor():
    from synthsr_amd import ops
    assert ops.SEG_LOGIT_LOSSES == {'wl2': 0, 'ce': 1}
    for f in (lambda: ops.seg_head_logit_loss_fwd(*[None] * 9, 'dice'),
              lambda: ops.seg_head_logit_loss_bwd(*[None] * 12, 'l2')):
        with pytest.raises(ValueError, match='kind should be \'wl2\' or \'ce\''):
            f()


# ------------------------------------------------------------------------- launcher
def test_launcher_has_the_loss_flags():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    try:
        import training_segmentation as launcher
    finally:
        sys.path.pop(0)
    from synthsr_amd.segmentation_training import training_segmentation
    positional = ['l', 'm', 'pm', 'ps', 'gl', 'sl']
    a = vars(launcher.build_parser().parse_args(positional))
    assert (a['wl2_epochs'], a['wl2_target_value'], a['segmentation_loss']) == (0, 5., 'dice')
    assert type(a['wl2_epochs']) is int and type(a['wl2_target_value']) is float
    a = vars(launcher.build_parser().parse_args(positional + ['--wl2_epochs', '2', '--wl2_target_value', '3.5',
                                                              '--segmentation_loss', 'cross_entropy']))
    assert (a['wl2_epochs'], a['wl2_target_value'], a['segmentation_loss']) == (2, 3.5, 'cross_entropy')
    with pytest.raises(SystemExit):
        launcher.build_parser().parse_args(positional + ['--segmentation_loss', 'wl2'])
    params = inspect.signature(training_segmentation).parameters
    assert set(a) <= set(params)
    for name in ('wl2_epochs', 'wl2_target_value', 'segmentation_loss'):
        assert params[name].default == launcher.build_parser().get_default(name)


# ------------------------------------------------------------------------- phase schedule
@pytest.mark.parametrize('wl2_epochs', [0, 1, 3])
@pytest.mark.parametrize('segmentation_loss', ['dice', 'cross_entropy'])
def test_phase_schedule(wl2_epochs, segmentation_loss):
    """epoch index -> loss, and the one epoch in front of which the optimizer starts afresh"""
    from synthsr_amd.segmentation_training import phase_loss, phase_resets_optimizer
    epochs = range(6)
    assert [phase_loss(e, wl2_epochs, segmentation_loss) for e in epochs] == \
        ['wl2'] * wl2_epochs + [segmentation_loss] * (6 - wl2_epochs)
    assert [e for e in epochs if phase_resets_optimizer(e, wl2_epochs)] == ([wl2_epochs] if wl2_epochs else [])


@pytest.mark.parametrize('wl2_epochs,init_epoch,want_losses,want_reset_steps', [
    (0, 0, ['dice'] * 6, []),
    (0, 2, ['dice'] * 6, []),
    (1, 0, ['wl2'] * 2 + ['dice'] * 4, [2]),
    (1, 1, ['dice'] * 6, [0]),            # resumed from the checkpoint of epoch 1: the reset falls on the first step
    (1, 2, ['dice'] * 6, []),             # resumed later: nothing is reset
    (3, 0, ['wl2'] * 6, []),
    (3, 2, ['wl2'] * 2 + ['dice'] * 4, [2]),
    (3, 3, ['dice'] * 6, [0]),
    (3, 4, ['dice'] * 6, []),
])
def test_trainer_follows_the_schedule_from_init_epoch_and_its_step_count(wl2_epochs, init_epoch, want_losses, want_reset_steps):
    """SegmentationTrainer._loss on a stand-in network: which loss each of six steps (two per epoch) calls and in front of
    which steps the moments and the iteration count are zeroed"""
    from synthsr_amd.segmentation_training import SegmentationTrainer

    class Moment:
        def __init__(self):
            self.zeroed = 0

        def zero_(self):
            self.zeroed += 1

    class Net:
        def __init__(self):
            self.adam_m, self.adam_v, self.iterations, self.calls = Moment(), Moment(), 7, []

        def loss_wl2(self, x, seg, lut, target_value):
            self.calls.append('wl2')
            assert target_value == 4.

        def loss_dice(self, x, seg, lut, **kw):
            self.calls.append('dice')

        def loss_cross_entropy(self, x, seg, lut):
            self.calls.append('cross_entropy')

    tr = SegmentationTrainer.__new__(SegmentationTrainer)
    tr.net, tr.lut, tr.dice = Net(), None, {}
    tr.wl2_epochs, tr.wl2_target_value, tr.segmentation_loss = wl2_epochs, 4., 'dice'
    tr.init_epoch, tr.steps_per_epoch, tr.steps_done = init_epoch, 2, 0
    resets = []
    for i in range(6):
        tr.net.iterations = 7
        before = tr.net.adam_m.zeroed
        tr._loss(None, None)
        if tr.net.adam_m.zeroed != before:
            assert tr.net.iterations == 0 and tr.net.adam_v.zeroed == tr.net.adam_m.zeroed
            resets.append(i)
        else:
            assert tr.net.iterations == 7
        tr.steps_done += 1
    assert tr.net.calls == want_losses and resets == want_reset_steps
