"""GPU end-to-end: the `training()` entry point on NIfTI label maps (checkpoint + resume), BrainGenerator.generate_brain,
and bench.py under torch.distributed.run with the RCCL gradient all-reduce path forced at world size 1."""
import json
import os
import subprocess
import sys
import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _write_labels(tmp_path, n=2, shape=(40, 36, 48)):
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import synthetic_label_map
    d = tmp_path / 'labels'
    d.mkdir()
    for i in range(n):
        write_nifti(str(d / ('brain%d_labels.nii.gz' % i)), synthetic_label_map(shape, 10 + i).astype(np.float32))
    return str(d)


def test_training_entry_point_checkpoint_and_resume(tmp_path):
    import torch
    from synthsr_amd.training import training
    from synthsr_amd.synthetic import GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR
    labels_dir = _write_labels(tmp_path)
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    np.save(tmp_path / 'gc.npy', GENERATION_CLASSES)
    np.save(tmp_path / 'pm.npy', PRIOR_MEANS_T1_HR)
    np.save(tmp_path / 'ps.npy', PRIOR_STDS_T1_HR)
    model_dir = str(tmp_path / 'models')
    kw = dict(path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3, unet_feat_count=24,
              nonlin_shape_factor=.125, bias_shape_factor=.125, steps_per_epoch=3, verbose=False)
    net = training(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                   epochs=1, **kw)
    assert net.iterations == 3
    ck = os.path.join(model_dir, '001.npz')
    assert os.path.exists(ck)
    z = np.load(ck)
    assert 'unet_conv_downarm_0_0/kernel' in z.files and z['unet_conv_downarm_0_0/kernel'].shape == (3, 3, 3, 2, 24)
    assert 'unet_bn_down_0/moving_variance' in z.files and 'unet_likelihood/kernel' in z.files
    log = open(os.path.join(model_dir, 'logs', 'loss.csv')).read().strip().split('\n')
    assert len(log) == 1 and np.isfinite(float(log[0].split(',')[1]))
    # resume from the checkpoint: epoch parsed from the file name, optimizer state restored
    net2 = training(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                    epochs=2, checkpoint=ck, **kw)
    assert net2.iterations == 6 and os.path.exists(os.path.join(model_dir, '002.npz'))
    # the reference's checkpoint name, Keras layout: same weights as the .npz, and training resumes from it by name
    from synthsr_amd.keras_h5 import load_keras_weights
    h5 = load_keras_weights(os.path.join(model_dir, '001.h5'))
    assert all(np.array_equal(h5[k].reshape(z[k].shape), z[k]) for k in z.files if not k.startswith('optimizer/'))
    assert len(h5) == len([k for k in z.files if not k.startswith('optimizer/')])
    net3 = training(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                    epochs=2, checkpoint=os.path.join(model_dir, '001.h5'), **kw)
    assert net3.iterations == 3  # weights only: the optimizer restarts, like load_weights(by_name=True) in the reference
    # argument validation mirrors the reference's exceptions
    with pytest.raises(Exception):
        training(labels_dir, model_dir, None, None, str(tmp_path / 'gl.npy'), output_channel=None)
    with pytest.raises(Exception):
        training(labels_dir, model_dir, None, None, str(tmp_path / 'gl.npy'), output_channel=3)


def test_brain_generator_generate_brain(tmp_path):
    from synthsr_amd.brain_generator import BrainGenerator
    from synthsr_amd.synthetic import GENERATION_LABELS
    labels_dir = _write_labels(tmp_path, 1, (40, 36, 48))
    bg = BrainGenerator(labels_dir, None, None, 'uniform', GENERATION_LABELS, output_shape=32, output_div_by_n=8,
                        build_reliability_maps=True)
    image, target = bg.generate_brain()
    assert image.shape == (32, 32, 32, 2) and target.shape == (32, 32, 32)
    assert np.isfinite(image).all() and (image[..., 1] == 1).all() and 0 <= target.min() and target.max() <= 1 + 1e-6
    assert bg.model_output_shape == [32, 32, 32, 2] and bg.n_dims == 3 and bg.aff.shape == (4, 4)
    # padding margin (PadAroundCentre) and 2 input channels with registration error run through
    bg2 = BrainGenerator(labels_dir, None, None, 'uniform', GENERATION_LABELS, output_shape=32, output_div_by_n=8,
                         padding_margin=4, input_channels=[True, True], output_channel=1,
                         data_res=np.array([[1., 1., 3.], [1., 1., 1.]]), thickness=np.array([[1., 1., 3.], [1., 1., 1.]]),
                         downsample=True, build_reliability_maps=True)
    im2, tg2 = bg2.generate_brain()
    assert im2.shape == (32, 32, 32, 4) and np.isfinite(im2).all()
    assert set(np.unique(np.round(im2[..., 1], 6)).tolist()) != {1.0}  # channel 0 is down-sampled in z: sparse map


def test_generate_brain_native_orientation_vs_oracle(tmp_path):
    """H19 (SynthSR/brain_generator.py:317-330): label maps stored in a NON-RAS orientation (axes permuted and two of them
    reversed).  The generator works in the RAS frame and generate_brain() re-orients every item back to the native frame of
    the label maps (`align_volume_to_ref(aff_ref=self.aff)`).  Checked end to end against the oracle: the same host draws
    (the model's numpy Philox stream replayed) and the in-kernel noise stream (oracle/philox_ref) go into
    oracle.generator_ref.labels_to_image on the RAS label map; its outputs are brought to the native frame by EXPLICIT index
    arithmetic written out for this affine (not by the product's align_volume_to_ref).  Also .mgz: the same volume stored as
    MGZ goes through the same path."""
    from conftest import tape_from_draws
    from oracle import generator_ref as R
    from oracle import philox_ref
    from synthsr_amd.brain_generator import BrainGenerator
    from synthsr_amd.mgh import write_mgh
    from synthsr_amd.model_inputs import build_model_inputs
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import GENERATION_LABELS, GENERATION_CLASSES, synthetic_label_map
    ras_shape = (40, 36, 48)
    lab_ras = synthetic_label_map(ras_shape, 21)
    nx, ny, nz = ras_shape
    # native voxel (i, j, k) sits at world (x, y, z) = (nx-1-k, i, nz-1-j): native axis 0 runs along +y (A), axis 1 along -z
    # (I), axis 2 along -x (L)  =>  N[i, j, k] = R[nx-1-k, i, nz-1-j]
    to_native = lambda r: np.ascontiguousarray(np.moveaxis(r, (0, 1, 2), (2, 0, 1))[:, ::-1, ::-1])
    native = to_native(lab_ras)
    assert native.shape == (ny, nz, nx) and native[3, 5, 7] == lab_ras[nx - 1 - 7, 3, nz - 1 - 5]
    aff = np.array([[0., 0., -1., nx - 1.], [1., 0., 0., 0.], [0., -1., 0., nz - 1.], [0., 0., 0., 1.]])
    kw = dict(output_shape=[32, 24, 40], output_div_by_n=8, build_reliability_maps=True, bias_shape_factor=.125,
              nonlin_shape_factor=.125, generation_classes=GENERATION_CLASSES)
    out = {}
    for ext in ('nii.gz', 'mgz'):
        d = tmp_path / ('labels_' + ext.replace('.', '_'))
        d.mkdir()
        path = str(d / ('brain_labels.' + ext))
        if ext == 'mgz':
            write_mgh(path, native.astype(np.int32), aff)
        else:
            write_nifti(path, native.astype(np.float32), aff)
        bg = BrainGenerator(str(d), None, None, 'uniform', GENERATION_LABELS, rng=np.random.default_rng(3), **kw)
        assert bg.labels_shape == list(ras_shape) and np.allclose(bg.aff, aff) and bg.n_dims == 3
        m = bg.labels_to_image_model
        m.seed(11)
        dr = m.sample_draws()
        m.seed(11)                                   # generate_brain() will draw exactly `dr` again
        twin = build_model_inputs([path], len(GENERATION_LABELS), None, None, 'uniform', n_channels=1,
                                  generation_classes=GENERATION_CLASSES, rng=np.random.default_rng(3))
        labels_in, means, stds = next(twin)
        assert np.array_equal(labels_in[0, ..., 0], lab_ras)      # loading re-oriented the stored map to RAS
        image, target = bg.generate_brain()
        out[ext] = (image, target)
        if ext == 'mgz':
            continue
        noise = philox_ref.normals(m.ncrop, 1, dr.philox_key, dr.philox_offset)
        ref = R.labels_to_image(lab_ras, means[0], stds[0], tape_from_draws(m, dr, noise), GENERATION_LABELS,
                                len(GENERATION_LABELS), input_channels=[True], output_channel=[0], output_shape=[32, 24, 40],
                                output_div_by_n=8, build_reliability_maps=True, bias_shape_factor=.125,
                                nonlin_shape_factor=.125, translation_bounds=5)
        want_image, want_target = to_native(ref['image']), to_native(ref['target'])[..., 0]
        assert image.shape == want_image.shape == (24, 40, 32, 2) and target.shape == (24, 40, 32)
        assert np.abs(image - want_image).max() < 3e-5, np.abs(image - want_image).max()
        assert np.abs(target - want_target).max() < 3e-5, np.abs(target - want_target).max()
        assert np.abs(image - ref['image'].transpose(1, 2, 0, 3)).max() > 1e-2   # the flips matter: a bare transpose is wrong
    # the MGZ copy of the same map (different container, same geometry) generates the same sample
    assert np.array_equal(out['mgz'][0], out['nii.gz'][0]) and np.array_equal(out['mgz'][1], out['nii.gz'][1])


def test_real_image_targets_images_dir(tmp_path):
    """images_dir: BrainGenerator / training() with real scans as regression targets"""
    from synthsr_amd.brain_generator import BrainGenerator
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import GENERATION_LABELS, synthetic_label_map
    from synthsr_amd.training import training
    labels_dir = _write_labels(tmp_path, 2, (40, 36, 48))
    d = tmp_path / 'images'
    d.mkdir()
    rng = np.random.RandomState(0)
    lut = rng.uniform(30, 220, 64)
    for i in range(2):  # a "scan" = intensity per label + noise, same grid as the label map
        lab = synthetic_label_map((40, 36, 48), 10 + i)
        write_nifti(str(d / ('brain%d.nii.gz' % i)), (lut[lab % 64] + rng.randn(*lab.shape)).astype(np.float32))
    bg = BrainGenerator(labels_dir, None, None, 'uniform', GENERATION_LABELS, images_dir=str(d), output_channel=None,
                        output_shape=32, output_div_by_n=8, build_reliability_maps=True)
    image, target = bg.generate_brain()
    assert image.shape == (32, 32, 32, 2) and target.shape == (32, 32, 32)
    assert np.isfinite(target).all() and target.min() == 0.0 and abs(target.max() - 1.0) < 1e-5
    assert len(np.unique(np.round(target, 3))) > 20  # a resampled scan, not a label map
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    net = training(labels_dir, str(tmp_path / 'models'), None, None, str(tmp_path / 'gl.npy'), images_dir=str(d),
                   output_channel=None, output_shape=32, n_levels=3, unet_feat_count=24, nonlin_shape_factor=.125,
                   bias_shape_factor=.125, steps_per_epoch=2, epochs=1, verbose=False)
    assert net.iterations == 2
    with pytest.raises(Exception, match='not both'):
        training(labels_dir, str(tmp_path / 'm2'), None, None, str(tmp_path / 'gl.npy'), images_dir=str(d), output_channel=0)


def test_training_with_segmentation_regularised_loss(tmp_path):
    """training(..., segmentation_model_file=...): frozen segmentation U-Net checkpoint, label list and
    equivalency from .npy files; loss = L1 + 0.25 * Dice"""
    import torch
    from synthsr_amd.training import training, save_checkpoint
    from synthsr_amd.synthetic import GENERATION_LABELS
    from synthsr_amd.unet import unet
    labels_dir = _write_labels(tmp_path, 2, (32, 32, 32))
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    seg_labels = np.array([0, 2, 3, 4, 41, 42, 17])
    np.save(tmp_path / 'seg_labels.npy', seg_labels)
    np.save(tmp_path / 'seg_eq.npy', np.array([0, 2, 3, 4, 2, 3, 17]))  # right-hemisphere labels merged onto the left ones
    seg_net = unet(24, [32, 32, 32, 1], 3, 3, len(seg_labels), feat_mult=2, nb_conv_per_level=2, batch_norm=-1,
                   activation='elu', final_pred_activation='softmax', seed=9)
    save_checkpoint(str(tmp_path / 'seg.npz'), seg_net)
    common = dict(output_shape=32, n_levels=3, unet_feat_count=24, nonlin_shape_factor=.125, bias_shape_factor=.125,
                  steps_per_epoch=2, epochs=1, verbose=False)
    net = training(labels_dir, str(tmp_path / 'm_seg'), None, None, str(tmp_path / 'gl.npy'),
                   segmentation_label_list=str(tmp_path / 'seg_labels.npy'),
                   segmentation_label_equivalency=str(tmp_path / 'seg_eq.npy'),
                   segmentation_model_file=str(tmp_path / 'seg.npz'), relative_weight_segmentation=0.25, **common)
    assert net.iterations == 2
    log = open(os.path.join(str(tmp_path / 'm_seg'), 'logs', 'loss.csv')).read().strip().split(',')
    total = float(log[1])
    net0 = training(labels_dir, str(tmp_path / 'm_plain'), None, None, str(tmp_path / 'gl.npy'), **common)
    plain = float(open(os.path.join(str(tmp_path / 'm_plain'), 'logs', 'loss.csv')).read().strip().split(',')[1])
    # same seeds, same first step: the regularised loss is the L1 loss plus 0.25 * Dice with 0 < Dice < 1
    assert np.isfinite(total) and plain < total < plain + 0.25
    # batchsize 2: the frozen network runs on the stacked batch, the Dice is the mean over the two volumes
    net2 = training(labels_dir, str(tmp_path / 'm_seg2'), None, None, str(tmp_path / 'gl.npy'), batchsize=2,
                    segmentation_label_list=str(tmp_path / 'seg_labels.npy'),
                    segmentation_label_equivalency=str(tmp_path / 'seg_eq.npy'),
                    segmentation_model_file=str(tmp_path / 'seg.npz'), relative_weight_segmentation=0.25, **common)
    total2 = float(open(os.path.join(str(tmp_path / 'm_seg2'), 'logs', 'loss.csv')).read().strip().split(',')[1])
    assert net2.iterations == 2 and net2.batch == 2 and np.isfinite(total2) and 0 < total2 < 2


def test_training_batchsize_2_with_dropout(tmp_path):
    """training(batchsize=2, dropout=.2) (SynthSR/training.py:52, 76): the U-Net draws one feature mask per sample
    (KL.Dropout noise_shape [None, 1, 1, 1, C]); the loss of a fixed pair of label maps goes down, checkpoints hold finite
    weights and the moving statistics"""
    from synthsr_amd.training import training
    from synthsr_amd.synthetic import GENERATION_LABELS
    labels_dir = _write_labels(tmp_path, 2, (32, 32, 32))
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    net = training(labels_dir, str(tmp_path / 'm'), None, None, str(tmp_path / 'gl.npy'), batchsize=2, dropout=.2,
                   output_shape=32, n_levels=3, unet_feat_count=24, nonlin_shape_factor=.125, bias_shape_factor=.125,
                   steps_per_epoch=4, epochs=3, verbose=False, lr=1e-3)
    assert net.iterations == 12 and net.batch == 2 and net.conv_dropout == .2
    assert net._drop is None and net._drop_ps is not None
    masks = next(iter(net._drop_ps.values())).cpu().numpy()
    assert masks.shape[0] == 2 and np.all((masks == 0) | (np.abs(masks - 1.25) < 1e-6))
    log = [float(l.split(',')[1]) for l in open(os.path.join(str(tmp_path / 'm'), 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 3 and all(np.isfinite(log)) and log[-1] < log[0]
    z = np.load(os.path.join(str(tmp_path / 'm'), '003.npz'))
    assert all(np.isfinite(z[k]).all() for k in z.files if z[k].dtype.kind == 'f')


@pytest.mark.parametrize('metric,cropping', [('l2', 16), ('laplace', None), ('laplace', [24, 16, 16]), ('ssim', None),
                                             ('ssim', 24)])
def test_training_regression_metrics_and_loss_cropping(tmp_path, metric, cropping):
    """training(regression_metric='l2'|'laplace', loss_cropping=...) (SynthSR/training.py:85-87): the loss of a fixed
    batch goes down over the steps, the laplace network carries the 2-channel head, unknown metrics raise"""
    from synthsr_amd.training import training
    from synthsr_amd.synthetic import GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR
    labels_dir = _write_labels(tmp_path, n=1)
    for nm, a in (('gl', GENERATION_LABELS), ('gc', GENERATION_CLASSES), ('pm', PRIOR_MEANS_T1_HR), ('ps', PRIOR_STDS_T1_HR)):
        np.save(tmp_path / (nm + '.npy'), a)
    model_dir = str(tmp_path / 'models')
    args = (labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'))
    kw = dict(path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3, unet_feat_count=24,
              nonlin_shape_factor=.125, bias_shape_factor=.125, steps_per_epoch=4, verbose=False, lr=1e-3)
    net = training(*args, epochs=3, regression_metric=metric, loss_cropping=cropping, **kw)
    assert net.nb_labels == (2 if metric == 'laplace' else 1) and net.iterations == 12
    z = np.load(os.path.join(model_dir, '003.npz'))
    assert z['unet_likelihood/kernel'].shape[-1] == net.nb_labels
    log = [float(l.split(',')[1]) for l in open(os.path.join(model_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 3 and all(np.isfinite(log)) and log[-1] < log[0]
    with pytest.raises(Exception):
        training(*args, regression_metric='huber', **kw)


def test_training_two_output_channels_with_residuals(tmp_path):
    """training(input_channels=[True, True], output_channel=[0, 1], work_with_residual_channel=[0, 1]) (SynthSR/
    training.py:246-249, metrics_model.py:53-64): 2-channel head, per-target residual channels"""
    from synthsr_amd.training import training
    from synthsr_amd.synthetic import GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR
    labels_dir = _write_labels(tmp_path, n=1)
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    np.save(tmp_path / 'gc.npy', GENERATION_CLASSES)
    np.save(tmp_path / 'pm.npy', np.concatenate([PRIOR_MEANS_T1_HR, PRIOR_MEANS_T1_HR[:, ::-1]]))
    np.save(tmp_path / 'ps.npy', np.concatenate([PRIOR_STDS_T1_HR, PRIOR_STDS_T1_HR]))
    model_dir = str(tmp_path / 'models')
    net = training(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                   path_generation_classes=str(tmp_path / 'gc.npy'), input_channels=[True, True], output_channel=[0, 1],
                   work_with_residual_channel=[0, 1], build_reliability_maps=False, output_shape=32, n_levels=3,
                   unet_feat_count=24, nonlin_shape_factor=.125, bias_shape_factor=.125, steps_per_epoch=4, epochs=3,
                   verbose=False, lr=1e-3)
    assert net.nb_labels == 2 and net.input_shape[3] == 2
    log = [float(l.split(',')[1]) for l in open(os.path.join(model_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 3 and all(np.isfinite(log)) and log[-1] < log[0]


def test_training_tutorial7_residual_channel_with_reliability_maps(tmp_path):
    """scripts/tutorials/7-training.py configuration: work_with_residual_channel=[0] together with build_reliability_maps
    (the reference repeats the list, SynthSR/training.py:270-271, F11): trains, and the residual is image_out[..., 0]"""
    from synthsr_amd.training import training
    from synthsr_amd.synthetic import GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR
    labels_dir = _write_labels(tmp_path, n=1)
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    np.save(tmp_path / 'gc.npy', GENERATION_CLASSES)
    np.save(tmp_path / 'pm.npy', PRIOR_MEANS_T1_HR)
    np.save(tmp_path / 'ps.npy', PRIOR_STDS_T1_HR)
    model_dir = str(tmp_path / 'models')
    kw = dict(path_generation_classes=str(tmp_path / 'gc.npy'), input_channels=[True], output_channel=[0],
              build_reliability_maps=True, data_res=[1., 1., 3.], output_shape=32, n_levels=3, unet_feat_count=24,
              nonlin_shape_factor=.125, bias_shape_factor=.125, steps_per_epoch=4, epochs=3, verbose=False, lr=1e-3)
    args = (labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'))
    net = training(*args, work_with_residual_channel=[0], **kw)
    assert net.input_shape[3] == 2
    log = [float(l.split(',')[1]) for l in open(os.path.join(model_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 3 and all(np.isfinite(log)) and log[-1] < log[0]
    kw2 = dict(kw, input_channels=[True, True], output_channel=[0, 1])
    with pytest.raises(ValueError):       # keras' Add cannot broadcast the repeated list [0, 1, 0, 1] against 2 channels
        training(*args, work_with_residual_channel=[0, 1], **kw2)


def test_bench_under_torchrun_with_forced_allreduce(tmp_path):
    port = 29600 + (os.getpid() % 300)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr',
           '127.0.0.1', '--master-port', str(port), os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', '3',
           '--warmup', '1', '--size', '64', '--full', '--no-cpu-baseline', '--force-allreduce', '--dump-outputs', str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('{')][-1]
    d = json.loads(line)
    assert d['n_gpus'] == 1 and d['steps'] == 3 and d['value'] > 0 and np.isfinite(d['final_loss'])
    assert d['roofline']['bound'] == 'mfma' and 0 < d['roofline']['frac'] < 1
    # --dump-outputs: the last timed step's loss, every weight, a gradient sample; float32, 64 MB at most
    out = {n: np.load(str(tmp_path / (n + '.npy'))) for n in ('loss', 'params', 'grads_sample')}
    assert all(a.dtype == np.float32 for a in out.values()) and sum(a.nbytes for a in out.values()) <= 64 << 20
    assert abs(float(out['loss'][0]) - d['final_loss']) < 1e-6 and out['params'].size == 13240489
    assert np.isfinite(out['params']).all() and np.isfinite(out['grads_sample']).all()


def test_training_entry_point_runs_at_the_benchmark_rate(tmp_path):
    """training() is the path a user runs, bench.py's loop is the path that is timed: at configs[1] (160^3, training()
    defaults) the entry point's own epoch rate must be within 5 % of the bench loop's in the same process (VERDICT r03 weak 4:
    training() used to pay a synchronous 16 MB label upload per step; it now keeps the maps it has used on the device, as
    uint8, like the bench's resident pool)"""
    import time
    import torch
    from synthsr_amd.training import training, Trainer
    from synthsr_amd.brain_generator import BrainGenerator
    from synthsr_amd.unet import unet
    from synthsr_amd.synthetic import (GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR,
                                       synthetic_label_pool)
    S, K = 160, 30
    labels_dir = _write_labels(tmp_path, 4, (S, S, S))
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    np.save(tmp_path / 'gc.npy', GENERATION_CLASSES)
    np.save(tmp_path / 'pm.npy', PRIOR_MEANS_T1_HR)
    np.save(tmp_path / 'ps.npy', PRIOR_STDS_T1_HR)
    model_dir = str(tmp_path / 'models')
    net = training(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                   path_generation_classes=str(tmp_path / 'gc.npy'), epochs=3, steps_per_epoch=K, verbose=False)
    assert net.iterations == 3 * K
    rows = [l.split(',') for l in open(os.path.join(model_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    # epoch 1 pays the first uploads / allocations and every epoch its two checkpoint files (after its clock stops)
    rate_training = K / min(float(r[2]) for r in rows[1:])
    # bench.py's loop: same generator settings, same network, resident pool, K steps between two synchronisations
    pool = synthetic_label_pool(4, (S, S, S), 1234)
    bg = BrainGenerator(None, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR, 'normal', GENERATION_LABELS,
                        generation_classes=GENERATION_CLASSES, n_neutral_labels=19, output_shape=S, output_div_by_n=32,
                        flipping=True, scaling_bounds=.15, rotation_bounds=15, shearing_bounds=.02, translation_bounds=5,
                        nonlin_std=4., nonlin_shape_factor=.03125, randomise_res=False, downsample=True, blur_range=1.15,
                        build_reliability_maps=True, bias_field_std=.3, bias_shape_factor=.03125, label_maps=pool,
                        rng=np.random.Generator(np.random.Philox(key=1000)))
    net2 = unet(24, bg.model_output_shape, 5, 3, 1, feat_mult=2, nb_conv_per_level=2, final_pred_activation='linear',
                batch_norm=-1, activation='elu', seed=0)
    tr = Trainer(bg, net2, lr=1e-4)
    tr.make_labels_resident(pool)
    pick = np.random.default_rng(0)
    for _ in range(5):
        tr.step(label_index=int(pick.integers(len(pool))))
    best = 0.0
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(K):
            tr.step(label_index=int(pick.integers(len(pool))))
        torch.cuda.synchronize()
        best = max(best, K / (time.perf_counter() - t0))
    print('training() %.2f volumes/s, bench loop %.2f volumes/s' % (rate_training, best))
    assert rate_training > 0.95 * best, (rate_training, best)
    assert all(t.dtype == torch.uint8 for t in tr.resident_labels)


def test_bench_gpus_2_launched_plainly_starts_two_ranks():
    """`python bench.py --gpus 2` with no launcher around it (the way the driver starts --gpus 1) must start its own two ranks
    and report them: n_gpus == n_ranks_seen == 2 (RCCL with one GPU per rank when the box has two, gloo on the shared GPU
    otherwise -- recorded in `backend`); value = the two ranks' volumes over the slower rank's wall time"""
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_ADDR', 'MASTER_PORT')}
    cmd = [sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--size', '32',
           '--no-cpu-baseline']
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=REPO, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith('{')][-1])
    assert d['n_gpus'] == 2 and d['n_ranks_seen'] == 2 and d['steps'] == 2 and d['value'] > 0
    assert d['backend'] in ('nccl', 'gloo') and len(d['per_rank']) == 2 and d['config']['global_batch'] == 2
    assert np.isfinite(d['final_loss'])


@pytest.mark.parametrize('case', ['sr', 'synthesis', 'multimodal', 'real'])
def test_generation_examples_script(tmp_path, case):
    """scripts/tutorials/generate_examples.py (the use cases of the reference's tutorials 1-6) end to end on NIfTI files"""
    import importlib.util
    from synthsr_amd.nifti import write_nifti, read_nifti
    from synthsr_amd.synthetic import (GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR,
                                       synthetic_label_map)
    labels_dir = _write_labels(tmp_path, 2, (64, 64, 64))
    pri = tmp_path / 'priors'
    pri.mkdir()
    np.save(pri / 'generation_labels.npy', GENERATION_LABELS)
    np.save(pri / 'generation_classes.npy', GENERATION_CLASSES)
    for c in ('t1_hr', 't1_lr', 't2'):
        np.save(pri / ('prior_means_%s.npy' % c), PRIOR_MEANS_T1_HR)
        np.save(pri / ('prior_stds_%s.npy' % c), PRIOR_STDS_T1_HR)
    argv = [case, '--labels', labels_dir, '--priors', str(pri), '--out', str(tmp_path / 'out'), '-n', '2', '--shape', '32']
    if case == 'real':
        img = tmp_path / 'images'
        img.mkdir()
        for i in range(2):
            lab = synthetic_label_map((64, 64, 64), 10 + i)
            write_nifti(str(img / ('brain%d.nii.gz' % i)), (10.0 * (lab % 17) + 5).astype(np.float32))
        argv += ['--images', str(img)]
    spec = importlib.util.spec_from_file_location('gen_examples', os.path.join(REPO, 'scripts', 'tutorials',
                                                                              'generate_examples.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.main(argv)
    n_in = {'sr': 2, 'synthesis': 1, 'multimodal': 4, 'real': 2}[case]      # input channels (+ reliability maps)
    for i in range(2):
        im, _, _ = read_nifti(str(tmp_path / 'out' / ('image_%d.nii.gz' % i)))
        tg, _, _ = read_nifti(str(tmp_path / 'out' / ('target_%d.nii.gz' % i)))
        assert im.shape[:3] == (32, 32, 32) and (im.shape[3] if im.ndim == 4 else 1) == n_in and tg.shape == (32, 32, 32)
        assert np.isfinite(im).all() and np.isfinite(tg).all() and tg.max() > 0


def test_label_pool_respects_its_budget_and_falls_back_to_per_step_copies():
    """Trainer.step() keeps the label maps it has used on the device (synthsr_amd/training.py: _pooled_labels): the pool's budget is
    derived from the free device memory (and POOL_BYTES), checked on the host array before anything is uploaded; a full pool
    stops growing and the remaining maps go through the per-step host path -- same training, no second upload."""
    import torch
    from synthsr_amd.brain_generator import BrainGenerator
    from synthsr_amd.training import Trainer
    from synthsr_amd.unet import unet
    from synthsr_amd.synthetic import (synthetic_label_pool, GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR,
                                       PRIOR_STDS_T1_HR)

    def losses(pool_bytes):
        pool = synthetic_label_pool(4, (32, 32, 32), 5)
        bg = BrainGenerator(None, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR, 'normal', GENERATION_LABELS,
                            generation_classes=GENERATION_CLASSES, output_shape=32, output_div_by_n=8, nonlin_std=4.,
                            nonlin_shape_factor=.125, bias_shape_factor=.125, build_reliability_maps=True, downsample=True,
                            shearing_bounds=.02, label_maps=pool, rng=np.random.default_rng(0))
        net = unet(24, bg.model_output_shape, 3, 3, 1, feat_mult=2, nb_conv_per_level=2, final_pred_activation='linear',
                   batch_norm=-1, seed=1)
        tr = Trainer(bg, net, lr=1e-3)
        bg.labels_to_image_model.seed(3, 0)
        if pool_bytes is not None:
            tr.POOL_BYTES = pool_bytes
        from synthsr_amd import ops
        prev = ops.set_deterministic(True)   # bit-identical steps: the three runs can be compared with ==
        try:
            out = [tr.step().item() for _ in range(12)]
        finally:
            ops.set_deterministic(prev)
        return tr, out

    tr, full = losses(None)
    assert 1 < len(tr._auto_pool) <= 4 and not tr.__dict__.get('_auto_pool_full')
    free, _ = torch.cuda.mem_get_info()
    assert tr._auto_pool_cap <= tr.POOL_FRACTION * free * 1.5 and tr._auto_pool_used == sum(t.numel() * t.element_size() for t in tr._auto_pool.values())
    tr1, capped = losses(32 ** 3)            # room for ONE uint8 map
    assert len(tr1._auto_pool) == 1 and tr1._auto_pool_full and tr1._auto_pool_used == 32 ** 3
    assert capped == full                     # the host path and the device-resident path feed the generator the same maps
    tr0, none = losses(0)
    assert len(tr0._auto_pool) == 0 and none == full
