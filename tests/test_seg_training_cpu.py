"""Host side of training_segmentation() (no GPU): the label lookup table, the scope limits and the parameter table of
softmax-headed networks."""
import numpy as np
import pytest


def test_segmentation_lut_from_a_label_list(tmp_path):
    from synthsr_amd.segmentation_training import segmentation_lut
    labels = np.array([0, 14, 2, 41, 1024, 17, 3])      # non-contiguous FreeSurfer values, in head-channel order
    lut = segmentation_lut(labels)
    assert lut.dtype == np.int32 and lut.shape == (1025,)
    for k, v in enumerate(labels):
        assert lut[v] == k
    assert lut[4] == -1 and lut[42] == -1 and lut[1023] == -1           # labels absent from the list have no class
    assert int((lut >= 0).sum()) == len(labels)
    np.save(tmp_path / 'sl.npy', labels)
    assert np.array_equal(segmentation_lut(str(tmp_path / 'sl.npy')), lut)
    assert np.array_equal(segmentation_lut(labels.astype(np.float64)), lut)
    for bad in ([0, 2, 2], [0, -1, 3], [0, 2.5], [7]):
        with pytest.raises(ValueError):
            segmentation_lut(np.array(bad))


@pytest.mark.parametrize('kw,exc,msg', [
    (dict(dtype='bf16'), NotImplementedError, 'fp32 only'),
    (dict(batchsize=2), NotImplementedError, 'batchsize=1'),
    (dict(images_dir='/nowhere'), NotImplementedError, 'images_dir is not supported'),
    (dict(fs_header_segnet=True), NotImplementedError, 'fs_header_segnet is not supported'),
    (dict(output_channel=[0, 1], input_channels=[True, True]), ValueError, 'ONE output_channel'),
    (dict(output_channel=None), ValueError, 'ONE output_channel'),
])
def test_scope_limits_raise_with_their_message(kw, exc, msg):
    """every follow-up is refused before anything is read or built"""
    from synthsr_amd.segmentation_training import training_segmentation
    with pytest.raises(exc, match=msg):
        training_segmentation('/nowhere/labels', '/nowhere/models', None, None, None, np.array([0, 2, 3]), **kw)


def test_multi_rank_runs_are_refused(monkeypatch):
    from synthsr_amd.segmentation_training import training_segmentation
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(NotImplementedError, match='one process'):
        training_segmentation('/nowhere/labels', '/nowhere/models', None, None, None, np.array([0, 2, 3]))


def test_softmax_nets_keep_their_parameter_table():
    """table_only softmax nets: the layer table of the frozen segmentation network, name by name (a trained file must keep
    loading into it); loss_dice() is refused on a linear head"""
    from synthsr_amd.unet import UNet3D
    kw = dict(feat_mult=2, nb_conv_per_level=2, batch_norm=-1, table_only=True)
    net = UNet3D(24, [16, 16, 16, 1], 3, 3, 5, final_pred_activation='softmax', **kw)
    want = []
    cin = 1
    for l, f in enumerate([24, 48, 96]):
        for k in range(2):
            want += [('unet_conv_downarm_%d_%d/kernel' % (l, k), (3, 3, 3, cin, f)), ('unet_conv_downarm_%d_%d/bias' % (l, k), (f,))]
            cin = f
        want += [('unet_bn_down_%d/beta' % l, (f,)), ('unet_bn_down_%d/gamma' % l, (f,))]
    for k, f in enumerate([48, 24]):
        cin = f + cin
        for j in range(2):
            want += [('unet_conv_uparm_%d_%d/kernel' % (3 + k, j), (3, 3, 3, cin, f)), ('unet_conv_uparm_%d_%d/bias' % (3 + k, j), (f,))]
            cin = f
        want += [('unet_bn_up_%d/beta' % k, (f,)), ('unet_bn_up_%d/gamma' % k, (f,))]
    want += [('unet_likelihood/kernel', (24, 5)), ('unet_likelihood/bias', (5,))]
    assert [(nm, tuple(shp)) for nm, shp, _ in net.specs] == want
    assert net.n_params == sum(int(np.prod(s)) for _, s in want)
    lin = UNet3D(24, [16, 16, 16, 1], 3, 3, 5, final_pred_activation='linear', **kw)
    assert [(nm, tuple(shp)) for nm, shp, _ in lin.specs] == want     # the head's activation adds no parameter
    with pytest.raises(ValueError, match='softmax'):
        lin.loss_dice(None, None, None)
