"""Linear U-Net heads with up to 16 output channels (training(output_channel=[...]) with five or more l1 / l2 targets, or
three or more laplace targets with a spread map each: SynthSR/training.py:246-249, 325-341): the layer table, no GPU."""
import pytest


def _net(K, act='linear'):
    from synthsr_amd.unet import UNet3D
    return UNet3D(24, [16, 16, 16, 2], 3, 3, K, feat_mult=2, nb_conv_per_level=2, batch_norm=-1, activation='elu',
                  final_pred_activation=act, table_only=True)


@pytest.mark.parametrize('K', [5, 6, 8, 16])
def test_wide_linear_head_builds(K):
    net = _net(K)
    shapes = {nm: tuple(shp) for nm, shp, _ in net.specs}
    C = net.head['cin']
    assert C == 24 and net.nb_labels == K
    assert shapes['unet_likelihood/kernel'] == (C, K) and shapes['unet_likelihood/bias'] == (K,)


@pytest.mark.parametrize('K', [0, 17])
def test_linear_head_width_outside_1_to_16_is_refused(K):
    with pytest.raises(NotImplementedError):
        _net(K)


def test_softmax_head_with_five_labels_builds_as_before():
    net = _net(5, 'softmax')
    shapes = {nm: tuple(shp) for nm, shp, _ in net.specs}
    assert net.final_pred_activation == 'softmax' and shapes['unet_likelihood/kernel'] == (24, 5)
