"""activation='relu' (SynthSR/training.py:209 'Can be elu, relu'): host-side checks, no GPU"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(activation):
    from synthsr_amd.unet import UNet3D
    net = UNet3D(24, [32, 32, 32, 2], 3, 3, 1, feat_mult=2, nb_conv_per_level=2, batch_norm=-1, activation=activation,
                 final_pred_activation='linear', table_only=True)
    return net


def test_relu_network_builds_with_the_elu_parameter_table():
    elu, relu = _table('elu'), _table('relu')
    assert relu.specs == elu.specs and relu.n_params == elu.n_params
    assert (relu._act, relu._act_dgrad) == (3, 4) and (elu._act, elu._act_dgrad) == (1, 2)


def test_other_activations_still_raise():
    with pytest.raises(NotImplementedError, match="'elu' or 'relu'"):
        _table('tanh')


def test_training_cli_builds_a_relu_network(monkeypatch):
    """scripts/training.py run as a program with --activation relu: its own call of training() receives 'relu', and the
    U-Net layer table that value builds (training() itself needs a GPU; its first step is the network constructor)"""
    import runpy
    import synthsr_amd.training as T
    seen = {}

    def fake_training(**kw):
        seen.update(kw)
        seen['net'] = _table(kw['activation'])

    monkeypatch.setattr(T, 'training', fake_training)
    monkeypatch.setattr(sys, 'argv', ['training.py', 'labels', 'model', 'm.npy', 's.npy', 'gl.npy', '--activation', 'relu'])
    runpy.run_path(os.path.join(ROOT, 'scripts', 'training.py'), run_name='__main__')
    assert seen['activation'] == 'relu' and seen['net'].activation == 'relu' and seen['net']._act == 3


def test_activation_generic_backward_entry_points_are_declared():
    from synthsr_amd import _lib
    for fam in ('act_bwd', 'bn_act_bwd', 'bn_act_bwd_head', 'act_bwd_drop', 'bn_pool_act_bwd'):
        assert 'synthsr_' + fam in _lib.SIGNATURES and 'synthsr_' + fam + '_bf16' in _lib.SIGNATURES
    with open(os.path.join(ROOT, 'include', 'synthsr_hip.h')) as f:
        header = f.read()
    assert '3 ReLU' in header and 'x ReLU\'(addend)' in header
