"""Linear heads with 5 to 16 output channels (csrc/unet_pointwise.hip: head_loss_fwd_wide_kernel / head_multi_bwd_wide_kernel,
two padded widths 8 and 16 with the real width at run time), from the kernels up to training() and the adversarial schedule.

Tolerances of the kernel tests are those of tests/test_unet_gpu.py::test_head_regression_losses_vs_autograd (the same
mathematics, sums of the same lengths or shorter): 2e-5 relative for pred, the loss and dbn; for dw and db 2e-5 of
max(|ref|max, 1e-2).  The reference is float64 autograd on `bn @ w + b` and oracle.unet_ref.regression_loss."""
import functools
import os

import numpy as np
import pytest

from conftest import single_shot_parity

pytestmark = pytest.mark.gpu

SHAPE = (5, 7, 9)            # 315 voxels: one full 256-voxel pass of the forward kernel plus a partial one
CROP = (3, 5, 4)
RES_STRIDE_EXTRA = 3
ROWS = [(5, 'l1'), (6, 'laplace'), (7, 'l2'), (8, 'laplace'), (9, 'l1'), (12, 'laplace'), (16, 'l2'), (16, 'laplace')]
GUARD, SENTINEL = 64, -12345.5


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def close(a, b, rel, name=''):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    scale = max(b.abs().max().item(), 1e-30)
    err = (a - b).abs().max().item() / scale
    print('%s: max err %.3e of scale %.3e' % (name, err, scale))
    assert err < rel, '%s: max rel err %.3e (scale %.3e)' % (name, err, scale)


def _res_channels(n):
    """a different, non-monotone residual channel per target out of n + 3"""
    return [(5 * k + 2) % (n + RES_STRIDE_EXTRA) for k in range(n)] if n > 1 else [2]


@functools.lru_cache(maxsize=None)
def _case(C, K, kind, cropped, with_res, bf16=False):
    """inputs (float32, host) and the float64 reference of one head configuration; computed once, never modified"""
    import torch
    from synthsr_amd import ops
    from oracle import unet_ref as U
    n = K // 2 if kind == 'laplace' else K
    g = torch.Generator().manual_seed(1000 * C + 10 * K + len(kind))
    x = torch.randn(*SHAPE, C, generator=g)
    if bf16:
        x = x.bfloat16().float()
    mean, var = torch.randn(C, generator=g) * .1, torch.rand(C, generator=g) + .5
    gamma, beta = torch.rand(C, generator=g) + .5, torch.randn(C, generator=g) * .1
    w = torch.randn(C, K, generator=g) * .2
    b = torch.randn(K, generator=g) * .1
    target = torch.rand(*SHAPE, n, generator=g)
    rs = n + RES_STRIDE_EXTRA
    image = torch.rand(*SHAPE, rs, generator=g)
    res_ch = _res_channels(n)
    d = lambda t: t.double()
    w64, b64 = d(w).requires_grad_(True), d(b).requires_grad_(True)
    bn = ((d(x) - d(mean)) * torch.rsqrt(d(var) + ops.BN_EPS) * d(gamma) + d(beta)).requires_grad_(True)
    pred_ref = bn @ w64 + b64
    res = d(image)[..., res_ch] if with_res else None
    loss_ref = U.regression_loss(pred_ref, d(target), kind, CROP if cropped else None, res)
    loss_ref.backward()
    expect = pred_ref.detach().clone()
    if with_res:
        expect[..., :n] += res
    return dict(C=C, K=K, n=n, kind=kind, x=x, stats=torch.cat([mean, var]), gamma=gamma, beta=beta, w=w, b=b, target=target,
                image=image, rs=rs, res_ch=res_ch, with_res=with_res,
                box=([int((s - c) / 2) for s, c in zip(SHAPE, CROP)], list(CROP)) if cropped else None,
                pred=expect, loss=float(loss_ref), dbn=bn.grad.clone(), dw=w64.grad.clone(), db=b64.grad.clone())


def _guarded(torch, numel, misalign=False):
    """a device buffer of `numel` floats with GUARD sentinel floats behind it (and one in front when misaligned)"""
    full = torch.full((numel + GUARD + 1,), SENTINEL, device='cuda')
    o = 1 if misalign else 0
    return full, full[o:o + numel]


def _run(torch, c, act_dtype=None, misalign=False):
    """forward + backward head kernels of one case; returns (pred, dpred, loss, dbn, dw, db) and checks the guards"""
    from synthsr_amd import ops
    C, K, n = c['C'], c['K'], c['n']
    nvox = int(np.prod(SHAPE))
    xd = c['x'].cuda() if act_dtype is None else c['x'].cuda().to(act_dtype)
    dev = lambda k: c[k].cuda()
    loss = torch.zeros(1, device='cuda')
    pfull, pred = _guarded(torch, nvox * K, misalign)
    dfull, dpred = _guarded(torch, nvox * K, misalign)
    ops.head_loss_fwd(xd, dev('stats'), dev('gamma'), dev('beta'), dev('w'), dev('b'), c['target'].reshape(-1).cuda(), loss,
                      kind=c['kind'], crop=c['box'], pred=pred, dpred=dpred, residual=dev('image') if c['with_res'] else None,
                      res_stride=c['rs'], res_off=c['res_ch'] if n > 1 else c['res_ch'][0])
    dw, db = torch.zeros(C, K, device='cuda'), torch.zeros(K, device='cuda')
    dbn = torch.empty_like(xd)
    if K == 1:
        ops.head_bwd(dpred, xd, dev('stats'), dev('gamma'), dev('beta'), dev('w').view(-1), dbn, dw.view(-1), db)
    else:
        ops.head_bwd_multi(dpred, xd, dev('stats'), dev('gamma'), dev('beta'), dev('w'), dbn, dw, db)
    torch.cuda.synchronize()
    o = 1 if misalign else 0
    for nm, full in (('pred', pfull), ('dpred', dfull)):   # the padded lanes k >= K store nothing
        assert bool((full[o + nvox * K:] == SENTINEL).all()) and bool((full[:o] == SENTINEL).all()), nm + ' guard overwritten'
    return pred, dpred, loss, dbn, dw, db


def _check_sums(dw, db, c):
    for got, ref, nm in ((dw, c['dw'], 'dw'), (db, c['db'], 'db')):   # sums of +-1/N can cancel to ~0: absolute floor
        err = (got.cpu().double() - ref).abs().max().item()
        bound = 2e-5 * max(ref.abs().max().item(), 1e-2)
        print('%s: abs err %.3e, bound %.3e' % (nm, err, bound))
        assert err < bound, '%s abs err %.3e (bound %.3e)' % (nm, err, bound)


def _check_outside_box_is_zero(dpred, c):
    if c['box'] is not None:
        d = dpred.view(*SHAPE, c['K']).clone()
        lo, sz = c['box']
        d[lo[0]:lo[0] + sz[0], lo[1]:lo[1] + sz[1], lo[2]:lo[2] + sz[2]] = 0
        assert not d.any()


@pytest.mark.parametrize('with_res', [False, True])
@pytest.mark.parametrize('cropped', [False, True])
@pytest.mark.parametrize('K,kind', ROWS)
@pytest.mark.parametrize('C', [4, 20, 24])
def test_wide_head_kernels_vs_autograd(T, C, K, kind, cropped, with_res):
    """both padded widths and their edges (5, 8, 9, 16), odd K, one channel quad (C = 4), the LDS-atomic branch of the backward
    kernel (C = 20: 384 % 5 != 0) and its register branch (C = 24); cropped cases with residuals run on buffers that are not
    16-byte aligned (scalar stores also where K % 4 == 0)"""
    torch = T
    c = _case(C, K, kind, cropped, with_res)
    pred, dpred, loss, dbn, dw, db = _run(torch, c, misalign=cropped and with_res)
    close(pred.view(*SHAPE, K), c['pred'], 2e-5, 'pred')
    print('loss %.9g ref %.9g' % (loss.item(), c['loss']))
    assert abs(loss.item() - c['loss']) < 2e-5 * abs(c['loss'])
    close(dbn, c['dbn'], 2e-5, 'dbn')
    _check_sums(dw, db, c)
    _check_outside_box_is_zero(dpred, c)


@pytest.mark.parametrize('K,kind', [(6, 'laplace'), (16, 'l2'), (16, 'laplace')])
def test_wide_head_kernels_bf16_activations(T, K, kind):
    """the bf16 instantiations: x is bfloat16 (the reference reads the same rounded values in float64), everything the head
    produces but dbn is float32 and keeps the fp32 bounds; dbn is stored as bfloat16: within one bf16 ulp of the reference"""
    torch = T
    c = _case(24, K, kind, True, True, bf16=True)
    pred, dpred, loss, dbn, dw, db = _run(torch, c, act_dtype=torch.bfloat16)
    close(pred.view(*SHAPE, K), c['pred'], 2e-5, 'pred')
    assert abs(loss.item() - c['loss']) < 2e-5 * abs(c['loss'])
    _check_sums(dw, db, c)
    _check_outside_box_is_zero(dpred, c)
    assert dbn.dtype == torch.bfloat16
    ref = c['dbn']
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(1e-30))) - 7)   # bf16: 8 significant bits
    err = (dbn.cpu().double() - ref).abs()
    print('dbn: worst %.3f bf16 ulp' % float((err / ulp)[ref != 0].max()))
    assert bool((err <= ulp).all())


def test_heads_wider_than_16_are_refused(T):
    torch = T
    from synthsr_amd import ops, _lib
    C, nvox = 24, int(np.prod(SHAPE))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(*SHAPE, C, generator=g).cuda()
    stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()

    def bufs(K):
        return (torch.randn(C, K, generator=g).cuda(), torch.zeros(K).cuda(), torch.rand(nvox * K, generator=g).cuda(),
                torch.full((1,), SENTINEL, device='cuda'), torch.full((nvox * K,), SENTINEL, device='cuda'),
                torch.full((nvox * K,), SENTINEL, device='cuda'))

    w, b, target, loss, pred, dpred = bufs(17)
    with pytest.raises(ValueError):
        ops.head_loss_fwd(x, stats, gamma, beta, w, b, target, loss, pred=pred, dpred=dpred)
    with pytest.raises(ValueError):
        ops.head_bwd_multi(dpred, x, stats, gamma, beta, w, torch.empty_like(x), torch.zeros(C, 17).cuda(), torch.zeros(17).cuda())
    lib = _lib.load()
    shape = _lib.I3(*SHAPE)
    for K in (17, 0):
        rc = lib.synthsr_head_loss_fwd(_lib.ptr(x), shape, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), ops.BN_EPS,
                                       _lib.ptr(w), _lib.ptr(b), K, None, 1, None, _lib.ptr(target), _lib.ptr(pred),
                                       _lib.ptr(dpred), _lib.ptr(loss), 0, None, _lib.stream())
        assert rc == -1   # SYNTHSR_EINVAL
    dbn, dw, db = torch.full_like(x, SENTINEL), torch.full((C, 17), SENTINEL).cuda(), torch.full((17,), SENTINEL).cuda()
    rc = lib.synthsr_head_bwd_multi(_lib.ptr(dpred), _lib.ptr(x), nvox, C, 17, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                    ops.BN_EPS, _lib.ptr(w), _lib.ptr(dbn), _lib.ptr(dw), _lib.ptr(db), _lib.stream())
    assert rc == -1
    torch.cuda.synchronize()
    for t in (loss, pred, dpred, dbn, dw, db):   # nothing was launched
        assert bool((t == SENTINEL).all())
    # laplace needs an even number of channels, at the new widths as at the old ones
    w, b, target, loss, pred, dpred = bufs(7)
    with pytest.raises(ValueError):
        ops.head_loss_fwd(x, stats, gamma, beta, w, b, target[:nvox * 3].contiguous(), loss, kind='laplace', pred=pred, dpred=dpred)
    rc = lib.synthsr_head_loss_fwd(_lib.ptr(x), shape, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), ops.BN_EPS,
                                   _lib.ptr(w), _lib.ptr(b), 7, None, 1, None, _lib.ptr(target), _lib.ptr(pred),
                                   _lib.ptr(dpred), _lib.ptr(loss), 2, None, _lib.stream())
    assert rc == -1
    # a last feature map too wide for the kernel's LDS tile is refused before the launch (include/synthsr_hip.h: C <= 48)
    C2 = 52
    x2 = torch.randn(*SHAPE, C2, generator=g).cuda()
    st2 = torch.cat([torch.zeros(C2), torch.ones(C2)]).cuda()
    w2 = torch.randn(C2, 8, generator=g).cuda()
    loss2 = torch.full((1,), SENTINEL, device='cuda')
    rc = lib.synthsr_head_loss_fwd(_lib.ptr(x2), shape, C2, _lib.ptr(st2), _lib.ptr(torch.ones(C2).cuda()),
                                   _lib.ptr(torch.zeros(C2).cuda()), ops.BN_EPS, _lib.ptr(w2), _lib.ptr(torch.zeros(8).cuda()), 8,
                                   None, 1, None, _lib.ptr(torch.rand(nvox * 8, generator=g).cuda()), None, None, _lib.ptr(loss2),
                                   0, None, _lib.stream())
    torch.cuda.synchronize()
    assert rc == -1 and float(loss2) == SENTINEL


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32).copy()


@pytest.mark.parametrize('K,kind', [(1, 'l1'), (2, 'laplace'), (4, 'l2'), (16, 'laplace'), (16, 'l2')])
def test_head_kernels_repeat_bit_for_bit_in_deterministic_mode(T, K, kind):
    """heads of up to four channels keep their own kernels (the launchers' switch sends only K >= 5 to the padded ones): the same
    call twice in deterministic mode gives the same bits in every output; so does the widest padded head (K = 16, C = 24)"""
    torch = T
    from synthsr_amd import ops
    c = _case(24, K, kind, True, True)
    prev = ops.set_deterministic(True)
    try:
        a = [_bits(t) for t in _run(torch, c)]
        b = [_bits(t) for t in _run(torch, c)]
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
    finally:
        ops.set_deterministic(prev)
    for nm, u, v in zip(('pred', 'dpred', 'loss', 'dbn', 'dw', 'db'), a, b):
        assert np.array_equal(u, v), nm + ' differs between two deterministic runs'
    if K <= 4:   # ... and they still compute what they did (the bounds of the wide heads)
        pred, dpred, loss, dbn, dw, db = _run(torch, c)
        close(pred.view(*SHAPE, K), c['pred'], 2e-5, 'pred')
        assert abs(loss.item() - c['loss']) < 2e-5 * abs(c['loss'])
        close(dbn, c['dbn'], 2e-5, 'dbn')
        _check_sums(dw, db, c)


def _randomise(net, torch, g):
    for nm, v in net.named_parameters():
        if nm.endswith('/gamma'):
            v.copy_(torch.rand(v.shape, generator=g) + .5)
        elif nm.endswith('/beta') or nm.endswith('/bias'):
            v.copy_(torch.randn(v.shape, generator=g) * .1)
    net.repack()


@pytest.mark.parametrize('K,kind,crop', [(6, 'laplace', None), (5, 'l1', (8, 8, 16))])
def test_unet_with_wide_head_gradients_vs_autograd(T, K, kind, crop):
    """whole network with a 6-channel laplace head (three targets) and a 5-channel l1 head under loss_cropping, one residual
    channel per target, against the oracle (conftest.single_shot_parity, as tests/test_unet_gpu.py::
    test_unet_other_losses_gradients_vs_autograd)"""
    torch = T
    from synthsr_amd.unet import unet
    from oracle import unet_ref as U
    shape, cin, levels = (16, 16, 32), 2, 3
    n = K // 2 if kind == 'laplace' else K
    res_ch = [1, 0, 1, 1, 0][:n]
    g = torch.Generator().manual_seed(12)
    tensors = {}

    def run():
        net = unet(nb_features=24, input_shape=list(shape) + [cin], nb_levels=levels, conv_size=3, nb_labels=K, feat_mult=2,
                   nb_conv_per_level=2, final_pred_activation='linear', batch_norm=-1, activation='elu', seed=5)
        g.manual_seed(12)
        _randomise(net, torch, g)
        x = torch.rand(*shape, cin, generator=g)
        target = torch.rand(*shape, n, generator=g)
        loss, pred = net.loss(x.cuda(), target.reshape(-1).cuda(), kind, crop, residual=x.cuda(), res_stride=cin, res_off=res_ch,
                              want_pred=True)
        net.test_loss, net.test_pred = loss.clone(), pred.clone()
        net.backward()
        tensors.update(x=x, target=target)
        return net

    def oracle(net, nudge):
        P = {nm: v.detach().cpu().clone().requires_grad_(True) for nm, v in net.named_parameters()}
        pin = []
        pr = U.unet_forward(tensors['x'], P, net.prefix, levels, 2, training=True, pool_inputs=pin, pool_nudge=nudge)
        lr = U.regression_loss(pr, tensors['target'], kind, crop, tensors['x'][..., res_ch])
        lr.backward()
        return (P, pr.detach(), lr.detach()), pin

    def compare(net, ref):
        _, pr, lr = ref
        expect = pr.clone()
        expect[..., :n] += tensors['x'][..., res_ch]
        close(net.test_pred.view(*shape, K), expect, 5e-4, 'prediction')
        assert abs(net.test_loss.item() - lr.item()) < 5e-5 * max(1.0, abs(lr.item()))
        # (every parameter gradient: the float64-anchored rule of conftest.single_shot_parity)

    net, _ = single_shot_parity(run, oracle, compare, loss_of=lambda n_: n_.test_loss)
    x, target = tensors['x'], tensors['target']
    net.update_moving_stats()
    out = net.predict(x.cuda())
    assert torch.isfinite(out).all() and list(out.shape) == list(shape) + [K]
    with pytest.raises(ValueError):   # a loss kind that does not fit the head: 6 channels are 3 laplace targets, 5 are 5 l1 targets
        net.loss(x.cuda(), target.reshape(-1).cuda(), 'l1' if kind == 'laplace' else 'laplace')


def test_unet_bf16_with_wide_head_vs_bf16_storage_oracle(T):
    """one step of the bf16 network with a 6-channel laplace head against the oracle with the bf16 storage roundings restated
    (oracle.unet_ref.round_bf16), with the bounds tests/test_bf16_gpu.py::test_unet_bf16_step_vs_oracle states for that
    comparison on this shape: prediction 2.5e-2 of range, loss 3e-3, every gradient cosine > 0.997 and within 8 % of range"""
    torch = T
    from synthsr_amd.unet import unet
    from oracle import unet_ref as U
    shape, cin, levels, K, n = (16, 16, 32), 2, 3, 6, 3
    net = unet(nb_features=24, input_shape=list(shape) + [cin], nb_levels=levels, conv_size=3, nb_labels=K, feat_mult=2,
               nb_conv_per_level=2, final_pred_activation='linear', batch_norm=-1, activation='elu', seed=3, dtype='bf16',
               fold_upsample=False)
    g = torch.Generator().manual_seed(11)
    _randomise(net, torch, g)
    x = torch.rand(*shape, cin, generator=g)
    target = torch.rand(*shape, n, generator=g)
    loss, pred = net.loss(x.cuda(), target.reshape(-1).cuda(), 'laplace', want_pred=True)
    pred = pred.clone()
    net.backward()
    assert net.saved['enc'][0][0].dtype == torch.bfloat16 and net.grads.dtype == torch.float32 and pred.dtype == torch.float32
    P = {nm: v.detach().cpu().clone().requires_grad_(True) for nm, v in net.named_parameters()}
    pr = U.unet_forward(x, P, net.prefix, levels, 2, training=True, quant=U.round_bf16)
    lr = U.regression_loss(pr, target, 'laplace')
    lr.backward()
    close(pred.view(*shape, K), pr, 2.5e-2, 'prediction')
    print('loss %.6f oracle %.6f' % (loss.item(), lr.item()))
    assert abs(loss.item() - lr.item()) < 3e-3 * abs(lr.item())
    for nm, _, _ in net.specs:
        got = net.view(nm, net.grads).cpu().double().reshape(-1)
        ref = P[nm].grad.double().reshape(-1)
        cos = float(torch.dot(got, ref) / (got.norm() * ref.norm()).clamp_min(1e-30))
        err = float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
        print('%s: err %.3e cos %.5f' % (nm, err, cos))
        assert cos > 0.997 and err < 8e-2, 'gradient of %s: err %.3e cos %.5f' % (nm, err, cos)
    net.update_moving_stats()
    out = net.predict(x.cuda())
    assert torch.isfinite(out).all() and list(out.shape) == list(shape) + [K] and out.dtype == torch.float32


def _write_inputs(tmp_path, n_channels):
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import (synthetic_label_map, GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR,
                                       PRIOR_STDS_T1_HR)
    d = tmp_path / 'labels'
    d.mkdir()
    write_nifti(str(d / 'brain0_labels.nii.gz'), synthetic_label_map((40, 36, 48), 10).astype(np.float32))
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    np.save(tmp_path / 'gc.npy', GENERATION_CLASSES)
    np.save(tmp_path / 'pm.npy', np.concatenate([PRIOR_MEANS_T1_HR[:, ::(-1 if i % 2 else 1)] for i in range(n_channels)]))
    np.save(tmp_path / 'ps.npy', np.concatenate([PRIOR_STDS_T1_HR] * n_channels))
    return str(d)


def test_training_three_laplace_targets(tmp_path):
    """training(output_channel=[0, 1, 2], regression_metric='laplace'): T1, T2 and FLAIR-like channels with a spread map each,
    a 6-channel head"""
    from synthsr_amd.training import training
    labels_dir = _write_inputs(tmp_path, 3)
    model_dir = str(tmp_path / 'models')
    net = training(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                   path_generation_classes=str(tmp_path / 'gc.npy'), input_channels=[True, True, True], output_channel=[0, 1, 2],
                   regression_metric='laplace', build_reliability_maps=False, output_shape=32, n_levels=3, unet_feat_count=24,
                   nonlin_shape_factor=.125, bias_shape_factor=.125, steps_per_epoch=4, epochs=1, verbose=False, lr=1e-3)
    assert net.nb_labels == 6 and net.input_shape[3] == 3 and net.iterations == 4
    log = [float(l.split(',')[1]) for l in open(os.path.join(model_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 1 and np.isfinite(log[0])
    z = np.load(os.path.join(model_dir, '001.npz'))
    assert z['unet_likelihood/kernel'].shape[-1] == 6


def test_adversarial_schedule_with_five_targets(tmp_path):
    """fine_tuning_with_adversary.training(output_channel=[0, 1, 2, 3, 4]): one critic and one generator update with a 5-channel
    head and a critic that reads the five predicted channels"""
    from synthsr_amd.fine_tuning_with_adversary import training
    labels_dir = _write_inputs(tmp_path, 5)
    gen, critic = training(labels_dir, None, str(tmp_path / 'models'), str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'),
                           str(tmp_path / 'gl.npy'), path_generation_classes=str(tmp_path / 'gc.npy'),
                           input_channels=[True, False, False, False, False], output_channel=[0, 1, 2, 3, 4], output_shape=32,
                           n_levels=3, nonlin_shape_factor=.125, bias_shape_factor=.125, epochs=1, steps_per_epoch=1,
                           first_training_ratio=1, training_ratio=1, verbose=False)
    assert gen.nb_labels == 5 and gen.iterations == 1 and critic.iterations == 1
    mdir = str(tmp_path / 'models')
    d, g = np.load(os.path.join(mdir, 'logs', 'discriminator_loss.npy')), np.load(os.path.join(mdir, 'logs', 'generator_loss.npy'))
    assert np.isfinite(d).all() and np.isfinite(g).all()
