"""The weighted-L2 warm-up and the cross-entropy of the segmentation U-Net on the GPU: the two head kernels alone
(csrc/unet_pointwise.hip: seg_head_logit_loss_fwd_kernel / seg_head_logit_loss_bwd_kernel, both kinds), their limits, deterministic
mode, UNet3D.loss_wl2 / loss_cross_entropy + backward() on a whole network, the two loss records of a network, and
training_segmentation() with the new keywords end to end.

The reference of the kernel tests is float64 autograd on the logits bn @ w + b with the formulas of tests/test_seg_losses_cpu.py
(WeightedL2Loss.call, ext/lab2im/layers.py:1408-1412; CrossEntropyLoss.call, :1498-1526), which that file checks against the
reference's own layers; whole networks go through oracle.unet_ref.unet_forward(..., softmax=False, training=True) under
conftest.single_shot_parity.  Shapes, label maps (`_case`: values outside the table, values mapped to -1, an empty class, a
single voxel of class 0 -- the one that carries the 1e-8 weight), sentinels and the small network are those of
tests/test_seg_training_gpu.py.

Tolerances of the kernel tests are the project's bounds for this mathematics (tests/test_seg_training_gpu.py): 2e-5 relative
for the loss and dbn (of max|ref|); 2e-5 of max(|ref|max, 1e-2) for dw and db.  Every test prints the device's distance from
float64 next to that of the same graph evaluated in float32 by torch on the CPU.
Measured on an MI355X over the twenty kernel cases (device / fp32 CPU, absolute, the largest over the cases):
loss <= 2.1e-6 / 2.1e-6 on a scale of 27 (at most 8e-8 relative), dbn <= 2.2e-9 / 2.7e-9 (at most 5e-7 of max|ref|),
dw <= 7.0e-7 / 9.7e-7, db <= 3.0e-7 / 3.9e-7: the device is as close to float64 as the fp32 CPU graph, the bounds hold with a
factor of 18 or more to spare, and the fp32 CPU graph exceeds none of them, so no quantity takes the anchored rule."""
import functools
import os

import numpy as np
import pytest

from conftest import single_shot_parity
from test_seg_losses_cpu import wl2_loss, ce_loss
from test_seg_training_gpu import (SHAPE, BIG, GUARD, SENTINEL, CASES, NET_SHAPE, LEVELS, N_SEG, _case, _guarded, _dist, _bits,
                                   _seg_net, _net_inputs, _write_inputs)

pytestmark = pytest.mark.gpu

FAR = (17, 64, 64)           # 69 632 voxels = 1088 tiles, more than the 1024 workgroups of head_grid(): 64 of them take a second tile
KINDS = ('wl2', 'ce')
TARGET_VALUE = 5.
# the nine cases of the soft-Dice kernels (every C of {8, 24, 64}, every N of {2, 5, 19, 33, 64}, C = 24 with N = 33 on SHAPE
# and BIG; misaligned outputs in three of them) and C = 24, N = 33 on FAR
LOSS_CASES = CASES + [(24, 33, FAR, False)]


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _logit_graph(c, kind, dtype):
    """loss(bn @ w + b) of one case in `dtype` under autograd: (loss, dbn, dw, db)"""
    import torch
    from synthsr_amd import ops
    d = lambda t: t.detach().to(dtype)   # (detached: the shared case stays as it is, whatever graph used it before)
    w, b = d(c['w']).requires_grad_(True), d(c['b']).requires_grad_(True)
    mean, var = d(c['stats'][:c['C']]), d(c['stats'][c['C']:])
    bn = ((d(c['x']) - mean) * torch.rsqrt(var + ops.BN_EPS) * d(c['gamma']) + d(c['beta'])).requires_grad_(True)
    z = bn @ w + b
    loss = wl2_loss(c['gt'], z, TARGET_VALUE) if kind == 'wl2' else ce_loss(c['gt'], z)
    loss.backward()
    return loss.detach(), bn.grad.clone(), w.grad.clone(), b.grad.clone()


@functools.lru_cache(maxsize=None)
def _refs(C, N, shape, kind):
    """(float64, float32-CPU) results of one case and kind; computed once, never modified"""
    import torch
    c = _case(C, N, shape)
    return _logit_graph(c, kind, torch.float64), _logit_graph(c, kind, torch.float32)


def _device_loss(sums, kind, N, nvox):
    if kind == 'wl2':
        return sums[0] / ((sums[1] + 1e-8 * sums[2]) * N)
    return sums[0] / nvox


def _run(torch, c, kind, misalign=False):
    """both kernels on one case; returns (loss, dbn, dw, db) and checks the guards and the two counts"""
    from synthsr_amd import ops
    C, N = c['C'], c['N']
    nvox = int(np.prod(c['shape']))
    dev = lambda k: c[k].cuda()
    x, seg, lut = dev('x'), dev('seg'), dev('lut')
    head = (dev('stats'), dev('gamma'), dev('beta'), dev('w'), dev('b'))
    sfull, sums = _guarded(torch, 3, misalign)
    ops.seg_head_logit_loss_fwd(x, *head, seg, lut, sums, kind, TARGET_VALUE)
    loss = _device_loss(sums, kind, N, nvox).clone()
    bfull, dbn = _guarded(torch, nvox * C, misalign)
    wfull, dw = _guarded(torch, C * N, misalign, fill=0.0)
    dfull, db = _guarded(torch, N, misalign, fill=0.0)
    ops.seg_head_logit_loss_bwd(seg, lut, x, *head, sums, dbn, dw, db, kind, TARGET_VALUE)
    torch.cuda.synchronize()
    o = 1 if misalign else 0
    for nm, full, n in (('sums', sfull, 3), ('dbn', bfull, nvox * C), ('dw', wfull, C * N), ('db', dfull, N)):
        assert bool((full[o + n:] == SENTINEL).all()) and bool((full[:o] == SENTINEL).all()), nm + ' guard overwritten'
    classed = int((c['gt'].sum(-1) > 0).sum())
    background = int(c['gt'][..., 0].sum())
    want = (nvox - background, background) if kind == 'wl2' else (classed, 0)
    assert (float(sums[1]), float(sums[2])) == want, (sums.tolist(), want)
    return loss, dbn.view(*c['shape'], C), dw.view(C, N), db


def _check(got, refs):
    names = ('loss', 'dbn', 'dw', 'db')
    bad = []
    for nm, dev, ref, cpu in zip(names, got, *refs):
        scale = ref.abs().max().item()
        bound = 2e-5 * (max(scale, 1e-2) if nm in ('dw', 'db') else scale)
        d, o = _dist(dev, ref), _dist(cpu, ref)
        print('%-5s device-float64 %.3e  fp32 CPU-float64 %.3e  bound %.3e (scale %.3e)' % (nm, d, o, bound, scale))
        if not d < bound:
            bad.append((nm, d, bound))
    assert not bad, bad


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('C,N,shape,misalign', LOSS_CASES)
def test_seg_head_logit_loss_kernels_vs_autograd(T, C, N, shape, misalign, kind):
    """label maps with values outside the table, values mapped to -1, a class without any voxel and a single voxel of class 0
    (weight 1e-8 in the weighted L2; the voxels without a class weigh 1 there and nothing in the cross-entropy); sentinels
    behind (and, misaligned, in front of) every output; the voxel counts in sums[1], sums[2] exactly"""
    _check(_run(T, _case(C, N, shape), kind, misalign), _refs(C, N, shape, kind))


def test_cross_entropy_stays_finite_where_a_posterior_underflows(T):
    """logits 200 apart: the posterior of the true class is 0 in fp32 (the reference's log would give inf); the log-softmax
    gives the float64 value of the logit form"""
    torch = T
    from synthsr_amd import ops
    C, N = 8, 5
    c = dict(_case(C, N, SHAPE))
    c['w'] = c['w'] * 0.
    c['b'] = torch.tensor([0., 200., -50., 3., 0.])
    ref = _logit_graph(c, 'ce', torch.float64)
    assert bool((torch.softmax(c['b'], 0)[[0, 2]] == 0).all())
    got = _run(torch, c, 'ce')
    assert bool(torch.isfinite(got[0])) and abs(got[0].item() - ref[0].item()) < 2e-5 * ref[0].item()
    assert _dist(got[3], ref[3]) < 2e-5 * max(ref[3].abs().max().item(), 1e-2)


def test_seg_head_logit_loss_limits_are_refused(T):
    """C = 68 (> 64), C = 6 (not whole channel quads), N = 1 and N = 65, NULL pointers and an unknown kind return the
    invalid-argument error and launch nothing; wrong dtypes, sums of the wrong length and an unknown kind raise in ops"""
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    nvox = int(np.prod(SHAPE))

    def tensors(C, N):
        x = torch.randn(*SHAPE, C).cuda()
        stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
        gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
        w, b = torch.randn(C, N).cuda(), torch.zeros(N).cuda()
        seg, lut = torch.zeros(nvox, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
        sums = torch.full((3,), SENTINEL).cuda()
        dbn, dw, db = torch.full((nvox * C,), SENTINEL).cuda(), torch.full((C * N,), SENTINEL).cuda(), torch.full((N,), SENTINEL).cuda()
        return x, stats, gamma, beta, w, b, seg, lut, sums, dbn, dw, db

    def raw(t, C, N, kind, null=None):
        x, stats, gamma, beta, w, b, seg, lut, sums, dbn, dw, db = [None if i == null else _lib.ptr(v) for i, v in enumerate(t)]
        f = lib.synthsr_seg_head_logit_loss_fwd(x, nvox, C, stats, gamma, beta, ops.BN_EPS, w, b, N, seg, lut, 4, kind, 5., sums,
                                                _lib.stream())
        g = lib.synthsr_seg_head_logit_loss_bwd(seg, lut, 4, x, nvox, C, N, stats, gamma, beta, ops.BN_EPS, w, b, kind, 5., sums,
                                                1., dbn, dw, db, _lib.stream())
        return f, g

    def untouched(t):
        torch.cuda.synchronize()
        return all(bool((v == SENTINEL).all()) for v in t[8:])

    for C, N in ((68, 5), (6, 5), (24, 1), (24, 65)):
        t = tensors(C, N)
        for kind in (0, 1):
            assert raw(t, C, N, kind) == (-1, -1)   # SYNTHSR_EINVAL
        for kind in KINDS:
            with pytest.raises(ValueError):
                ops.seg_head_logit_loss_fwd(*t[:8], t[8].clone(), kind)
            with pytest.raises(ValueError):
                ops.seg_head_logit_loss_bwd(t[6], t[7], *t[:6], *t[8:], kind)
        assert untouched(t)
    t = tensors(24, 5)
    for kind in (-1, 2, 7):
        assert raw(t, 24, 5, kind) == (-1, -1)
    for null in range(8):                       # every input pointer in turn (fwd has no dbn / dw / db: those are bwd's)
        assert raw(t, 24, 5, 0, null) == (-1, -1)
    assert raw(t, 24, 5, 1, 8) == (-1, -1)      # sums
    for null in (9, 10, 11):
        assert raw(t, 24, 5, 1, null)[1] == -1
    t[8].fill_(SENTINEL)                        # (the three valid forward calls of the loop above accumulated into sums)
    x, stats, gamma, beta, w, b, seg, lut, sums, dbn, dw, db = t
    bad_calls = [
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut, sums, 'dice'),
        lambda: ops.seg_head_logit_loss_bwd(seg, lut, x, stats, gamma, beta, w, b, sums, dbn, dw, db, 'l2'),
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut, torch.full((2,), SENTINEL).cuda(), 'wl2'),
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut, torch.full((10,), SENTINEL).cuda(), 'ce'),
        lambda: ops.seg_head_logit_loss_bwd(seg, lut, x, stats, gamma, beta, w, b, sums[:2], dbn, dw, db, 'wl2'),
        lambda: ops.seg_head_logit_loss_fwd(x.half(), stats, gamma, beta, w, b, seg, lut, sums, 'wl2'),
        lambda: ops.seg_head_logit_loss_fwd(x.bfloat16(), stats, gamma, beta, w, b, seg, lut, sums, 'ce'),
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w.double(), b, seg, lut, sums, 'ce'),
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg.long(), lut, sums, 'wl2'),
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut.long(), sums, 'wl2'),
        lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut, sums.double(), 'wl2'),
        lambda: ops.seg_head_logit_loss_bwd(seg, lut, x, stats, gamma, beta, w, b, sums, dbn.double(), dw, db, 'ce'),
        lambda: ops.seg_head_logit_loss_bwd(seg.long(), lut, x, stats, gamma, beta, w, b, sums, dbn, dw, db, 'ce'),
        lambda: ops.seg_head_logit_loss_bwd(seg, lut, x, stats, gamma, beta, w, b, sums, dbn[:-1], dw, db, 'ce'),
    ]
    for f in bad_calls:
        with pytest.raises(ValueError):
            f()
    assert untouched(t)


def test_seg_head_logit_loss_kernels_repeat_bit_for_bit_in_deterministic_mode(T):
    from synthsr_amd import ops
    c = _case(24, 33, BIG)
    prev = ops.set_deterministic(True)
    try:
        for kind in KINDS:
            a = [_bits(t) for t in _run(T, c, kind)]
            b = [_bits(t) for t in _run(T, c, kind)]
            assert ops.deterministic_status() == 1, 'an ordered wait timed out'
            for nm, u, v in zip(('loss', 'dbn', 'dw', 'db'), a, b):
                assert np.array_equal(u, v), '%s: %s differs between two deterministic runs' % (kind, nm)
            assert np.any(a[2] != 0)
    finally:
        ops.set_deterministic(prev)


# ---------------------------------------------------------------------------------------------------- whole network
def _logit_step(net, kind, x, seg, lut):
    loss = net.loss_wl2(x.cuda(), seg.cuda(), lut.cuda(), TARGET_VALUE) if kind == 'wl2' else \
        net.loss_cross_entropy(x.cuda(), seg.cuda(), lut.cuda())
    net.test_loss = loss.clone()
    net.backward()
    return net


def _dice_step(net, x, seg, lut):
    loss = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda())
    net.test_loss = loss.clone()
    net.backward()
    return net


@pytest.mark.parametrize('kind', KINDS)
def test_unet_logit_losses_and_gradients_vs_autograd(T, kind):
    """one loss_wl2 / loss_cross_entropy + backward() of the whole network against the oracle on its logits (loss, every
    BatchNorm batch statistic, every parameter gradient by the float64-anchored rule of conftest.single_shot_parity, max-pool
    ties aligned by it)"""
    torch = T
    from oracle import unet_ref as U
    from synthsr_amd import ops
    x, seg, lut, gt = _net_inputs()

    def run():
        net = _logit_step(_seg_net(torch), kind, x, seg, lut)
        # what single_shot_parity reads as d(loss)/d(prediction): here the derivative w.r.t. the logits, formed from the kept
        # feature map and sums (neither loss has a kink: the oracle's must simply agree)
        low, bn = net.saved['last']
        C = low.shape[3]
        stats = net._stats(bn)
        z = ((low.reshape(-1, C) - stats[:C]) * torch.rsqrt(stats[C:] + ops.BN_EPS) * net.view(bn['gamma']) + net.view(bn['beta'])) \
            @ net.view(net.head['w']).reshape(C, N_SEG) + net.view(net.head['b'])
        g = gt.float().cuda().view(-1, N_SEG)
        sums = net._loss_state.sums
        if kind == 'wl2':
            a = torch.where(g[:, :1] > 0, torch.full_like(g[:, :1], 1e-8), torch.ones_like(g[:, :1]))
            dz = 2 * a * (z - TARGET_VALUE * (2 * g - 1)) / ((sums[1] + 1e-8 * sums[2]) * N_SEG)
        else:
            dz = (torch.softmax(z, -1) - g) * g.sum(-1, keepdim=True) / z.shape[0]
        net.dpred = dz.reshape(-1)
        net.test_stats = net.bn_batch.clone()
        return net

    def oracle(net, nudge):
        P = {nm: v.detach().cpu().clone().requires_grad_(True) for nm, v in net.named_parameters()}
        stats, pin = {}, []
        z = U.unet_forward(x, P, net.prefix, LEVELS, 2, training=True, softmax=False, collect=stats, pool_inputs=pin,
                           pool_nudge=nudge)
        lr = wl2_loss(gt, z, TARGET_VALUE) if kind == 'wl2' else ce_loss(gt, z)
        lr.backward()
        return (P, stats, lr.detach()), pin

    def compare(net, ref):
        P, stats, lr = ref
        print('%s loss %.9g oracle %.9g' % (kind, net.test_loss.item(), lr.item()))
        assert abs(net.test_loss.item() - lr.item()) < 2e-5 * max(1.0, abs(lr.item()))
        for bn in net.bn_layers:
            o, C = bn['soff'], bn['C']
            for i, what in enumerate(('mean', 'var')):
                got, want = net.test_stats[o + i * C:o + (i + 1) * C].cpu().double(), stats[bn['name']][i].double()
                err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
                assert err < 1e-4, (bn['name'], what, err)

    single_shot_parity(run, oracle, compare, loss_of=lambda n_: n_.test_loss)


def test_the_two_loss_records_do_not_leak_into_each_other(T):
    """deterministic mode: a Dice step after a weighted-L2 step on the same network equals, bit for bit, the Dice step of a
    network in the same state that never ran the weighted L2 -- and the other way round, for both logit losses; after
    predict_probs() neither record is left"""
    torch = T
    from synthsr_amd import ops
    x, seg, lut, _ = _net_inputs()
    out = lambda net: (_bits(net.grads), _bits(net.test_loss))
    prev = ops.set_deterministic(True)
    try:
        dice_alone = out(_dice_step(_seg_net(torch), x, seg, lut))
        for kind in KINDS:
            alone = out(_logit_step(_seg_net(torch), kind, x, seg, lut))
            net = _logit_step(_seg_net(torch), kind, x, seg, lut)
            assert net._loss_state.kind == 'logits'
            after = out(_dice_step(net, x, seg, lut))
            assert net._loss_state.kind == 'dice'
            assert np.array_equal(after[0], dice_alone[0]) and np.array_equal(after[1], dice_alone[1]), kind
            back = out(_logit_step(net, kind, x, seg, lut))
            assert np.array_equal(back[0], alone[0]) and np.array_equal(back[1], alone[1]), kind
            assert np.any(alone[0] != dice_alone[0])
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
        net.training = False
        net.predict_probs(x.cuda())
        assert net._loss_state is None
        with pytest.raises(RuntimeError):
            net.backward()
    finally:
        ops.set_deterministic(prev)


# ---------------------------------------------------------------------------------------------------- end to end
def _training_args(tmp_path):
    labels_dir, seg_labels = _write_inputs(tmp_path)
    kw = dict(path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3, unet_feat_count=24,
              nonlin_shape_factor=.125, bias_shape_factor=.125, lr=1e-3, verbose=False, deterministic=True)
    args = (labels_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'), str(tmp_path / 'sl.npy'))
    return args, kw


def _record_losses(monkeypatch):
    """every UNet3D loss call of a run: (name, x, seg, lut, returned loss), the tensors cloned"""
    from synthsr_amd.unet import UNet3D
    calls = []
    for name in ('loss_wl2', 'loss_dice', 'loss_cross_entropy'):
        original = getattr(UNet3D, name)

        def wrapped(self, x, seg, lut, *a, _original=original, _name=name, **kw):
            loss = _original(self, x, seg, lut, *a, **kw)
            calls.append((_name, x.clone(), seg.clone(), lut.clone(), loss.clone(), a, kw))
            return loss
        monkeypatch.setattr(UNet3D, name, wrapped)
    return calls


def test_training_segmentation_warm_up_then_dice_and_resume(tmp_path, monkeypatch):
    """wl2_epochs=1 of epochs=2 x 3 steps: the three warm-up losses are loss_wl2 values (the first recomputed on a fresh
    identical network from the recorded sample), three Dice steps follow, two log rows and two checkpoint pairs, and the
    optimizer started afresh in between (iterations == 3 at the end); resumed from 001.npz the second epoch trains with the Dice
    and ends at iterations == 3 as well"""
    import torch
    from synthsr_amd import ops
    from synthsr_amd.segmentation_training import training_segmentation
    (labels_dir, *rest), kw = _training_args(tmp_path)
    calls = _record_losses(monkeypatch)
    full_dir = str(tmp_path / 'full')
    rec = []
    net = training_segmentation(labels_dir, full_dir, *rest, wl2_epochs=1, epochs=2, steps_per_epoch=3, step_losses=rec, **kw)
    assert [c[0] for c in calls] == ['loss_wl2'] * 3 + ['loss_dice'] * 3
    assert all(c[5] == (5.,) for c in calls[:3])                      # wl2_target_value's default reaches loss_wl2
    assert len(rec) == 6 and np.isfinite(rec).all()
    assert [np.float32(v).tobytes() for v in rec] == [np.float32(c[4].item()).tobytes() for c in calls]
    assert net.iterations == 3, 'the optimizer did not start afresh behind the warm-up'
    log = open(os.path.join(full_dir, 'logs', 'loss.csv')).read().strip().split('\n')
    assert len(log) == 2
    assert abs(float(log[0].split(',')[1]) - np.mean(rec[:3])) < 1e-5 * np.mean(rec[:3])
    for e in (1, 2):
        assert os.path.exists(os.path.join(full_dir, '%03d.npz' % e)) and os.path.exists(os.path.join(full_dir, '%03d.h5' % e))
    assert not os.path.exists(os.path.join(full_dir, '003.npz'))
    # the first warm-up loss, from a fresh identical network (epochs=0: built and seeded, not trained) and the first sample
    first = calls[0]
    del calls[:]
    fresh = training_segmentation(labels_dir, str(tmp_path / 'fresh'), *rest, wl2_epochs=1, epochs=0, steps_per_epoch=3, **kw)
    assert not calls and fresh.iterations == 0
    prev = ops.set_deterministic(True)
    try:
        again = fresh.loss_wl2(first[1], first[2], first[3], 5.).item()
    finally:
        ops.set_deterministic(prev)
    assert np.float32(again).tobytes() == np.float32(rec[0]).tobytes(), (again, rec[0])
    # a weighted L2 of logits near 0 against targets +-5 is about 25; a Dice is at most 1
    assert 5. < rec[0] and all(0. < v <= 1. for v in rec[3:]), rec
    # resumed at the epoch behind the warm-up: Dice only, and the same fresh optimizer
    del calls[:]
    rec2 = []
    net2 = training_segmentation(labels_dir, str(tmp_path / 'part'), *rest, wl2_epochs=1, epochs=2, steps_per_epoch=3,
                                 step_losses=rec2, checkpoint=os.path.join(full_dir, '001.npz'), **kw)
    assert [c[0] for c in calls] == ['loss_dice'] * 3 and len(rec2) == 3
    assert net2.iterations == 3
    # resumed later, nothing is reset: the checkpoint of epoch 2 holds iterations == 3, one more epoch makes 6
    net3 = training_segmentation(labels_dir, str(tmp_path / 'later'), *rest, wl2_epochs=1, epochs=3, steps_per_epoch=3,
                                 checkpoint=os.path.join(full_dir, '002.npz'), **kw)
    assert net3.iterations == 6


@pytest.mark.parametrize('loss_kw', [dict(segmentation_loss='cross_entropy'), dict(wl2_epochs=2)])
def test_training_segmentation_lowers_the_new_losses_on_a_fixed_sample(tmp_path, monkeypatch, loss_kw):
    from synthsr_amd.segmentation_training import training_segmentation
    (labels_dir, *rest), kw = _training_args(tmp_path)
    calls = _record_losses(monkeypatch)
    rec = []
    training_segmentation(labels_dir, str(tmp_path / 'm'), *rest, epochs=2, steps_per_epoch=5, fixed_sample=True, step_losses=rec,
                          **loss_kw, **kw)
    assert {c[0] for c in calls} == {'loss_cross_entropy' if 'segmentation_loss' in loss_kw else 'loss_wl2'}
    assert len(rec) == 10 and np.isfinite(rec).all() and rec[-1] < rec[0], rec
