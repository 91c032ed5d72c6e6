"""Training the softmax-headed segmentation U-Net with the soft Dice: the two fused head kernels alone
(csrc/unet_pointwise.hip: seg_head_dice_fwd_kernel / seg_head_dice_bwd_kernel), UNet3D.loss_dice + backward() on a whole network,
deterministic mode, the untouched frozen path, and training_segmentation() end to end.

The reference of the kernel tests is float64 autograd on softmax(bn @ w + b) and oracle.unet_ref.dice_loss; whole networks go
through oracle.unet_ref.unet_forward(..., softmax=True, training=True) under conftest.single_shot_parity.

Tolerances of the kernel tests are the project's bounds for this mathematics (tests/test_unet_gpu.py, tests/test_wide_head_gpu.py):
2e-5 relative for probs, the loss and dbn; 2e-5 of max(|ref|max, 1e-2) for dw and db.  Every test prints the device's distance
from float64 next to that of the same graph evaluated in float32 by torch on the CPU.  Measured on an MI355X over the nine
kernel cases (device / fp32 CPU, absolute): probs <= 6.9e-7 / 6.8e-7, loss <= 4.1e-8 / 9.4e-8, dbn <= 5.7e-10 / 5.3e-10 on a scale
of 1e-3, dw <= 2.9e-9 / 3.7e-9, db <= 8.5e-10 / 6.5e-10: the bounds hold with a factor of 25 or more to spare."""
import functools
import os

import numpy as np
import pytest

from conftest import single_shot_parity

pytestmark = pytest.mark.gpu

SHAPE = (5, 7, 9)            # 315 voxels: four full 64-voxel tiles (one full sweep of a 256-thread workgroup) and a partial one
BIG = (33, 16, 16)           # 8448 voxels = 132 tiles: as many workgroups flush their partial sums
GUARD, SENTINEL = 64, -12345.5
# (C, N, shape, misaligned outputs): every C of {8, 24, 64} and every N of {2, 5, 19, 33, 64}, C = 24 with N = 33 (neither a
# multiple of 16) on both shapes
CASES = [(8, 2, SHAPE, False), (8, 19, SHAPE, True), (24, 5, SHAPE, False), (24, 33, SHAPE, True), (24, 33, BIG, False),
         (64, 64, SHAPE, False), (64, 19, SHAPE, True), (24, 64, SHAPE, False), (64, 33, SHAPE, False)]


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dist(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item()


def _head_graph(c, dtype):
    """softmax(bn @ w + b) + soft Dice of one case in `dtype` under autograd: (probs, loss, dbn, dw, db)"""
    import torch
    from synthsr_amd import ops
    from oracle import unet_ref as U
    d = lambda t: t.to(dtype)
    w, b = d(c['w']).requires_grad_(True), d(c['b']).requires_grad_(True)
    mean, var = d(c['stats'][:c['C']]), d(c['stats'][c['C']:])
    bn = ((d(c['x']) - mean) * torch.rsqrt(var + ops.BN_EPS) * d(c['gamma']) + d(c['beta'])).requires_grad_(True)
    probs = torch.softmax(bn @ w + b, -1)
    loss = U.dice_loss(d(c['gt']), probs)
    loss.backward()
    return probs.detach(), loss.detach(), bn.grad.clone(), w.grad.clone(), b.grad.clone()


@functools.lru_cache(maxsize=None)
def _case(C, N, shape):
    """inputs (host) and the float64 / float32-CPU results of one head configuration; computed once, never modified"""
    import torch
    g = torch.Generator().manual_seed(1000 * C + N + shape[0])
    nvox = int(np.prod(shape))
    x = torch.randn(*shape, C, generator=g)
    mean, var = torch.randn(C, generator=g) * .1, torch.rand(C, generator=g) + .5
    gamma, beta = torch.rand(C, generator=g) + .5, torch.randn(C, generator=g) * .1
    w = torch.randn(C, N, generator=g) * .3
    b = torch.randn(N, generator=g) * .1
    # label VALUES: N of them out of a table of 2 N + 8, in no order; class N - 1 has no voxel, class 0 exactly one
    lut_n = 2 * N + 8
    values = torch.randperm(lut_n, generator=g)
    label_list, unlisted = values[:N], values[N:]
    lut = torch.full((lut_n,), -1, dtype=torch.int32)
    lut[label_list] = torch.arange(N, dtype=torch.int32)
    if N > 2:
        cls = torch.randint(1, N - 1, (nvox,), generator=g)
        seg = label_list[cls].to(torch.int32)
    else:
        seg = torch.full((nvox,), int(unlisted[0]), dtype=torch.int32)
    pos = torch.randperm(nvox, generator=g)
    seg[pos[0]] = int(label_list[0])                    # the single voxel of class 0
    seg[pos[1:9]] = unlisted[:8].to(torch.int32)        # values of the table mapped to -1
    seg[pos[9:12]] = torch.tensor([-3, lut_n, lut_n + 1000], dtype=torch.int32)   # values outside the table
    k = torch.where((seg >= 0) & (seg < lut_n), lut[seg.clamp(0, lut_n - 1).long()], torch.full_like(seg, -1))
    gt = torch.zeros(nvox, N, dtype=torch.float64)
    gt[k >= 0, k[k >= 0].long()] = 1.0
    assert gt[:, N - 1].sum() == 0 and gt[:, 0].sum() == 1 and int((k < 0).sum()) >= 11
    c = dict(C=C, N=N, shape=shape, x=x, stats=torch.cat([mean, var]), gamma=gamma, beta=beta, w=w, b=b, seg=seg, lut=lut,
             gt=gt.view(*shape, N))
    c['ref'] = _head_graph(c, torch.float64)
    c['cpu32'] = _head_graph(c, torch.float32)
    return c


def _guarded(torch, numel, misalign=False, fill=SENTINEL):
    """a device buffer of `numel` floats with GUARD sentinel floats behind it (and one in front when misaligned)"""
    full = torch.full((numel + GUARD + 1,), SENTINEL, device='cuda')
    o = 1 if misalign else 0
    view = full[o:o + numel]
    if fill != SENTINEL:
        view.fill_(fill)
    return full, view


def _run(torch, c, misalign=False):
    """both kernels on one case; returns (probs, loss, dbn, dw, db) and checks the guards"""
    from synthsr_amd import ops
    C, N = c['C'], c['N']
    nvox = int(np.prod(c['shape']))
    dev = lambda k: c[k].cuda()
    x, seg, lut = dev('x'), dev('seg'), dev('lut')
    sums = torch.empty(2 * N, device='cuda')
    pfull, probs = _guarded(torch, nvox * N, misalign)
    ops.seg_head_dice_fwd(x, dev('stats'), dev('gamma'), dev('beta'), dev('w'), dev('b'), seg, lut, probs, sums)
    loss = (1.0 - (sums[:N] + 1e-7) / (sums[N:] + 1e-7)).mean()
    bfull, dbn = _guarded(torch, nvox * C, misalign)
    wfull, dw = _guarded(torch, C * N, misalign, fill=0.0)
    dfull, db = _guarded(torch, N, misalign, fill=0.0)
    ops.seg_head_dice_bwd(probs, seg, lut, x, dev('stats'), dev('gamma'), dev('beta'), dev('w'), sums, dbn, dw, db)
    torch.cuda.synchronize()
    o = 1 if misalign else 0
    for nm, full, n in (('probs', pfull, nvox * N), ('dbn', bfull, nvox * C), ('dw', wfull, C * N), ('db', dfull, N)):
        assert bool((full[o + n:] == SENTINEL).all()) and bool((full[:o] == SENTINEL).all()), nm + ' guard overwritten'
    return probs.view(*c['shape'], N), loss, dbn.view(*c['shape'], C), dw.view(C, N), db


def _check(got, c):
    names = ('probs', 'loss', 'dbn', 'dw', 'db')
    bad = []
    for nm, dev, ref, cpu in zip(names, got, c['ref'], c['cpu32']):
        scale = ref.abs().max().item()
        bound = 2e-5 * (max(scale, 1e-2) if nm in ('dw', 'db') else scale)
        d, o = _dist(dev, ref), _dist(cpu, ref)
        print('%-5s device-float64 %.3e  fp32 CPU-float64 %.3e  bound %.3e (scale %.3e)' % (nm, d, o, bound, scale))
        if not d < bound:
            bad.append((nm, d, bound))
    assert not bad, bad


@pytest.mark.parametrize('C,N,shape,misalign', CASES)
def test_seg_head_dice_kernels_vs_autograd(T, C, N, shape, misalign):
    """label maps with values outside the table, values mapped to -1, a class without any voxel (its Dice term is
    1 - 1e-7 / (sum p^2 + 1e-7)) and a class of a single voxel; sentinels behind (and, misaligned, in front of) every output"""
    c = _case(C, N, shape)
    _check(_run(T, c, misalign), c)


def test_seg_head_dice_limits_are_refused(T):
    """C = 68 (> 64), C = 6 (not whole channel quads) and N = 65 return the invalid-argument error and launch nothing"""
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    nvox = int(np.prod(SHAPE))
    for C, N in ((68, 5), (6, 5), (24, 65)):
        x = torch.randn(*SHAPE, C).cuda()
        stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
        gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
        w, b = torch.randn(C, N).cuda(), torch.zeros(N).cuda()
        seg, lut = torch.zeros(nvox, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
        probs, sums = torch.full((nvox * N,), SENTINEL).cuda(), torch.full((2 * N,), SENTINEL).cuda()
        dbn, dw, db = torch.full((nvox * C,), SENTINEL).cuda(), torch.full((C * N,), SENTINEL).cuda(), torch.full((N,), SENTINEL).cuda()
        rc = lib.synthsr_seg_head_dice_fwd(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), ops.BN_EPS,
                                           _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(seg), _lib.ptr(lut), 4, _lib.ptr(probs),
                                           _lib.ptr(sums), _lib.stream())
        assert rc == -1   # SYNTHSR_EINVAL
        rc = lib.synthsr_seg_head_dice_bwd(_lib.ptr(probs), _lib.ptr(seg), _lib.ptr(lut), 4, _lib.ptr(x), nvox, C, N,
                                           _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), ops.BN_EPS, _lib.ptr(w),
                                           _lib.ptr(sums), 1.0, _lib.ptr(dbn), _lib.ptr(dw), _lib.ptr(db), _lib.stream())
        assert rc == -1
        with pytest.raises(ValueError):
            ops.seg_head_dice_fwd(x, stats, gamma, beta, w, b, seg, lut, probs, sums.clone())
        with pytest.raises(ValueError):
            ops.seg_head_dice_bwd(probs, seg, lut, x, stats, gamma, beta, w, sums, dbn, dw, db)
        torch.cuda.synchronize()
        for t in (probs, sums, dbn, dw, db):
            assert bool((t == SENTINEL).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32).copy()


def test_seg_head_dice_kernels_repeat_bit_for_bit_in_deterministic_mode(T):
    from synthsr_amd import ops
    c = _case(24, 33, BIG)
    prev = ops.set_deterministic(True)
    try:
        a = [_bits(t) for t in _run(T, c)]
        b = [_bits(t) for t in _run(T, c)]
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
    finally:
        ops.set_deterministic(prev)
    for nm, u, v in zip(('probs', 'loss', 'dbn', 'dw', 'db'), a, b):
        assert np.array_equal(u, v), nm + ' differs between two deterministic runs'


# ---------------------------------------------------------------------------------------------------- whole network
NET_SHAPE, LEVELS, N_SEG = (16, 16, 16), 3, 5
SEG_LABELS = np.array([0, 14, 2, 41, 17])      # head channel order (label values); 3 and 42 appear in the maps but not here


def _seg_net(torch, activation='elu', dropout=0., seed=5):
    from synthsr_amd.unet import UNet3D
    net = UNet3D(24, list(NET_SHAPE) + [1], LEVELS, 3, N_SEG, feat_mult=2, nb_conv_per_level=2, batch_norm=-1,
                 final_pred_activation='softmax', activation=activation, conv_dropout=dropout, seed=seed)
    g = torch.Generator().manual_seed(12)
    for nm, v in net.named_parameters():
        if nm.endswith('/gamma'):
            v.copy_(torch.rand(v.shape, generator=g) + .5)
        elif nm.endswith('/beta') or nm.endswith('/bias'):
            v.copy_(torch.randn(v.shape, generator=g) * .1)
    net.repack()
    return net


@functools.lru_cache(maxsize=None)
def _net_inputs():
    import torch
    from synthsr_amd.segmentation_training import segmentation_lut
    g = torch.Generator().manual_seed(21)
    x = torch.rand(*NET_SHAPE, 1, generator=g)
    values = torch.tensor([0, 14, 2, 41, 17, 3, 42], dtype=torch.int32)
    seg = values[torch.randint(0, len(values), NET_SHAPE, generator=g)]
    lut = torch.from_numpy(segmentation_lut(SEG_LABELS))
    k = torch.where(seg < len(lut), lut[seg.clamp(max=len(lut) - 1).long()], torch.full_like(seg, -1))   # 42 lies beyond the table
    gt = torch.zeros(*NET_SHAPE, N_SEG, dtype=torch.float64)
    for n in range(N_SEG):
        gt[..., n] = (k == n).double()
    return x, seg, lut, gt


def _dice_step(net, x, seg, lut):
    loss = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda())
    net.test_loss = loss.clone()
    net.backward()
    return net


@pytest.mark.parametrize('activation,dropout', [('elu', 0.), ('elu', .2)])
def test_unet_dice_loss_and_gradients_vs_autograd(T, activation, dropout):
    """one loss_dice + backward() of the whole network against the oracle (loss, every BatchNorm batch statistic, every
    parameter gradient by the float64-anchored rule of conftest.single_shot_parity, max-pool ties aligned by it)"""
    torch = T
    from oracle import unet_ref as U
    x, seg, lut, gt = _net_inputs()
    scales = None
    if dropout:
        rng = np.random.default_rng(7)
        scales = {}
        for c in _seg_net(torch, activation, dropout).all_convs():
            keep = rng.random(c['cout']) >= dropout
            keep[:2] = [False, True]
            scales[c['name']] = (keep / (1.0 - dropout)).astype(np.float32)

    def run():
        net = _seg_net(torch, activation, dropout)
        if scales is not None:
            net.set_dropout_scales(scales)
        _dice_step(net, x, seg, lut)
        # what single_shot_parity reads as d(loss)/d(prediction): here the derivative w.r.t. the posteriors, from the kept
        # posteriors and Dice sums (the Dice has no kinks: the oracle's must simply agree)
        probs, sums = net._loss_state.probs, net._loss_state.sums
        Tn, Bn = sums[:N_SEG] + 1e-7, sums[N_SEG:] + 1e-7
        net.dpred = (-(1.0 / N_SEG) * (2 * gt.float().cuda().view(-1, N_SEG) * Bn - 2 * probs * Tn) / (Bn * Bn)).reshape(-1)
        net.test_stats = (net.bn_true if scales is not None else net.bn_batch).clone()
        return net

    def oracle(net, nudge):
        P = {nm: v.detach().cpu().clone().requires_grad_(True) for nm, v in net.named_parameters()}
        stats, pin = {}, []
        pr = U.unet_forward(x, P, net.prefix, LEVELS, 2, training=True, softmax=True, collect=stats, pool_inputs=pin,
                            pool_nudge=nudge, dropout=None if scales is None else {k: torch.from_numpy(v) for k, v in scales.items()})
        if U._PRED_TAP is not None:   # (unet_forward taps linear heads only)
            pr = U._PRED_TAP(pr)
        lr = U.dice_loss(gt.to(pr.dtype), pr)
        lr.backward()
        return (P, stats, lr.detach()), pin

    def compare(net, ref):
        P, stats, lr = ref
        print('loss %.9g oracle %.9g' % (net.test_loss.item(), lr.item()))
        assert abs(net.test_loss.item() - lr.item()) < 2e-5 * max(1.0, abs(lr.item()))
        for bn in net.bn_layers:
            o, C = bn['soff'], bn['C']
            for i, what in enumerate(('mean', 'var')):
                got, want = net.test_stats[o + i * C:o + (i + 1) * C].cpu().double(), stats[bn['name']][i].double()
                err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
                assert err < 1e-4, (bn['name'], what, err)

    single_shot_parity(run, oracle, compare, loss_of=lambda n_: n_.test_loss)


def test_unet_dice_relu_network_vs_oracle(T, monkeypatch):
    """the same step with activation='relu'.  oracle.unet_ref has no ReLU: the oracle is the one of tests/test_relu_gpu.py (its
    ELU swapped for ReLU, imported) with that test's protocol -- one deterministic step; a ReLU site counts as a rounding tie
    only where the device's mask differs from the float64 oracle's and |z64| <= 64 eps32 S, at most 8, the oracle then takes
    the device's side -- and max-pool ties aligned by conftest.align_pool_ties; loss, BatchNorm statistics, every gradient by
    conftest.assert_grads_anchored"""
    torch = T
    import contextlib
    from synthsr_amd import ops
    from conftest import assert_grads_anchored, net_grads, align_pool_ties, _pool_choices
    from test_relu_gpu import _ReluOracle
    R = _ReluOracle(monkeypatch, torch)
    U = R.U
    x, seg, lut, gt = _net_inputs()
    prev = ops.set_deterministic(True)
    try:
        net = _seg_net(torch, 'relu')
        assert net._act == 3
        loss = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda()).item()
        masks = [a.detach().cpu().reshape(-1) > 0 for lv in net.saved['enc'] + net.saved['dec'] for a in lv]
        net.backward()
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
        det_pool = _pool_choices(net)
        dev = net_grads(net)
    finally:
        ops.set_deterministic(prev)
    P0 = {nm: v.detach().cpu().clone() for nm, v in net.named_parameters()}
    with U.compute_dtype(torch.float64):
        with torch.no_grad():
            R.forward(x, P0, net.prefix, LEVELS, rec=True, softmax=True)
    assert len(R.zs) == len(masks)
    force, ties = [], 0
    eps32 = float(torch.finfo(torch.float32).eps)
    for m, z, S in zip(masks, R.zs, R.Ss):
        z, S = z.reshape(-1), S.reshape(-1)
        diff = m != (z > 0)
        if not bool(diff.any()):
            force.append(None)
            continue
        r = z.abs()[diff] / S[diff].clamp_min(1e-300)
        assert bool((r <= 64 * eps32).all()), 'ReLU masks differ at a site %.1f eps32 S from 0: not a rounding tie' % (
            float(r.max()) / eps32)
        ties += int(diff.sum())
        force.append((diff, m[diff]))
    assert ties <= 8, '%d ReLU ties in one network' % ties
    R.force = force

    def oracle(dtype, nudge):
        P = {nm: v.clone().requires_grad_(True) for nm, v in P0.items()}
        stats, pin = {}, []
        with (U.compute_dtype(torch.float64) if dtype == torch.float64 else contextlib.nullcontext()):
            pr = R.forward(x, P, net.prefix, LEVELS, collect=stats, softmax=True, pool_inputs=pin, pool_nudge=nudge)
            lr = U.dice_loss(gt.to(pr.dtype), pr)
        lr.backward()
        return {nm: v.grad.double() for nm, v in P.items()}, stats, lr.item(), pin

    g32, stats, lr32, pin = oracle(torch.float32, None)
    nudges, n_ties = align_pool_ties(det_pool, pin)
    if n_ties:
        g32, stats, lr32, _ = oracle(torch.float32, nudges)
    g64 = oracle(torch.float64, nudges)[0]
    print('relu: %d ReLU tie(s), %d pooling tie(s); loss %.9g oracle %.9g' % (ties, n_ties, loss, lr32))
    assert abs(loss - lr32) < 2e-5 * max(1.0, abs(lr32))
    for bn in net.bn_layers:
        o, C = bn['soff'], bn['C']
        for i, what in enumerate(('mean', 'var')):
            got, want = net.bn_batch[o + i * C:o + (i + 1) * C].cpu().double(), stats[bn['name']][i].double()
            assert (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30) < 1e-4, (bn['name'], what)
    assert_grads_anchored(dev, g32, g64, tag='dice relu')


def test_dice_training_step_repeats_bit_for_bit_in_deterministic_mode(T):
    torch = T
    from synthsr_amd import ops
    x, seg, lut, _ = _net_inputs()
    prev = ops.set_deterministic(True)
    try:
        outs = []
        for _ in range(2):
            net = _dice_step(_seg_net(torch), x, seg, lut)
            outs.append((_bits(net.grads), _bits(net.test_loss)))
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
    finally:
        ops.set_deterministic(prev)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.any(outs[0][0] != 0)


def test_frozen_path_is_untouched_by_a_training_step(T):
    """after loss_dice + backward + Adam on a softmax net, predict_probs + backward_input on the same net equal those of a
    fresh frozen net loaded from its state dict; backward() without a loss_dice() in between raises"""
    torch = T
    x, seg, lut, _ = _net_inputs()
    from synthsr_amd import ops
    net = _dice_step(_seg_net(torch), x, seg, lut)
    net.adam_step(1e-3)
    net.update_moving_stats()
    fresh = _seg_net(torch, seed=9)
    fresh.load_state_dict(net.state_dict())
    g = torch.Generator().manual_seed(3)
    dbn = torch.randn(*NET_SHAPE, 24, generator=g).cuda()
    outs = []
    prev = ops.set_deterministic(True)   # (the default path's float atomics would make two runs of ONE net differ in the last bits)
    try:
        for n_ in (net, fresh):
            n_.training = False
            n_.enable_input_grad()
            probs = n_.predict_probs(x.cuda()).clone()
            outs.append((probs, n_.backward_input(dbn.clone()).clone()))
    finally:
        ops.set_deterministic(prev)
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert float(outs[0][1].abs().max()) > 0
    with pytest.raises(RuntimeError):
        net.backward()
    # and the trained net trains on: the gradient weights of the first conv kept for backward_input do not disturb it
    _dice_step(net, x, seg, lut)
    assert bool(torch.isfinite(net.grads).all()) and float(net.grads.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- end to end
def _write_inputs(tmp_path):
    """the tiny synthetic label maps of tests/test_training_gpu.py"""
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import (synthetic_label_map, GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR,
                                       PRIOR_STDS_T1_HR)
    d = tmp_path / 'labels'
    d.mkdir()
    for i in range(2):
        write_nifti(str(d / ('brain%d_labels.nii.gz' % i)), synthetic_label_map((40, 36, 48), 10 + i).astype(np.float32))
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    np.save(tmp_path / 'gc.npy', GENERATION_CLASSES)
    np.save(tmp_path / 'pm.npy', PRIOR_MEANS_T1_HR)
    np.save(tmp_path / 'ps.npy', PRIOR_STDS_T1_HR)
    seg_labels = np.asarray(GENERATION_LABELS)[::2].copy()    # every other generation label: the rest has no class
    np.save(tmp_path / 'sl.npy', seg_labels)
    return str(d), seg_labels


def test_training_segmentation_end_to_end(tmp_path):
    """20 steps on a fixed sample lower the loss; checkpoints appear as .npz and .h5; resuming from the .npz reproduces the
    next step's loss of the uninterrupted run bit for bit (deterministic mode); the checkpoint plugs into
    training(segmentation_model_file=...)"""
    import torch
    from synthsr_amd import ops
    from synthsr_amd.segmentation_training import training_segmentation
    from synthsr_amd.training import training, read_weights
    labels_dir, seg_labels = _write_inputs(tmp_path)
    kw = dict(path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3, unet_feat_count=24,
              nonlin_shape_factor=.125, bias_shape_factor=.125, lr=1e-3, verbose=False, deterministic=True)
    args = (labels_dir, None, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'), str(tmp_path / 'sl.npy'))
    def run(model_dir, epochs, checkpoint=None):
        rec = []   # fixed_sample: the same generated sample (same model_inputs and draws) every step
        net = training_segmentation(args[0], model_dir, *args[2:], epochs=epochs, steps_per_epoch=10, checkpoint=checkpoint,
                                    fixed_sample=True, step_losses=rec, **kw)
        return net, rec

    full_dir, part_dir = str(tmp_path / 'full'), str(tmp_path / 'part')
    net, rec = run(full_dir, 3)
    assert net.nb_labels == len(seg_labels) and net.final_pred_activation == 'softmax' and net.iterations == 30
    assert np.isfinite(rec).all() and rec[19] < rec[0], (rec[0], rec[19])
    for e in (1, 2, 3):
        assert os.path.exists(os.path.join(full_dir, '%03d.npz' % e)) and os.path.exists(os.path.join(full_dir, '%03d.h5' % e))
    log = open(os.path.join(full_dir, 'logs', 'loss.csv')).read().strip().split('\n')
    assert len(log) == 3
    # resume from epoch 2's .npz: its first step is step 21 of the uninterrupted run
    _, rec2 = run(part_dir, 3, checkpoint=os.path.join(full_dir, '002.npz'))
    assert len(rec2) == 10
    assert np.float32(rec2[0]).tobytes() == np.float32(rec[20]).tobytes(), (rec2[0], rec[20])
    # the trained file as the frozen network of the segmentation-regularised loss
    ckpt = os.path.join(full_dir, '003.h5')
    z = read_weights(ckpt)
    from synthsr_amd.unet import UNet3D
    table = UNet3D(24, [32, 32, 32, 1], 3, 3, len(seg_labels), feat_mult=2, nb_conv_per_level=2, batch_norm=-1,
                   final_pred_activation='softmax', table_only=True)
    missing = [nm for nm, _, _ in table.specs if nm not in z]
    missing += [b['name'] + s for b in table.bn_layers for s in ('/moving_mean', '/moving_variance') if b['name'] + s not in z]
    assert not missing, missing
    reg_dir = str(tmp_path / 'reg')
    training(labels_dir, reg_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
             segmentation_label_list=str(tmp_path / 'sl.npy'), segmentation_label_equivalency=str(tmp_path / 'sl.npy'),
             segmentation_model_file=ckpt, path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3,
             unet_feat_count=24, nonlin_shape_factor=.125, bias_shape_factor=.125, epochs=1, steps_per_epoch=1, verbose=False)
    log = [float(l.split(',')[1]) for l in open(os.path.join(reg_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 1 and np.isfinite(log[0])
