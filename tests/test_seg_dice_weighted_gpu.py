"""The weighted soft Dice on the device: the boundary-mask kernel (csrc/unet_pointwise.hip: seg_boundary_mask_kernel) bit for bit
against the integer rule, the weighted forms of the two fused head kernels against float64 autograd on the restatement of
tests/test_seg_dice_weighted_cpu.py (weighted_dice), the untouched unweighted path, deterministic mode, the argument limits,
UNet3D.loss_dice(class_weights=-1, boundary_weights=.5) on a whole network and training_segmentation() end to end.

Bounds of the kernel tests: the project's (tests/test_seg_training_gpu.py) -- 2e-5 of the reference's largest value for probs,
the loss and dbn, 2e-5 of max(that, 1e-2) for dw and db -- except where the same graph evaluated in float32 by torch on the CPU
is itself farther from float64 than a sixth of that: there the bound is 6 x the CPU's distance (dynamic weights of a one-voxel
class magnify rounding in a way the plain Dice never saw).  Every case prints both distances.
Measured on an MI355X over the 8 cases x 4 modes (device / fp32 CPU, absolute maxima): probs 6.9e-7 / 6.8e-7, loss 1.6e-7 /
1.6e-7, dbn 8.0e-9 / 8.0e-9 (on a scale of 1e-2), dw 2.5e-8 / 1.8e-8, db 1.1e-8 / 8.0e-9; the device used at most 5.3 % of a
bound, and the 6 x widening was needed by no case (the CPU's own distance never reached a sixth of the project bound).
The mask equalled the integer rule in all 20 cases."""
import functools
import os

import numpy as np
import pytest

from conftest import single_shot_parity
from test_seg_dice_weighted_cpu import SHAPE, BIG, HEADS, GEOMETRIES, label_case, weighted_dice, boundary_map, integer_mask

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, -12345.5
MASK_SENTINEL = -0x0123456789ABCDEF
BETA = 0.5
# every head on the small volume with d = 3, C = 24 / N = 33 on the big one, and the other two distances on one head
KERNEL_CASES = [(C, N, SHAPE, 3, i % 2 == 1) for i, (C, N) in enumerate(HEADS)] + \
               [(24, 33, BIG, 3, False), (24, 5, SHAPE, 1, True), (24, 5, SHAPE, 5, False)]
MODES = ('boundary', 'fixed', 'dynamic', 'dynamic+boundary')


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _dist(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return (a - b).abs().max().item()


def _bits(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint32).copy()


def _mode_kw(mode, N, d):
    """keywords of weighted_dice for one mode; the fixed weights are uneven and hold a zero"""
    kw = {}
    if 'boundary' in mode:
        kw.update(boundary_weights=BETA, boundary_dist=d)
    if 'dynamic' in mode:
        kw['class_weights'] = -1
    if mode == 'fixed':
        w = np.random.default_rng(N).uniform(.5, 2., N)
        w[1] = 0.
        kw['class_weights'] = tuple(w.tolist())
    return kw


def _head_graph(c, dtype, kw):
    """softmax(bn @ w + b) + the weighted Dice of one case in `dtype` under autograd: (probs, loss, dbn, dw, db)"""
    import torch
    from synthsr_amd import ops
    d = lambda t: t.detach().to(dtype).clone()   # (a copy: the case's tensors stay as they are)
    w, b = d(c['w']).requires_grad_(True), d(c['b']).requires_grad_(True)
    mean, var = d(c['stats'][:c['C']]), d(c['stats'][c['C']:])
    bn = ((d(c['x']) - mean) * torch.rsqrt(var + ops.BN_EPS) * d(c['gamma']) + d(c['beta'])).requires_grad_(True)
    probs = torch.softmax(bn @ w + b, -1)
    loss = weighted_dice(d(c['gt']), probs, **kw)
    loss.backward()
    return probs.detach(), loss.detach(), bn.grad.clone(), w.grad.clone(), b.grad.clone()


@functools.lru_cache(maxsize=None)
def _case(C, N, shape):
    """inputs (host) of one head configuration on the label map of label_case(N, shape); computed once, never modified"""
    import torch
    g = torch.Generator().manual_seed(1000 * C + N + shape[0])
    x = torch.randn(*shape, C, generator=g)
    mean, var = torch.randn(C, generator=g) * .1, torch.rand(C, generator=g) + .5
    gamma, beta = torch.rand(C, generator=g) + .5, torch.randn(C, generator=g) * .1
    w = torch.randn(C, N, generator=g) * .3
    b = torch.randn(N, generator=g) * .1
    c = dict(label_case(N, shape))
    c.update(C=C, x=x, stats=torch.cat([mean, var]), gamma=gamma, beta=beta, w=w, b=b)
    return c


@functools.lru_cache(maxsize=None)
def _refs(C, N, shape, d, mode):
    """float64 and float32-CPU results of one case and mode"""
    import torch
    c, kw = _case(C, N, shape), _mode_kw(mode, N, d)
    return _head_graph(c, torch.float64, kw), _head_graph(c, torch.float32, kw)


def _guarded(torch, numel, misalign=False, fill=SENTINEL, dtype=None):
    """a device buffer of `numel` elements with GUARD sentinels behind it (and one in front when misaligned)"""
    full = torch.full((numel + GUARD + 1,), SENTINEL if dtype is None else MASK_SENTINEL, device='cuda', dtype=dtype)
    o = 1 if misalign else 0
    view = full[o:o + numel]
    if fill != SENTINEL:
        view.fill_(fill)
    return full, view


def _guards_intact(full, n, misalign, sentinel=SENTINEL):
    o = 1 if misalign else 0
    return bool((full[o + n:] == sentinel).all()) and bool((full[:o] == sentinel).all())


def _device_mask(torch, c, d, skip=True, misalign=False):
    from synthsr_amd import ops
    nvox = int(np.prod(c['shape']))
    full, mask = _guarded(torch, nvox, misalign, dtype=torch.int64)
    ops.seg_boundary_mask(c['seg'].cuda(), c['lut'].cuda(), c['N'], d, skip, mask=mask)
    torch.cuda.synchronize()
    assert _guards_intact(full, nvox, misalign, MASK_SENTINEL), 'mask guard overwritten'
    return mask


def _class_weights(torch, sums, N, kw):
    """c [N] on the device, as UNet3D.loss_dice forms it"""
    cw = kw.get('class_weights')
    if cw is None:
        return torch.full((N,), 1.0 / N, device='cuda')
    if np.ndim(cw) == 0:
        vol = sums[2 * N:]
        inv = torch.where(vol > 0, 1.0 / vol.clamp_min(1e-30), torch.zeros_like(vol))
        return inv / inv.sum().clamp_min(1e-30)
    cw = np.asarray(cw, dtype=np.float64)
    return torch.tensor(cw / cw.sum(), dtype=torch.float32, device='cuda')


def _run(torch, c, kw, misalign=False, mask=None):
    """mask kernel + both weighted kernels on one case; returns (probs, loss, dbn, dw, db) and checks the guards"""
    from synthsr_amd import ops
    C, N = c['C'], c['N']
    nvox = int(np.prod(c['shape']))
    dev = lambda k: c[k].cuda()
    x, seg, lut = dev('x'), dev('seg').view(-1), dev('lut')
    bw = kw.get('boundary_weights', 0.)
    if bw and mask is None:
        mask = _device_mask(torch, c, kw['boundary_dist'], misalign=misalign)
    sums = torch.empty(3 * N, device='cuda')
    pfull, probs = _guarded(torch, nvox * N, misalign)
    ops.seg_head_dice_fwd(x, dev('stats'), dev('gamma'), dev('beta'), dev('w'), dev('b'), seg, lut, probs, sums, mask=mask,
                          boundary_weights=bw, class_weights=True)
    cw = _class_weights(torch, sums, N, kw)
    loss = (cw * (1.0 - (sums[:N] + 1e-7) / (sums[N:2 * N] + 1e-7))).sum()
    bfull, dbn = _guarded(torch, nvox * C, misalign)
    wfull, dw = _guarded(torch, C * N, misalign, fill=0.0)
    dfull, db = _guarded(torch, N, misalign, fill=0.0)
    ops.seg_head_dice_bwd(probs, seg, lut, x, dev('stats'), dev('gamma'), dev('beta'), dev('w'), sums, dbn, dw, db, mask=mask,
                          boundary_weights=bw, class_weights=cw)
    torch.cuda.synchronize()
    for nm, full, n in (('probs', pfull, nvox * N), ('dbn', bfull, nvox * C), ('dw', wfull, C * N), ('db', dfull, N)):
        assert _guards_intact(full, n, misalign), nm + ' guard overwritten'
    return probs.view(*c['shape'], N), loss, dbn.view(*c['shape'], C), dw.view(C, N), db


def _check(tag, got, ref, cpu):
    bad = []
    for nm, dev, r, o32 in zip(('probs', 'loss', 'dbn', 'dw', 'db'), got, ref, cpu):
        scale = r.abs().max().item()
        bound = 2e-5 * (max(scale, 1e-2) if nm in ('dw', 'db') else scale)
        d, o = _dist(dev, r), _dist(o32, r)
        if o > bound / 6:
            bound = 6 * o
        print('%-16s %-5s device-float64 %.3e  fp32 CPU-float64 %.3e  bound %.3e (scale %.3e)' % (tag, nm, d, o, bound, scale))
        if not d < bound:
            bad.append((nm, d, bound))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------- the mask kernel
@pytest.mark.parametrize('N', sorted({n for _, n in HEADS}))
@pytest.mark.parametrize('shape,d', GEOMETRIES)
def test_boundary_mask_equals_the_integer_rule_bit_for_bit(T, N, shape, d):
    """skip_background on and off, aligned and (one word in) behind a front sentinel; guards intact.  The integer rule is the
    float rule on these very maps: tests/test_seg_dice_weighted_cpu.py::test_integer_boundary_rule_is_the_float_rule"""
    c = label_case(N, shape)
    for skip, misalign in ((True, False), (False, True)):
        got = _device_mask(T, c, d, skip, misalign).cpu().numpy().view(np.uint64).reshape(shape)
        want = integer_mask(c['k'], N, d, skip)
        assert np.array_equal(got, want), '%d voxels differ' % int((got != want).sum())
        assert skip or N == 2 or (want >> np.uint64(N - 1)).any()   # the highest bit is in use
        if skip and N > 1:
            assert not (got & np.uint64(1)).any()


# ---------------------------------------------------------------------------------------------------- the fused kernels
@pytest.mark.parametrize('C,N,shape,d,misalign', KERNEL_CASES)
def test_weighted_head_kernels_vs_autograd(T, C, N, shape, d, misalign):
    """boundary weights alone, fixed class weights (uneven, one zero), dynamic weights (the absent class gets 0, the one-voxel
    class the largest weight), dynamic + boundary: probs, loss, dbn, dw, db against float64"""
    c = _case(C, N, shape)
    if N > 2:
        assert c['gt'][..., c['absent']].sum() == 0   # the dynamic-weight zero rule is exercised
    for mode in MODES:
        kw = _mode_kw(mode, N, d)
        ref, cpu = _refs(C, N, shape, d, mode)
        _check(mode, _run(T, c, kw, misalign), ref, cpu)


def test_unweighted_path_is_unchanged(T):
    """deterministic mode: ops.seg_head_dice_fwd / _bwd without mask and weights = the old entry points called directly, bit
    for bit; the new entry points with an all-zero mask, boundary weight .5 and c = 1 / N as well"""
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    prev = ops.set_deterministic(True)
    try:
        for C, N, shape in ((24, 33, BIG), (64, 64, SHAPE), (24, 5, SHAPE)):
            c = _case(C, N, shape)
            nvox = int(np.prod(shape))
            dev = lambda k: c[k].cuda()
            x, seg, lut, stats, gamma, beta, w, b = (dev(k) for k in ('x', 'seg', 'lut', 'stats', 'gamma', 'beta', 'w', 'b'))
            seg = seg.view(-1)
            outs = []
            for how in ('abi', 'ops', 'weighted'):
                rows = 3 if how == 'weighted' else 2
                probs, sums = torch.empty(nvox, N, device='cuda'), torch.zeros(rows * N, device='cuda')
                dbn, dw, db = torch.empty(nvox, C, device='cuda'), torch.zeros(C, N, device='cuda'), torch.zeros(N, device='cuda')
                if how == 'abi':
                    assert lib.synthsr_seg_head_dice_fwd(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                         ops.BN_EPS, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(seg), _lib.ptr(lut),
                                                         int(lut.numel()), _lib.ptr(probs), _lib.ptr(sums), _lib.stream()) == 0
                    assert lib.synthsr_seg_head_dice_bwd(_lib.ptr(probs), _lib.ptr(seg), _lib.ptr(lut), int(lut.numel()),
                                                         _lib.ptr(x), nvox, C, N, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                         ops.BN_EPS, _lib.ptr(w), _lib.ptr(sums), 1.0, _lib.ptr(dbn), _lib.ptr(dw),
                                                         _lib.ptr(db), _lib.stream()) == 0
                else:
                    kw = {}
                    if how == 'weighted':
                        kw = dict(mask=torch.zeros(nvox, dtype=torch.int64, device='cuda'), boundary_weights=BETA,
                                  class_weights=torch.full((N,), 1.0 / N, device='cuda'))
                    ops.seg_head_dice_fwd(x, stats, gamma, beta, w, b, seg, lut, probs, sums, **kw)
                    ops.seg_head_dice_bwd(probs, seg, lut, x, stats, gamma, beta, w, sums, dbn, dw, db, **kw)
                torch.cuda.synchronize()
                outs.append([_bits(t) for t in (probs, sums[:2 * N], dbn, dw, db)])
                if how == 'weighted':   # the third row with an all-zero mask: the plain class volumes
                    assert torch.equal(sums[2 * N:].cpu().double(), c['gt'].sum((0, 1, 2)))
            assert ops.deterministic_status() == 1, 'an ordered wait timed out'
            for how, other in zip(('ops', 'weighted'), outs[1:]):
                for nm, u, v in zip(('probs', 'sums', 'dbn', 'dw', 'db'), outs[0], other):
                    assert np.array_equal(u, v), '%s of the %s path differs from the old entry points (C %d, N %d)' % (nm, how, C, N)
    finally:
        ops.set_deterministic(prev)


def test_weighted_kernels_repeat_bit_for_bit_in_deterministic_mode(T):
    from synthsr_amd import ops
    c = _case(24, 33, BIG)
    kw = _mode_kw('dynamic+boundary', 33, 3)
    prev = ops.set_deterministic(True)
    try:
        a = [_bits(t) for t in _run(T, c, kw)]
        b = [_bits(t) for t in _run(T, c, kw)]
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
    finally:
        ops.set_deterministic(prev)
    for nm, u, v in zip(('probs', 'loss', 'dbn', 'dw', 'db'), a, b):
        assert np.array_equal(u, v), nm + ' differs between two deterministic runs'


def test_weighted_limits_are_refused(T):
    """C = 68, C = 6, N = 65 (head functions; N = 65 the mask function as well) and boundary_dist 0 and 6 return the
    invalid-argument error and leave sentinel-filled outputs untouched"""
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    nvox = int(np.prod(SHAPE))
    seg, lut = torch.zeros(nvox, dtype=torch.int32).cuda(), torch.zeros(4, dtype=torch.int32).cuda()
    for N, d in ((65, 3), (5, 0), (5, 6)):
        mask = torch.full((nvox,), MASK_SENTINEL, dtype=torch.int64).cuda()
        assert lib.synthsr_seg_boundary_mask(_lib.ptr(seg), _lib.i3(SHAPE), _lib.ptr(lut), 4, N, d, 1, _lib.ptr(mask),
                                             _lib.stream()) == -1
        with pytest.raises(ValueError):
            ops.seg_boundary_mask(seg.view(SHAPE), lut, N, d, mask=mask)
        torch.cuda.synchronize()
        assert bool((mask == MASK_SENTINEL).all())
    mask = torch.zeros(nvox, dtype=torch.int64).cuda()
    for C, N in ((68, 5), (6, 5), (24, 65)):
        x = torch.randn(*SHAPE, C).cuda()
        stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
        gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
        w, b, cw = torch.randn(C, N).cuda(), torch.zeros(N).cuda(), torch.full((N,), 1.0 / N).cuda()
        probs, sums = torch.full((nvox * N,), SENTINEL).cuda(), torch.full((3 * N,), SENTINEL).cuda()
        dbn, dw, db = torch.full((nvox * C,), SENTINEL).cuda(), torch.full((C * N,), SENTINEL).cuda(), torch.full((N,), SENTINEL).cuda()
        rc = lib.synthsr_seg_head_dice_fwd_weighted(_lib.ptr(x), nvox, C, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
                                                    ops.BN_EPS, _lib.ptr(w), _lib.ptr(b), N, _lib.ptr(seg), _lib.ptr(lut), 4,
                                                    _lib.ptr(mask), BETA, _lib.ptr(probs), _lib.ptr(sums), _lib.stream())
        assert rc == -1   # SYNTHSR_EINVAL
        rc = lib.synthsr_seg_head_dice_bwd_weighted(_lib.ptr(probs), _lib.ptr(seg), _lib.ptr(lut), 4, _lib.ptr(x), nvox, C, N,
                                                    _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), ops.BN_EPS, _lib.ptr(w),
                                                    _lib.ptr(sums), _lib.ptr(mask), BETA, _lib.ptr(cw), 1.0, _lib.ptr(dbn),
                                                    _lib.ptr(dw), _lib.ptr(db), _lib.stream())
        assert rc == -1
        with pytest.raises(ValueError):
            ops.seg_head_dice_fwd(x, stats, gamma, beta, w, b, seg, lut, probs, sums.clone(), mask=mask, boundary_weights=BETA)
        with pytest.raises(ValueError):
            ops.seg_head_dice_bwd(probs, seg, lut, x, stats, gamma, beta, w, sums, dbn, dw, db, mask=mask, class_weights=cw)
        torch.cuda.synchronize()
        for t in (probs, sums, dbn, dw, db):
            assert bool((t == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- whole network
NET_KW = dict(class_weights=-1, boundary_weights=BETA, boundary_dist=2)


@functools.lru_cache(maxsize=None)
def _net_inputs():
    """the image of tests/test_seg_training_gpu.py with a label map of 4^3-voxel blocks of its label values (3 and 42 are not
    in the head's list; 42 lies beyond the table)"""
    import torch
    from test_seg_training_gpu import _net_inputs as plain_inputs, NET_SHAPE, N_SEG
    x, _, lut, _ = plain_inputs()
    g = torch.Generator().manual_seed(33)
    values = torch.tensor([0, 14, 2, 41, 17, 3, 42], dtype=torch.int32)
    blocks = values[torch.randint(0, len(values), (4, 4, 4), generator=g)]
    seg = blocks.repeat_interleave(4, 0).repeat_interleave(4, 1).repeat_interleave(4, 2).contiguous()
    k = torch.where(seg < len(lut), lut[seg.clamp(max=len(lut) - 1).long()], torch.full_like(seg, -1))
    gt = torch.zeros(*NET_SHAPE, N_SEG, dtype=torch.float64)
    for n in range(N_SEG):
        gt[..., n] = (k == n).double()
    wmap = 1 + BETA * boundary_map(gt, NET_KW['boundary_dist'], True)
    assert 0 < int((wmap > 1).sum()) < wmap.numel() // 2
    return x, seg, lut, gt, wmap


def test_unet_weighted_dice_loss_and_gradients_vs_autograd(T):
    """one loss_dice(class_weights=-1, boundary_weights=.5, boundary_dist=2) + backward() of the whole network against the
    oracle with the weighted loss: the loss, every BatchNorm batch statistic, every gradient by the float64-anchored rule"""
    torch = T
    from oracle import unet_ref as U
    from test_seg_training_gpu import _seg_net, LEVELS, N_SEG
    x, seg, lut, gt, wmap = _net_inputs()

    def run():
        net = _seg_net(torch)
        loss = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda(), **NET_KW)
        net.test_loss = loss.clone()
        net.backward()
        # d(loss)/d(posteriors), what single_shot_parity reads as the loss derivative, from what the step kept
        st = net._loss_state
        assert st.kind == 'dice'
        probs, sums, mask, bw, c = st.probs, st.sums, st.mask, st.boundary_weights, st.class_weights
        assert mask is not None and bw == BETA
        Tn, Bn = sums[:N_SEG] + 1e-7, sums[N_SEG:2 * N_SEG] + 1e-7
        g = -c * wmap.float().cuda().view(-1, N_SEG) * (2 * gt.float().cuda().view(-1, N_SEG) * Bn - 2 * probs * Tn) / (Bn * Bn)
        net.dpred = g.reshape(-1)
        net.test_stats = net.bn_batch.clone()
        return net

    def oracle(net, nudge):
        P = {nm: v.detach().cpu().clone().requires_grad_(True) for nm, v in net.named_parameters()}
        stats, pin = {}, []
        pr = U.unet_forward(x, P, net.prefix, LEVELS, 2, training=True, softmax=True, collect=stats, pool_inputs=pin,
                            pool_nudge=nudge)
        if U._PRED_TAP is not None:   # (unet_forward taps linear heads only)
            pr = U._PRED_TAP(pr)
        lr = weighted_dice(gt.to(pr.dtype), pr.reshape(gt.shape), **NET_KW)
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


def test_default_loss_dice_is_the_step_it_was(T):
    """loss_dice() with the new parameters at their defaults keeps the record of the plain step and its loss bit for bit
    (deterministic mode), and a weighted call in between does not disturb the next plain one"""
    torch = T
    from synthsr_amd import ops
    from test_seg_training_gpu import _seg_net
    x, seg, lut, _, _ = _net_inputs()
    prev = ops.set_deterministic(True)
    try:
        net = _seg_net(torch)
        a = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda()).clone()
        st = net._loss_state
        assert st.kind == 'dice' and st.mask is None and st.class_weights is None
        net.backward()
        ga = net.grads.clone()
        w = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda(), **NET_KW).clone()
        net.backward()
        b = net.loss_dice(x.cuda(), seg.cuda(), lut.cuda(), None, 0., 3, True).clone()
        net.backward()
        assert torch.equal(a, b) and torch.equal(ga, net.grads) and not torch.equal(a, w)
    finally:
        ops.set_deterministic(prev)


# ---------------------------------------------------------------------------------------------------- end to end
def test_training_segmentation_with_weights_end_to_end(tmp_path):
    """20 steps on a fixed sample with dynamic class weights and boundary weights lower the loss; the checkpoint is written
    and loads into SegmentationPredictor"""
    from synthsr_amd.segmentation_training import training_segmentation
    from synthsr_amd.predict_segmentation import SegmentationPredictor
    from test_seg_training_gpu import _write_inputs
    labels_dir, seg_labels = _write_inputs(tmp_path)
    rec = []
    model_dir = str(tmp_path / 'model')
    net = training_segmentation(labels_dir, model_dir, str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'), str(tmp_path / 'gl.npy'),
                                str(tmp_path / 'sl.npy'), path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32,
                                n_levels=3, unet_feat_count=24, nonlin_shape_factor=.125, bias_shape_factor=.125, lr=1e-3,
                                verbose=False, deterministic=True, epochs=2, steps_per_epoch=10, fixed_sample=True,
                                step_losses=rec, dice_class_weights=-1, dice_boundary_weights=.5)
    assert net._loss_state.kind == 'dice' and net._loss_state.mask is not None
    assert len(rec) == 20 and np.isfinite(rec).all() and rec[19] < rec[0], (rec[0], rec[19])
    ckpt = os.path.join(model_dir, '002.npz')
    assert os.path.exists(ckpt)
    pred = SegmentationPredictor(ckpt, seg_labels, n_levels=3, unet_feat_count=24)
    out = pred.segment_volume(np.random.default_rng(0).random((32, 32, 32)), flipping=False)
    assert out.shape == (32, 32, 32) and set(np.unique(out).tolist()) <= set(np.asarray(seg_labels).tolist())
