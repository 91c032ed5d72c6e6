"""A frozen or inference softmax-headed U-Net in bf16: the four _bf16 entry points of csrc/unet_pointwise.hip alone
(synthsr_seg_head_fwd_bf16, _seg_head_argmax_bf16, _seg_head_tta_argmax_bf16, _seg_dice_bwd_bf16), then predict_probs /
predict_labels / backward_input of a whole bf16 network, SegmentationRegulariser on one, and training(segnet_dtype='bf16') /
predict_segmentation(dtype='bf16') end to end.

Kernels.  The feature map is rounded to bf16 on the host and the reference is float64 on x.bfloat16().double(): the device
arithmetic is fp32 on exactly representable inputs, so the fp32 bounds of tests/test_seg_training_gpu.py (posteriors: 2e-5
relative) and the gap rule of tests/test_seg_predict_gpu.py (labels compared where the float64 top-two gap exceeds 1e-4
max|logit|, 1e-5 for averaged posteriors; at most 1 % of the voxels left out, no mismatch outside the gap) apply unchanged.
seg_dice_bwd with a bf16 dbn: |d - ref| <= 2^-8 |ref| + 2e-5 max|ref| -- one round-to-nearest is 2^-9 relative (a factor of
two allowed), the second term is the fp32 kernel's own bound.
FAR = (17, 64, 64) = 69 632 voxels is more than head_grid() x 64 = 65 536: a workgroup takes a second tile.

Whole networks: see the docstrings of the tests for the measured distances the bounds come from."""
import functools
import importlib.util
import os

import numpy as np
import pytest

import test_seg_predict_gpu as P
from test_seg_predict_gpu import SHAPE, EVEN, BIG, SENTINEL, ISENTINEL, _guarded, _guards_intact, _compare_labels, _logits, \
    _top_two_gap
from test_seg_training_gpu import NET_SHAPE, LEVELS, SEG_LABELS, _write_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = (17, 64, 64)           # 69 632 voxels = 1088 tiles > the 1024 workgroups of head_grid(): 64 workgroups take a second tile
# (C, N, shape, misaligned outputs): every C of {8, 24, 64} and every N of {2, 5, 19, 33, 64} on SHAPE, 132 tiles, FAR
CASES = [(8, 2, SHAPE, False), (8, 19, SHAPE, True), (24, 5, SHAPE, False), (24, 33, SHAPE, True), (64, 64, SHAPE, False),
         (64, 19, SHAPE, True), (24, 64, SHAPE, True), (64, 33, SHAPE, False), (24, 33, BIG, False), (24, 5, FAR, False),
         (8, 33, FAR, True)]
TTA_CASES = [(24, 33, SHAPE, ((3, 17), (4, 30), (0, 32)), True), (24, 33, EVEN, ((3, 17), (4, 30), (0, 32)), False),
             (8, 2, SHAPE, (), False), (8, 2, EVEN, (), True), (24, 5, FAR, ((1, 3),), False)]


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _bf16_exact(x):
    """x rounded to bf16 on the host: (the bf16 tensor the device reads, the same values as float32 for the references)"""
    import torch
    xb = x.to(torch.bfloat16)
    return xb, xb.float()


@functools.lru_cache(maxsize=None)
def _case(C, N, shape):
    """the inputs of test_seg_predict_gpu._head_inputs with x rounded to bf16; float64 logits, posteriors, argmax, the voxels
    the gap rule compares and the float32-CPU argmax; never modified"""
    import torch
    c, _ = P._head_inputs(C, N, shape, 1000 * C + N + shape[0])
    c['xb'], c['x'] = _bf16_exact(c['x'])
    l64 = _logits(c, torch.float64)
    c['probs'] = torch.softmax(l64, -1)
    c['probs32'] = torch.softmax(_logits(c, torch.float32), -1)
    c['ref'] = l64.argmax(-1)
    c['sure'] = _top_two_gap(l64) > 1e-4 * l64.abs().max().item()
    c['cpu32'] = _logits(c, torch.float32).argmax(-1)
    return c


def _head(c):
    return [c[k].cuda() for k in ('xb', 'stats', 'gamma', 'beta', 'w', 'b')]


# ---------------------------------------------------------------------------------------------------- posteriors
@pytest.mark.parametrize('C,N,shape,misalign', CASES)
def test_seg_head_fwd_bf16_vs_float64(T, C, N, shape, misalign):
    torch = T
    from synthsr_amd import ops
    c = _case(C, N, shape)
    nvox = int(np.prod(shape))
    full, probs = _guarded(torch, nvox * N, misalign)
    ops.seg_head_fwd(*_head(c), probs.view(nvox, N))
    torch.cuda.synchronize()
    assert _guards_intact(full, nvox * N, misalign), 'guard overwritten'
    scale = c['probs'].abs().max().item()
    d = (probs.cpu().double().reshape(c['probs'].shape) - c['probs']).abs().max().item()
    d32 = (c['probs32'].double() - c['probs']).abs().max().item()
    print('posteriors C=%d N=%d %s: device-float64 %.3e  fp32 CPU-float64 %.3e  bound %.3e' % (C, N, shape, d, d32, 2e-5 * scale))
    assert d < 2e-5 * scale


# ---------------------------------------------------------------------------------------------------- label maps
@pytest.mark.parametrize('C,N,shape,misalign', CASES)
def test_seg_head_argmax_bf16_vs_float64(T, C, N, shape, misalign):
    torch = T
    from synthsr_amd import ops
    c = _case(C, N, shape)
    nvox = int(np.prod(shape))
    full, out = _guarded(torch, nvox, misalign, torch.int32, ISENTINEL)
    ops.seg_head_argmax(*_head(c), c['labels'].cuda(), out)
    torch.cuda.synchronize()
    assert _guards_intact(full, nvox, misalign, ISENTINEL), 'guard overwritten'
    _compare_labels('argmax bf16 C=%d N=%d %s' % (C, N, shape), out, c)


@functools.lru_cache(maxsize=None)
def _tta_case(C, N, shape, pairs):
    """test_seg_predict_gpu._tta_case with the flipped pass's x rounded to bf16 (prev stays float32)"""
    import torch
    c, g = P._head_inputs(C, N, shape, 2000 * C + N + shape[0])
    perm = torch.arange(N)
    for i, j in pairs:
        perm[i], perm[j] = j, i
    x0 = torch.randn(*shape, C, generator=g)
    c['prev'] = torch.softmax(_logits(c, torch.float64, x0), -1).float()
    c['xb'], c['x'] = _bf16_exact(c['x'])
    c['perm'] = perm.to(torch.int32)

    def average(dtype):
        q = torch.softmax(_logits(c, dtype), -1)
        return 0.5 * (torch.flip(q, dims=[0])[..., perm] + c['prev'].to(dtype))
    c['avg'] = average(torch.float64)
    c['ref'] = c['avg'].argmax(-1)
    c['sure'] = _top_two_gap(c['avg']) > 1e-5
    c['avg32'] = average(torch.float32)
    c['cpu32'] = c['avg32'].argmax(-1)
    return c


@pytest.mark.parametrize('C,N,shape,pairs,misalign', TTA_CASES)
def test_seg_head_tta_argmax_bf16_vs_float64(T, C, N, shape, pairs, misalign):
    torch = T
    from synthsr_amd import ops
    c = _tta_case(C, N, shape, pairs)
    nvox = int(np.prod(shape))
    head = _head(c) + [c['labels'].cuda()]
    prev, perm = c['prev'].reshape(nvox, N).cuda(), c['perm'].cuda()
    ofull, out = _guarded(torch, nvox, misalign, torch.int32, ISENTINEL)
    pfull, probs = _guarded(torch, nvox * N, misalign)
    ops.seg_head_tta_argmax(*head, prev, perm, out, probs)
    torch.cuda.synchronize()
    assert _guards_intact(ofull, nvox, misalign, ISENTINEL) and _guards_intact(pfull, nvox * N, misalign), 'guard overwritten'
    assert torch.equal(prev.cpu(), c['prev'].reshape(nvox, N)), 'prev was written'
    scale = c['avg'].abs().max().item()
    d = (probs.cpu().double().reshape(c['avg'].shape) - c['avg']).abs().max().item()
    d32 = (c['avg32'].double() - c['avg']).abs().max().item()
    print('averaged posteriors: device-float64 %.3e  fp32 CPU-float64 %.3e  bound %.3e' % (d, d32, 2e-5 * scale))
    assert d < 2e-5 * scale
    _compare_labels('tta bf16 C=%d N=%d %s' % (C, N, shape), out, c)
    # without probs_out: the same label map, and the posteriors' buffer keeps its sentinels
    ofull2, out2 = _guarded(torch, nvox, misalign, torch.int32, ISENTINEL)
    pfull.fill_(SENTINEL)
    ops.seg_head_tta_argmax(*head, prev, perm, out2, None)
    torch.cuda.synchronize()
    assert bool((pfull == SENTINEL).all()) and _guards_intact(ofull2, nvox, misalign, ISENTINEL)
    assert torch.equal(out2, out)
    # prev and probs_out sharing memory stay refused
    with pytest.raises(ValueError):
        ops.seg_head_tta_argmax(*head, prev, perm, out2, prev)


def test_exact_ties_go_to_the_lowest_channel_bf16(T):
    """the construction of test_seg_predict_gpu.test_exact_ties_go_to_the_lowest_channel on a bf16 x: channels 7 and 20 share
    their column and their bias (100.0: representable), equal logits bit for bit, channel 7 wins everywhere, in the averaged
    posteriors of the flip pass as well"""
    torch = T
    from synthsr_amd import ops
    c = dict(_case(24, 33, SHAPE))
    w, b = c['w'].clone(), c['b'].clone()
    w[:, 20] = w[:, 7]
    b[7] = b[20] = 100.0
    c['w'], c['b'] = w, b
    l64 = _logits(c, torch.float64)
    assert bool((l64[..., 7] == l64[..., 20]).all()) and bool((l64.argmax(-1) == 7).all())
    nvox = int(np.prod(SHAPE))
    out = torch.full((nvox,), ISENTINEL, dtype=torch.int32, device='cuda')
    head = _head(c) + [c['labels'].cuda()]
    ops.seg_head_argmax(*head, out)
    assert bool((out == int(c['labels'][7])).all())
    prev = torch.softmax(l64, -1).float().reshape(nvox, 33).cuda()
    out.fill_(ISENTINEL)
    ops.seg_head_tta_argmax(*head, prev, torch.arange(33, dtype=torch.int32).cuda(), out)
    assert bool((out == int(c['labels'][7])).all())


# ---------------------------------------------------------------------------------------------------- regulariser backward
@functools.lru_cache(maxsize=None)
def _dice_bwd_case(C, N, shape):
    """float32 posteriors, a label map, K merged classes (class k = labels k and, where it exists, k + K) and the float64
    gradient of scale * mean_k(1 - (T_k + e) / (B_k + e)) w.r.t. the BatchNorm output, by the algebra of seg_dice_bwd_kernel"""
    import torch
    g = torch.Generator().manual_seed(3000 * C + N + shape[0])
    nvox = int(np.prod(shape))
    K = max(1, (N + 1) // 2 - 1)                     # some labels belong to no class
    probs = torch.softmax(torch.randn(nvox, N, generator=g) * 2, -1)
    w = torch.randn(C, N, generator=g) * .3
    idx = torch.full((K, 3), -1, dtype=torch.int32)
    idx[:, 0] = torch.arange(K, dtype=torch.int32)
    second = torch.arange(K) + K
    idx[second < N, 1] = second[second < N].to(torch.int32)
    gt_values = (torch.randperm(K + 4, generator=g)[:K]).to(torch.int32)
    seg = torch.randint(0, K + 4, (nvox,), generator=g, dtype=torch.int32)
    scale = 0.25
    p = probs.double()
    pred = torch.zeros(nvox, K, dtype=torch.float64)
    member = torch.zeros(K, N, dtype=torch.float64)
    for k in range(K):
        for j in idx[k].tolist():
            if j >= 0:
                pred[:, k] += p[:, j]
                member[k, j] = 1.0
    gt = (seg[:, None] == gt_values[None, :]).double()
    sums = torch.cat([(2 * gt * pred).sum(0), (gt + pred * pred).sum(0)])
    Tk, Bk = sums[:K] + 1e-7, sums[K:] + 1e-7
    dpred = -scale / K * (2 * gt * Bk - 2 * pred * Tk) / (Bk * Bk)
    S = (dpred * pred).sum(1, keepdim=True)
    dlogit = p * (dpred @ member - S)
    return dict(C=C, N=N, K=K, probs=probs, w=w, idx=idx.reshape(-1), gt=gt_values, seg=seg, sums=sums.float(), scale=scale,
                ref=dlogit @ w.double().t())


@pytest.mark.parametrize('C,N,shape,misalign', [(24, 5, SHAPE, False), (8, 19, SHAPE, True), (24, 33, BIG, False),
                                                (64, 64, SHAPE, True), (64, 5, SHAPE, False)])
def test_seg_dice_bwd_bf16_vs_float64(T, C, N, shape, misalign):
    torch = T
    from synthsr_amd import ops
    c = _dice_bwd_case(C, N, shape)
    nvox = int(np.prod(shape))
    dev = lambda k: c[k].cuda()
    full, dbn = _guarded(torch, nvox * C, misalign, torch.bfloat16)
    ops.seg_dice_bwd(dev('probs'), dev('seg'), dev('w'), dev('idx'), dev('gt'), dev('sums'), c['scale'], dbn.view(nvox, C))
    f32full, dbn32 = _guarded(torch, nvox * C, misalign)
    ops.seg_dice_bwd(dev('probs'), dev('seg'), dev('w'), dev('idx'), dev('gt'), dev('sums'), c['scale'], dbn32.view(nvox, C))
    torch.cuda.synchronize()
    assert _guards_intact(full, nvox * C, misalign) and _guards_intact(f32full, nvox * C, misalign), 'guard overwritten'
    ref = c['ref']
    top = ref.abs().max().item()
    err = (dbn.cpu().double().view(nvox, C) - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + 2e-5 * top
    e32 = (dbn32.cpu().double().view(nvox, C) - ref).abs().max().item()
    print('dice_bwd C=%d N=%d K=%d: bf16 worst error / bound %.3f, max error %.3e (max|ref| %.3e); fp32 kernel %.3e, its bound %.3e'
          % (C, N, c['K'], (err / bound).max().item(), err.max().item(), top, e32, 2e-5 * top))
    assert e32 < 2e-5 * top
    assert bool((err <= bound).all())
    # what was written is the fp32 kernel's result rounded to nearest even
    assert torch.equal(dbn, dbn32.to(torch.bfloat16))


# ---------------------------------------------------------------------------------------------------- limits
def test_limits_and_mixed_dtypes_are_refused(T):
    """C = 68, C = 6, N = 65 and an x pointer off its 8-byte alignment return -1 from the four entry points and raise
    ValueError from ops; sentinel-filled outputs stay untouched.  Mixed dtypes raise ValueError from ops."""
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    nvox = int(np.prod(SHAPE))
    P_ = _lib.ptr
    for C, N, off in ((68, 5, 0), (6, 5, 0), (24, 65, 0), (24, 5, 1), (24, 5, 2)):
        xfull = torch.randn(nvox * C + 4).to(torch.bfloat16).cuda()
        x = xfull[off:off + nvox * C].view(*SHAPE, C)
        assert x.data_ptr() % 8 == 2 * off
        stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
        gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
        w, b = torch.randn(C, N).cuda(), torch.zeros(N).cuda()
        labels = torch.arange(N, dtype=torch.int32).cuda()
        perm = torch.arange(N, dtype=torch.int32).cuda()
        prev = torch.full((nvox, N), 1.0 / N).cuda()
        out = torch.full((nvox,), ISENTINEL, dtype=torch.int32).cuda()
        probs = torch.full((nvox, N), SENTINEL).cuda()
        bn = (ops.BN_EPS,)
        assert lib.synthsr_seg_head_fwd_bf16(P_(x), nvox, C, P_(stats), P_(gamma), P_(beta), *bn, P_(w), P_(b), N, P_(probs),
                                             _lib.stream()) == -1
        assert lib.synthsr_seg_head_argmax_bf16(P_(x), nvox, C, P_(stats), P_(gamma), P_(beta), *bn, P_(w), P_(b), N, P_(labels),
                                                P_(out), _lib.stream()) == -1
        assert lib.synthsr_seg_head_tta_argmax_bf16(P_(x), _lib.i3(SHAPE), C, P_(stats), P_(gamma), P_(beta), *bn, P_(w), P_(b), N,
                                                    P_(labels), P_(prev), P_(perm), P_(out), P_(probs), _lib.stream()) == -1
        with pytest.raises(ValueError):
            ops.seg_head_fwd(x, stats, gamma, beta, w, b, probs)
        with pytest.raises(ValueError):
            ops.seg_head_argmax(x, stats, gamma, beta, w, b, labels, out)
        with pytest.raises(ValueError):
            ops.seg_head_tta_argmax(x, stats, gamma, beta, w, b, labels, prev, perm, out, probs)
        if off == 0:   # seg_dice_bwd has no x; its limits are C and N
            dbn = torch.full((nvox, C), SENTINEL).to(torch.bfloat16).cuda()
            idx, gt = torch.tensor([0, 1, -1], dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
            seg, sums = torch.zeros(nvox, dtype=torch.int32).cuda(), torch.ones(2).cuda()
            if C > 64 or N > 64:
                assert lib.synthsr_seg_dice_bwd_bf16(P_(probs), P_(seg), nvox, C, N, P_(w), P_(idx), P_(gt), 1, P_(sums), 1.0,
                                                     P_(dbn), _lib.stream()) == -1
                with pytest.raises(ValueError):
                    ops.seg_dice_bwd(probs, seg, w, idx, gt, sums, 1.0, dbn)
                assert bool((dbn == dbn.flatten()[0]).all()) and float(dbn.flatten()[0]) == float(torch.tensor(SENTINEL).bfloat16())
        torch.cuda.synchronize()
        assert bool((out == ISENTINEL).all()) and bool((probs == SENTINEL).all())
    # mixed dtypes
    C, N = 24, 5
    xb = torch.randn(*SHAPE, C).to(torch.bfloat16).cuda()
    stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
    w, b = torch.randn(C, N).cuda(), torch.zeros(N).cuda()
    labels = torch.arange(N, dtype=torch.int32).cuda()
    perm = torch.arange(N, dtype=torch.int32).cuda()
    probs = torch.full((nvox, N), SENTINEL).cuda()
    out = torch.full((nvox,), ISENTINEL, dtype=torch.int32).cuda()
    idx, gt = torch.tensor([0, 1, -1], dtype=torch.int32).cuda(), torch.zeros(1, dtype=torch.int32).cuda()
    seg, sums = torch.zeros(nvox, dtype=torch.int32).cuda(), torch.ones(2).cuda()
    h = torch.bfloat16
    with pytest.raises(ValueError):
        ops.seg_head_fwd(xb, stats, gamma, beta, w, b, probs.to(h))                      # bf16 posteriors
    with pytest.raises(ValueError):
        ops.seg_head_fwd(xb, stats, gamma, beta, w.to(h), b, probs)                      # bf16 head
    with pytest.raises(ValueError):
        ops.seg_head_fwd(xb.to(torch.float16), stats, gamma, beta, w, b, probs)          # neither float32 nor bfloat16
    with pytest.raises(ValueError):
        ops.seg_head_argmax(xb, stats, gamma.to(h), beta, w, b, labels, out)
    with pytest.raises(ValueError):
        ops.seg_head_tta_argmax(xb, stats, gamma, beta, w, b, labels, probs.to(h), perm, out)   # bf16 prev
    with pytest.raises(ValueError):
        ops.seg_dice_bwd(probs.to(h), seg, w, idx, gt, sums, 1.0, torch.zeros(nvox, C, dtype=h).cuda())   # bf16 posteriors
    with pytest.raises(ValueError):
        ops.seg_dice_bwd(probs, seg, w, idx, gt, sums, 1.0, torch.zeros(nvox, C, dtype=torch.float16).cuda())
    torch.cuda.synchronize()
    assert bool((out == ISENTINEL).all()) and bool((probs == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------- whole networks
FEATS = 24
HEAD_SCALE = 4.0     # the head's weights are scaled so that the fp32 network is decided at most voxels (see _net_case)
# the posterior bound: twice the measured maximum against the bf16-storage oracle, rounded up to one digit (bf16 rounding
# flips are discrete events that differ between machines and summation orders); measured values in the docstring of
# test_predict_probs_bf16_vs_fp32_net_and_bf16_oracle
EPS = {'inference': 8e-2, 'batch': 2e-1}


@functools.lru_cache(maxsize=None)
def _net_case(head_scale=HEAD_SCALE):
    """random weights and moving statistics of the 16^3, 3-level, 24-feature, 5-label network (host), an input volume, and
    the oracle with bf16 storage (oracle.unet_ref.unet_forward(quant=round_bf16)) in both BatchNorm modes"""
    import torch
    from oracle import unet_ref as U
    from synthsr_amd.unet import UNet3D
    table = UNet3D(FEATS, list(NET_SHAPE) + [1], LEVELS, 3, len(SEG_LABELS), feat_mult=2, nb_conv_per_level=2, batch_norm=-1,
                   final_pred_activation='softmax', table_only=True)
    g = torch.Generator().manual_seed(41)
    sd = {}
    for nm, shp, kind in table.specs:
        if kind in ('kernel', 'head_w'):
            fan = int(np.prod(shp[:-1]))
            sd[nm] = torch.randn(*shp, generator=g) * (1.5 / np.sqrt(fan)) * (head_scale if kind == 'head_w' else 1.0)
        elif kind == 'gamma':
            sd[nm] = torch.rand(*shp, generator=g) + .5
        else:
            sd[nm] = torch.randn(*shp, generator=g) * .1
    for bn in table.bn_layers:
        sd[bn['name'] + '/moving_mean'] = torch.randn(bn['C'], generator=g) * .2
        sd[bn['name'] + '/moving_variance'] = torch.rand(bn['C'], generator=g) * 1.5 + .5
    x = torch.rand(*NET_SHAPE, 1, generator=g)
    Pm = {k: v for k, v in sd.items() if 'moving_' not in k}
    moving = {k: v for k, v in sd.items() if 'moving_' in k}
    out = dict(sd=sd, x=x, labels=torch.from_numpy(SEG_LABELS).to(torch.int32), prefix=table.prefix)
    with torch.no_grad():   # (float32: round_bf16 hands float32 back, as in tests/test_bf16_gpu.py)
        out['inference'] = U.unet_forward(x, Pm, table.prefix, LEVELS, 2, training=False, moving=moving, softmax=True,
                                          quant=U.round_bf16)
        out['batch'] = U.unet_forward(x, Pm, table.prefix, LEVELS, 2, training=True, softmax=True, quant=U.round_bf16)
    return out


def _net(c, dtype):
    from synthsr_amd.unet import unet
    net = unet(nb_features=FEATS, input_shape=list(NET_SHAPE) + [1], nb_levels=LEVELS, conv_size=3, nb_labels=len(SEG_LABELS),
               feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax', seed=2, dtype=dtype)
    net.load_state_dict(c['sd'], strict=True)
    net.repack()
    net.training = False
    return net


def posterior_distances(c):
    """{mode: (bf16 device - fp32 device, bf16 device - bf16 oracle, fp32 posteriors)}, max over voxels and labels"""
    x = c['x'].cuda()
    n32, n16 = _net(c, 'f32'), _net(c, 'bf16')
    out = {}
    for mode in ('inference', 'batch'):
        p32 = n32.predict_probs(x, batch_stats=mode == 'batch').clone()
        p16 = n16.predict_probs(x, batch_stats=mode == 'batch').clone()
        assert p16.dtype == p32.dtype and p16.shape == p32.shape
        a = (p16 - p32).abs().max().item()
        b = (p16.cpu().double().view(*NET_SHAPE, -1) - c[mode]).abs().max().item()
        out[mode] = (a, b, p32)
    return out


def test_predict_probs_bf16_vs_fp32_net_and_bf16_oracle(T):
    """posteriors of the bf16 network in both BatchNorm modes against (a) the fp32 device network and (b) the oracle with
    bf16 storage.  Measured on an MI355X, maximum over voxels and labels, head weights scaled by HEAD_SCALE = 4:
      inference BatchNorm: bf16 - fp32 device 7.091e-02, bf16 - oracle 3.523e-02  ->  eps = 2 x 3.523e-02 -> 8e-2
      batch BatchNorm:     bf16 - fp32 device 1.133e-01, bf16 - oracle 5.036e-02  ->  eps = 2 x 5.036e-02 -> 2e-1
    (head scale 1: 1.763e-02 / 1.017e-02 and 2.715e-02 / 1.489e-02; the distance grows with the head's scale, the share of
    voxels whose fp32 top-two gap is within 4 x the oracle distance falls from 15 % to 11 %)"""
    c = _net_case()
    for mode, (a, b, _) in posterior_distances(c).items():
        print('posteriors, %s BatchNorm: bf16 - fp32 device %.3e   bf16 - bf16-storage oracle %.3e   bound %.1e' % (mode, a, b, EPS[mode]))
        assert b <= EPS[mode]


def _undecided(p32, eps):
    top = p32.topk(2, dim=-1).values
    return (top[..., 0] - top[..., 1]) <= 2 * eps


def test_predict_labels_and_segment_volume_bf16_vs_fp32(T):
    """predict_labels (plain, and the flip pass with prev) and SegmentationPredictor.segment_volume(flipping=True) of the bf16
    network against the fp32 one: posteriors within eps can change a label only where the fp32 top-two posterior gap is
    <= 2 eps; labels are equal everywhere else, and the rule leaves out at most 20 % of the voxels.  The flip average runs on
    the same weights with every conv kernel made symmetric along the first axis and no left-right pairs: the network then
    commutes with the flip, as a trained one does approximately, and the fp32 average is as decided as the single pass (with
    the unsymmetric random network the two passes disagree at half of the voxels and their average is a near tie there: 2198
    of 4096 voxels left out, measured)."""
    torch = T
    from synthsr_amd.predict_segmentation import SegmentationPredictor
    c = _net_case()
    eps = EPS['inference']
    x, labels = c['x'].cuda(), c['labels'].cuda()
    n32, n16 = _net(c, 'f32'), _net(c, 'bf16')
    p32 = n32.predict_probs(x).clone()
    out = _undecided(p32, eps).view(NET_SHAPE)
    l32, l16 = n32.predict_labels(x, labels).clone(), n16.predict_labels(x, labels).clone()
    assert l16.dtype == torch.int32 and tuple(l16.shape) == NET_SHAPE
    assert len(torch.unique(l32)) >= 3, 'a network that predicts one label everywhere tests nothing'
    left, bad = int(out.sum()), int(((l16 != l32) & ~out).sum())
    print('predict_labels: %d of %d voxels left out (fp32 gap <= 2 eps = %.1e), %d differ in all, %d outside the gap'
          % (left, out.numel(), 2 * eps, int((l16 != l32).sum()), bad))
    assert left <= 0.2 * out.numel() and bad == 0
    # the flip average: both networks average their own two passes
    sd = {k: (0.5 * (v + torch.flip(v, dims=[0])) if k.endswith('/kernel') and v.dim() == 5 else v).numpy()
          for k, v in c['sd'].items()}
    S = c['x'][..., 0].numpy()
    res = {}
    for dt in ('f32', 'bf16'):
        pred = SegmentationPredictor(None, SEG_LABELS, n_levels=LEVELS, unet_feat_count=FEATS, state_dict=sd, dtype=dt)
        res[dt] = pred.segment_volume(S, flipping=True, lr_pairs=None, return_posteriors=True)
        assert pred.net_for(NET_SHAPE).bf16 == (dt == 'bf16')
        assert np.array_equal(pred.segment_volume(S, flipping=True, lr_pairs=None), res[dt][0])
    (s32, q32), (s16, q16) = res['f32'], res['bf16']
    assert s16.dtype == np.int32 and q16.dtype == np.float32 and q16.shape == NET_SHAPE + (len(SEG_LABELS),)
    d = float(np.abs(q16 - q32).max())
    out = _undecided(torch.from_numpy(q32), eps).numpy()
    left, bad = int(out.sum()), int(((s16 != s32) & ~out).sum())
    print('segment_volume(flipping): averaged posteriors bf16 - fp32 %.3e; %d of %d voxels left out, %d differ in all, %d '
          'outside the gap' % (d, left, out.size, int((s16 != s32).sum()), bad))
    assert len(np.unique(s32)) >= 3
    assert left <= 0.2 * out.size and bad == 0


def test_backward_input_bf16_reaches_the_network_input(T):
    """the first conv's data gradient has one output channel: backward_input() of a bf16 network returns float32
    [d0, d1, d2, 1] (no padding channels) close to the fp32 network's"""
    torch = T
    c = _net_case()
    x = c['x'].cuda()
    g = torch.Generator().manual_seed(3)
    dbn = torch.randn(*NET_SHAPE, FEATS, generator=g)
    got = {}
    for dt in ('f32', 'bf16'):
        net = _net(c, dt)
        net.enable_input_grad()
        for mode in (False, True):
            net.predict_probs(x, batch_stats=mode)
            d = dbn.cuda().to(net.act_dtype)
            got[dt, mode] = net.backward_input(d).clone()
    for mode in (False, True):
        a, b = got['f32', mode], got['bf16', mode]
        assert b.dtype == torch.float32 and tuple(b.shape) == NET_SHAPE + (1,) and tuple(a.shape) == tuple(b.shape)
        cos = float((a * b).sum() / (a.norm() * b.norm()))
        print('backward_input, batch_stats=%s: cosine bf16 / fp32 %.5f, norms %.4e / %.4e' % (mode, cos, float(b.norm()), float(a.norm())))
        assert bool(torch.isfinite(b).all()) and cos >= 0.9


@pytest.mark.parametrize('frozen_bn,crop,stack', [('batch', None, 1), ('inference', (8, 12, 10), 1), ('batch', None, 2),
                                                  ('inference', None, 2)])
def test_segmentation_regulariser_bf16_vs_fp32(T, frozen_bn, crop, stack):
    """SegmentationRegulariser on a bf16 segmentation network against the same call on the fp32 one: Dice within 1 % (the bf16
    loss tolerance of tests/test_bf16_gpu.py), cosine of the dpred increment >= 0.9 (that file's loose gradient bound for
    comparisons across pooling decisions); the increment is float32 and has the shape of pred.  Measured on an MI355X over the
    four cases: Dice relative difference 3.5e-05 .. 4.0e-04, cosine 0.9883 .. 0.9907."""
    torch = T
    from synthsr_amd.seg_loss import SegmentationRegulariser
    c = _net_case()
    gen_labels = np.array([0, 14, 2, 3, 41, 42, 17])
    equivalency = np.array([0, 14, 2, 41, 41])                 # the five labels of the network; two of them merge
    g = torch.Generator().manual_seed(7)
    pred = torch.rand(stack * NET_SHAPE[0], *NET_SHAPE[1:], generator=g)
    seg = torch.randint(0, len(gen_labels), tuple(pred.shape), generator=g, dtype=torch.int32)
    res = {}
    for dt in ('f32', 'bf16'):
        reg = SegmentationRegulariser(_net(c, dt), gen_labels, equivalency, 0.5, frozen_bn=frozen_bn)
        dpred = torch.zeros(pred.numel(), device='cuda')
        dice = float(reg(pred.cuda().reshape(-1), seg.cuda(), dpred, crop).item())
        res[dt] = (dice, dpred)
    (d32, g32), (d16, g16) = res['f32'], res['bf16']
    assert g16.dtype == torch.float32 and g16.shape == g32.shape == (pred.numel(),)
    cos = float((g16 * g32).sum() / (g16.norm() * g32.norm()))
    print('regulariser %s crop=%s stack=%d: Dice fp32 %.6f bf16 %.6f (relative %.2e), cosine of the increment %.5f'
          % (frozen_bn, crop, stack, d32, d16, abs(d16 - d32) / abs(d32), cos))
    assert float(g32.abs().max()) > 0 and bool(torch.isfinite(g16).all())
    assert abs(d16 - d32) <= 0.01 * abs(d32)
    assert cos >= 0.9


# ---------------------------------------------------------------------------------------------------- end to end
def test_bf16_segmentation_network_end_to_end(T, tmp_path):
    """a short fp32 training_segmentation run writes a checkpoint; training(dtype='bf16', segnet_dtype='bf16',
    segmentation_model_file=ckpt) runs one step to a finite logged loss; predict_segmentation(dtype='bf16') and the script
    with --dtype bf16 write int32 label maps, whose per-label Dice against the fp32 run is printed"""
    from synthsr_amd.nifti import write_nifti, read_nifti
    from synthsr_amd.segmentation_training import training_segmentation
    from synthsr_amd.training import training
    from synthsr_amd.predict_segmentation import predict_segmentation, dice_scores, mean_dice
    labels_dir, seg_labels = _write_inputs(tmp_path)
    files = [str(tmp_path / n) for n in ('pm.npy', 'ps.npy', 'gl.npy', 'sl.npy')]
    common = dict(path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3, unet_feat_count=24,
                  nonlin_shape_factor=.125, bias_shape_factor=.125, verbose=False)
    full_dir = str(tmp_path / 'full')
    training_segmentation(labels_dir, full_dir, *files, epochs=1, steps_per_epoch=5, lr=1e-3, fixed_sample=True, **common)
    ckpt = os.path.join(full_dir, '001.npz')
    assert os.path.exists(ckpt)
    reg_dir = str(tmp_path / 'reg')
    training(labels_dir, reg_dir, *files[:3], segmentation_label_list=files[3], segmentation_label_equivalency=files[3],
             segmentation_model_file=ckpt, epochs=1, steps_per_epoch=1, dtype='bf16', segnet_dtype='bf16', **common)
    log = [float(l.split(',')[1]) for l in open(os.path.join(reg_dir, 'logs', 'loss.csv')).read().strip().split('\n')]
    assert len(log) == 1 and np.isfinite(log[0])
    rng = np.random.default_rng(5)
    d = tmp_path / 'images'
    d.mkdir()
    shape = (20, 18, 22)
    write_nifti(str(d / 'scan0.nii.gz'), rng.random(shape).astype(np.float32) * 100)
    kw = dict(n_levels=3, unet_feat_count=24, verbose=False)
    o32 = predict_segmentation(str(d), str(tmp_path / 'segs32'), ckpt, files[3], **kw)
    o16 = predict_segmentation(str(d), str(tmp_path / 'segs16'), ckpt, files[3], dtype='bf16', **kw)
    spec = importlib.util.spec_from_file_location('predict_segmentation_script', os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    one, post = str(tmp_path / 'one_seg.nii.gz'), str(tmp_path / 'one_post.nii.gz')
    script.main([str(d / 'scan0.nii.gz'), one, '--model', ckpt, '--labels', files[3], '--n_levels', '3', '--unet_feat', '24',
                 '--dtype', 'bf16', '--posteriors', post])
    assert read_nifti(post)[0].dtype == np.float32
    a = read_nifti(o32[0])[0]
    for path in (o16[0], one):
        data = read_nifti(path)[0]
        assert data.dtype == np.int32 and data.shape == shape and set(np.unique(data)) <= set(seg_labels.tolist())
        row = dice_scores(path, o32[0], seg_labels)
        print('%s against the fp32 label map: mean Dice %.4f, per label %s; %d of %d voxels differ'
              % (os.path.basename(path), mean_dice(row), np.array2string(row, precision=3), int((data != a).sum()), a.size))
    assert np.array_equal(read_nifti(o16[0])[0], read_nifti(one)[0]), 'the script and the function disagree'
