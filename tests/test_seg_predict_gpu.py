"""Segmenting with a trained softmax-headed U-Net and scoring with Dice: the three kernels alone (csrc/unet_pointwise.hip:
seg_head_argmax_kernel, seg_head_tta_argmax_kernel, seg_label_counts_kernel), UNet3D.predict_labels and
SegmentationPredictor.segment_volume on a whole network, predict_segmentation() and the script end to end.

The reference of the head kernels is float64 on the same inputs.  An argmax is discontinuous: which of two classes within
float32 rounding of each other wins is not a property of the algorithm, so labels are compared at the voxels whose float64
top-two gap exceeds a threshold (the GAP RULE) and the voxels left out may be at most 1 % of the volume:
  * logits (kernel 1, predict_labels):      gap > 1e-4 max|logit|, the maximum taken over the volume;
  * averaged posteriors (kernel 2):         gap > 1e-5;
  * averaged posteriors of a whole network: gap > 1e-4 max|logit|.  A logit error of d moves every posterior by at most d / 2
    (|dp_n / dlogit_m| <= 1/4, summed over the two directions that matter), so posteriors that are averages of two passes are
    off by at most d / 2 each and the gap of two of them by at most d: the logit rule carried over to posteriors.
Every case also evaluates the same graph in float32 with torch on the CPU: it has no mismatch outside the gap, and the test
prints its count next to the device's and the number of voxels the gap leaves out.  Float32 on the CPU over the eight
kernel-1 cases: no mismatch at any voxel, inside the gap or outside; the gap leaves out at most 1 voxel of 315 and 12 of
8448; 2 of 4096 on the whole network, 23 of 4096 on its flip average.

Averaged posteriors are held to 2e-5 relative of float64, the bound of tests/test_seg_training_gpu.py for this mathematics.
Label counts are integers: they equal numpy's exactly."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (5, 7, 9)            # 315 voxels: four full 64-voxel tiles and a partial one; odd d0: the centre plane mirrors onto itself
EVEN = (6, 4, 8)             # 192 voxels = three full tiles, even d0
BIG = (33, 16, 16)           # 8448 voxels = 132 tiles
GUARD, SENTINEL, ISENTINEL = 64, -12345.5, -12345
# (C, N, shape, misaligned output)
CASES = [(8, 2, SHAPE, False), (8, 19, SHAPE, True), (24, 5, SHAPE, False), (24, 33, SHAPE, True), (64, 64, SHAPE, False),
         (64, 19, SHAPE, True), (24, 64, SHAPE, True), (24, 33, BIG, False)]
TTA_CASES = [(24, 33, SHAPE, ((3, 17), (4, 30), (0, 32)), True), (24, 33, EVEN, ((3, 17), (4, 30), (0, 32)), False),
             (8, 2, SHAPE, (), False), (8, 2, EVEN, (), True)]


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def _head_inputs(C, N, shape, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, C, generator=g)
    mean, var = torch.randn(C, generator=g) * .1, torch.rand(C, generator=g) + .5
    gamma, beta = torch.rand(C, generator=g) + .5, torch.randn(C, generator=g) * .1
    w = torch.randn(C, N, generator=g) * .3
    b = torch.randn(N, generator=g) * .1
    labels = torch.randperm(2 * N + 8, generator=g)[:N].to(torch.int32)      # label VALUES, in no order
    return dict(C=C, N=N, shape=shape, x=x, stats=torch.cat([mean, var]), gamma=gamma, beta=beta, w=w, b=b, labels=labels), g


def _logits(c, dtype, x=None):
    import torch
    from synthsr_amd import ops
    d = lambda t: t.to(dtype)
    mean, var = d(c['stats'][:c['C']]), d(c['stats'][c['C']:])
    bn = (d(c['x'] if x is None else x) - mean) * torch.rsqrt(var + ops.BN_EPS) * d(c['gamma']) + d(c['beta'])
    return bn @ d(c['w']) + d(c['b'])


def _top_two_gap(v):
    top = v.double().topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


@functools.lru_cache(maxsize=None)
def _case(C, N, shape):
    """inputs (host), the float64 argmax, the voxels the gap rule compares and the float32-CPU argmax; never modified"""
    import torch
    c, _ = _head_inputs(C, N, shape, 1000 * C + N + shape[0])
    l64 = _logits(c, torch.float64)
    c['ref'] = l64.argmax(-1)
    c['sure'] = _top_two_gap(l64) > 1e-4 * l64.abs().max().item()
    c['cpu32'] = _logits(c, torch.float32).argmax(-1)
    return c


def _guarded(torch, numel, misalign=False, dtype=None, sentinel=SENTINEL):
    """a device buffer of `numel` elements with GUARD sentinels behind it (and one in front when misaligned)"""
    full = torch.full((numel + GUARD + 1,), sentinel, device='cuda', dtype=dtype or torch.float32)
    o = 1 if misalign else 0
    return full, full[o:o + numel]


def _guards_intact(full, numel, misalign, sentinel=SENTINEL):
    o = 1 if misalign else 0
    return bool((full[o + numel:] == sentinel).all()) and bool((full[:o] == sentinel).all())


def _compare_labels(what, got, c, ref=None, sure=None, cpu32=None):
    """the gap rule: `got` (label values) against labels[float64 argmax] where the float64 gap is wide enough"""
    ref = c['ref'] if ref is None else ref
    sure = c['sure'] if sure is None else sure
    cpu32 = c['cpu32'] if cpu32 is None else cpu32
    want = c['labels'][ref]
    nvox = want.numel()
    left_out = int((~sure).sum())
    bad_dev = int(((got.cpu().reshape(want.shape) != want) & sure).sum())
    bad_cpu = int(((c['labels'][cpu32] != want) & sure).sum())
    print('%s: %d voxels, %d left out by the gap, mismatches outside it: device %d, fp32 CPU %d'
          % (what, nvox, left_out, bad_dev, bad_cpu))
    assert left_out <= 0.01 * nvox, 'the gap leaves out %d of %d voxels' % (left_out, nvox)
    assert bad_cpu == 0, 'float32 on the CPU disagrees with float64 outside the gap'
    assert bad_dev == 0


def _dev(c, *keys):
    return [c[k].cuda() for k in keys]


# ---------------------------------------------------------------------------------------------------- kernel 1
@pytest.mark.parametrize('C,N,shape,misalign', CASES)
def test_seg_head_argmax_vs_float64(T, C, N, shape, misalign):
    torch = T
    from synthsr_amd import ops
    c = _case(C, N, shape)
    nvox = int(np.prod(shape))
    full, out = _guarded(torch, nvox, misalign, torch.int32, ISENTINEL)
    ops.seg_head_argmax(*_dev(c, 'x', 'stats', 'gamma', 'beta', 'w', 'b', 'labels'), out)
    torch.cuda.synchronize()
    assert _guards_intact(full, nvox, misalign, ISENTINEL), 'guard overwritten'
    _compare_labels('argmax C=%d N=%d' % (C, N), out, c)


def test_exact_ties_go_to_the_lowest_channel(T):
    """channels 7 and 20 of a (24, 33) head share their column and their bias, large enough to dominate every voxel: equal
    logits bit for bit, and channel 7 -- another 16-class block, another lane -- wins everywhere; so it does in the averaged
    posteriors of the flip pass, whose two terms are equal for the two channels as well"""
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
    head = _dev(c, 'x', 'stats', 'gamma', 'beta', 'w', 'b', 'labels')
    ops.seg_head_argmax(*head, out)
    assert bool((out == int(c['labels'][7])).all())
    prev = torch.softmax(l64, -1).float().reshape(nvox, 33).cuda()
    out.fill_(ISENTINEL)
    ops.seg_head_tta_argmax(*head, prev, torch.arange(33, dtype=torch.int32).cuda(), out)
    assert bool((out == int(c['labels'][7])).all())


def test_limits_are_refused(T):
    """C = 68 (> 64), C = 6 (not whole channel quads) and N = 65 return the invalid-argument error from every entry point they
    apply to and launch nothing; the ops wrappers raise ValueError"""
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    nvox = int(np.prod(SHAPE))
    for C, N in ((68, 5), (6, 5), (24, 65)):
        x = torch.randn(*SHAPE, C).cuda()
        stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
        gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
        w, b = torch.randn(C, N).cuda(), torch.zeros(N).cuda()
        labels = torch.arange(N, dtype=torch.int32).cuda()
        perm = torch.arange(N, dtype=torch.int32).cuda()
        prev = torch.full((nvox, N), 1.0 / N).cuda()
        out = torch.full((nvox,), ISENTINEL, dtype=torch.int32).cuda()
        probs = torch.full((nvox * N,), SENTINEL).cuda()
        P = _lib.ptr
        rc = lib.synthsr_seg_head_argmax(P(x), nvox, C, P(stats), P(gamma), P(beta), ops.BN_EPS, P(w), P(b), N, P(labels), P(out),
                                         _lib.stream())
        assert rc == -1   # SYNTHSR_EINVAL
        rc = lib.synthsr_seg_head_tta_argmax(P(x), _lib.i3(SHAPE), C, P(stats), P(gamma), P(beta), ops.BN_EPS, P(w), P(b), N,
                                             P(labels), P(prev), P(perm), P(out), P(probs), _lib.stream())
        assert rc == -1
        with pytest.raises(ValueError):
            ops.seg_head_argmax(x, stats, gamma, beta, w, b, labels, out)
        with pytest.raises(ValueError):
            ops.seg_head_tta_argmax(x, stats, gamma, beta, w, b, labels, prev, perm, out, probs)
        torch.cuda.synchronize()
        assert bool((out == ISENTINEL).all()) and bool((probs == SENTINEL).all())
    a = torch.zeros(nvox, dtype=torch.int32).cuda()
    lut = torch.zeros(4, dtype=torch.int32).cuda()
    counts = torch.full((3 * 65,), ISENTINEL, dtype=torch.int64).cuda()
    assert lib.synthsr_seg_label_counts(_lib.ptr(a), _lib.ptr(a), nvox, _lib.ptr(lut), 4, 65, _lib.ptr(counts), _lib.stream()) == -1
    with pytest.raises(ValueError):
        ops.seg_label_counts(a, a, lut, 65)
    torch.cuda.synchronize()
    assert bool((counts == ISENTINEL).all())


# ---------------------------------------------------------------------------------------------------- kernel 2
@functools.lru_cache(maxsize=None)
def _tta_case(C, N, shape, pairs):
    """a flipped pass (x), the posteriors of an unflipped pass (prev, float32) and the float64 flip average"""
    import torch
    c, g = _head_inputs(C, N, shape, 2000 * C + N + shape[0])
    perm = torch.arange(N)
    for i, j in pairs:
        perm[i], perm[j] = j, i
    x0 = torch.randn(*shape, C, generator=g)                                   # the unflipped pass sees other features
    c['prev'] = torch.softmax(_logits(c, torch.float64, x0), -1).float()
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
def test_seg_head_tta_argmax_vs_float64(T, C, N, shape, pairs, misalign):
    torch = T
    from synthsr_amd import ops
    c = _tta_case(C, N, shape, pairs)
    nvox = int(np.prod(shape))
    head = _dev(c, 'x', 'stats', 'gamma', 'beta', 'w', 'b', 'labels')
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
    _compare_labels('tta C=%d N=%d' % (C, N), out, c)
    # without probs_out: the same label map, and the posteriors' buffer keeps its sentinels
    ofull2, out2 = _guarded(torch, nvox, misalign, torch.int32, ISENTINEL)
    pfull.fill_(SENTINEL)
    ops.seg_head_tta_argmax(*head, prev, perm, out2, None)
    torch.cuda.synchronize()
    assert bool((pfull == SENTINEL).all()) and _guards_intact(ofull2, nvox, misalign, ISENTINEL)
    assert torch.equal(out2, out)


# ---------------------------------------------------------------------------------------------------- kernel 3
@functools.lru_cache(maxsize=None)
def _maps(shape, N):
    """two label maps over a table of 2 N + 8 values, N of them listed: values mapped to -1, values beyond the table and
    negative ones in both; channel N - 2 in `a` only, channel N - 1 in neither map (N = 2 has no third channel to overlap
    on: there channel 1 is in both); numpy's counts"""
    rng = np.random.default_rng(100 * N + shape[0])
    lut_n = 2 * N + 8
    values = rng.permutation(lut_n)
    listed, unlisted = values[:N], values[N:]
    both = listed[:N - 2] if N > 2 else listed[1:]
    pool = np.concatenate([both, both, unlisted[:3], [-1, -7, lut_n, lut_n + 1000]])     # listed values twice as likely
    a = rng.choice(pool, size=shape).astype(np.int32)
    b = np.where(rng.random(shape) < .6, a, rng.choice(pool, size=shape)).astype(np.int32)
    a.reshape(-1)[rng.choice(a.size, 5, replace=False)] = listed[N - 2]                   # present in a only
    labels = listed.astype(np.int32)
    ka = np.full(a.shape, -1)
    kb = np.full(b.shape, -1)
    for k, v in enumerate(labels):
        ka[a == v] = k
        kb[b == v] = k
    counts = np.zeros((3, N), dtype=np.int64)
    counts[0] = np.bincount(ka[(ka >= 0) & (ka == kb)], minlength=N)
    counts[1] = np.bincount(ka[ka >= 0], minlength=N)
    counts[2] = np.bincount(kb[kb >= 0], minlength=N)
    assert counts[1, N - 2] >= 5 and counts[2, N - 2] == 0 and counts[0].sum() > 0
    assert N == 2 or (counts[1, N - 1] == 0 and counts[2, N - 1] == 0)
    assert (ka < 0).sum() > 0 and (kb < 0).sum() > 0
    return a, b, labels, counts


@pytest.mark.parametrize('shape', [SHAPE, BIG])
@pytest.mark.parametrize('N', [2, 19, 64])
def test_seg_label_counts_and_dice_equal_numpy(T, shape, N):
    torch = T
    from synthsr_amd import ops
    from synthsr_amd.segmentation_training import segmentation_lut
    from synthsr_amd.predict_segmentation import dice_scores
    a, b, labels, want = _maps(shape, N)
    lut = torch.from_numpy(segmentation_lut(labels)).cuda()
    full, counts = _guarded(torch, 3 * N, False, torch.int64, ISENTINEL)
    got = ops.seg_label_counts(torch.from_numpy(a).cuda().reshape(-1), torch.from_numpy(b).cuda().reshape(-1), lut, N, counts)
    torch.cuda.synchronize()
    assert _guards_intact(full, 3 * N, False, ISENTINEL)
    assert np.array_equal(got.cpu().numpy().reshape(3, N), want)
    with np.errstate(invalid='ignore', divide='ignore'):
        dice = 2.0 * want[0] / (want[1].astype(np.float64) + want[2])
    assert N == 2 or np.isnan(dice[N - 1])
    assert dice[N - 2] == 0.0
    scores = dice_scores(a, b, labels)
    assert scores.dtype == np.float64 and np.array_equal(scores, dice, equal_nan=True)
    same = dice_scores(a, a.copy(), labels)
    assert np.array_equal(np.isnan(same), want[1] == 0) and bool(np.all(same[want[1] > 0] == 1.0))
    with pytest.raises(ValueError):
        dice_scores(a, b[:-1], labels)


# ---------------------------------------------------------------------------------------------------- whole network
NET_SHAPE, LEVELS, FEATS = (16, 16, 16), 3, 8
SEG_LABELS = np.array([0, 14, 2, 41, 17], dtype=np.int32)       # head channel order (label values)
LR_PAIRS = [(2, 41)]                                            # channels 2 and 3


@functools.lru_cache(maxsize=None)
def _net_case():
    """random weights and moving statistics of the 8-feature, 3-level, 5-label network (host), an input volume, and the
    float64 oracle: logits and posteriors of the volume and of its flip, the flip average"""
    import torch
    from oracle import unet_ref as U
    from synthsr_amd.unet import UNet3D
    table = UNet3D(FEATS, list(NET_SHAPE) + [1], LEVELS, 3, len(SEG_LABELS), feat_mult=2, nb_conv_per_level=2, batch_norm=-1,
                   final_pred_activation='softmax', table_only=True)
    g = torch.Generator().manual_seed(31)
    sd = {}
    for nm, shp, kind in table.specs:
        if kind in ('kernel', 'head_w'):
            fan = int(np.prod(shp[:-1]))
            sd[nm] = torch.randn(*shp, generator=g) * (1.5 / np.sqrt(fan))
        elif kind == 'gamma':
            sd[nm] = torch.rand(*shp, generator=g) + .5
        else:
            sd[nm] = torch.randn(*shp, generator=g) * .1
    for bn in table.bn_layers:
        sd[bn['name'] + '/moving_mean'] = torch.randn(bn['C'], generator=g) * .2
        sd[bn['name'] + '/moving_variance'] = torch.rand(bn['C'], generator=g) * 1.5 + .5
    x = torch.rand(*NET_SHAPE, 1, generator=g)
    P = {k: v for k, v in sd.items() if 'moving_' not in k}
    moving = {k: v for k, v in sd.items() if 'moving_' in k}

    def oracle(inp, dtype, softmax):
        with U.compute_dtype(dtype), torch.no_grad():
            return U.unet_forward(inp, P, table.prefix, LEVELS, 2, training=False, moving=moving, softmax=softmax)
    out = dict(sd=sd, x=x, labels=torch.from_numpy(SEG_LABELS))
    xf = torch.flip(x, dims=[0])
    perm = torch.tensor([0, 1, 3, 2, 4])
    for tag, dtype in (('', torch.float64), ('32', torch.float32)):
        p, q = oracle(x, dtype, True), oracle(xf, dtype, True)
        out['probs' + tag] = p
        out['avg' + tag] = 0.5 * (p + torch.flip(q, dims=[0])[..., perm])
    logits = oracle(x, torch.float64, False)
    assert torch.allclose(torch.softmax(logits, -1), out['probs'], rtol=0, atol=1e-12)
    scale = max(logits.abs().max().item(), oracle(xf, torch.float64, False).abs().max().item())
    out.update(ref=logits.argmax(-1), sure=_top_two_gap(logits) > 1e-4 * scale, cpu32=out['probs32'].argmax(-1),
               avg_ref=out['avg'].argmax(-1), avg_sure=_top_two_gap(out['avg']) > 1e-4 * scale,
               avg_cpu32=out['avg32'].argmax(-1))
    assert len(torch.unique(out['ref'])) >= 3, 'a network that predicts one label everywhere tests nothing'
    return out


def _loaded_net(torch, c):
    from synthsr_amd.unet import unet
    net = unet(nb_features=FEATS, input_shape=list(NET_SHAPE) + [1], nb_levels=LEVELS, conv_size=3, nb_labels=len(SEG_LABELS),
               feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax', seed=2)
    net.load_state_dict(c['sd'], strict=True)
    net.repack()
    return net


def test_predict_labels_vs_float64_oracle(T):
    """predict_labels against the argmax of the float64 oracle in inference mode; the fused path against predict_probs +
    torch.argmax + table; the training path afterwards"""
    torch = T
    c = _net_case()
    net = _loaded_net(torch, c)
    labels = c['labels'].cuda()
    x = c['x'].cuda()
    got = net.predict_labels(x, labels).clone()
    assert got.dtype == torch.int32 and tuple(got.shape) == NET_SHAPE and net._loss_state is None
    _compare_labels('predict_labels', got, c)
    composed = labels[torch.argmax(net.predict_probs(x), dim=1)].reshape(NET_SHAPE)
    sure = c['sure'].cuda()
    assert bool((composed == got)[sure].all())
    with pytest.raises(ValueError):
        net.predict_labels(x, labels, want_probs=True)       # posteriors exist only in the averaging pass
    # the training path is undisturbed: backward() still asks for a loss_dice() first, then trains
    with pytest.raises(RuntimeError):
        net.backward()
    from synthsr_amd.segmentation_training import segmentation_lut
    lut = torch.from_numpy(segmentation_lut(SEG_LABELS)).cuda()
    seg = labels[torch.randint(0, 5, NET_SHAPE, generator=torch.Generator().manual_seed(4))]
    loss = net.loss_dice(x, seg, lut)
    net.backward()
    assert np.isfinite(loss.item()) and bool(torch.isfinite(net.grads).all()) and float(net.grads.abs().max()) > 0


def test_segment_volume_flip_average_vs_float64_oracle(T):
    torch = T
    from synthsr_amd.predict_segmentation import SegmentationPredictor
    c = _net_case()
    pred = SegmentationPredictor(None, SEG_LABELS, n_levels=LEVELS, unet_feat_count=FEATS,
                                 state_dict={k: v.numpy() for k, v in c['sd'].items()})
    S = c['x'][..., 0].numpy().astype(np.float64)
    seg, post = pred.segment_volume(S, flipping=True, lr_pairs=LR_PAIRS, return_posteriors=True)
    net = pred.net_for(NET_SHAPE)
    assert net._loss_state is None
    assert seg.dtype == np.int32 and seg.shape == NET_SHAPE and post.shape == NET_SHAPE + (5,) and post.dtype == np.float32
    kw = dict(ref=c['avg_ref'], sure=c['avg_sure'], cpu32=c['avg_cpu32'])
    _compare_labels('segment_volume, flipping', torch.from_numpy(seg), c, **kw)
    d = np.abs(post.astype(np.float64) - c['avg'].numpy()).max()
    d32 = (c['avg32'].double() - c['avg']).abs().max().item()
    print('flip-averaged posteriors of the network: device-float64 %.3e  fp32 CPU-float64 %.3e' % (d, d32))
    assert bool((seg == SEG_LABELS[post.argmax(-1)]).all()), 'the label map is not the argmax of the posteriors returned with it'
    seg2 = pred.segment_volume(S, flipping=True, lr_pairs=LR_PAIRS)
    assert np.array_equal(seg2, seg)
    assert 'probs_avg' in net._bufs
    plain = SegmentationPredictor(None, SEG_LABELS, n_levels=LEVELS, unet_feat_count=FEATS,
                                  state_dict={k: v.numpy() for k, v in c['sd'].items()})
    seg3 = plain.segment_volume(S, flipping=False)
    _compare_labels('segment_volume, no flipping', torch.from_numpy(seg3), c)
    bufs = plain.net_for(NET_SHAPE)._bufs
    assert 'probs' not in bufs and 'probs_avg' not in bufs, 'flipping=False formed posteriors'
    with pytest.raises(ValueError):
        pred.segment_volume(S, lr_pairs=[(2, 99)])
    # and the network trains on after segmenting
    from synthsr_amd.segmentation_training import segmentation_lut
    lut = torch.from_numpy(segmentation_lut(SEG_LABELS)).cuda()
    loss = net.loss_dice(c['x'].cuda(), torch.from_numpy(seg).cuda(), lut)
    net.backward()
    assert np.isfinite(loss.item()) and float(net.grads.abs().max()) > 0


# ---------------------------------------------------------------------------------------------------- end to end
def test_predict_segmentation_end_to_end(T, tmp_path, capsys):
    """two NIfTI volumes in a folder -> *_seg.nii.gz of the inputs' own shape, int32, listed label values only; the script
    on one file, scoring what it wrote against itself"""
    torch = T
    from synthsr_amd.nifti import write_nifti, read_nifti
    from synthsr_amd.unet import unet
    from synthsr_amd.training import save_checkpoint
    from synthsr_amd.predict_segmentation import predict_segmentation
    rng = np.random.default_rng(5)
    d = tmp_path / 'images'
    d.mkdir()
    shapes = [(20, 18, 22), (17, 32, 9)]
    for i, s in enumerate(shapes):
        write_nifti(str(d / ('scan%d.nii.gz' % i)), rng.random(s).astype(np.float32) * 100)
    net = unet(nb_features=FEATS, input_shape=[32, 32, 32, 1], nb_levels=LEVELS, conv_size=3, nb_labels=len(SEG_LABELS),
               feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax', seed=3)
    g = torch.Generator().manual_seed(6)
    net.view(net.head['w']).copy_(torch.randn(FEATS, len(SEG_LABELS), generator=g))
    ckpt = str(tmp_path / 'seg.npz')
    save_checkpoint(ckpt, net)
    np.save(tmp_path / 'labels.npy', SEG_LABELS)
    np.save(tmp_path / 'pairs.npy', np.array(LR_PAIRS))
    outs = predict_segmentation(str(d), str(tmp_path / 'segs'), ckpt, str(tmp_path / 'labels.npy'), lr_pairs=LR_PAIRS,
                                n_levels=LEVELS, unet_feat_count=FEATS, verbose=False)
    assert [os.path.basename(o) for o in outs] == ['scan0_seg.nii.gz', 'scan1_seg.nii.gz']
    for o, s in zip(outs, shapes):
        data, aff, _ = read_nifti(o)
        assert data.dtype == np.int32 and data.shape == s
        assert set(np.unique(data)) <= set(SEG_LABELS.tolist())
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    one = str(tmp_path / 'one_seg.nii.gz')
    table = script.main([str(d / 'scan0.nii.gz'), one, '--model', ckpt, '--labels', str(tmp_path / 'labels.npy'),
                         '--lr_pairs', str(tmp_path / 'pairs.npy'), '--n_levels', str(LEVELS), '--unet_feat', str(FEATS),
                         '--truth', one, '--scores', str(tmp_path / 'scores.csv')])
    from synthsr_amd.predict_segmentation import mean_dice
    assert table.shape == (1, len(SEG_LABELS)) and mean_dice(table[0]) == 1.0
    assert 'mean Dice 1.0000' in capsys.readouterr().out
    rows = open(tmp_path / 'scores.csv').read().strip().split('\n')
    assert rows[0] == ','.join(str(v) for v in SEG_LABELS) and len(rows) == 2
