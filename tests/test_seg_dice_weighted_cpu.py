"""The weighted soft Dice (class weights, boundary weights, skip_background of DiceLoss, ext/lab2im/layers.py:1264-1376) without
a GPU: the float64 restatement that tests/test_seg_dice_weighted_gpu.py holds the kernels to, the integer boundary rule against
the float rule on every label map those tests use, argument checks of training_segmentation / UNet3D.loss_dice, the launcher's
flags."""
import functools
import inspect
import os
import sys

import numpy as np
import pytest

SHAPE = (5, 7, 9)            # with d = 3 the window exceeds the volume on two axes: W differs voxel to voxel; partial last tile
BIG = (33, 16, 16)           # 132 head tiles, 18 mask tiles
HEADS = [(8, 2), (24, 5), (24, 33), (64, 64), (64, 19)]                 # (C, N)
SEED = 5                     # of the label maps: one at which every map has what test_integer_boundary_rule_... asserts
GEOMETRIES = [(SHAPE, 1), (SHAPE, 3), (SHAPE, 5), (BIG, 3)]             # (shape, boundary_dist)


# ------------------------------------------------------------------------------------------------ the restatement
def _box_sum(t, d):
    """sums over the (2 d + 1)^3 window clipped to the volume, t [1, K, d0, d1, d2]"""
    import torch.nn.functional as F
    return F.avg_pool3d(F.pad(t, (d,) * 6), 2 * d + 1, stride=1, divisor_override=1)


def same_avg_pool(gt, d):
    """Keras AvgPool3D(2 d + 1, strides 1, padding='same') of gt [d0,d1,d2,N]: padding does not enter the divisor, i.e.
    avg_pool3d(gt, 2 d + 1, stride=1, padding=d, count_include_pad=False).  torch refuses that call where the window is
    larger than the volume (SHAPE with d >= 3), so it is written out as window sum / window count, the same two numbers and
    the same division (test_same_avg_pool_is_avg_pool3d holds it to the call where torch accepts it)"""
    import torch
    t = gt.permute(3, 0, 1, 2)[None]
    return (_box_sum(t, d) / _box_sum(torch.ones_like(t[:, :1]), d))[0].permute(1, 2, 3, 0)


def boundary_map(gt, d, skip_background=True):
    """DiceLoss's boundary map (layers.py:1349-1353) of a one-hot gt [d0,d1,d2,N] (float64), the float thresholds as there"""
    import torch
    avg = same_avg_pool(gt, d)
    bnd = (avg > 0.).to(gt.dtype) * (avg < (1 / 3 - 1e-4)).to(gt.dtype)
    if skip_background and gt.shape[-1] > 1:
        bnd = torch.cat([torch.zeros_like(bnd[..., :1]), bnd[..., 1:]], -1)
    return bnd


def weighted_dice(gt, pred, class_weights=None, boundary_weights=0., boundary_dist=3, skip_background=True, eps=1e-7):
    """DiceLoss.call (layers.py:1343-1376, enable_checks=False) of one volume, gt / pred [d0,d1,d2,N], in their dtype.  Dynamic
    weights (-1) are the reference's 1 / volume normalised, except that a label without a voxel gets weight 0 (the reference
    divides by zero: NaN) and a map without any label gives 0."""
    import torch
    w = torch.ones_like(gt)
    if boundary_weights:
        w = 1 + boundary_weights * boundary_map(gt.detach(), boundary_dist, skip_background)
    top = (w * 2 * gt * pred).sum((0, 1, 2))
    bottom = (w * (gt * gt + pred * pred)).sum((0, 1, 2))
    loss = 1 - (top + eps) / (bottom + eps)
    if class_weights is None:
        return loss.mean()
    if np.ndim(class_weights) == 0 and class_weights == -1:
        vol = (gt * w).sum((0, 1, 2)).detach()
        c = torch.where(vol > 0, 1 / vol.clamp_min(1e-30), torch.zeros_like(vol))
        if float(c.sum()) == 0:
            return (loss * 0).sum()
    else:
        c = torch.as_tensor(np.asarray(class_weights, dtype=np.float64)).to(gt.dtype)
    return (loss * (c / c.sum())).sum()


def integer_mask(k, N, d, skip_background=True):
    """the rule the kernel evaluates, on the class map k [d0,d1,d2] (int, -1 = no class): bit n of mask[v] = [0 < 3 count_n <
    W], count_n = voxels of class n and W = voxels inside the volume in the window.  Returns uint64 [d0,d1,d2]"""
    import torch
    import torch.nn.functional as F
    box = lambda t: _box_sum(t[None, None].double(), d)[0, 0].round().long()
    W = box(torch.ones_like(k))
    mask = np.zeros(tuple(k.shape), dtype=np.uint64)
    for n in range(1 if (skip_background and N > 1) else 0, N):
        cnt = box(k == n)
        mask |= ((cnt > 0) & (3 * cnt < W)).numpy().astype(np.uint64) << np.uint64(n)
    return mask


# ------------------------------------------------------------------------------------------------ label maps of the tests
@functools.lru_cache(maxsize=None)
def label_case(N, shape):
    """a blocky label map (blocks of 2 x 3 x 4 voxels, so that interior and boundary voxels both exist) of label VALUES out of a
    table of 2 N + 8 in no order, with values mapped to -1, values outside the table, one class (0) of a single voxel and one
    (N - 2) without any; the classes of the blocks are 1, 2, N // 2 and N - 1, so that N = 33 sets bit 32 and N = 64 bit 63 of
    the mask words.  N = 2 has no room for an absent class: both of its classes are blocks.
    Returns dict(seg int32 [shape], lut int32, k class map (long, -1 = none), gt float64 one-hot [shape, N], absent)"""
    import torch
    g = torch.Generator().manual_seed(SEED + 77 * N + shape[0])
    lut_n = 2 * N + 8
    values = torch.randperm(lut_n, generator=g)
    label_list, unlisted = values[:N], values[N:]
    lut = torch.full((lut_n,), -1, dtype=torch.int32)
    lut[label_list] = torch.arange(N, dtype=torch.int32)
    grid = [-(-s // b) for s, b in zip(shape, (2, 3, 4))]
    absent = N - 2 if N > 2 else None
    # the classes of the blocks; the first two share 60 % of the blocks, the first one towards low x and the second towards
    # high x, so that even a window as large as the volume (SHAPE, d = 5) sees each on both sides of a third
    used = torch.tensor(sorted({1, 2, N // 2, N - 1} - {absent}) if N > 2 else [0, 1])
    t = (torch.arange(grid[2]).float() / max(grid[2] - 1, 1)).expand(*grid)
    rest = used[torch.randint(0, len(used), grid, generator=g)] if N > 2 else torch.full(grid, -1)
    pair = torch.where(torch.rand(grid, generator=g) > t, used[0], used[1])
    blocks = torch.where(torch.rand(grid, generator=g) < .6, pair, rest)
    cls = blocks.repeat_interleave(2, 0).repeat_interleave(3, 1).repeat_interleave(4, 2)[:shape[0], :shape[1], :shape[2]]
    seg = torch.where(cls >= 0, label_list[cls.clamp_min(0)], unlisted[8]).to(torch.int32).contiguous()
    flat = seg.view(-1)
    pos = torch.randperm(flat.numel(), generator=g)
    if N > 2:
        flat[pos[0]] = int(label_list[0])                    # the single voxel of class 0
    flat[pos[1:9]] = unlisted[:8].to(torch.int32)            # values of the table mapped to -1
    flat[pos[9:12]] = torch.tensor([-3, lut_n, lut_n + 1000], dtype=torch.int32)   # values outside the table
    k = torch.where((seg >= 0) & (seg < lut_n), lut[seg.clamp(0, lut_n - 1).long()], torch.full_like(seg, -1)).long()
    gt = torch.zeros(*shape, N, dtype=torch.float64)
    for n in range(N):
        gt[..., n] = (k == n).double()
    return dict(N=N, shape=shape, seg=seg, lut=lut, k=k, gt=gt, absent=absent)


@pytest.mark.parametrize('N', sorted({n for _, n in HEADS}))
@pytest.mark.parametrize('shape,d', GEOMETRIES)
def test_integer_boundary_rule_is_the_float_rule(N, shape, d):
    """0 < 3 k < W reproduces [avg > 0][avg < 1/3 - 1e-4] bit for bit on every label map of the GPU tests, with skip_background
    on and off; the maps hold what those tests rely on: >= 2 classes with boundary and non-boundary voxels, a one-voxel class
    and an absent one (N > 2), voxels without a class"""
    c = label_case(N, shape)
    for skip in (True, False):
        bnd = boundary_map(c['gt'], d, skip).numpy() > 0
        want = np.zeros(shape, dtype=np.uint64)
        for n in range(N):
            want |= bnd[..., n].astype(np.uint64) << np.uint64(n)
        assert np.array_equal(integer_mask(c['k'], N, d, skip), want)
    bnd = boundary_map(c['gt'], d, False).numpy() > 0
    both = [n for n in range(N) if bnd[..., n].any() and not bnd[..., n].all()]
    assert len(both) >= 2, both
    assert int((c['k'] < 0).sum()) >= 11
    if N > 2:
        assert c['gt'][..., c['absent']].sum() == 0 and c['gt'][..., 0].sum() == 1 and bnd[..., N - 1].any()
    if d == 1:   # voxels OF a class on both sides of the rule: interior and boundary
        own = [n for n in range(N) if (bnd[..., n] & (c['k'].numpy() == n)).any() and (~bnd[..., n] & (c['k'].numpy() == n)).any()]
        assert len(own) >= 1, own


def test_same_avg_pool_is_avg_pool3d():
    import torch
    import torch.nn.functional as F
    for shape, d in ((BIG, 3), (BIG, 5), (SHAPE, 1), ((11, 12, 13), 5)):
        gt = label_case(5, shape)['gt']
        want = F.avg_pool3d(gt.permute(3, 0, 1, 2)[None], 2 * d + 1, stride=1, padding=d, count_include_pad=False)
        assert torch.equal(same_avg_pool(gt, d), want[0].permute(1, 2, 3, 0))


def test_restatement_without_weights_is_the_plain_dice():
    import torch
    from oracle import unet_ref as U
    c = label_case(5, SHAPE)
    g = torch.Generator().manual_seed(3)
    pred = torch.softmax(torch.randn(*SHAPE, 5, generator=g, dtype=torch.float64), -1)
    a, b = weighted_dice(c['gt'], pred), U.dice_loss(c['gt'], pred)
    assert abs(a.item() - b.item()) <= 1e-15
    # uniform fixed weights: the same mean; boundary weights change it; dynamic weights skip the absent class without NaN
    assert abs(weighted_dice(c['gt'], pred, class_weights=[2.] * 5).item() - b.item()) <= 1e-12
    assert abs(weighted_dice(c['gt'], pred, boundary_weights=.5, boundary_dist=1).item() - b.item()) > 1e-6
    dyn = weighted_dice(c['gt'], pred, class_weights=-1, boundary_weights=.5)
    assert np.isfinite(dyn.item())
    assert weighted_dice(torch.zeros_like(c['gt']), pred, class_weights=-1).item() == 0


# ------------------------------------------------------------------------------------------------ arguments
def test_dice_settings_are_checked(tmp_path):
    from synthsr_amd.segmentation_training import dice_settings
    assert dice_settings(5) == dict(class_weights=None, boundary_weights=0., boundary_dist=3, skip_background=True)
    assert dice_settings(5, -1)['class_weights'] == -1 and dice_settings(5, '-1')['class_weights'] == -1
    got = dice_settings(4, [1, 1, 2, 0], .5, 5, False)
    assert got == dict(class_weights=(.25, .25, .5, 0.), boundary_weights=.5, boundary_dist=5, skip_background=False)
    np.save(tmp_path / 'cw.npy', np.array([3., 1.]))
    assert dice_settings(2, str(tmp_path / 'cw.npy'))['class_weights'] == (.75, .25)
    for bad in (0, 6, -1, 2.5, True):
        with pytest.raises(ValueError, match='boundary_dist'):
            dice_settings(5, dice_boundary_dist=bad)
    for bad in ([1, 2, 3], [1, 1, 1, 1, -1], [0] * 5, [1, 1, 1, 1, float('nan')], 3):
        with pytest.raises(ValueError, match='class_weights'):
            dice_settings(5, bad)
    for bad in (-.5, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='boundary_weights'):
            dice_settings(5, dice_boundary_weights=bad)


@pytest.mark.parametrize('kw', [dict(dice_boundary_dist=0), dict(dice_boundary_dist=6), dict(dice_class_weights=[1., 2.]),
                                dict(dice_class_weights=[1., -1., 1.]), dict(dice_class_weights=[0., 0., 0.])])
def test_training_segmentation_refuses_bad_dice_settings(kw):
    """before anything is read or built (the label directory does not exist)"""
    from synthsr_amd.segmentation_training import training_segmentation
    with pytest.raises(ValueError, match='boundary_dist|class_weights'):
        training_segmentation('/nonexistent/labels', '/nonexistent/model', None, None, None, np.array([0, 2, 41]), **kw)


def test_loss_dice_checks_its_weights_before_it_runs():
    from synthsr_amd.unet import UNet3D
    net = UNet3D(24, [16, 16, 16, 1], 3, 3, 5, feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax',
                 table_only=True)
    p = inspect.signature(net.loss_dice).parameters
    assert [(n, p[n].default) for n in list(p)[3:]] == [('class_weights', None), ('boundary_weights', 0.), ('boundary_dist', 3),
                                                        ('skip_background', True)]
    for kw in (dict(boundary_weights=.5, boundary_dist=0), dict(boundary_weights=.5, boundary_dist=6),
               dict(class_weights=[1.] * 4), dict(class_weights=[-1.] + [1.] * 4), dict(class_weights=[0.] * 5),
               dict(boundary_weights=-1.)):
        with pytest.raises(ValueError):
            net.loss_dice(None, None, None, **kw)


def test_launcher_has_the_dice_flags():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'scripts'))
    try:
        import training_segmentation as launcher
    finally:
        sys.path.pop(0)
    from synthsr_amd.segmentation_training import training_segmentation
    positional = ['l', 'm', 'pm', 'ps', 'gl', 'sl']
    a = vars(launcher.build_parser().parse_args(positional))
    assert (a['dice_class_weights'], a['dice_boundary_weights'], a['dice_boundary_dist'], a['dice_skip_background']) == \
        (None, 0., 3, True)
    a = vars(launcher.build_parser().parse_args(positional + ['--dice_class_weights', '-1', '--dice_boundary_weights', '0.5',
                                                              '--dice_boundary_dist', '2', '--dice_no_skip_background']))
    assert (a['dice_class_weights'], a['dice_boundary_weights'], a['dice_boundary_dist'], a['dice_skip_background']) == \
        ('-1', .5, 2, False)
    params = inspect.signature(training_segmentation).parameters
    assert set(a) <= set(params)
    for name, default in (('dice_class_weights', None), ('dice_boundary_weights', 0.), ('dice_boundary_dist', 3),
                          ('dice_skip_background', True)):
        assert params[name].default == default
