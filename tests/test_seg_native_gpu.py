"""Label maps on the input image's own voxel grid, on the device (csrc/seg_resample.hip through ops.seg_resample_argmax,
SegmentationPredictor.segment_volume(native=...) and predict_segmentation(native_space=True)).

The reference is the float64 oracle of tests/_seg_native_oracle.py (tests/test_seg_native_cpu.py holds it against the host
resampler).  Where the weights are 0 or 1 the device must return the source rows and their argmax bit for bit.  Elsewhere:
  posteriors  |device - oracle| <= 2e-6 absolute.  A convex combination of values <= 1 whose terms each pass through at most 14
              fp32 roundings (the weight's rounding, 1 - w, two products, the multiply-add, seven further additions) is off by at
              most 14 * 2^-24 = 8.3e-7; the factor 2 is left for another summation order or FMA contraction.
  labels      equal wherever the oracle's two largest posteriors are more than 1e-5 apart (five times the bound above on either
              of them); the voxels at or below that margin are left out, and may be at most 0.5 % of the inside voxels, which is
              asserted on the oracle before the device is looked at.
  boundaries  no coordinate may lie within 1e-9 of lo - 0.5 or hi + 0.5: the oracle counts them and the test fails on any."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _seg_native_oracle as O  # noqa: E402

SRC, BOX = (16, 24, 40), (2, 1, 3, 13, 22, 36)
LO, HI = np.array(BOX[:3]), np.array(BOX[3:])
GUARD, GARBAGE, CANARY = 64, int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0]), -777.25
PROB_TOL, MARGIN, MAX_EXCLUDED = 2e-6, 1e-5, 0.005
FILL = -7


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


@functools.lru_cache(maxsize=None)
def source(N):
    p = O.softmax_posteriors(SRC, N, seed=100 + N)
    p.setflags(write=False)
    return p


def label_values(N):
    return (3 * np.arange(N) + 2).astype(np.int32)[::-1].copy()      # not sorted, none equal to its channel


@functools.lru_cache(maxsize=None)
def _device_source(N):
    import torch
    return torch.from_numpy(source(N).copy()).cuda()


def run_device(torch, probs, box, M, out_shape, labels, fill_value=FILL):
    """(out, probs_out) on the host; both outputs sit in front of canary words, and the call without probs_out must give the
    same map"""
    from synthsr_amd import ops
    N = probs.shape[3]
    n = int(np.prod(out_shape))
    dp = _device_source(N) if probs is source(N) else torch.from_numpy(np.ascontiguousarray(probs)).cuda()
    dl = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)).cuda()
    obuf = torch.full((n + GUARD,), GARBAGE, dtype=torch.int32, device='cuda')
    pbuf = torch.full((n * N + GUARD,), CANARY, dtype=torch.float32, device='cuda')
    before = dp.clone()
    out, pout = ops.seg_resample_argmax(dp, box, M, out_shape, dl, fill_value, out=obuf[:n].view(*out_shape),
                                        probs_out=pbuf[:n * N].view(*out_shape, N))
    alone = ops.seg_resample_argmax(dp, box, M, out_shape, dl, fill_value)
    torch.cuda.synchronize()
    assert out.data_ptr() == obuf.data_ptr() and pout.data_ptr() == pbuf.data_ptr()
    assert bool((obuf[n:] == GARBAGE).all()) and bool((pbuf[n * N:] == CANARY).all()), 'canary overwritten'
    assert torch.equal(dp, before), 'the source was written'
    assert alone.dtype == torch.int32 and tuple(alone.shape) == tuple(out_shape)
    assert torch.equal(alone, out), 'the map depends on whether the posteriors are asked for'
    return out.cpu().numpy(), pout.cpu().numpy()


def check_against_oracle(torch, what, N, M, out_shape, box=BOX, probs=None):
    probs = source(N) if probs is None else probs
    labels = label_values(N)
    want = O.resample_argmax(probs, box, M, out_shape, labels, FILL)
    inside = want['inside']
    assert want['near_boundary'] == 0, '%s: %d voxels sit on an inside / outside boundary' % (what, want['near_boundary'])
    excluded = inside & (want['margin'] <= MARGIN)
    share = excluded.sum() / max(int(inside.sum()), 1)
    assert share <= MAX_EXCLUDED, '%s: %.3g of the inside voxels are within the margin' % (what, share)
    out, pout = run_device(torch, probs, box, M, out_shape, labels)
    err = float(np.abs(pout - want['probs']).max())
    wrong = int(((out != want['label']) & ~excluded).sum())
    print('%s N = %d -> %s: %d of %d voxels inside, %d within the margin, posteriors off by %.3g, %d labels differ'
          % (what, N, tuple(out_shape), int(inside.sum()), inside.size, int(excluded.sum()), err, wrong))
    assert out.dtype == np.int32 and pout.dtype == np.float32
    assert np.all(out[~inside] == FILL) and np.all(pout[~inside] == 0), 'outside voxels: the fill value and zero posteriors'
    assert err <= PROB_TOL, what
    assert wrong == 0, what
    return want, out, pout


def oblique(scales=(0.37, 0.9, 1.7), offset=(3.2, 5.1, -0.4), angle=0.3, axis=0):
    c, s = np.cos(angle), np.sin(angle)
    R = np.eye(3)
    a, b = [x for x in range(3) if x != axis]
    R[a, a], R[a, b], R[b, a], R[b, b] = c, -s, s, c
    return np.concatenate([R @ np.diag(scales), np.asarray(offset, dtype=np.float64).reshape(3, 1)], axis=1)


# ---------------------------------------------------------------------------------------------------- exact
def test_identity_over_the_box_returns_the_rows(T):
    for N in (5, 33):
        probs, labels = source(N), label_values(N)
        M = np.concatenate([np.eye(3), LO.reshape(3, 1).astype(np.float64)], axis=1)
        shape = tuple(HI - LO + 1)
        out, pout = run_device(T, probs, BOX, M, shape, labels)
        rows = probs[LO[0]:HI[0] + 1, LO[1]:HI[1] + 1, LO[2]:HI[2] + 1]
        assert np.array_equal(pout.view(np.uint32), rows.view(np.uint32))
        assert np.array_equal(out, labels[np.argmax(rows, -1)])


def test_permutation_flip_and_offset_returns_the_rows(T):
    """output (i, j, k) -> source (hi0 - j, lo1 + k, lo2 + 3 + i); the output is a little larger than what falls inside"""
    N = 33
    probs, labels = source(N), label_values(N)
    M = np.array([[0, -1.0, 0, HI[0]], [0, 0, 1.0, LO[1]], [1.0, 0, 0, LO[2] + 3]])
    shape = (33, 13, 23)
    out, pout = run_device(T, probs, BOX, M, shape, labels)
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    z, y, x = HI[0] - j, LO[1] + k, LO[2] + 3 + i
    inside = (z >= LO[0]) & (y <= HI[1]) & (x <= HI[2])
    assert 0 < (~inside).sum() < inside.sum()
    rows = probs[np.clip(z, 0, SRC[0] - 1), np.clip(y, 0, SRC[1] - 1), np.clip(x, 0, SRC[2] - 1)]
    rows = np.where(inside[..., None], rows, np.float32(0))
    assert np.array_equal(pout.view(np.uint32), rows.view(np.uint32))
    assert np.array_equal(out, np.where(inside, labels[np.argmax(rows, -1)], FILL))


@pytest.mark.parametrize('N,pair', [(5, (1, 3)), (33, (2, 10)), (64, (17, 63))])
def test_equal_channels_give_the_lower_one(T, N, pair):
    """two channels equal everywhere and larger than the rest: in different lanes of a voxel's group (1, 3), in one lane
    (2, 10: both channel = 2 mod 8) and in the last lane's last slot (63)"""
    probs = source(N).copy()
    top = probs.max(-1) + np.float32(0.125)
    probs[..., pair[0]] = top
    probs[..., pair[1]] = top
    labels = label_values(N)
    ident = np.concatenate([np.eye(3), LO.reshape(3, 1).astype(np.float64)], axis=1)
    for M, shape in ((ident, tuple(HI - LO + 1)), (oblique(), (40, 28, 26))):
        want = O.resample_argmax(probs, BOX, M, shape, labels, FILL)
        out, pout = run_device(T, probs, BOX, M, shape, labels)
        assert np.array_equal(pout[..., pair[0]].view(np.uint32), pout[..., pair[1]].view(np.uint32))
        assert np.array_equal(out, np.where(want['inside'], labels[pair[0]], FILL))
        assert want['inside'].sum() > 0 and np.array_equal(out, want['label'])


# ---------------------------------------------------------------------------------------------------- against float64
@pytest.mark.parametrize('N', [2, 5, 33, 64])
def test_oblique_matrix(T, N):
    want, _, _ = check_against_oracle(T, 'oblique', N, oblique(), (40, 28, 26))
    outside = 1.0 - want['inside'].mean()
    assert 0.3 < outside < 0.7, outside              # 55 % of the voxels of this grid fall outside the box


@pytest.mark.parametrize('N', [5, 33])
def test_upsampling_by_two(T, N):
    M = np.concatenate([0.5 * np.eye(3), (LO - 0.25).reshape(3, 1)], axis=1)
    want, _, _ = check_against_oracle(T, 'x2', N, M, tuple(2 * (HI - LO + 1) + 2))     # two planes past the box on each axis
    assert 0 < (~want['inside']).sum() < want['inside'].sum()


@pytest.mark.parametrize('axis', [0, 2])
def test_thick_slices(T, axis):
    scale = np.ones(3)
    scale[axis] = 5.0
    M = np.concatenate([np.diag(scale), LO.reshape(3, 1).astype(np.float64)], axis=1)
    shape = list(HI - LO + 1)
    shape[axis] = (HI[axis] - LO[axis]) // 5 + 2                                       # the last slice lies outside
    want, _, _ = check_against_oracle(T, 'thick slices along %d' % axis, 33, M, tuple(shape))
    assert (~want['inside']).sum() == np.prod(shape) // shape[axis]


@pytest.mark.parametrize('shape', [(1, 1, 1), (3, 5, 67), (2, 2, 130)])
def test_launch_edges(T, shape):
    """one voxel; more than one tile along k with a ragged end; 130 = 8 tiles of 16 and two voxels"""
    scale = (np.array(HI - LO, dtype=np.float64) - 0.3) / np.maximum(np.array(shape) - 1, 1)
    M = np.concatenate([np.diag(scale), (LO + 0.15).reshape(3, 1)], axis=1)
    want, _, _ = check_against_oracle(T, 'edge', 33, M, shape)
    assert want['inside'].all()
    check_against_oracle(T, 'edge', 5, oblique(offset=(5.2, 9.1, 11.6)), shape)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_box_one_voxel_thick(T, axis):
    box = list(BOX)
    box[axis] = box[3 + axis] = 7
    scales, offset = [0.9, 0.9, 0.9], [LO[0] + 0.2, LO[1] + 0.2, LO[2] + 0.2]
    scales[axis], offset[axis] = 0.31, 7 - 0.45                   # -0.45, -0.14, 0.17, 0.48 inside; 0.79, ... outside
    M = np.concatenate([np.diag(scales), np.array(offset).reshape(3, 1)], axis=1)
    shape = [9, 11, 19]
    shape[axis] = 6
    want, out, pout = check_against_oracle(T, 'box one voxel thick along %d' % axis, 33, M, tuple(shape), box=tuple(box))
    assert want['inside'].sum() * 6 == 4 * want['inside'].size
    assert all(np.all(i == 7) for i in want['index'][axis]) and np.all(want['weight'][axis] == 0)


# ---------------------------------------------------------------------------------------------------- end to end
E2E_LABELS = np.array([0, 14, 2, 41, 17], dtype=np.int32)


@pytest.fixture(scope='module')
def e2e(T, tmp_path_factory):
    """random-weight networks (3 levels, 5 labels; 4 features, and 8 for bf16: the bf16 convs take channel counts that are
    multiples of 8) and a 20 x 18 x 12 image of 1.5 x 1.5 x 3 mm voxels, PIL-like"""
    torch = T
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.unet import unet
    from synthsr_amd.training import save_checkpoint
    from synthsr_amd.predict_segmentation import SegmentationPredictor
    d = tmp_path_factory.mktemp('seg_native')
    rng = np.random.default_rng(11)
    im = (rng.random((20, 18, 12)) * 100).astype(np.float32)
    im[4:15, 3:14, 2:9] += 150
    aff = np.array([[0, -1.5, 0, 14.0], [-1.5, 0, 0, 9.5], [0, 0, -3.0, 21.25], [0, 0, 0, 1]])
    scan = str(d / 'scan.nii')
    write_nifti(scan, im, aff)
    feats, ckpts, predictors = {'f32': 4, 'bf16': 8}, {}, {}
    for dt, feat in feats.items():
        net = unet(nb_features=feat, input_shape=[32, 32, 32, 1], nb_levels=3, conv_size=3, nb_labels=len(E2E_LABELS),
                   feat_mult=2, nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax', seed=3)
        net.view(net.head['w']).copy_(torch.randn(feat, len(E2E_LABELS), generator=torch.Generator().manual_seed(6)))
        ckpts[dt] = str(d / ('seg_%s.npz' % dt))
        save_checkpoint(ckpts[dt], net)
        predictors[dt] = SegmentationPredictor(ckpts[dt], E2E_LABELS, n_levels=3, unet_feat_count=feat, dtype=dt)
    return dict(dir=d, scan=scan, im=im, aff=aff, ckpt=ckpts['f32'], predictors=predictors, feats=feats,
                arch=dict(n_levels=3, unet_feat_count=4, verbose=False))


@pytest.mark.parametrize('dtype,flipping', [('f32', True), ('f32', False), ('bf16', True)])
def test_predict_segmentation_in_native_space(T, e2e, dtype, flipping):
    from synthsr_amd import volumes as V
    from synthsr_amd.nifti import read_nifti
    from synthsr_amd.predict import prepare_volume
    from synthsr_amd.predict_segmentation import predict_segmentation, native_grid_affine
    d, predictor = e2e['dir'], e2e['predictors'][dtype]
    tag = '%s_%d' % (dtype, flipping)
    pairs = [[14, 41]]
    seg, post = str(d / ('native_%s.nii' % tag)), str(d / ('native_post_%s.nii' % tag))
    outs = predict_segmentation(e2e['scan'], seg, None, E2E_LABELS, path_posteriors=post, lr_pairs=pairs,
                                disable_flipping=not flipping, predictor=predictor, dtype=dtype, native_space=True, n_levels=3,
                                unet_feat_count=e2e['feats'][dtype], verbose=False)
    assert outs == [seg]
    got, got_aff, _ = read_nifti(seg)
    got_post, post_aff, _ = read_nifti(post)
    assert got.dtype == np.int32 and got.shape == e2e['im'].shape and got_post.shape == e2e['im'].shape + (5,)
    assert np.array_equal(got_aff, e2e['aff']) and np.array_equal(post_aff, e2e['aff'])
    # the 1 mm posteriors of the same predictor, and the oracle on them
    im, aff, _ = V.load_volume(e2e['scan'], im_only=False, dtype='float')
    S, idx, shape, aff2 = prepare_volume(im, aff)
    crop = tuple(slice(int(o), int(o) + int(n)) for o, n in zip(idx, shape))
    _, probs = predictor.segment_volume(S, flipping=flipping, lr_pairs=pairs, return_posteriors=True, crop=crop)
    assert probs.shape == tuple(shape) + (5,) and probs.dtype == np.float32
    M = native_grid_affine(aff, aff2, np.zeros(3))
    want = O.resample_argmax(probs, [0, 0, 0] + [int(n) - 1 for n in shape], M, im.shape, E2E_LABELS, int(E2E_LABELS[0]))
    inside = want['inside']
    assert want['near_boundary'] == 0 and inside.mean() > 0.9
    excluded = inside & (want['margin'] <= MARGIN)
    assert excluded.sum() <= MAX_EXCLUDED * inside.sum()
    err = float(np.abs(got_post - want['probs']).max())
    wrong = int(((got != want['label']) & ~excluded).sum())
    print('%s: %d of %d voxels inside, %d within the margin, posteriors off by %.3g, %d labels differ, %d labels present'
          % (tag, inside.sum(), inside.size, excluded.sum(), err, wrong, len(np.unique(got))))
    assert err <= PROB_TOL and wrong == 0
    assert len(np.unique(got)) >= 3, 'the map of this network is not trivial'


def test_native_space_with_the_largest_components_and_without(T, e2e):
    from synthsr_amd.nifti import read_nifti
    from synthsr_amd.predict_segmentation import predict_segmentation, keep_largest_components
    d, predictor = e2e['dir'], e2e['predictors']['f32']
    common = dict(predictor=predictor, **e2e['arch'])
    raw = predict_segmentation(e2e['scan'], str(d / 'raw.nii'), e2e['ckpt'], E2E_LABELS, native_space=True, **common)
    kept = predict_segmentation(e2e['scan'], str(d / 'kept.nii'), e2e['ckpt'], E2E_LABELS, native_space=True,
                                keep_largest='per_label', **common)
    a, b = read_nifti(raw[0])[0], read_nifti(kept[0])[0]
    assert a.shape == e2e['im'].shape and np.array_equal(b, keep_largest_components(a, E2E_LABELS))
    assert (a != b).sum() > 0, 'the raw argmax of this network has stray components'
    # another fill label: outside voxels and removed voxels take it
    filled = predict_segmentation(e2e['scan'], str(d / 'filled.nii'), e2e['ckpt'], E2E_LABELS, native_space=True,
                                  keep_largest='foreground', connectivity=26, fill_label=2, **common)
    assert np.array_equal(read_nifti(filled[0])[0], keep_largest_components(a, E2E_LABELS, 'foreground', 26, 2))
    # native_space=False is what a call without the argument writes, byte for byte
    for name, kw in (('plain', {}), ('false', dict(native_space=False))):
        predict_segmentation(e2e['scan'], str(d / (name + '.nii')), e2e['ckpt'], E2E_LABELS,
                             path_posteriors=str(d / (name + '_post.nii')), keep_largest='per_label', **kw, **common)
    for suffix in ('.nii', '_post.nii'):
        assert open(d / ('plain' + suffix), 'rb').read() == open(d / ('false' + suffix), 'rb').read()
    assert read_nifti(str(d / 'plain.nii'))[0].shape != e2e['im'].shape      # the 1 mm RAS frame
