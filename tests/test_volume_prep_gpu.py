"""Inference pre- and post-processing on the device (csrc/volume_prep.hip, predict.prepare_volume_device / predict_cropped) against
float64: scipy and the reference's goldens for the kernels alone, predict.prepare_volume / postprocess / prepare_hyperfine for the
steps built of them, the oracle U-Net for predict(preprocessing='device').

Bound: the project's fp32 bound for pointwise kernels, 2e-5 of max |reference| (tests/test_seg_training_gpu.py).  Every test
prints the device's distance from float64 and, next to it, that of the same steps evaluated in float32 by numpy
(tests/_volume_prep_oracle.py).  Inputs are cast to float32 first; the float64 references are built from the cast values."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _volume_prep_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, 'tests', 'golden', 'inference.npz')
BOUND = 2e-5
SENTINEL = -777.25
f32, f64 = np.float32, np.float64


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=f32)).cuda()


def _guarded(shape, pad=96):
    """(buffer filled with the sentinel, its middle as a contiguous tensor of `shape`)"""
    import torch
    n = int(np.prod(shape))
    big = torch.full((n + 2 * pad,), SENTINEL, dtype=torch.float32, device='cuda')
    return big, big[pad:pad + n].view(*shape)


def _report(what, dev, ref, host32):
    scale = np.abs(ref).max()
    d, o = np.abs(dev.astype(f64) - ref).max() / scale, np.abs(host32.astype(f64) - ref).max() / scale
    print('%s: device %.3g, float32 numpy %.3g of max |float64 reference| = %.4g' % (what, d, o, scale))
    return d


# ------------------------------------------------------------------------------------------------------------ blur
@pytest.mark.parametrize('shape', [(5, 7, 9), (2, 70, 3)])
@pytest.mark.parametrize('sigma', [0.25, 0.625, 2.0])
@pytest.mark.parametrize('axis', [0, 1, 2])
def test_blur_axis_vs_scipy(axis, sigma, shape):
    from scipy.ndimage import gaussian_filter1d
    from synthsr_amd import ops, volumes as V
    rng = np.random.RandomState(10 * axis + int(8 * sigma))
    x = (rng.rand(*shape) * 200 - 50).astype(f32)
    taps = V.gaussian_taps(sigma)
    big, out = _guarded(shape)
    got = ops.volume_blur_axis(_dev(x), axis, taps, out=out)
    assert got is out
    ref = gaussian_filter1d(x.astype(f64), sigma, axis=axis, mode='reflect')
    d = _report('blur axis %d sigma %g %s' % (axis, sigma, shape), out.cpu().numpy(), ref, O.blur_axis(x, axis, taps, f32))
    assert d <= BOUND
    big = big.cpu().numpy()
    assert np.all(big[:96] == SENTINEL) and np.all(big[-96:] == SENTINEL)


# ------------------------------------------------------------------------------------------------------------ resample
def _device_blur(x, sigmas):
    from synthsr_amd import ops, volumes as V
    x = _dev(x)
    for ax in range(3):
        if sigmas[ax] > 0:
            x = ops.volume_blur_axis(x, ax, V.gaussian_taps(sigmas[ax]))
    return x


def _numpy_blur(x, sigmas, dtype):
    from synthsr_amd import volumes as V
    for ax in range(3):
        if sigmas[ax] > 0:
            x = O.blur_axis(x, ax, V.gaussian_taps(sigmas[ax]), dtype)
    return np.asarray(x, dtype=dtype)


@pytest.mark.parametrize('case', ['down', 'up', 'mixed'])
def test_resample_clamp_vs_goldens(case):
    """down-sampling with blur, 5x up-sampling without, a permuted and flipped orientation; the box at a non-zero offset of
    channel 1 of a sentinel-filled [D][2] buffer"""
    import torch
    from synthsr_amd import ops, volumes as V
    z = np.load(GOLD)
    vol = z[case + '_vol'].astype(f32)
    ref = z[case + '_ras_vol']
    sigmas, M, shape, _ = V.resample_plan(vol.shape, z[case + '_aff'])
    off = (3, 1, 2)
    D = tuple(s + o + 2 for s, o in zip(shape, off))
    dst = torch.full(D + (2,), SENTINEL, dtype=torch.float32, device='cuda')
    out, mm = ops.volume_resample(_device_blur(vol, sigmas), M, shape, 'clamp', out=dst, offset=off, channel=1)
    assert out is dst
    got = dst.cpu().numpy()
    box = got[off[0]:off[0] + shape[0], off[1]:off[1] + shape[1], off[2]:off[2] + shape[2], 1].copy()
    host32 = O.sample(_numpy_blur(vol, sigmas, f32), M, shape, dtype=f32)
    d = _report('resample %s -> %s' % (case, shape), box, ref, host32)
    assert d <= BOUND
    from scipy.ndimage import gaussian_filter
    own = O.sample(gaussian_filter(vol.astype(f64), sigmas), M, shape)
    print('    against the float64 evaluation of the cast input: %.3g' % (np.abs(box - own).max() / np.abs(own).max()))
    assert np.array_equal(mm.cpu().numpy(), np.array([box.min(), box.max()], dtype=f32))
    got[off[0]:off[0] + shape[0], off[1]:off[1] + shape[1], off[2]:off[2] + shape[2], 1] = SENTINEL
    assert np.all(got == SENTINEL)


def test_resample_zero_outside_vs_golden():
    from synthsr_amd import ops, volumes as V
    z = np.load(GOLD)
    flo = z['like_flo'].astype(f32)
    ref = z['like_out']
    M = V.resample_like_matrix(z['mixed_ras_aff'], z['like_flo_aff'])
    out, mm = ops.volume_resample(_dev(flo), M, ref.shape, 'zero_outside')
    got = out.cpu().numpy()
    near = O.near_a_face(M, ref.shape, flo.shape)
    print('zero_outside: %d of %d voxels within 1e-9 of a face of the source grid are left out' % (near.sum(), near.size))
    assert near.sum() <= 1e-3 * near.size
    host32 = O.sample(flo, M, ref.shape, zero_outside=True, dtype=f32)
    d = _report('resample like', np.where(near, ref, got), ref, np.where(near, ref, host32))
    assert d <= BOUND
    assert 0.2 < (got == 0).mean() < 0.8
    assert np.array_equal(mm.cpu().numpy(), np.array([got.min(), got.max()], dtype=f32))


# ------------------------------------------------------------------------------------------------------------ prepare_volume
def _oblique_case():
    rng = np.random.RandomState(7)
    c, s = np.cos(0.03), np.sin(0.03)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    Pm = np.array([[0, 0, -1.0], [1.0, 0, 0], [0, -1.0, 0]])              # permuted, two axes flipped
    aff = np.eye(4)
    aff[:3, :3] = R @ Pm @ np.diag([0.8, 3.0, 1.0])
    aff[:3, 3] = [12.5, -30.0, 8.25]
    return rng.rand(24, 9, 31) * 700 + 20, aff, False


def _prepare_cases():
    rng = np.random.RandomState(0)
    yield 'identity-ct', (rng.rand(20, 35, 33) * 90 - 10, np.eye(4), True)
    rng = np.random.RandomState(3)
    yield 'anisotropic', (rng.rand(30, 22, 26) * 1000,
                          np.array([[-1.2, 0, 0, 40.], [0, 1.0, 0, -30.], [0, 0, 1.4, 5.], [0, 0, 0, 1.]]), False)
    yield 'oblique', _oblique_case()


@pytest.mark.parametrize('name', ['identity-ct', 'anisotropic', 'oblique'])
def test_prepare_volume_device_vs_host(name):
    import torch
    from synthsr_amd import volumes as V
    from synthsr_amd.predict import prepare_volume, prepare_volume_device
    im, aff, ct = dict(_prepare_cases())[name]
    im = im.astype(f32)
    S_ref, idx_ref, shape_ref, aff_ref = prepare_volume(im.astype(f64), aff, ct=ct)
    buf = torch.full(S_ref.shape, SENTINEL, dtype=torch.float32, device='cuda')
    S, idx, shape, aff2 = prepare_volume_device(im, aff, ct=ct, out=buf)
    assert S is buf and S.dtype == torch.float32
    assert np.array_equal(idx, idx_ref) and idx.dtype == idx_ref.dtype
    assert np.array_equal(shape, shape_ref) and shape.dtype == shape_ref.dtype
    assert np.array_equal(aff2, aff_ref)
    got = S.cpu().numpy()
    # the same steps in float32 numpy
    sigmas, M, _, _ = V.resample_plan(im.shape, aff)
    h = O.normalise(O.sample(_numpy_blur(np.clip(im, 0, 80) if ct else im, sigmas, f32), M, tuple(shape), dtype=f32), dtype=f32)
    box = tuple(slice(int(i), int(i + s)) for i, s in zip(idx, shape))
    d = _report('prepare_volume %s %s -> %s in %s' % (name, im.shape, tuple(shape), got.shape), got[box], S_ref[box], h)
    assert np.abs(got - S_ref).max() <= BOUND                               # absolute: the values lie in [0, 1]
    assert got[box].min() == 0.0 and got[box].max() == 1.0
    pad = np.ones(got.shape, dtype=bool)
    pad[box] = False
    assert pad.any() and np.all(got[pad] == 0.0)


# ------------------------------------------------------------------------------------------------------------ post-processing
def test_sr_postprocess_vs_host():
    import torch
    from synthsr_amd import ops
    from synthsr_amd.predict import postprocess, postprocess_hyperfine
    W, shape, idx = (32, 64, 64), np.array([20, 35, 33]), np.array([6, 14, 15])
    rng = np.random.RandomState(11)
    a, b = (rng.randn(*W) * 0.4 + 0.2).astype(f32), (rng.randn(*W) * 0.4 + 0.2).astype(f32)
    da, db = _dev(a), _dev(b)
    box = tuple(slice(int(i), int(i + s)) for i, s in zip(idx, shape))
    # the flip average: the asymmetric offset along axis 0 (6 of 12 spare planes would hide a wrong mirror index)
    ref = postprocess(0.5 * a.astype(f64) + 0.5 * np.flip(b.astype(f64), 0), idx, shape)
    big, out = _guarded(tuple(shape))
    got = ops.sr_postprocess(da, idx, shape, netf=db, a=255.0, b=0.0, lo=0.0, hi=128.0, out=out).cpu().numpy()
    h = np.clip(f32(255) * (f32(0.5) * a + f32(0.5) * np.flip(b, 0)), f32(0), f32(128))[box]
    assert _report('postprocess, flip average', got, ref, h) <= BOUND
    assert (ref == 0).any() and (ref == 128).any()
    big = big.cpu().numpy()
    assert np.all(big[:96] == SENTINEL) and np.all(big[-96:] == SENTINEL)
    ref = postprocess(a.astype(f64), idx, shape)
    got = ops.sr_postprocess(da, idx, shape, a=255.0, b=0.0, lo=0.0, hi=128.0).cpu().numpy()
    assert _report('postprocess, one pass', got, ref, np.clip(f32(255) * a, f32(0), f32(128))[box]) <= BOUND
    # Hyperfine: residual on the normalised T1, which lies in channel 0 of the network's input
    S = (rng.rand(*W, 2) * 3).astype(f32)
    minimum, spread = f32(-17.5), f32(231.0625)
    t1n = S[box + (0,)]
    ref = postprocess_hyperfine(a.astype(f64), idx, shape, (float(minimum), float(spread)), t1n.astype(f64))
    dS = _dev(S)
    got = ops.sr_postprocess(da, idx, shape, addend=dS[box + (0,)], a=float(spread), b=float(minimum), lo=0.0,
                             hi=np.inf).cpu().numpy()
    h = np.maximum(minimum + spread * (a[box] + t1n), f32(0))
    assert _report('postprocess_hyperfine', got, ref, h) <= BOUND
    assert (ref == 0).any()


# ------------------------------------------------------------------------------------------------------------ Hyperfine
def test_prepare_hyperfine_device_vs_host():
    from synthsr_amd import volumes as V
    from synthsr_amd.predict import prepare_hyperfine, prepare_hyperfine_device
    rng = np.random.RandomState(5)
    aff1 = np.array([[1.5, 0, 0, -20.], [0, 1.5, 0, -18.], [0, 0, 5.0, -30.], [0, 0, 0, 1.]])
    aff2 = aff1 @ np.array([[1, 0.02, 0, 0.5], [-0.02, 1, 0, -0.4], [0, 0, 1, 0.3], [0, 0, 0, 1.]])
    im1, im2 = (rng.rand(24, 22, 8) * 400 + 30).astype(f32), (rng.rand(20, 24, 7) * 900).astype(f32)
    S_ref, idx_ref, shape_ref, aff_ref, (min_ref, spread_ref), t1_ref = prepare_hyperfine(im1.astype(f64), aff1, im2.astype(f64), aff2)
    S, idx, shape, aff_mod, (minimum, spread), t1n = prepare_hyperfine_device(im1, aff1, im2, aff2)
    assert np.array_equal(idx, idx_ref) and np.array_equal(shape, shape_ref) and np.array_equal(aff_mod, aff_ref)
    got = S.cpu().numpy()
    assert got.shape == S_ref.shape and got.dtype == f32
    box = tuple(slice(int(i), int(i + s)) for i, s in zip(idx, shape))
    near = O.near_a_face(V.resample_like_matrix(aff_mod, aff2), tuple(shape), im2.shape)
    print('hyperfine T2: %d of %d voxels within 1e-9 of a face of the T2 grid are left out' % (near.sum(), near.size))
    assert near.sum() <= 1e-3 * near.size
    sigmas, M, _, _ = V.resample_plan(im1.shape, aff1)
    h1 = O.normalise(O.sample(_numpy_blur(im1, sigmas, f32), M, tuple(shape), dtype=f32), 3.0, f32)
    h2 = O.normalise(O.sample(im2, V.resample_like_matrix(aff_mod, aff2), tuple(shape), True, f32), 2.0, f32)
    _report('hyperfine T1 (gain 3)', got[box + (0,)], S_ref[box + (0,)], h1)
    _report('hyperfine T2 (gain 2)', np.where(near, S_ref[box + (1,)], got[box + (1,)]), S_ref[box + (1,)],
            np.where(near, S_ref[box + (1,)], h2))
    assert np.abs(got[..., 0] - S_ref[..., 0]).max() <= 3 * BOUND
    keep = np.ones(S_ref.shape[:3], dtype=bool)
    keep[box] = ~near
    assert np.abs(got[..., 1] - S_ref[..., 1])[keep].max() <= 2 * BOUND
    pad = np.ones(S_ref.shape[:3], dtype=bool)
    pad[box] = False
    assert np.all(got[pad] == 0.0)
    assert got[box + (0,)].min() == 0.0 and got[box + (0,)].max() == 3.0 and got[box + (1,)].max() == 2.0
    # what the post-processing needs
    top = np.abs(im1).max()
    assert abs(minimum - min_ref) <= BOUND * top and abs(spread - spread_ref) <= BOUND * top
    assert t1n.is_cuda and tuple(t1n.shape) == tuple(shape) and np.array_equal(t1n.cpu().numpy(), got[box + (0,)])
    assert np.abs(t1n.cpu().numpy() - t1_ref).max() <= 3 * BOUND


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def scan_and_model(tmp_path_factory):
    """the set-up of tests/test_inference.py::test_predict_end_to_end_vs_oracle"""
    import torch
    from synthsr_amd import volumes as V
    from synthsr_amd.training import save_checkpoint
    from synthsr_amd.unet import unet
    tmp = tmp_path_factory.mktemp('volume_prep')
    rng = np.random.RandomState(3)
    vol = rng.rand(30, 22, 26) * 1000
    aff = np.array([[-1.2, 0, 0, 40.], [0, 1.0, 0, -30.], [0, 0, 1.4, 5.], [0, 0, 0, 1.]])
    pin = str(tmp / 'scan.nii.gz')
    V.save_volume(vol, aff, None, pin)
    net = unet(24, [32, 32, 32, 1], 5, 3, 1, feat_mult=2, nb_conv_per_level=2, batch_norm=-1, activation='elu',
               final_pred_activation='linear', seed=1)
    g = torch.Generator().manual_seed(0)
    net.bn_moving.copy_((torch.rand(net.bn_moving.shape, generator=g) * 0.5 + 0.25).to(net.bn_moving.device))
    ck = str(tmp / 'model.npz')
    save_checkpoint(ck, net)
    P = {k: v.float().cpu() for k, v in net.state_dict().items()}
    return dict(tmp=tmp, pin=pin, ck=ck, P=P, prefix=net.prefix)


@pytest.mark.parametrize('flip', [True, False])
def test_predict_device_preprocessing_vs_oracle(scan_and_model, flip):
    """predict(preprocessing='device') against the oracle's inference forward on the DEVICE-prepared volume (downloaded),
    post-processed on the host: 2e-4 of the output range, the bound of test_predict_end_to_end_vs_oracle"""
    import torch
    from synthsr_amd import volumes as V
    from synthsr_amd.predict import predict, prepare_volume, prepare_volume_device, postprocess
    from oracle import unet_ref as U
    e = scan_and_model
    pout = str(e['tmp'] / ('flip%d' % flip) / 'pred.nii.gz')
    predict(e['pin'], pout, path_model=e['ck'], disable_flipping=not flip, verbose=False, preprocessing='device')
    got, aff_out, _ = V.load_volume(pout, im_only=False)
    im, aff_in, _ = V.load_volume(e['pin'], im_only=False, dtype='float')
    S, idx, shape, aff2 = prepare_volume_device(im, aff_in)
    _, idx_h, shape_h, aff_h = prepare_volume(im, aff_in)
    assert tuple(S.shape) == (64, 32, 64) and np.array_equal(idx, idx_h) and np.array_equal(shape, shape_h)
    assert np.array_equal(aff2, aff_h)
    np.testing.assert_allclose(aff_out, aff_h, atol=1e-5)
    x = S.cpu()[..., None]
    P = e['P']
    with torch.no_grad():
        out = U.unet_forward(x, P, e['prefix'], 5, 2, training=False, moving=P)[..., 0]
        if flip:
            outf = U.unet_forward(torch.flip(x, dims=[0]), P, e['prefix'], 5, 2, training=False, moving=P)[..., 0]
            out = 0.5 * out + 0.5 * torch.flip(outf, dims=[0])
    ref = postprocess(out.numpy(), idx, shape)
    assert got.shape == ref.shape == tuple(shape)
    scale = max(np.abs(255 * out.numpy()).max(), 1.0)
    err = np.abs(got - ref).max() / scale
    print('predict(preprocessing=device), flip %s: %.3g of the output range %.4g' % (flip, err, scale))
    assert err < 2e-4
    assert ref.std() > 0


def test_script_with_device_preprocessing(scan_and_model):
    from synthsr_amd import volumes as V
    from synthsr_amd.predict import predict
    e = scan_and_model
    spec = importlib.util.spec_from_file_location('predict_command_line', os.path.join(ROOT, 'scripts', 'predict_command_line.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    pout, pref = str(e['tmp'] / 'script' / 'pred.nii.gz'), str(e['tmp'] / 'script' / 'ref.nii.gz')
    mod.main([e['pin'], pout, '--model', e['ck'], '--preprocessing', 'device'])
    predict(e['pin'], pref, path_model=e['ck'], verbose=False, preprocessing='device')
    got, aff_got, _ = V.load_volume(pout, im_only=False)
    ref, aff_ref, _ = V.load_volume(pref, im_only=False)
    # two runs of the network differ in their last bits (float atomics in its statistics), so the script's file is held to the
    # function's by the end-to-end bound above, 2e-4, here of the written range [0, 128]
    err = np.abs(got - ref).max() / 128.0
    print('script against predict(): %.3g of the written range' % err)
    assert got.shape == ref.shape and got.std() > 0 and err < 2e-4 and np.array_equal(aff_got, aff_ref)
