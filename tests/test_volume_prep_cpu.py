"""Host side of inference pre- and post-processing on the device (no GPU): volumes.gaussian_taps against scipy, the matrix, shape
and affine of volumes.resample_plan against the reference's goldens (tests/golden/inference.npz), resample_like_matrix, the
declarations and the refusals of the four C entry points of csrc/volume_prep.hip (they return before any HIP call), the checks of
their ops wrappers, and the `preprocessing` keyword and flag."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden', 'inference.npz')
ENTRY_POINTS = {'synthsr_volume_blur_axis': 7, 'synthsr_volume_resample': 14, 'synthsr_volume_normalise_pad': 9,
                'synthsr_sr_postprocess': 13}


def sample_through_matrix(vol, M, out_shape, zero_outside=False):
    """float64 evaluation of the contract of synthsr_volume_resample (include/synthsr_hip.h) with exact weights: positions
    M (i, j, k, 1), clamp or zero outside, the corner rule of volumes._interp_axis, trilinear.  Also returns the positions."""
    g = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in out_shape], indexing='ij'), 0)
    M = np.asarray(M, dtype=np.float64)
    pos = np.einsum('ab,b...->a...', M[:3, :3], g) + M[:3, 3].reshape(3, 1, 1, 1)
    n = np.array(vol.shape).reshape(3, 1, 1, 1)
    inside = np.all((pos >= 0) & (pos <= n - 1), axis=0)
    p = np.clip(pos, 0, n - 1)
    i0 = np.minimum(np.floor(p).astype(np.int64), np.maximum(n - 2, 0))
    i1 = np.minimum(i0 + 1, n - 1)
    w = p - i0
    out = np.zeros(out_shape)
    for c0 in (0, 1):
        for c1 in (0, 1):
            for c2 in (0, 1):
                wt = (w[0] if c0 else 1 - w[0]) * (w[1] if c1 else 1 - w[1]) * (w[2] if c2 else 1 - w[2])
                out += wt * vol[(i1 if c0 else i0)[0], (i1 if c1 else i0)[1], (i1 if c2 else i0)[2]]
    if zero_outside:
        out[~inside] = 0.0
    return out, pos


@pytest.mark.parametrize('sigma', [0.25, 0.3125, 0.625, 2.0])
def test_gaussian_taps_are_scipys(sigma):
    from scipy.ndimage import gaussian_filter1d
    from synthsr_amd import volumes as V
    taps = V.gaussian_taps(sigma)
    r = int(4 * sigma + 0.5)
    assert taps.dtype == np.float32 and taps.shape == (2 * r + 1,)
    impulse = np.zeros(4 * r + 9)
    impulse[2 * r + 4] = 1.0
    want = gaussian_filter1d(impulse, sigma, mode='reflect')
    assert np.all(want[:r + 4] == 0) and np.all(want[-(r + 4):] == 0)
    want = want[r + 4:-(r + 4)]
    err = np.abs(taps.astype(np.float64) - want).max()
    print('sigma %g: radius %d, taps against scipy on an impulse %.3g' % (sigma, r, err))
    assert np.all(np.abs(taps.astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want))     # float32 rounding, tap by tap
    assert abs(float(taps.astype(np.float64).sum()) - 1.0) < (2 * r + 1) * 2.0 ** -24


def test_gaussian_taps_radius_limit():
    from synthsr_amd import volumes as V
    assert len(V.gaussian_taps(4.12)) == 33
    with pytest.raises(ValueError, match='host path'):
        V.gaussian_taps(4.2)
    aff = np.diag([0.05, 1.0, 1.0, 1.0])                          # 0.05 mm voxels: sigma 5
    with pytest.raises(ValueError, match='host path'):
        V.resample_plan((8, 8, 8), aff)


@pytest.mark.parametrize('case', ['down', 'up', 'mixed'])
def test_resample_plan_against_the_goldens(case):
    from scipy.ndimage import gaussian_filter
    from synthsr_amd import volumes as V
    z = np.load(GOLD)
    vol, aff = z[case + '_vol'], z[case + '_aff']
    sigmas, M, shape, aff_ras = V.resample_plan(vol.shape, aff)
    assert shape == z[case + '_ras_vol'].shape and all(type(s) is int for s in shape)
    np.testing.assert_allclose(aff_ras, z[case + '_ras_aff'], rtol=0, atol=1e-12)
    # exactly what the host functions return
    v2, a2 = V.resample_volume(vol, aff, [1.0, 1.0, 1.0])
    v3, a3 = V.align_volume_to_ref(v2, a2, aff_ref=np.eye(4), return_aff=True, n_dims=3)
    assert shape == v3.shape and np.array_equal(aff_ras, a3)
    assert M.shape == (3, 4) and M.dtype == np.float64
    got, _ = sample_through_matrix(gaussian_filter(vol, sigmas), M, shape)
    err = np.abs(got - z[case + '_ras_vol']).max()
    print('%s: sigmas %s, M + clamp + corner rule against the golden %.3g' % (case, sigmas, err))
    assert err <= 1e-10
    if case == 'up':
        assert np.all(sigmas == 0)
    if case == 'mixed':
        assert np.count_nonzero(M[:, :3]) == 3 and not np.array_equal(np.abs(M[:, :3]) > 0, np.eye(3, dtype=bool))
        assert (M[:, :3] < 0).any()


def test_resample_like_matrix():
    from synthsr_amd import volumes as V
    z = np.load(GOLD)
    M = V.resample_like_matrix(z['mixed_ras_aff'], z['like_flo_aff'])
    assert M.shape == (3, 4) and M.dtype == np.float64 and M.flags['C_CONTIGUOUS']
    assert np.array_equal(M, (np.linalg.inv(z['like_flo_aff']) @ z['mixed_ras_aff'])[:3])
    got, pos = sample_through_matrix(z['like_flo'], M, z['like_out'].shape, zero_outside=True)
    n = np.array(z['like_flo'].shape).reshape(3, 1, 1, 1)
    near = np.any((np.abs(pos) < 1e-9) | (np.abs(pos - (n - 1)) < 1e-9), axis=0)
    print('like: %d of %d voxels within 1e-9 of a face of the floating grid' % (near.sum(), near.size))
    assert near.sum() <= 1e-3 * near.size
    assert np.abs(got - z['like_out'])[~near].max() <= 1e-10


def test_entry_points_are_declared_and_bound():
    from synthsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'synthsr_hip.h')).read()
    lib = _lib.load()
    for name, nargs in ENTRY_POINTS.items():
        decl = re.search(r'^int %s\(([^;]*)\);' % name, header, re.M)
        assert decl, name
        assert len(decl.group(1).split(',')) == nargs, name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert getattr(lib, name) is not None
    assert lib.synthsr_abi_version() == 2


P, Q = 4096, 1 << 30                                             # two non-NULL addresses far apart; never followed
IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
BAD_SIDES = (0, 1025, -1)


def _i3(v):
    from synthsr_amd import _lib
    return None if v is None else _lib.i3(v)


def _each_bad_shape(shape):
    for a in range(3):
        for side in BAD_SIDES:
            s = list(shape)
            s[a] = side
            yield s


def test_blur_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()

    def call(inp=P, shape=(5, 7, 9), axis=1, taps=(0.25, 0.5, 0.25), radius=1, out=Q):
        t = None if taps is None else (ctypes.c_float * len(taps))(*taps)
        return lib.synthsr_volume_blur_axis(inp, _i3(shape), axis, t, radius, out, None)
    for name in ('inp', 'shape', 'taps', 'out'):
        assert call(**{name: None}) == -1, name
    for axis in (-1, 3):
        assert call(axis=axis) == -1
    for radius in (0, 17, -1):
        assert call(taps=[0.0] * 35, radius=radius) == -1
    for bad in (float('nan'), float('inf')):
        assert call(taps=(0.25, bad, 0.25)) == -1
    for s in _each_bad_shape((5, 7, 9)):
        assert call(shape=s) == -1
    assert call(out=P) == -1 and call(out=P + 4 * (5 * 7 * 9 - 1)) == -1 and call(inp=Q + 4, out=Q) == -1     # overlap


def test_resample_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()

    def call(src=P, src_shape=(16, 24, 40), M=IDENT, mode=0, out_shape=(8, 9, 10), dst=Q, dst_shape=(32, 32, 32), Cd=2,
             offset=(12, 11, 10), c=1, minmax=P, workspace=P, workspace_bytes=8192):
        return lib.synthsr_volume_resample(src, _i3(src_shape), None if M is None else (ctypes.c_double * 12)(*M), mode,
                                           _i3(out_shape), dst, _i3(dst_shape), Cd, _i3(offset), c, minmax, workspace,
                                           workspace_bytes, None)
    for name in ('src', 'src_shape', 'M', 'out_shape', 'dst', 'dst_shape', 'offset', 'minmax', 'workspace'):
        assert call(**{name: None}) == -1, name
    for mode in (-1, 2):
        assert call(mode=mode) == -1
    for Cd, c in ((0, 0), (3, 0), (2, 2), (2, -1), (1, 1)):
        assert call(Cd=Cd, c=c) == -1
    for s in _each_bad_shape((16, 24, 40)):
        assert call(src_shape=s) == -1
    for s in _each_bad_shape((8, 9, 10)):
        assert call(out_shape=s, offset=(0, 0, 0)) == -1
    for s in _each_bad_shape((32, 32, 32)):
        assert call(dst_shape=s, offset=(0, 0, 0)) == -1
    for a in range(3):
        off = [12, 11, 10]
        off[a] = 32 - (8, 9, 10)[a] + 1                          # the box ends one past the destination
        assert call(offset=off) == -1
        off[a] = -1
        assert call(offset=off) == -1
    for e in range(12):
        for bad in (float('nan'), float('inf'), -float('inf')):
            M = list(IDENT)
            M[e] = bad
            assert call(M=M) == -1
    assert call(workspace_bytes=8191) == -1 and call(workspace=P + 2) == -1


def test_normalise_pad_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()

    def call(dst=P, dst_shape=(32, 32, 64), Cd=2, offset=(6, 7, 8), box_shape=(20, 18, 33), c=0, minmax=Q, gain=3.0):
        return lib.synthsr_volume_normalise_pad(dst, _i3(dst_shape), Cd, _i3(offset), _i3(box_shape), c, minmax, gain, None)
    for name in ('dst', 'dst_shape', 'offset', 'box_shape', 'minmax'):
        assert call(**{name: None}) == -1, name
    for Cd, c in ((0, 0), (3, 0), (2, 2), (2, -1), (1, 1)):
        assert call(Cd=Cd, c=c) == -1
    for s in _each_bad_shape((32, 32, 64)):
        assert call(dst_shape=s, offset=(0, 0, 0)) == -1
    for s in _each_bad_shape((20, 18, 33)):
        assert call(box_shape=s, offset=(0, 0, 0)) == -1
    for a in range(3):
        off = [6, 7, 8]
        off[a] = (32, 32, 64)[a] - (20, 18, 33)[a] + 1
        assert call(offset=off) == -1
        off[a] = -1
        assert call(offset=off) == -1
    for bad in (float('nan'), float('inf')):
        assert call(gain=bad) == -1


def test_postprocess_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()
    inf = float('inf')

    def call(net=P, netf=None, net_shape=(32, 64, 64), offset=(6, 14, 15), out_shape=(20, 35, 33), addend=None, stride=None,
             a=255.0, b=0.0, lo=0.0, hi=128.0, out=Q):
        st = None if stride is None else (ctypes.c_int64 * 3)(*stride)
        return lib.synthsr_sr_postprocess(net, netf, _i3(net_shape), _i3(offset), _i3(out_shape), addend, st, a, b, lo, hi, out,
                                          None)
    for name in ('net', 'net_shape', 'offset', 'out_shape', 'out'):
        assert call(**{name: None}) == -1, name
    assert call(addend=P, stride=None) == -1
    for a in range(3):
        st = [64 * 64, 64, 1]
        st[a] = 0
        assert call(addend=P, stride=st) == -1
    for s in _each_bad_shape((32, 64, 64)):
        assert call(net_shape=s, offset=(0, 0, 0)) == -1
    for s in _each_bad_shape((20, 35, 33)):
        assert call(out_shape=s, offset=(0, 0, 0)) == -1
    for a in range(3):
        off = [6, 14, 15]
        off[a] = (32, 64, 64)[a] - (20, 35, 33)[a] + 1
        assert call(offset=off) == -1
        off[a] = -1
        assert call(offset=off) == -1
    for bad in (float('nan'), inf, -inf):
        assert call(a=bad) == -1 and call(b=bad) == -1
    assert call(lo=1.0, hi=0.0) == -1 and call(lo=float('nan')) == -1 and call(hi=float('nan')) == -1 and call(lo=inf, hi=-inf) == -1


def test_ops_wrappers_check_before_the_library():
    import torch
    from synthsr_amd import ops
    x = torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match='float32'):
        ops.volume_blur_axis(x.double(), 0, [0.25, 0.5, 0.25])
    with pytest.raises(ValueError, match='axis'):
        ops.volume_blur_axis(x, 3, [0.25, 0.5, 0.25])
    for taps in ([1.0], [0.5, 0.5], [0.0] * 35, [0.25, np.nan, 0.25]):
        with pytest.raises(ValueError, match='taps'):
            ops.volume_blur_axis(x, 0, taps)
    with pytest.raises(ValueError, match='another float32 volume'):
        ops.volume_blur_axis(x, 0, [0.25, 0.5, 0.25], out=x)
    with pytest.raises(ValueError, match='sides 1 .. 1024'):
        ops.volume_blur_axis(torch.zeros(1, 1, 1025), 0, [0.25, 0.5, 0.25])
    M = np.eye(4)[:3]
    with pytest.raises(ValueError, match='mode'):
        ops.volume_resample(x, M, (4, 5, 6), mode='nearest')
    with pytest.raises(ValueError, match='finite'):
        ops.volume_resample(x, M + np.inf, (4, 5, 6))
    with pytest.raises(ValueError, match='out_shape'):
        ops.volume_resample(x, M, (4, 5))
    with pytest.raises(ValueError, match='does not lie inside'):
        ops.volume_resample(x, M, (4, 5, 6), out=torch.zeros(8, 8, 8, 2), offset=(5, 0, 0))
    with pytest.raises(ValueError, match='channel'):
        ops.volume_resample(x, M, (4, 5, 6), out=torch.zeros(8, 8, 8, 2), channel=2)
    with pytest.raises(ValueError, match='channel'):
        ops.volume_resample(x, M, (4, 5, 6), out=torch.zeros(8, 8, 8, 3))
    with pytest.raises(ValueError, match='minmax'):
        ops.volume_resample(x, M, (4, 5, 6), minmax=torch.zeros(3))
    with pytest.raises(ValueError, match='workspace'):
        ops.volume_resample(x, M, (4, 5, 6), workspace=torch.zeros(100, dtype=torch.uint8))
    buf = torch.zeros(8, 8, 8)
    with pytest.raises(ValueError, match='does not lie inside'):
        ops.volume_normalise_pad(buf, (1, 1, 4), (4, 5, 6), torch.zeros(2))
    with pytest.raises(ValueError, match='minmax'):
        ops.volume_normalise_pad(buf, (1, 1, 1), (4, 5, 6), torch.zeros(2, dtype=torch.float64))
    with pytest.raises(ValueError, match='gain'):
        ops.volume_normalise_pad(buf, (1, 1, 1), (4, 5, 6), torch.zeros(2), gain=np.inf)
    with pytest.raises(ValueError, match='does not lie inside'):
        ops.sr_postprocess(buf, (3, 3, 3), (4, 5, 6))
    with pytest.raises(ValueError, match='netf'):
        ops.sr_postprocess(buf, (1, 1, 1), (4, 5, 6), netf=torch.zeros(8, 8, 9))
    with pytest.raises(ValueError, match='addend'):
        ops.sr_postprocess(buf, (1, 1, 1), (4, 5, 6), addend=torch.zeros(4, 5, 7))
    with pytest.raises(ValueError, match='lo <= hi'):
        ops.sr_postprocess(buf, (1, 1, 1), (4, 5, 6), lo=2.0, hi=1.0)
    with pytest.raises(ValueError, match='out should be'):
        ops.sr_postprocess(buf, (1, 1, 1), (4, 5, 6), out=torch.zeros(4, 5, 7))


def test_preprocessing_keyword_and_flag(tmp_path):
    from synthsr_amd.predict import predict, predict_hyperfine
    with pytest.raises(ValueError, match="'host' or 'device'"):
        predict(str(tmp_path / 'a.nii.gz'), str(tmp_path / 'b.nii.gz'), predictor=object(), preprocessing='nonsense')
    with pytest.raises(ValueError, match="'host' or 'device'"):
        predict_hyperfine(str(tmp_path / 'a.nii.gz'), str(tmp_path / 'a.nii.gz'), str(tmp_path / 'b.nii.gz'), predictor=object(),
                          preprocessing='nonsense')
    for script in ('predict_command_line.py', 'predict_command_line_hyperfine.py'):
        spec = importlib.util.spec_from_file_location(script[:-3], os.path.join(ROOT, 'scripts', script))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        paths = ['in', 'out'] if 'hyperfine' not in script else ['t1', 't2', 'out']
        assert mod.build_parser().parse_args(paths).preprocessing == 'host'
        assert mod.build_parser().parse_args(paths + ['--preprocessing', 'device']).preprocessing == 'device'
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(paths + ['--preprocessing', 'nonsense'])
