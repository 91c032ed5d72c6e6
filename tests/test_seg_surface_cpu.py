"""Host side of the surface distances (no GPU): the float64 scores formed from exact squared distances
(predict_segmentation.surface_scores_from_d2), the surface rule restated in numpy against scipy's binary erosion, the command
line of scripts/predict_segmentation.py, and the argument checks of the two C entry points (csrc/seg_surface.hip), which return
before any HIP call."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = np.iinfo(np.int32).max


def _script():
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def surface_classes(cls):
    """the surface rule: the class of a voxel whose class is >= 0 and differs from that of a face neighbour (outside the volume
    counts as different), -1 elsewhere"""
    cls = np.asarray(cls)
    padded = np.pad(cls, 1, constant_values=-2)
    inner = tuple(slice(1, -1) for _ in range(3))
    differs = np.zeros(cls.shape, dtype=bool)
    for axis in range(3):
        for step in (-1, 1):
            differs |= np.roll(padded, step, axis=axis)[inner] != cls
    return np.where((cls >= 0) & differs, cls, -1)


def test_scores_in_closed_form():
    from synthsr_amd.predict_segmentation import surface_scores_from_d2
    # class 0: one voxel in each map, offset (1, 2, 2): 3.0 in all three; class 1 in a only; class 2 in b only; class 3 nowhere;
    # class 4: distances 0, 0, 3 from a and 4 from b: max 4, mean 7 / 4, 95th percentile of [0, 0, 3, 4] = 3 + 0.85
    cls_a, d2_ab = np.array([0, 1, 4, 4, 4]), np.array([9, FAR, 0, 9, 0], dtype=np.int32)
    cls_b, d2_ba = np.array([2, 0, 4]), np.array([FAR, 9, 16], dtype=np.int32)
    s = surface_scores_from_d2(cls_a, d2_ab, cls_b, d2_ba, 5, 95, 1.0)
    assert set(s) == {'hausdorff', 'hd_percentile', 'mean', 'n_seg', 'n_truth'}
    for key in ('hausdorff', 'hd_percentile', 'mean'):
        assert s[key].dtype == np.float64 and s[key].shape == (5,)
        assert s[key][0] == 3.0
        assert np.isnan(s[key][1]) and np.isnan(s[key][2]), 'a class absent from one map scores NaN'
        assert np.isnan(s[key][3]), 'a class absent from both maps scores NaN'
    assert s['hausdorff'][4] == 4.0 and s['mean'][4] == 7.0 / 4.0
    assert s['hd_percentile'][4] == pytest.approx(3.85, rel=1e-15)
    assert s['n_seg'].dtype == np.int64 and s['n_seg'].tolist() == [1, 1, 0, 0, 3] and s['n_truth'].tolist() == [1, 0, 1, 0, 1]
    # voxel_size scales linearly; the 100th percentile is the Hausdorff distance
    t = surface_scores_from_d2(cls_a, d2_ab, cls_b, d2_ba, 5, 100, 0.5)
    for key in ('hausdorff', 'mean'):
        assert np.array_equal(t[key], 0.5 * s[key], equal_nan=True)
    assert np.array_equal(t['hd_percentile'], t['hausdorff'], equal_nan=True)
    # whole volumes: the voxels with d2 < 0 are left out, whatever class they carry
    full = surface_scores_from_d2(np.array([[0, 3], [1, 4], [4, 4]]), np.array([[9, -1], [FAR, 0], [9, 0]]),
                                  np.array([2, 0, 4, 3]), np.array([FAR, 9, 16, -1]), 5, 95, 1.0)
    for key in s:
        assert np.array_equal(full[key], s[key], equal_nan=True)
    with pytest.raises(ValueError):
        surface_scores_from_d2(cls_a, d2_ab[:-1], cls_b, d2_ba, 5)
    with pytest.raises(ValueError):
        surface_scores_from_d2(cls_a, d2_ab, cls_b, d2_ba, 4)          # class 4 of 4
    with pytest.raises(ValueError):
        surface_scores_from_d2(cls_a, d2_ab, cls_b, d2_ba, 5, percentile=101)


def test_surface_rule_equals_mask_minus_its_erosion():
    from scipy.ndimage import binary_erosion
    rng = np.random.default_rng(7)
    cls = rng.integers(-1, 4, size=(9, 7, 5))
    cls[2:7, 1:6, 1:4] = 2                   # a block with an interior
    cls[3, 3, 2] = -1                        # and a hole without a class in it
    surf = surface_classes(cls)
    assert (cls == -1).sum() > 10
    for k in range(4):
        m = cls == k
        want = m & ~binary_erosion(m)
        assert want.sum() > 0 and np.array_equal(surf == k, want), k
    assert (surf[cls == 2] == -1).sum() > 0, 'the block has interior voxels'
    assert np.all(surf[cls < 0] == -1)


def test_script_arguments(tmp_path):
    S = _script()
    p = S.build_parser()
    base = ['in', 'out', '--model', 'm.npz', '--labels', 'l.npy']
    a = p.parse_args(base)
    assert a.surface_scores is None and a.surface_percentile == 95
    a = p.parse_args(base + ['--truth', 'gt', '--surface_scores', 'd.csv', '--surface_percentile', '99.5'])
    assert (a.truth, a.surface_scores, a.surface_percentile) == ('gt', 'd.csv', 99.5)
    for bad in (['--surface_scores', 'd.npy'], ['--truth', 'gt', '--surface_scores', 'd.txt'],
                ['--truth', 'gt', '--surface_scores', 'd.npy', '--surface_percentile', '120']):
        with pytest.raises(SystemExit):
            S.main(base + bad)
    table = np.array([[[1.0, np.nan], [0.5, np.nan], [0.25, np.nan]], [[3.0, 2.0], [2.5, 2.0], [1.0, 2.0]]])
    S.write_surface_scores(str(tmp_path / 'd.npy'), [0, 14], table)
    assert np.array_equal(np.load(tmp_path / 'd.npy'), table, equal_nan=True)
    S.write_surface_scores(str(tmp_path / 'd.csv'), [0, 14], table)
    assert open(tmp_path / 'd.csv').read().split('\n') == ['0,14', '1.0,nan', '0.5,nan', '0.25,nan', '3.0,2.0', '2.5,2.0',
                                                          '1.0,2.0', '']
    with pytest.raises(ValueError):
        S.write_surface_scores(str(tmp_path / 'd.txt'), [0, 14], table)


def test_workspace_size_and_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()
    size = lambda shape, N: lib.synthsr_seg_surface_workspace_bytes(_lib.i3(shape), N)
    sizes = [size([5, 7, 9], N) for N in range(1, 65)]
    assert sizes[0] > 0 and all(y >= x for x, y in zip(sizes, sizes[1:])) and sizes[1] > sizes[0] and sizes[-1] > sizes[0]
    for N in (1, 33, 64):
        grown = [size(s, N) for s in ([1, 1, 1], [5, 7, 9], [5, 7, 10], [5, 8, 10], [6, 8, 10], [160, 160, 160],
                                      [1024, 1024, 1024])]
        assert grown[0] > 0 and all(y > x for x, y in zip(grown, grown[1:])), grown
    assert size([160, 160, 160], 33) >= 2 * 160 ** 3       # at least the two byte maps
    p = 4096                                                 # a non-NULL, 16-byte aligned address; never followed
    shape, N = [5, 7, 9], 5
    need = size(shape, N)

    def call(shape=shape, N=N, a=p, lut=p, lut_n=8, out=p, ws=p, ws_bytes=need):
        return lib.synthsr_seg_surface_dist2(a, p, _lib.i3(shape), lut, lut_n, N, out, p, ws, ctypes.c_int64(ws_bytes), None)
    for bad in ([0, 7, 9], [5, 0, 9], [5, 7, 0], [1025, 7, 9], [5, 1025, 9], [5, 7, 1025]):
        assert size(bad, N) == -1
        assert call(shape=bad, ws_bytes=1 << 40) == -1
    for bad in (0, 65, -1):
        assert size(shape, bad) == -1
        assert call(N=bad, ws_bytes=1 << 40) == -1
    assert call(out=None) == -1 and call(a=None) == -1 and call(lut=None) == -1 and call(ws=None) == -1
    assert lib.synthsr_seg_surface_dist2(p, p, _lib.i3(shape), p, 8, N, p, None, p, ctypes.c_int64(need), None) == -1
    assert lib.synthsr_seg_surface_dist2(p, p, None, p, 8, N, p, p, p, ctypes.c_int64(need), None) == -1
    assert call(lut_n=0) == -1
    assert call(ws_bytes=need - 1) == -1                     # one byte too small
    assert call(ws=p + 8) == -1                              # not 16-byte aligned
    assert lib.synthsr_abi_version() == 2


def test_ops_wrapper_checks_before_the_library():
    import torch
    from synthsr_amd import ops
    a = torch.zeros(5, 7, 9, dtype=torch.int32)
    lut = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(ValueError, match='int32'):
        ops.seg_surface_dist2(a.long(), a, lut, 2)
    with pytest.raises(ValueError, match='shapes'):
        ops.seg_surface_dist2(a, a[:, :, :8], lut, 2)
    with pytest.raises(ValueError, match='shapes'):
        ops.seg_surface_dist2(a.reshape(-1), a.reshape(-1), lut, 2)
    with pytest.raises(ValueError, match='1 <= N <= 64'):
        ops.seg_surface_dist2(a, a, lut, 65)
    with pytest.raises(ValueError, match='sides'):
        ops.seg_surface_dist2(torch.zeros(1025, 1, 1, dtype=torch.int32), torch.zeros(1025, 1, 1, dtype=torch.int32), lut, 2)
    with pytest.raises(ValueError, match='one value per voxel'):
        ops.seg_surface_dist2(a, a, lut, 2, d2_ab=torch.zeros(5, 7, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match='workspace'):
        ops.seg_surface_dist2(a, a, lut, 2, workspace=torch.zeros(16, dtype=torch.uint8))
    assert ops.seg_surface_workspace_bytes((160, 160, 160), 33) > 0
