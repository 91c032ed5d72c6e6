"""Surface distances on the device (csrc/seg_surface.hip through ops.seg_surface_dist2, predict_segmentation.surface_distances
and the script).

The reference is a restatement on the CPU, written here: the class of every voxel by the lookup table, the surface voxels by
the rule of include/synthsr_hip.h (a face neighbour outside the volume or of another class), and for every surface voxel the
minimum over ALL surface voxels of its class in the other map of the squared distance, in int64 numpy.  It is cross-checked
once against scipy's Euclidean distance transform.  The kernels compute in integers, so the device maps must equal the
reference at every voxel; the scores add only float64 sqrt, mean and percentile, hence rtol = 1e-12."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAR = np.iinfo(np.int32).max
GUARD, GARBAGE = 64, -777


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------------------------------------------- the reference
def classes(m, lut, N):
    m = np.asarray(m, dtype=np.int64)
    inside = (m >= 0) & (m < len(lut))
    k = np.where(inside, np.asarray(lut, dtype=np.int64)[np.clip(m, 0, len(lut) - 1)], -1)
    return np.where((k >= 0) & (k < N), k, -1)


def surface_classes(cls):
    padded = np.pad(cls, 1, constant_values=-2)
    inner = tuple(slice(1, -1) for _ in range(3))
    differs = np.zeros(cls.shape, dtype=bool)
    for axis in range(3):
        for step in (-1, 1):
            differs |= np.roll(padded, step, axis=axis)[inner] != cls
    return np.where((cls >= 0) & differs, cls, -1)


def brute_d2(sq, ss):
    """int32 map: at the voxels of sq >= 0 the squared distance to the nearest voxel of the same value in ss (FAR: none), else -1"""
    out = np.full(sq.shape, -1, dtype=np.int64)
    for k in np.unique(sq[sq >= 0]):
        q, s = np.argwhere(sq == k), np.argwhere(ss == k)
        if len(s) == 0:
            out[sq == k] = FAR
            continue
        best = np.empty(len(q), dtype=np.int64)
        for i in range(0, len(q), 512):
            best[i:i + 512] = ((q[i:i + 512, None, :] - s[None, :, :]) ** 2).sum(-1).min(1)
        out[tuple(q.T)] = best
    return out.astype(np.int32)


def reference(a, b, lut, N):
    """(class of a's surface voxels or -1, d2_ab, the same for b, d2_ba)"""
    sa, sb = surface_classes(classes(a, lut, N)), surface_classes(classes(b, lut, N))
    return sa, brute_d2(sa, sb), sb, brute_d2(sb, sa)


def make_lut(N, rng):
    """label values 0 .. 2 N + 7, N of them listed in a random order (the others map to -1); values beyond the table and
    negative ones have no class either"""
    lut_n = 2 * N + 8
    values = rng.permutation(lut_n)
    lut = np.full(lut_n, -1, dtype=np.int32)
    lut[values[:N]] = np.arange(N, dtype=np.int32)
    return lut, values[:N].astype(np.int32), values[N:].astype(np.int32)


@functools.lru_cache(maxsize=None)
def random_case(shape, N, seed=0):
    """blocks of 3^3 voxels of random label values with 15 % of the voxels relabelled at random (so: interiors, surfaces and
    single voxels), and a second map that is the first shifted by one voxel along every axis with another 10 % relabelled.
    Three corners of the first map hold a negative value, one beyond the table and one mapped to -1.  For N > 2 the last channel
    is in neither map and the one before it in the first map only.  Never modified."""
    rng = np.random.default_rng(1000 * N + 7 * shape[0] + shape[2] + seed)
    lut, listed, unlisted = make_lut(N, rng)
    few = listed[:min(N, 6)]                       # most voxels in a few classes, so that they have interiors and two maps overlap
    pool = np.concatenate([few, few, few, listed, unlisted[:2], [-1, -9, len(lut), len(lut) + 1000]]).astype(np.int32)
    coarse = rng.choice(pool, size=[(s + 2) // 3 for s in shape])
    a = np.kron(coarse, np.ones((3, 3, 3), dtype=np.int32))[:shape[0], :shape[1], :shape[2]]
    a = np.where(rng.random(shape) < .15, rng.choice(pool, size=shape), a).astype(np.int32)
    a[0, 0, 0], a[-1, -1, -1], a[0, -1, 0] = -9, len(lut) + 1000, unlisted[0]
    b = np.roll(a, (1, 1, 1), axis=(0, 1, 2))
    b = np.where(rng.random(shape) < .10, rng.choice(pool, size=shape), b).astype(np.int32)
    if N > 2:
        a[a == listed[N - 1]] = unlisted[1]
        b[b == listed[N - 1]] = unlisted[1]
        b[b == listed[N - 2]] = unlisted[1]
        a[-1, 0, -1] = listed[N - 2]
    return a, b, lut, N, reference(a, b, lut, N)


def run_device(torch, a, b, lut, N, misalign=True):
    """both maps and both outputs as views one element into larger buffers (misalign), the outputs full of garbage with guards
    behind them -> (d2_ab, d2_ba) on the host"""
    from synthsr_amd import ops
    n, o = a.size, 1 if misalign else 0
    ins = []
    for m in (a, b):
        buf = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
        buf[o:o + n] = torch.from_numpy(np.ascontiguousarray(m)).cuda().reshape(-1)
        ins.append(buf[o:o + n].view(a.shape))
    bufs = [torch.full((n + GUARD + 1,), GARBAGE, dtype=torch.int32, device='cuda') for _ in range(2)]
    outs = [buf[o:o + n].view(a.shape) for buf in bufs]
    got = ops.seg_surface_dist2(ins[0], ins[1], torch.from_numpy(lut).cuda(), N, d2_ab=outs[0], d2_ba=outs[1])
    torch.cuda.synchronize()
    assert got[0].data_ptr() == outs[0].data_ptr() and got[1].data_ptr() == outs[1].data_ptr()
    for buf in bufs:
        assert bool((buf[o + n:] == GARBAGE).all()) and bool((buf[:o] == GARBAGE).all()), 'guard overwritten'
    for t, m in zip(ins, (a, b)):
        assert torch.equal(t.cpu(), torch.from_numpy(np.ascontiguousarray(m))), 'an input was written'
    return outs[0].cpu(), outs[1].cpu()


def check(torch, a, b, lut, N, ref=None, misalign=True):
    sa, want_ab, sb, want_ba = ref or reference(a, b, lut, N)
    got_ab, got_ba = run_device(torch, a, b, lut, N, misalign)
    assert got_ab.dtype == torch.int32 and tuple(got_ab.shape) == a.shape
    for name, got, want in (('d2_ab', got_ab, want_ab), ('d2_ba', got_ba, want_ba)):
        bad = int((got != torch.from_numpy(want)).sum())
        print('%s %s N=%d: %d voxels, %d surface voxels, %d differ' % (name, a.shape, N, want.size, int((want >= 0).sum()), bad))
        assert torch.equal(got, torch.from_numpy(want)), name
    return (sa, want_ab, sb, want_ba), (got_ab, got_ba)


def test_reference_equals_scipy_distance_transform():
    """the brute-force squared distances against np.rint(distance_transform_edt(~edge) ** 2), evaluated at the other map's
    surface voxels, for every class that both maps hold"""
    from scipy.ndimage import distance_transform_edt
    a, b, lut, N, (sa, d2_ab, sb, d2_ba) = random_case((33, 20, 17), 33)
    both = 0
    for k in range(N):
        for sq, ss, d2 in ((sa, sb, d2_ab), (sb, sa, d2_ba)):
            if (ss == k).any() and (sq == k).any():
                edt2 = np.rint(distance_transform_edt(ss != k) ** 2).astype(np.int64)
                assert np.array_equal(d2[sq == k], edt2[sq == k]), k
                both += 1
            elif (sq == k).any():
                assert np.all(d2[sq == k] == FAR)
    assert both >= 12
    assert np.all((d2_ab >= 0) == (sa >= 0)) and np.all((d2_ba >= 0) == (sb >= 0))
    assert 0 < (sa >= 0).sum() < (classes(a, lut, N) >= 0).sum(), 'the case has interior voxels'


# ---------------------------------------------------------------------------------------------------- the kernels
ODD = [(5, 7, 9), (16, 16, 16), (33, 20, 17)]
FLAT = [(1, 8, 8), (8, 1, 8), (8, 8, 1)]
LONG = [(300, 4, 4), (4, 300, 4), (4, 4, 300)]


@pytest.mark.parametrize('N', [2, 33, 64])
@pytest.mark.parametrize('shape', ODD)
def test_random_maps_equal_the_reference(T, shape, N):
    a, b, lut, N, ref = random_case(shape, N)
    assert (classes(a, lut, N) < 0).sum() > 0 and (a >= len(lut)).sum() > 0 and (a < 0).sum() > 0
    check(T, a, b, lut, N, ref, misalign=(N != 33))


@pytest.mark.parametrize('shape', FLAT + LONG)
def test_degenerate_and_long_axes(T, shape):
    """a side of 1: every classed voxel is a surface voxel; a side of 300: a line longer than one workgroup, along each axis"""
    a, b, lut, N, ref = random_case(shape, 5)
    if 1 in shape:
        assert np.array_equal(ref[0], classes(a, lut, N))
    check(T, a, b, lut, N, ref)


def test_longest_line(T):
    """(1024, 2, 2): class 1 at one end of a and at the other end of b, class 0 one voxel further in; nothing else has a class"""
    shape = (1024, 2, 2)
    lut = np.array([-1, 0, 1], dtype=np.int32)
    a, b = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    a[0, 0, 0], b[1023, 1, 1] = 2, 2
    a[1, 1, 0], b[1022, 0, 1] = 1, 1
    ref, (got_ab, got_ba) = check(T, a, b, lut, 2)
    assert int(got_ab[0, 0, 0]) == 1023 ** 2 + 2 and int(got_ba[1023, 1, 1]) == 1023 ** 2 + 2
    assert int(got_ab[1, 1, 0]) == 1021 ** 2 + 2 and int((got_ab >= 0).sum()) == 2
    b = a.copy()
    b[0, 0, 0], b[1023, 0, 0] = 0, 2          # the same voxel column: 1023^2 exactly, the largest distance on a line
    ref, (got_ab, got_ba) = check(T, a, b, lut, 2)
    assert int(got_ab[0, 0, 0]) == 1023 ** 2


def test_special_maps(T):
    torch = T
    from synthsr_amd.predict_segmentation import surface_scores_from_d2
    lut = np.array([0, -1, 1, 2], dtype=np.int32)            # values 0, 2, 3 -> classes 0, 1, 2; value 1: no class
    shape = (6, 5, 7)
    # a class that fills the volume in a and is absent from b (and the other way round): INT32_MAX on the volume's shell
    a, b = np.zeros(shape, dtype=np.int32), np.full(shape, 2, dtype=np.int32)
    ref, (got_ab, got_ba) = check(torch, a, b, lut, 3)
    shell = ref[0] >= 0
    assert shell.sum() == 6 * 5 * 7 - 4 * 3 * 5 and bool((got_ab[torch.from_numpy(shell)] == FAR).all())
    assert bool((got_ab[torch.from_numpy(~shell)] == -1).all()) and bool((got_ba[torch.from_numpy(shell)] == FAR).all())
    # a class that is a single voxel, in both maps, inside a background class
    a, b = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    a[2, 2, 3], b[4, 1, 5] = 3, 3
    ref, (got_ab, got_ba) = check(torch, a, b, lut, 3)
    assert int(got_ab[2, 2, 3]) == 4 + 1 + 4 and int(got_ba[4, 1, 5]) == 9
    # a == b: every surface voxel at distance 0
    a, _, lut33, N, ref = random_case((16, 16, 16), 33)
    (sa, want_ab, _, _), (got_ab, got_ba) = check(torch, a, a.copy(), lut33, N)
    assert bool((got_ab[got_ab >= 0] == 0).all()) and torch.equal(got_ab, got_ba) and int((got_ab == 0).sum()) == (sa >= 0).sum()
    # two solid boxes offset by (3, 0, 0) in a classed background: the Hausdorff distance of the box is exactly 3
    shape = (14, 9, 10)
    a, b = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    a[2:8, 2:7, 3:8] = 2
    b[5:11, 2:7, 3:8] = 2
    ref, (got_ab, got_ba) = check(torch, a, b, lut, 3)
    s = surface_scores_from_d2(ref[0], got_ab.numpy(), ref[2], got_ba.numpy(), 3)
    assert s['hausdorff'][1] == 3.0 and 0 < s['mean'][1] < 3.0 and s['n_seg'][1] == 6 * 5 * 5 - 4 * 3 * 3


def test_repeatable_and_stream_independent(T):
    torch = T
    from synthsr_amd import ops
    a, b, lut, N, ref = random_case((33, 20, 17), 33)
    da, db, dl = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda(), torch.from_numpy(lut).cuda()
    first = [t.clone() for t in ops.seg_surface_dist2(da, db, dl, N)]
    ws = torch.full((ops.seg_surface_workspace_bytes(a.shape, N) + 16,), 0xA5, dtype=torch.uint8, device='cuda')
    ws = ws[(-ws.data_ptr()) % 16:][:ops.seg_surface_workspace_bytes(a.shape, N)]
    second = ops.seg_surface_dist2(da, db, dl, N, workspace=ws)          # a caller-owned workspace full of garbage
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        third = ops.seg_surface_dist2(da, db, dl, N)
    side.synchronize()
    assert torch.equal(first[0], third[0]) and torch.equal(first[1], third[1])
    assert torch.equal(first[0].cpu(), torch.from_numpy(ref[1])) and torch.equal(first[1].cpu(), torch.from_numpy(ref[3]))


def test_limits_are_refused_and_nothing_is_written(T):
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    shape, N = (5, 7, 9), 5
    a = torch.zeros(shape, dtype=torch.int32, device='cuda')
    lut = torch.zeros(4, dtype=torch.int32, device='cuda')
    out = torch.full(shape, GARBAGE, dtype=torch.int32, device='cuda')
    need = ops.seg_surface_workspace_bytes(shape, N)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    P = _lib.ptr
    for n, bytes_ in ((65, need), (0, need), (N, need - 1)):
        assert lib.synthsr_seg_surface_dist2(P(a), P(a), _lib.i3(shape), P(lut), 4, n, P(out), P(out), P(ws), bytes_,
                                             _lib.stream()) == -1
    with pytest.raises(ValueError):
        ops.seg_surface_dist2(a, a, lut, 65, d2_ab=out)
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all())


# ---------------------------------------------------------------------------------------------------- scores
def test_surface_distances_equal_the_scores_of_the_reference(T, tmp_path):
    from synthsr_amd import volumes as V
    from synthsr_amd.predict_segmentation import surface_distances, surface_scores_from_d2
    a, b, lut, N, (sa, d2_ab, sb, d2_ba) = random_case((33, 20, 17), 33)
    labels = np.argsort(np.where(lut >= 0, lut, N + 1), kind='stable')[:N].astype(np.int32)      # channel -> label value
    assert np.array_equal(lut[labels], np.arange(N))
    pa, pb = str(tmp_path / 'a.nii.gz'), str(tmp_path / 'b.nii.gz')
    V.save_volume(a, np.eye(4), None, pa, dtype='int32')
    V.save_volume(b, np.eye(4), None, pb, dtype='int32')
    for percentile, voxel_size in ((95, 1.0), (50, 0.7)):
        want = surface_scores_from_d2(sa, d2_ab, sb, d2_ba, N, percentile, voxel_size)
        present = ~np.isnan(want['hausdorff'])
        assert present.sum() >= 6 and (~present).sum() >= 1
        for got in (surface_distances(a, b, labels, percentile, voxel_size), surface_distances(pa, pb, labels, percentile, voxel_size)):
            for key in ('hausdorff', 'hd_percentile', 'mean'):
                assert got[key].dtype == np.float64 and got[key].shape == (N,)
                np.testing.assert_allclose(got[key], want[key], rtol=1e-12, atol=0, equal_nan=True)
            assert got['n_seg'].dtype == np.int64 and np.array_equal(got['n_seg'], want['n_seg'])
            assert np.array_equal(got['n_truth'], want['n_truth'])
    with pytest.raises(ValueError):
        surface_distances(a, b[:-1], labels)


# ---------------------------------------------------------------------------------------------------- end to end
def test_script_writes_surface_scores_next_to_dice(T, tmp_path, capsys):
    """the tiny setup of tests/test_seg_predict_gpu.py's script test: a 3-level, 8-feature network on a 20 x 18 x 22 scan; the
    ground truth is the script's own label map shifted by one voxel"""
    torch = T
    from synthsr_amd.nifti import write_nifti, read_nifti
    from synthsr_amd.unet import unet
    from synthsr_amd.training import save_checkpoint
    labels = np.array([0, 14, 2, 41, 17], dtype=np.int32)
    rng = np.random.default_rng(5)
    scan = str(tmp_path / 'scan0.nii.gz')
    write_nifti(scan, rng.random((20, 18, 22)).astype(np.float32) * 100)
    net = unet(nb_features=8, input_shape=[32, 32, 32, 1], nb_levels=3, conv_size=3, nb_labels=len(labels), feat_mult=2,
               nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax', seed=3)
    net.view(net.head['w']).copy_(torch.randn(8, len(labels), generator=torch.Generator().manual_seed(6)))
    ckpt = str(tmp_path / 'seg.npz')
    save_checkpoint(ckpt, net)
    np.save(tmp_path / 'labels.npy', labels)
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    seg, truth = str(tmp_path / 'one_seg.nii.gz'), str(tmp_path / 'truth.nii.gz')
    common = [scan, seg, '--model', ckpt, '--labels', str(tmp_path / 'labels.npy'), '--n_levels', '3', '--unet_feat', '8']
    script.main(common)
    data = read_nifti(seg)[0]
    write_nifti(truth, np.roll(data, 1, axis=0).astype(np.int32))
    plain, a_csv, b_csv = str(tmp_path / 'plain.csv'), str(tmp_path / 'a.csv'), str(tmp_path / 'b.csv')
    script.main(common + ['--truth', truth, '--scores', plain])
    capsys.readouterr()
    table = script.main(common + ['--truth', truth, '--scores', a_csv, '--surface_scores', b_csv])
    out = capsys.readouterr().out
    assert open(a_csv, 'rb').read() == open(plain, 'rb').read()
    assert 'mean Dice' in out and 'mean Hausdorff' in out and 'mean HD95' in out and 'mean surface distance' in out
    rows = open(b_csv).read().strip().split('\n')
    assert rows[0] == ','.join(str(v) for v in labels) and len(rows) == 1 + 3
    values = np.array([[float(v) for v in row.split(',')] for row in rows[1:]])
    assert values.shape == (3, len(labels))
    truth_data = read_nifti(truth)[0]
    present = np.array([(data == v).any() and (truth_data == v).any() for v in labels])
    assert present.sum() >= 1
    assert np.all(np.isfinite(values[:, present])) and np.all(np.isnan(values[:, ~present]))
    assert np.all(values[0, present] >= values[1, present]) and np.all(values[1, present] >= 0)
    b_npy = str(tmp_path / 'b.npy')
    script.main(common + ['--truth', truth, '--surface_scores', b_npy, '--surface_percentile', '95'])
    assert np.load(b_npy).shape == (1, 3, len(labels))
    assert np.array_equal(np.load(b_npy)[0], values, equal_nan=True)
