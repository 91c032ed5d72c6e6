"""Connected components and the largest-component filter on the device (csrc/seg_components.hip through ops.seg_components and
ops.seg_keep_largest, predict_segmentation's functions and the script).

The reference, written here: scipy.ndimage.label per group with generate_binary_structure(3, 1 | 2 | 3) for connectivity
6 | 18 | 26, every component renamed to its smallest linear index, the largest picked by size and then by smallest root
(tests/test_seg_components_cpu.py checks the same functions against a flood fill).  The kernels compute in integers and the
component map is unique, so every device result must equal the reference at every voxel: array_equal everywhere."""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = (8, 8, 32)          # csrc/seg_components.hip: CC_TZ, CC_TY, CC_TX
GUARD, GARBAGE = 64, int(np.array([0xA5A5A5A5], dtype=np.uint32).view(np.int32)[0])
CONNECTIVITIES = (6, 18, 26)


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


# ---------------------------------------------------------------------------------------------------- the reference
def groups_of(m, lut, G):
    m = np.asarray(m, dtype=np.int64)
    inside = (m >= 0) & (m < len(lut))
    g = np.where(inside, np.asarray(lut, dtype=np.int64)[np.clip(m, 0, len(lut) - 1)], -1)
    return np.where((g >= 0) & (g < G), g, -1)


def reference_components(m, lut, G, connectivity):
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    grp = groups_of(m, lut, G)
    comp = np.full(grp.shape, -1, dtype=np.int64)
    index = np.arange(grp.size, dtype=np.int64).reshape(grp.shape)
    for g in range(G):
        lab, n = ndimage.label(grp == g, structure=structure)
        if n:
            roots = ndimage.minimum(index, lab, np.arange(1, n + 1)).astype(np.int64)
            comp[lab > 0] = roots[lab[lab > 0] - 1]
    return comp.astype(np.int32)


def reference_keep_largest(m, comp, lut, G, fill_value):
    grp = groups_of(m, lut, G)
    out = np.array(m, dtype=np.int32)
    stats = np.zeros((G, 4), dtype=np.int64)
    for g in range(G):
        roots, sizes = np.unique(comp[grp == g], return_counts=True)
        if len(roots) == 0:
            stats[g] = (-1, 0, 0, 0)
            continue
        kept = roots[np.lexsort((roots, -sizes))[0]]
        stats[g] = (kept, sizes[roots == kept][0], len(roots), sizes.sum())
        out[(grp == g) & (comp != kept)] = fill_value
    return out, stats


# ---------------------------------------------------------------------------------------------------- the device
def run_device(torch, m, lut, G, connectivity, fill_value, alias=False):
    """component map, filtered map and stats on the host; workspace and outputs start as 0xA5 bytes, with guards behind the
    outputs; alias: the filtered map is written over the label map"""
    from synthsr_amd import ops
    n = m.size
    labels = torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32)).cuda()
    lut_d = torch.from_numpy(np.ascontiguousarray(lut, dtype=np.int32)).cuda()
    need = ops.seg_components_workspace_bytes(m.shape)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device='cuda')
    bufs = [torch.full((n + GUARD,), GARBAGE, dtype=torch.int32, device='cuda') for _ in range(2)]
    comp = ops.seg_components(labels, lut_d, G, connectivity, comp=bufs[0][:n].view(m.shape), workspace=ws)
    assert comp.data_ptr() == bufs[0].data_ptr()
    assert torch.equal(labels.cpu(), torch.from_numpy(np.ascontiguousarray(m, dtype=np.int32))), 'the label map was written'
    ws.fill_(0xA5)
    stats = torch.full((G + 1, 4), GARBAGE, dtype=torch.int64, device='cuda')
    target = labels if alias else bufs[1][:n].view(m.shape)
    out, st = ops.seg_keep_largest(labels, comp, lut_d, G, fill_value, out=target, stats=stats[:G], workspace=ws)
    torch.cuda.synchronize()
    assert out.data_ptr() == target.data_ptr() and st.data_ptr() == stats.data_ptr()
    assert bool((bufs[0][n:] == GARBAGE).all()) and bool((bufs[1][n:] == GARBAGE).all()), 'guard overwritten'
    assert bool((stats[G] == GARBAGE).all()), 'stats guard overwritten'
    return comp.cpu().numpy(), out.cpu().numpy(), st.cpu().numpy()


def check(torch, what, m, lut, G, connectivity, fill_value=0, alias=False):
    want_comp = reference_components(m, lut, G, connectivity)
    want_out, want_stats = reference_keep_largest(m, want_comp, lut, G, fill_value)
    comp, out, stats = run_device(torch, m, lut, G, connectivity, fill_value, alias)
    print('%s %s connectivity %d: %d voxels in groups, %d components, %d voxels differ, %d filtered voxels differ'
          % (what, m.shape, connectivity, int((want_comp >= 0).sum()), int(want_stats[:, 2].sum()), int((comp != want_comp).sum()),
             int((out != want_out).sum())))
    assert comp.dtype == np.int32 and comp.shape == m.shape and out.dtype == np.int32 and stats.dtype == np.int64
    assert np.array_equal(comp, want_comp), what
    assert np.array_equal(out, want_out), what
    assert np.array_equal(stats, want_stats), what
    return want_comp, want_out, want_stats


# ---------------------------------------------------------------------------------------------------- the maps
LUT3 = np.array([-1, 0, 1, 2, -1, 1], dtype=np.int32)     # values 1, 2, 3 -> groups 0, 1, 2; 5 -> group 1 too; 0 and 4: none


def random_map(shape, density, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, 4, size=shape), 0).astype(np.int32)


def serpentine(shape):
    """value 2 on a comb: in even planes every other row along x, joined at alternating ends; the planes joined through one
    voxel of the odd planes at alternating ends: one 6-connected path through every tile"""
    d0, d1, d2 = shape
    z, y, x = np.meshgrid(np.arange(d0), np.arange(d1), np.arange(d2), indexing='ij')
    row = y % 2 == 0
    link = (y % 2 == 1) & (x == np.where(y // 2 % 2 == 1, 0, d2 - 1))
    between = (y == 0) & (x == np.where(z // 2 % 2 == 1, 0, d2 - 1))
    return np.where(np.where(z % 2 == 0, row | link, between), 2, 0).astype(np.int32)


def checkerboard(shape):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    return np.where((z + y + x) % 2 == 0, 3, 0).astype(np.int32)


def special_values(shape, seed):
    """a random map with values < 0, >= lut_n and values mapped to -1 sprinkled in"""
    rng = np.random.default_rng(seed)
    m = random_map(shape, 0.6, seed)
    odd = rng.choice(np.array([-1, -77, 4, 6, 1000, 2 ** 31 - 1, -2 ** 31], dtype=np.int64), size=shape).astype(np.int32)
    return np.where(rng.random(shape) < 0.3, odd, m).astype(np.int32)


@functools.lru_cache(maxsize=None)
def maps(shape):
    planes = np.broadcast_to(np.where(np.arange(shape[0]) % 2 == 0, 1, 2)[:, None, None], shape).astype(np.int32)
    rows = np.broadcast_to(np.where(np.arange(shape[1]) % 2 == 0, 3, 5)[None, :, None], shape).astype(np.int32)
    return (('random 0.2', random_map(shape, 0.2, 1)), ('random 0.31', random_map(shape, 0.31, 2)),
            ('random 0.9', random_map(shape, 0.9, 3)), ('serpentine', serpentine(shape)), ('checkerboard', checkerboard(shape)),
            ('planes of two groups', planes), ('rows of two groups', rows), ('one group', np.full(shape, 5, dtype=np.int32)),
            ('special values', special_values(shape, 4)))


SHAPES = [(1, 1, 1), (1, 1, 70), (5, 7, 9), (9, 33, 65), (40, 24, 72), (7, 1, 33),
          (TILE[0] - 1, TILE[1], TILE[2]), (TILE[0] + 1, TILE[1], TILE[2]), (TILE[0], TILE[1] - 1, TILE[2]),
          (TILE[0], TILE[1] + 1, TILE[2]), (TILE[0], TILE[1], TILE[2] - 1), (TILE[0], TILE[1], TILE[2] + 1)]


@pytest.mark.parametrize('shape', SHAPES)
def test_maps_equal_the_reference(T, shape):
    for what, m in maps(shape):
        for connectivity in CONNECTIVITIES:
            comp, out, stats = check(T, what, m, LUT3, 3, connectivity)
            if what == 'serpentine' and shape == (40, 24, 72):
                assert stats[1, 2] == 1 and stats[1, 1] == (m == 2).sum() > 15000, 'one path through every tile'
            if what == 'checkerboard' and min(shape) > 1:
                assert stats[2, 2] == ((m == 3).sum() if connectivity == 6 else 1)
            if what.endswith('two groups') and shape == (9, 33, 65):
                assert stats[:, 2].sum() == (5 + 4 if what.startswith('planes') else 17 + 16), 'adjacent groups did not merge'
            if what == 'one group':
                assert stats.tolist() == [[-1, 0, 0, 0], [0, m.size, 1, m.size], [-1, 0, 0, 0]]
                assert np.all(comp == 0) and np.array_equal(out, m)


def test_edge_and_corner_neighbours_tell_the_connectivities_apart(T):
    """pairs that touch by an edge only and by a corner only, inside a tile and across the borders of all three tile axes"""
    shape = (TILE[0] + 3, TILE[1] + 3, TILE[2] + 3)
    z, y, x = TILE[0] - 1, TILE[1] - 1, TILE[2] - 1
    # no voxel of one pair is adjacent to a voxel of another, under any connectivity
    edges = [((1, 1, 1), (1, 2, 2)), ((3, 1, 5), (4, 1, 6)), ((1, 5, 9), (2, 6, 9)),               # inside the first tile
             ((z, 1, 20), (z + 1, 2, 20)), ((1, y, 24), (1, y + 1, 23)), ((4, 4, x), (5, 4, x + 1)),   # across one tile border
             ((z, 5, x + 1), (z + 1, 5, x))]                                                         # across two
    corners = [((5, 1, 12), (6, 2, 13)), ((z, y, x), (z + 1, y + 1, x + 1)), ((z, 3, x + 1), (z + 1, 2, x)),
               ((3, y, x + 1), (2, y + 1, x)), ((z, 10, 12), (z + 1, 9, 13))]
    m = np.zeros(shape, dtype=np.int32)
    for pair in edges + corners:
        for p in pair:
            assert m[p] == 0
            m[p] = 1
    n = 2 * (len(edges) + len(corners))
    for connectivity, components in ((6, n), (18, n - len(edges)), (26, n // 2)):
        comp, _, stats = check(T, 'pairs', m, LUT3, 3, connectivity)
        assert stats[0, 2] == components and stats[0, 3] == n, connectivity


def test_filter_rules(T):
    torch = T
    shape = (6, 10, 40)
    m = np.zeros(shape, dtype=np.int32)
    m[1, 1, 1:4] = 1                       # group 0: three components of 3, 5 and 5 voxels: the first of the two of 5 is kept
    m[2, 3, 30:35] = 1
    m[4, 8, 33:38] = 1
    m[0, 0, 0] = 2                         # group 1 (values 2 and 5): one component made of both values next to each other
    m[0, 0, 1] = 5
    m[5, 9, 39] = 5                        # and a single voxel
    m[3, 3, 3], m[3, 3, 5], m[3, 3, 7] = 4, -5, 99           # in no group
    for connectivity in CONNECTIVITIES:
        comp, out, stats = check(torch, 'rules', m, LUT3, 3, connectivity, fill_value=0)
        at = lambda zyx: int(np.ravel_multi_index(zyx, shape))
        assert stats.tolist() == [[at((2, 3, 30)), 5, 3, 13], [0, 2, 2, 3], [-1, 0, 0, 0]]
        assert np.all(out[2, 3, 30:35] == 1) and np.all(out[4, 8, 33:38] == 0) and np.all(out[1, 1, 1:4] == 0)
        assert out[0, 0, 0] == 2 and out[0, 0, 1] == 5 and out[5, 9, 39] == 0
        assert (out[3, 3, 3], out[3, 3, 5], out[3, 3, 7]) == (4, -5, 99), 'voxels in no group are untouched'
        # the filtered map written over the label map
        check(torch, 'rules, in place', m, LUT3, 3, connectivity, fill_value=0, alias=True)
        # a fill value that is itself in a group is written as it is: the removed voxels of group 0 become value 3 (group 2),
        # and nothing is filtered again
        comp, out, stats = check(torch, 'rules, fill 3', m, LUT3, 3, connectivity, fill_value=3)
        assert np.all(out[4, 8, 33:38] == 3) and out[5, 9, 39] == 3 and stats[2].tolist() == [-1, 0, 0, 0]
        comp, out, stats = check(torch, 'rules, fill -7', m, LUT3, 3, connectivity, fill_value=-7)
        assert (out == -7).sum() == 3 + 5 + 1
    # G smaller than the table's groups: group 2 of the table is then no group
    check(torch, 'two of three groups', random_map((9, 9, 33), 0.5, 9), LUT3, 2, 6)
    # 64 groups, one value each, and a value range that begins above 0
    lut = np.concatenate([np.full(3, -1), np.arange(64)]).astype(np.int32)
    rng = np.random.default_rng(11)
    m = rng.integers(0, 70, size=(9, 17, 33)).astype(np.int32)
    m[2:7, 3:12, 5:20] = 40
    comp, out, stats = check(torch, '64 groups', m, lut, 64, 18, fill_value=1)
    assert (stats[:, 2] > 1).all() and stats[37, 1] >= 5 * 9 * 15


def test_repeatable_on_a_side_stream_and_another_device(T):
    torch = T
    from synthsr_amd import ops
    m = random_map((40, 24, 72), 0.31, 2)
    want = check(torch, 'default stream', m, LUT3, 3, 6)
    labels, lut = torch.from_numpy(m).cuda(), torch.from_numpy(LUT3).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        comp = ops.seg_components(labels, lut, 3, 6)
        out, stats = ops.seg_keep_largest(labels, comp, lut, 3, 0)
    side.synchronize()
    for got, ref in zip((comp, out, stats), want):
        assert np.array_equal(got.cpu().numpy(), ref)
    again = ops.seg_components(labels, lut, 3, 6)
    assert torch.equal(again, comp)


def test_result_on_a_non_default_device(T):
    torch = T
    from synthsr_amd import ops
    if torch.cuda.device_count() < 2:
        pytest.skip('one device visible')
    m = random_map((9, 33, 65), 0.31, 2)
    want_comp = reference_components(m, LUT3, 3, 18)
    want_out, want_stats = reference_keep_largest(m, want_comp, LUT3, 3, 0)
    with torch.cuda.device(1):
        labels, lut = torch.from_numpy(m).to('cuda:1'), torch.from_numpy(LUT3).to('cuda:1')
        comp = ops.seg_components(labels, lut, 3, 18)
        out, stats = ops.seg_keep_largest(labels, comp, lut, 3, 0)
        torch.cuda.synchronize()
    assert comp.device.index == 1
    assert np.array_equal(comp.cpu().numpy(), want_comp) and np.array_equal(out.cpu().numpy(), want_out)
    assert np.array_equal(stats.cpu().numpy(), want_stats)


def test_limits_are_refused_and_nothing_is_written(T):
    torch = T
    from synthsr_amd import ops, _lib
    lib = _lib.load()
    shape = (5, 7, 9)
    a = torch.zeros(shape, dtype=torch.int32, device='cuda')
    lut = torch.zeros(4, dtype=torch.int32, device='cuda')
    out = torch.full(shape, GARBAGE, dtype=torch.int32, device='cuda')
    stats = torch.full((2, 4), GARBAGE, dtype=torch.int64, device='cuda')
    need = ops.seg_components_workspace_bytes(shape)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    P = _lib.ptr
    for G, conn, nbytes in ((65, 6, need), (0, 6, need), (2, 8, need), (2, 6, need - 1)):
        assert lib.synthsr_seg_components(P(a), _lib.i3(shape), P(lut), 4, G, conn, P(out), P(ws), nbytes, _lib.stream()) == -1
    for G, nbytes in ((65, need), (0, need), (2, need - 1)):
        assert lib.synthsr_seg_keep_largest(P(a), P(a), _lib.i3(shape), P(lut), 4, G, 0, P(out), P(stats), P(ws), nbytes,
                                            _lib.stream()) == -1
    with pytest.raises(ValueError):
        ops.seg_components(a, lut, 2, connectivity=7, comp=out)
    torch.cuda.synchronize()
    assert bool((out == GARBAGE).all()) and bool((stats == GARBAGE).all())


# ---------------------------------------------------------------------------------------------------- the Python layer
LABELS = np.array([0, 14, 2, 41, 17], dtype=np.int32)


def test_functions_take_arrays_and_paths(T, tmp_path):
    from synthsr_amd import volumes as V
    from synthsr_amd.predict_segmentation import (component_groups, connected_components, keep_largest_components,
                                                  label_volumes)
    rng = np.random.default_rng(8)
    m = LABELS[rng.integers(0, 5, size=(9, 33, 20))].astype(np.int32)
    m[2:7, 5:25, 3:15] = 41
    m[0, 0, 0] = 7                                                  # not listed: in no group, counted in no volume
    path = str(tmp_path / 'm.nii.gz')
    V.save_volume(m, np.eye(4), None, path, dtype='int32')
    for groups, connectivity, fill in (('per_label', 6, None), ('foreground', 26, None), (np.array([0, 1, 1, -1, 0]), 18, 17)):
        lut, G, fill_value = component_groups(LABELS, groups, fill)
        want_comp = reference_components(m, lut, G, connectivity)
        want_out, want_stats = reference_keep_largest(m, want_comp, lut, G, fill_value)
        for source in (m, path, m.astype(np.int64), m.astype(np.float32)):
            got = connected_components(source, LABELS, groups, connectivity)
            assert got.dtype == np.int32 and np.array_equal(got, want_comp)
            out, stats = keep_largest_components(source, LABELS, groups, connectivity, fill, return_stats=True)
            assert out.dtype == np.int32 and np.array_equal(out, want_out) and np.array_equal(stats, want_stats)
        assert np.array_equal(keep_largest_components(m, LABELS, groups, connectivity, fill), want_out)
        if isinstance(groups, str) and groups == 'per_label':     # (a dense foreground at 26 may well be one component)
            assert (want_out != m).sum() > 0
    for source in (m, path):
        vol = label_volumes(source, LABELS, voxel_volume=0.5)
        assert vol.dtype == np.float64 and np.array_equal(vol, 0.5 * np.bincount(m.reshape(-1), minlength=42)[LABELS])
    assert label_volumes(m, LABELS).sum() == m.size - 1
    with pytest.raises(ValueError, match='3-D'):
        connected_components(m[0], LABELS)
    with pytest.raises(ValueError, match='3-D'):
        keep_largest_components(m[0], LABELS)


def test_far_island_and_the_hausdorff_distance(T):
    """two boxes of label 14 offset by (3, 0, 0), and in the segmentation one stray voxel of label 14 far away: the Hausdorff
    distance is the island's distance to the box before filtering and the boxes' own 3.0 after"""
    from synthsr_amd.predict_segmentation import keep_largest_components, surface_distances
    shape = (40, 12, 12)
    seg, truth = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    seg[2:8, 3:8, 3:8] = 14
    truth[5:11, 3:8, 3:8] = 14
    seg[38, 5, 5] = 14                                               # nearest voxel of the truth's box: (10, 5, 5)
    before = surface_distances(seg, truth, LABELS)
    assert before['hausdorff'][1] == np.sqrt(28.0 ** 2)
    cleaned, stats = keep_largest_components(seg, LABELS, return_stats=True)
    assert cleaned[38, 5, 5] == 0 and (cleaned != seg).sum() == 1 and stats[0].tolist() == [int(np.ravel_multi_index((2, 3, 3), shape)),
                                                                                            150, 2, 151]
    after = surface_distances(cleaned, truth, LABELS)
    assert after['hausdorff'][1] == np.sqrt(9.0)
    # the island off the box's axis: sqrt(28^2 + 4^2 + 3^2) before
    seg[38, 5, 5], seg[38, 11, 10] = 0, 14
    assert surface_distances(seg, truth, LABELS)['hausdorff'][1] == np.sqrt(28.0 ** 2 + 4 ** 2 + 3 ** 2)
    assert surface_distances(keep_largest_components(seg, LABELS), truth, LABELS)['hausdorff'][1] == 3.0


# ---------------------------------------------------------------------------------------------------- end to end
def test_predict_segmentation_keeps_the_largest_components(T, tmp_path):
    """the tiny network of tests/test_seg_predict_gpu.py's end-to-end test (3 levels, 8 features, random weights, volumes padded
    to 32^3): its argmax is noisy, so every label has many components"""
    torch = T
    from synthsr_amd.nifti import write_nifti, read_nifti
    from synthsr_amd.unet import unet
    from synthsr_amd.training import save_checkpoint
    from synthsr_amd import volumes as V
    from synthsr_amd.predict import prepare_volume
    from synthsr_amd.predict_segmentation import predict_segmentation, keep_largest_components, SegmentationPredictor
    rng = np.random.default_rng(5)
    d = tmp_path / 'images'
    d.mkdir()
    shapes = [(20, 18, 22), (17, 32, 9)]
    for i, s in enumerate(shapes):
        write_nifti(str(d / ('scan%d.nii.gz' % i)), rng.random(s).astype(np.float32) * 100)
    net = unet(nb_features=8, input_shape=[32, 32, 32, 1], nb_levels=3, conv_size=3, nb_labels=len(LABELS), feat_mult=2,
               nb_conv_per_level=2, batch_norm=-1, final_pred_activation='softmax', seed=3)
    net.view(net.head['w']).copy_(torch.randn(8, len(LABELS), generator=torch.Generator().manual_seed(6)))
    ckpt = str(tmp_path / 'seg.npz')
    save_checkpoint(ckpt, net)
    np.save(tmp_path / 'labels.npy', LABELS)
    arch = dict(n_levels=3, unet_feat_count=8, verbose=False)
    # a folder
    raw = predict_segmentation(str(d), str(tmp_path / 'raw'), ckpt, LABELS, **arch)
    kept = predict_segmentation(str(d), str(tmp_path / 'kept'), ckpt, LABELS, keep_largest='per_label', **arch)
    predictor = SegmentationPredictor(ckpt, LABELS, n_levels=3, unet_feat_count=8)
    changed = 0
    for r, k, s, i in zip(raw, kept, shapes, range(2)):
        a, b = read_nifti(r)[0], read_nifti(k)[0]
        assert a.dtype == np.int32 and b.dtype == np.int32 and a.shape == s and b.shape == s
        assert np.array_equal(b, keep_largest_components(a, LABELS)), 'the file is the filter of the unfiltered file'
        changed += int((a != b).sum())
        # keep_largest=None writes what the plain path gives: the whole padded map, cropped on the host
        im, aff, _ = V.load_volume(str(d / ('scan%d.nii.gz' % i)), im_only=False, dtype='float')
        S, idx, shape, _ = prepare_volume(im, aff)
        crop = tuple(slice(int(o), int(o) + int(n)) for o, n in zip(idx, shape))
        assert np.array_equal(a, predictor.segment_volume(S)[crop])
    assert changed > 0, 'the raw argmax of this network has stray components'
    # a file, another grouping, connectivity and fill label; the posteriors are written unchanged
    one = str(d / 'scan0.nii.gz')
    plain = predict_segmentation(one, str(tmp_path / 'a.nii.gz'), ckpt, LABELS, path_posteriors=str(tmp_path / 'pa.nii.gz'), **arch)
    filt = predict_segmentation(one, str(tmp_path / 'b.nii.gz'), ckpt, LABELS, path_posteriors=str(tmp_path / 'pb.nii.gz'),
                                keep_largest='foreground', connectivity=26, fill_label=2, **arch)
    a, b = read_nifti(plain[0])[0], read_nifti(filt[0])[0]
    assert np.array_equal(a, read_nifti(raw[0])[0])
    assert np.array_equal(b, keep_largest_components(a, LABELS, 'foreground', 26, 2))
    assert np.array_equal(read_nifti(str(tmp_path / 'pa.nii.gz'))[0], read_nifti(str(tmp_path / 'pb.nii.gz'))[0])
    # the script: --keep_largest with a grouping from a file, and the volumes of what it wrote
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    groups = np.array([-1, 0, 1, 1, 0])
    np.save(tmp_path / 'groups.npy', groups)
    seg = str(tmp_path / 'script_seg.nii.gz')
    common = [one, seg, '--model', ckpt, '--labels', str(tmp_path / 'labels.npy'), '--n_levels', '3', '--unet_feat', '8']
    for ext in ('npy', 'csv'):
        script.main(common + ['--keep_largest', str(tmp_path / 'groups.npy'), '--connectivity', '18', '--volumes',
                              str(tmp_path / ('vol.' + ext))])
    written = read_nifti(seg)[0]
    assert np.array_equal(written, keep_largest_components(a, LABELS, groups, 18))
    want = np.bincount(written.reshape(-1), minlength=42)[LABELS].astype(np.float64)
    assert np.array_equal(np.load(tmp_path / 'vol.npy'), want[None])
    rows = open(tmp_path / 'vol.csv').read().split('\n')
    assert rows == [','.join(str(v) for v in LABELS), ','.join(repr(float(v)) for v in want), '']
    script.main(common + ['--volumes', str(tmp_path / 'vol_raw.npy')])
    assert np.array_equal(read_nifti(seg)[0], a), 'without --keep_largest the script writes the raw argmax'
    assert np.array_equal(np.load(tmp_path / 'vol_raw.npy')[0], np.bincount(a.reshape(-1), minlength=42)[LABELS])
