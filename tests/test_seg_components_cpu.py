"""Host side of the connected components (no GPU): the reference the GPU tests compare with (scipy.ndimage.label per group,
made canonical) against a plain flood fill, the declarations and argument checks of the C entry points (csrc/seg_components.hip),
which return before any HIP call, the checks of the ops wrappers, component_groups, and the command line of
scripts/predict_segmentation.py."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _script():
    spec = importlib.util.spec_from_file_location('predict_segmentation_script',
                                                  os.path.join(ROOT, 'scripts', 'predict_segmentation.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------------------------------------------- the reference
def groups_of(m, lut, G):
    m = np.asarray(m, dtype=np.int64)
    inside = (m >= 0) & (m < len(lut))
    g = np.where(inside, np.asarray(lut, dtype=np.int64)[np.clip(m, 0, len(lut) - 1)], -1)
    return np.where((g >= 0) & (g < G), g, -1)


def reference_components(m, lut, G, connectivity):
    """scipy.ndimage.label per group with the matching structure, every component renamed to its smallest linear index"""
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
    """(out, stats): the largest component per group by size, then by smallest root"""
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


def flood_fill(grp, connectivity):
    d0, d1, d2 = grp.shape
    steps = [(a, b, c) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)
             if 1 <= abs(a) + abs(b) + abs(c) <= {6: 1, 18: 2, 26: 3}[connectivity]]
    comp = np.full(grp.shape, -1, dtype=np.int32)
    for v in range(grp.size):
        z, y, x = np.unravel_index(v, grp.shape)
        if grp[z, y, x] < 0 or comp[z, y, x] >= 0:
            continue
        comp[z, y, x] = v
        stack = [(z, y, x)]
        while stack:
            z, y, x = stack.pop()
            for a, b, c in steps:
                p = (z + a, y + b, x + c)
                if 0 <= p[0] < d0 and 0 <= p[1] < d1 and 0 <= p[2] < d2 and comp[p] < 0 and grp[p] == grp[z, y, x]:
                    comp[p] = v
                    stack.append(p)
    return comp


def test_reference_equals_a_flood_fill():
    rng = np.random.default_rng(3)
    lut = np.array([-1, 0, 1, 2, 1], dtype=np.int32)             # values 2 and 4 share a group
    m = rng.integers(-1, 7, size=(4, 5, 6)).astype(np.int32)
    distinct = set()
    for connectivity in (6, 18, 26):
        want = flood_fill(groups_of(m, lut, 3), connectivity)
        got = reference_components(m, lut, 3, connectivity)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert np.all((got >= 0) == (groups_of(m, lut, 3) >= 0))
        distinct.add(len(np.unique(got)))
        out, stats = reference_keep_largest(m, got, lut, 3, 0)
        for g in range(3):
            sizes = np.bincount(got[groups_of(m, lut, 3) == g])
            assert stats[g, 1] == sizes.max() and stats[g, 0] == np.argmax(sizes)     # argmax: the first of equal sizes
            assert stats[g, 2] == (sizes > 0).sum() and stats[g, 3] == sizes.sum()
            assert np.all(out[got == stats[g, 0]] == m[got == stats[g, 0]])
        assert np.array_equal(out[groups_of(m, lut, 3) < 0], m[groups_of(m, lut, 3) < 0])
    assert len(distinct) == 3, 'the three connectivities differ on this map'


# ---------------------------------------------------------------------------------------------------- the C interface
def test_symbols_are_declared_and_bound():
    from synthsr_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'synthsr_hip.h')).read()
    lib = _lib.load()
    for name, nargs in (('synthsr_seg_components_workspace_bytes', 1), ('synthsr_seg_components', 10),
                        ('synthsr_seg_keep_largest', 12)):
        decl = re.search(r'^int(?:64_t)? %s\(([^;]*)\);' % name, header, re.M)
        assert decl, name
        assert len(decl.group(1).split(',')) == nargs
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name) is not None
    assert _lib.SIGNATURES['synthsr_seg_components_workspace_bytes'][0] is ctypes.c_int64
    assert lib.synthsr_abi_version() == 2


def test_workspace_size_and_refusals_without_a_device():
    from synthsr_amd import _lib
    lib = _lib.load()
    size = lambda shape: lib.synthsr_seg_components_workspace_bytes(_lib.i3(shape))
    grown = [size(s) for s in ([1, 1, 1], [5, 7, 9], [5, 7, 10], [5, 8, 10], [6, 8, 10], [160, 160, 160], [1024, 1024, 1024])]
    assert grown[0] > 0 and all(y > x for x, y in zip(grown, grown[1:])), grown
    assert size([160, 160, 160]) >= 4 * 160 ** 3              # a size per root
    assert lib.synthsr_seg_components_workspace_bytes(None) == -1
    p = 4096                                                    # a non-NULL, 16-byte aligned address; never followed
    shape, G = [5, 7, 9], 5
    need = size(shape)

    def label(shape=shape, G=G, labels=p, lut=p, lut_n=8, conn=6, comp=p, ws=p, ws_bytes=need):
        return lib.synthsr_seg_components(labels, None if shape is None else _lib.i3(shape), lut, lut_n, G, conn, comp, ws,
                                          ctypes.c_int64(ws_bytes), None)

    def keep(shape=shape, G=G, labels=p, comp=p, lut=p, lut_n=8, out=p, stats=p, ws=p, ws_bytes=need):
        return lib.synthsr_seg_keep_largest(labels, comp, None if shape is None else _lib.i3(shape), lut, lut_n, G, 0, out, stats,
                                            ws, ctypes.c_int64(ws_bytes), None)
    for bad in ([0, 7, 9], [5, 0, 9], [5, 7, 0], [1025, 7, 9], [5, 1025, 9], [5, 7, 1025]):
        assert size(bad) == -1
        assert label(shape=bad, ws_bytes=1 << 40) == -1 and keep(shape=bad, ws_bytes=1 << 40) == -1
    for bad in (0, 65, -1):
        assert label(G=bad) == -1 and keep(G=bad) == -1
    for bad in (0, 4, 8, 7, 27, -6):
        assert label(conn=bad) == -1
    for name in ('labels', 'lut', 'comp', 'ws', 'shape'):
        assert label(**{name: None}) == -1, name
    for name in ('labels', 'comp', 'lut', 'out', 'stats', 'ws', 'shape'):
        assert keep(**{name: None}) == -1, name
    assert label(lut_n=0) == -1 and keep(lut_n=0) == -1
    assert label(ws_bytes=need - 1) == -1 and keep(ws_bytes=need - 1) == -1      # one byte too small
    assert label(ws=p + 8) == -1 and keep(ws=p + 8) == -1                        # not 16-byte aligned


def test_ops_wrappers_check_before_the_library():
    import torch
    from synthsr_amd import ops
    a = torch.zeros(5, 7, 9, dtype=torch.int32)
    lut = torch.zeros(4, dtype=torch.int32)
    stats = torch.zeros(2, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match='int32'):
        ops.seg_components(a.long(), lut, 2)
    with pytest.raises(ValueError, match='int32'):
        ops.seg_components(a, lut.long(), 2)
    with pytest.raises(ValueError, match=r'\[d0, d1, d2\]'):
        ops.seg_components(a.reshape(-1), lut, 2)
    with pytest.raises(ValueError, match='sides'):
        ops.seg_components(torch.zeros(1025, 1, 1, dtype=torch.int32), lut, 2)
    for G in (0, 65):
        with pytest.raises(ValueError, match='1 <= G <= 64'):
            ops.seg_components(a, lut, G)
        with pytest.raises(ValueError, match='1 <= G <= 64'):
            ops.seg_keep_largest(a, a, lut, G, 0)
    for connectivity in (4, 8, 27, None):
        with pytest.raises(ValueError, match='connectivity'):
            ops.seg_components(a, lut, 2, connectivity=connectivity)
    with pytest.raises(ValueError, match='one value per voxel'):
        ops.seg_components(a, lut, 2, comp=torch.zeros(5, 7, 8, dtype=torch.int32))
    with pytest.raises(ValueError, match='workspace'):
        ops.seg_components(a, lut, 2, workspace=torch.zeros(16, dtype=torch.uint8))
    with pytest.raises(ValueError, match='one value per voxel'):
        ops.seg_keep_largest(a, a.long(), lut, 2, 0)
    with pytest.raises(ValueError, match='one value per voxel'):
        ops.seg_keep_largest(a, a, lut, 2, 0, out=torch.zeros(5, 7, 9, dtype=torch.int64))
    with pytest.raises(ValueError, match='stats'):
        ops.seg_keep_largest(a, a, lut, 2, 0, stats=stats[:1])
    with pytest.raises(ValueError, match='stats'):
        ops.seg_keep_largest(a, a, lut, 2, 0, stats=stats.int())
    with pytest.raises(ValueError, match='fill_value'):
        ops.seg_keep_largest(a, a, lut, 2, 2 ** 31)
    with pytest.raises(ValueError, match='workspace'):
        ops.seg_keep_largest(a, a, lut, 2, 0, workspace=torch.zeros(16, dtype=torch.uint8))
    assert ops.seg_components_workspace_bytes((160, 160, 160)) >= 4 * 160 ** 3
    with pytest.raises(ValueError, match='sides'):
        ops.seg_components_workspace_bytes((0, 1, 1))


# ---------------------------------------------------------------------------------------------------- groupings
def test_component_groups():
    from synthsr_amd.predict_segmentation import component_groups
    labels = [0, 14, 2, 41, 17]
    lut, G, fill = component_groups(labels)
    assert lut.dtype == np.int32 and len(lut) == 42 and (G, fill) == (4, 0)
    assert [lut[v] for v in labels] == [-1, 0, 1, 2, 3] and (lut >= 0).sum() == 4
    lut, G, fill = component_groups(labels, 'foreground')
    assert (G, fill) == (1, 0) and [lut[v] for v in labels] == [-1, 0, 0, 0, 0] and (lut >= 0).sum() == 4
    lut, G, fill = component_groups(labels, 'per_label', fill_label=2)
    assert (G, fill) == (4, 2) and [lut[v] for v in labels] == [0, 1, -1, 2, 3]
    lut, G, fill = component_groups(labels, 'foreground', fill_label=99)      # not listed: every label is in the group
    assert (G, fill) == (1, 99) and [lut[v] for v in labels] == [0] * 5
    lut, G, fill = component_groups(labels, np.array([-1, 1, 0, 1, -1]))
    assert (G, fill) == (2, 0) and [lut[v] for v in labels] == [-1, 1, 0, 1, -1] and lut.dtype == np.int32
    lut, G, fill = component_groups(labels, [0, 0, 0, 0, 0], fill_label=17)   # a grouping given as ids is taken as it is
    assert (G, fill) == (1, 17) and [lut[v] for v in labels] == [0] * 5
    many = np.arange(66)
    assert component_groups(many[:65])[1] == 64
    with pytest.raises(ValueError, match='at most 64 groups'):
        component_groups(many)
    with pytest.raises(ValueError, match='at most 64 groups'):
        component_groups(many, np.arange(66) - 1)
    assert component_groups(many, 'foreground')[1] == 1
    for bad in (np.array([-1, 0, 2, 2, -1]), np.array([1, 1, 1, 1, 1])):
        with pytest.raises(ValueError, match='without gaps'):
            component_groups(labels, bad)
    with pytest.raises(ValueError, match='one group id per listed label'):
        component_groups(labels, np.array([0, 1, 2]))
    with pytest.raises(ValueError, match='integer group ids'):
        component_groups(labels, np.array([0, .5, 0, 0, 0]))
    with pytest.raises(ValueError, match='integer group ids'):
        component_groups(labels, np.array([0, -2, 0, 0, 0]))
    with pytest.raises(ValueError, match='no label in any group'):
        component_groups(labels, np.full(5, -1))
    with pytest.raises(ValueError, match="'per_label', 'foreground'"):
        component_groups(labels, 'topology')
    with pytest.raises(ValueError, match='fill_label'):
        component_groups(labels, fill_label=1.5)


# ---------------------------------------------------------------------------------------------------- the command line
def test_script_arguments_and_volume_table(tmp_path):
    S = _script()
    p = S.build_parser()
    base = ['in', 'out', '--model', 'm.npz', '--labels', 'l.npy']
    a = p.parse_args(base)
    assert (a.keep_largest, a.connectivity, a.fill_label, a.volumes) == (None, 6, None, None)
    assert (a.truth, a.scores, a.surface_scores, a.surface_percentile, a.dtype) == (None, None, None, 95, 'f32')
    a = p.parse_args(base + ['--keep_largest', 'foreground', '--connectivity', '26', '--fill_label', '3', '--volumes', 'v.csv'])
    assert (a.keep_largest, a.connectivity, a.fill_label, a.volumes) == ('foreground', 26, 3, 'v.csv')
    assert p.parse_args(base + ['--keep_largest', 'g.npy', '--connectivity', '18']).connectivity == 18
    for bad in (['--connectivity', '8'], ['--connectivity', 'faces'], ['--fill_label', '1.5'], ['--keep_largest', 'largest'],
                ['--keep_largest', 'g.txt'], ['--volumes', 'v.txt'], ['--keep_largest']):
        with pytest.raises(SystemExit):
            S.main(base + bad)
    table = np.array([[1200.0, 0.0, 35.0], [1.0, 2.0, 3.0]])
    S.write_volumes(str(tmp_path / 'v.npy'), [0, 14, 2], table)
    assert np.array_equal(np.load(tmp_path / 'v.npy'), table)
    S.write_volumes(str(tmp_path / 'v.csv'), [0, 14, 2], table)
    assert open(tmp_path / 'v.csv').read().split('\n') == ['0,14,2', '1200.0,0.0,35.0', '1.0,2.0,3.0', '']
    S.write_scores(str(tmp_path / 's.csv'), [0, 14, 2], table)
    assert open(tmp_path / 's.csv', 'rb').read() == open(tmp_path / 'v.csv', 'rb').read()
    with pytest.raises(ValueError, match='--volumes'):
        S.write_volumes(str(tmp_path / 'v.txt'), [0, 14, 2], table)
