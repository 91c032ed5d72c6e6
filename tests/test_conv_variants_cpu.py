"""The routing half of tests/test_conv_variants_gpu.py without a GPU: the dispatcher rules restated there (_expect / _route) against
the library's own plan query, which is host code (synthsr_conv3d_plan on a workspace-less context).

The deterministic mode is per-device library state: without a device the query always plans as if it were off, so a row that
runs with it on is compared with the rules evaluated for det = False here; its ksplit under the mode it runs in is asserted on the
GPU (test_conv_variants_gpu._route_holds)."""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from synthsr_amd import _lib, ops

from test_conv_variants_gpu import BF16_CASES, CASES, F32_CASES, PLAN_FIELDS, ROUTES, _expect, _expect_bf16, _route, check_plan

HERE = os.path.dirname(os.path.abspath(__file__))


def test_the_plan_query_initialises_no_device():
    """in a fresh interpreter (this one may have run GPU tests before): importing the package and the table and asking for a plan
    leaves torch's device runtime untouched"""
    code = ('import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import torch; import test_conv_variants_gpu as t; '
            'from synthsr_amd import ops; ops.set_conv_arithmetic("fp32_mfma"); t.check_plan(t.BY_ID["lean_ks"], False); '
            'assert not torch.cuda.is_initialized()' % (os.path.dirname(HERE), HERE))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_conv_variant_table_is_complete_and_routes_as_declared():
    assert {c.route for c in CASES} == ROUTES
    for c in CASES:
        assert _route(c) == c.route, (c.id, _route(c))


@pytest.mark.parametrize('cid', [c.id for c in F32_CASES])
def test_restated_plan_agrees_with_the_library(cid):
    """ck, ncc, pack_nt, nchunks, mt, ksplit, nv of every f32 row under the row's arithmetic"""
    c = next(c for c in F32_CASES if c.id == cid)
    prev = ops.set_conv_arithmetic(c.arith)
    try:
        check_plan(c, det=False)
    finally:
        ops.set_conv_arithmetic(prev)
    if c.det:       # the rules themselves say what the mode changes: split-K off, everything else as planned
        on, off = _expect(c, True), _expect(c, False)
        assert on['ksplit'] == 1 or on['route'] == 'split_fwd2_halves'
        assert all(on[f] == off[f] for f in PLAN_FIELDS if f != 'ksplit')


def test_bf16_rows_cover_every_chunk_width_and_tile_count():
    plain = [_expect_bf16(c) for c in BF16_CASES if c.entry == 'plain']
    assert {p['ck'] for p in plain} == {8, 24, 32} and {p['mt'] for p in plain} == {1, 2, 3, 4}
    assert any(p['ksplit'] > 1 for p in plain) and any(p['ksplit'] == 1 for p in plain)


# ---- the routing of a whole grid of layers, pinned --------------------------------------------------------------------------
# Every host-only answer of the fp32 conv planner over shapes x Cin x Cout x kind x arithmetic, recorded once by
# tests/golden/gen/make_conv_plan_golden.py (which calls plan_sweep below) and replayed here: a change of csrc/conv3d.hip that
# moves a layer to another kernel, grid or packed layout without meaning to shows up as a changed row.
SWEEP_SHAPES = sorted({c.shape for c in F32_CASES}) + [(n, n, n) for n in (10, 20, 40, 80, 160)]
SWEEP_CIN = (1, 2, 8, 24, 32, 40, 48, 96, 128, 192, 384)
SWEEP_COUT = (8, 16, 18, 20, 24, 40, 48, 64, 96, 128, 192, 384)
SWEEP_KINDS = (0, 1, 2)         # synthsr_conv3d_plan: 1 plain, 2 forward parity convs of a folded decoder conv, 0 their data gradient
SWEEP_ARITH = (0, 1, 2)         # fp32_mfma, split, split9
SWEEP_COLUMNS = ('plan_rc', 'ck', 'ncc', 'pack_nt', 'nchunks', 'mt', 'ksplit', 'reserved', 'count', 'pack_fwd', 'pack_dgrad',
                 'wgrad_split', 'up_wgrad_split')
# synthsr_conv3d_pack_ex (mode, up) of the weight sets whose EFFECTIVE conv has the kind: (forward-oriented set, transposed set)
_PACK_OF_KIND = {1: ((0, 0), (1, 0)), 2: ((0, 1), (1, 2)), 0: ((0, 2), (1, 1))}
GOLDEN_SWEEP = os.path.join(HERE, 'golden', 'conv_plan_sweep.npz')


def plan_sweep(lib):
    """int64 [combinations][SWEEP_COLUMNS], combinations in itertools.product order of (arithmetic, kind, shape, Cin, Cout), where
    Cin -> Cout is the effective conv: the return code and the eight outputs of synthsr_conv3d_plan, the sizes
    synthsr_conv3d_pack_ex(packed = NULL) reports for the two weight sets of that effective conv, and the two weight-gradient
    queries -- error returns included.  Host code only: no device is touched."""
    rows = []
    for arith, kind, shape, cin, cout in itertools.product(SWEEP_ARITH, SWEEP_KINDS, SWEEP_SHAPES, SWEEP_CIN, SWEEP_COUT):
        ctx = ctypes.byref(_lib.ConvCtx(arithmetic=arith))
        s3 = _lib.i3(shape)
        out = (ctypes.c_int64 * 8)(*([-1] * 8))
        row = [lib.synthsr_conv3d_plan(ctx, s3, cin, cout, kind, out)] + [int(v) for v in out]
        for mode, up in _PACK_OF_KIND[kind]:
            lci, lco = (cout, cin) if mode else (cin, cout)     # the layer whose (transposed) conv is cin -> cout
            row.append(lib.synthsr_conv3d_pack_ex(ctx, None, None, s3, lci, 0, lci, lco, mode, up, None))
        row.append(lib.synthsr_conv3d_wgrad_runs_split(ctx, s3, cin, cout))
        row.append(lib.synthsr_conv3d_up_wgrad_runs_split(ctx, s3, cin, cout))
        rows.append(row)
    return np.asarray(rows, dtype=np.int64)


def test_plan_sweep_matches_the_recorded_routing():
    """plan, packed sizes and weight-gradient routing of SWEEP_* are what tests/golden/conv_plan_sweep.npz recorded"""
    g = np.load(GOLDEN_SWEEP)
    assert [tuple(s) for s in g['shapes']] == list(SWEEP_SHAPES) and tuple(g['cin']) == SWEEP_CIN and tuple(g['cout']) == SWEEP_COUT
    assert tuple(g['kinds']) == SWEEP_KINDS and tuple(g['arith']) == SWEEP_ARITH and tuple(g['columns']) == SWEEP_COLUMNS
    got, want = plan_sweep(_lib.load()), g['table']
    assert got.shape == want.shape
    assert (want[:, SWEEP_COLUMNS.index('reserved')] == 0).all()
    combos = list(itertools.product(SWEEP_ARITH, SWEEP_KINDS, SWEEP_SHAPES, SWEEP_CIN, SWEEP_COUT))
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, '%d of %d rows differ, first: (arith, kind, shape, cin, cout) = %r got %r want %r' % (
        bad.size, len(combos), combos[bad[0]], dict(zip(SWEEP_COLUMNS, got[bad[0]])), dict(zip(SWEEP_COLUMNS, want[bad[0]])))
