"""The routing half of tests/test_conv_variants_gpu.py without a GPU: the dispatcher rules restated there (_expect / _route) against
the library's own plan query, which is host code (synthsr_conv3d_plan on a workspace-less context).

The deterministic mode is per-device library state: without a device the query always plans as if it were off, so a row that
runs with it on is compared with the rules evaluated for det = False here; its ksplit under the mode it runs in is asserted on the
GPU (test_conv_variants_gpu._route_holds)."""
import os
import subprocess
import sys

import pytest

from synthsr_amd import ops

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
