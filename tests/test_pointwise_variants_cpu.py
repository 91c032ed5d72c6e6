"""The launch half of tests/test_pointwise_variants_gpu.py without a GPU: every row of its table reaches the launch regime it
declares under the launch rules restated there (syn_grid, red_grid() = 768, the 4096 default, RB = 384, `fixed`), the table covers
every regime listed in REGIMES, and the restated constants are the ones csrc/unet_pointwise.hip and csrc/common.h compile.

A fact the bit-identity rows of that file rest on, checked on the host once and not repeated here: for every n < 2**24,
1.0f / (float)n == (float)(1.0 / (double)n), so the two spellings of inv_n in bn_pool_elu_bwd_t and act_bwd_t agree at every size
the table uses."""
import os
import re
import types

import pytest

from test_pointwise_variants_gpu import (BY_ID, CASES, GRID_256, RB, RED_GRID, REGIMES, _cases, _grid, _lanes, _launch, _regime,
                                         check_table)

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'synthsr_amd', 'csrc')


def test_the_pointwise_table_reaches_every_regime_it_declares():
    check_table()


@pytest.mark.parametrize('cid', [c.id for c in CASES])
def test_declared_regime_is_the_computed_one(cid):
    c, got = BY_ID[cid], _launch(BY_ID[cid])
    assert (got['red'], got['g256'], got['body'], got['lds']) == (c.red, c.g256, c.body, c.lds), got


def test_the_regime_rule_at_its_edges():
    """one lane either side of every threshold of the restated syn_grid"""
    assert [_regime(n, 256, 4096) for n in (1, 255, 256, 257, 512)] == ['partial', 'partial', 'one_full', 'ragged', 'even']
    top = RED_GRID * RB
    assert [_regime(n, RB, RED_GRID) for n in (top - 1, top, top + 1, 2 * top)] == ['ragged', 'even', 'clamped_ragged', 'clamped_even']
    assert (_grid(0, RB, RED_GRID), _grid(top + 1, RB, RED_GRID), _grid(top - RB, RB, RED_GRID)) == (1, RED_GRID, RED_GRID - 1)
    for kind in ('flat', 'pool'):       # a clamped row's loop takes at least two trips, the last one ragged
        for c in _cases(kind):
            if c.red == 'clamped_ragged':
                assert _lanes(c)[0] > top and _lanes(c)[0] % top, c.id


def test_the_restated_constants_are_the_compiled_ones():
    """RB, red_grid(), syn_grid's default cap, the `fixed` rule and ok_c4 as the sources spell them"""
    pw = open(os.path.join(CSRC, 'unet_pointwise.hip')).read()
    common = open(os.path.join(CSRC, 'common.h')).read()
    assert int(re.search(r'constexpr int RB = (\d+);', pw).group(1)) == RB
    assert int(re.search(r'constexpr int red_grid\(\) \{ return (\d+); \}', pw).group(1)) == RED_GRID
    m = re.search(r'syn_grid\(int64_t n, int block, int max_blocks = (\d+) \* (\d+)\)', common)
    assert int(m.group(1)) * int(m.group(2)) == GRID_256
    assert pw.count('const bool fixed = (RB % C4) == 0;') >= 5        # the five channel-sum kernels in scope (and the head's)
    assert 'inline bool ok_c4(int C) { return C > 0 && (C % 4) == 0 && C <= 4096; }' in pw


def test_unet_refuses_deterministic_mode_for_channel_counts_without_a_fixed_group(monkeypatch):
    """UNet3D.backward under ops.set_deterministic: feature counts whose C / 4 does not divide 384 (20: the atomics body, whose LDS
    float atomics land in arbitration order) are refused before anything runs; 24 goes on to the backward pass"""
    from synthsr_amd import ops, unet
    monkeypatch.setattr(ops, '_deterministic', True)
    ran = []
    net = types.SimpleNamespace(nb_levels=2, grads=None, bf16=True, _drop=None,
                                _backward_inner=lambda *a: ran.append(a) or 'ran')
    for feats in ([20, 40], [24, 28], [6, 12]):
        net.feats = feats
        with pytest.raises(ValueError, match='deterministic mode'):
            unet.UNet3D.backward(net)
    assert not ran
    for feats in ([24, 48], [4, 8, 16], [512]):
        net.feats = feats
        assert unet.UNet3D.backward(net) == 'ran'
    assert len(ran) == 3
