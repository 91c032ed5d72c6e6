"""Every HBM-bound U-Net kernel of csrc/unet_pointwise.hip on its own against float64: BatchNorm statistics / apply / backward,
BN + max-pool and its backward forms, the one-pass pool + BN + activation backward, the activation backward with its BatchNorm,
rank-1-head and per-sample-dropout groups, upsample + concat and its backward, scale_channels, Adam.

One table (CASES).  Every row declares the launch regime it is there for; _launch restates the launch rules (csrc/common.h
syn_grid, red_grid() = 768 workgroups of RB = 384 threads for the channel reductions, 4096 workgroups of 256 threads for the rest,
`fixed = RB % (C / 4) == 0` chooses register partials or per-element LDS atomics) and tests/test_pointwise_variants_cpu.py
asserts computed == declared and that the table covers every regime of REGIMES -- without a GPU.

Comparand: the same formula on the same operands (bf16 rows: the bf16-rounded operands) evaluated on the host in float64.
Bounds (README "Parity", conftest.single_shot_parity): the same formula is also evaluated in float32 on the host, o is that
evaluation's distance from float64, and the device must satisfy d <= 6 o + floor.  Floors: element-wise outputs 2e-5 of the
reference rms (d, o = worst element / reference rms; MAX_BOUND of tests/test_conv_variants_gpu.py), channel sums and statistics
1e-6 of the largest float64 value of the group (STATS_BOUND).  bf16 element-wise outputs: |y - ref| <= 2**-8 |ref| + the fp32
bound; bf16 reductions are fp32 sums of the rounded inputs and are held to the fp32 bound.

Deterministic mode covers channel counts with 384 % (C / 4) == 0 only (UNet3D refuses the others): those rows run every reduction
twice with the mode on, bit-identical; the atomics-body rows (C = 20, 40, 400) never run with it.

Measured on an MI355X (the file takes 15 s there).  Worst d with its o over a row's checks: element-wise outputs in units of the
reference rms (bf16: what is left beyond one bf16 ulp), sums / statistics in units of the group's largest value.
  row                       f32 outputs d / o     f32 sums d / o        bf16 outputs d / o    bf16 sums d / o
  flat_c4_one_wg            2.92e-07 / 5.05e-07   2.18e-07 / 3.85e-07   0        / 8.33e-08   1.61e-07 / 1.61e-07
  flat_c24                  1.06e-06 / 1.06e-06   3.80e-07 / 1.67e-07   2.14e-08 / 2.17e-07   5.53e-07 / 2.73e-07
  flat_c20                  9.17e-07 / 9.17e-07   5.91e-07 / 3.85e-07   1.26e-08 / 2.05e-07   6.08e-07 / 4.02e-08
  flat_c40                  1.25e-06 / 1.25e-06   3.53e-07 / 3.87e-07   1.66e-08 / 2.51e-07   4.66e-07 / 5.35e-07
  flat_c512                 1.18e-06 / 1.18e-06   2.47e-07 / 2.73e-07   3.93e-08 / 3.08e-07   2.65e-07 / 3.02e-07
  flat_c400                 1.44e-06 / 1.44e-06   1.95e-07 / 1.77e-07   4.94e-08 / 3.11e-07   2.06e-07 / 3.10e-07
  flat_c24_red_clamped      1.54e-06 / 1.54e-06   4.55e-06 / 4.46e-06   5.84e-08 / 8.73e-07   5.83e-06 / 5.59e-06
  flat_c400_red_clamped     1.69e-06 / 2.00e-06   1.17e-06 / 1.18e-07   5.71e-08 / 7.46e-07   1.85e-06 / 8.49e-07
  flat_c512_both_clamped    2.23e-06 / 2.23e-06   1.86e-06 / 1.65e-06   7.56e-08 / 4.05e-07   2.30e-06 / 2.96e-07
  pool_c4_one_wg            1.84e-07 / 2.36e-07   3.00e-08 / 3.00e-08   0        / 0          6.19e-08 / 3.09e-08
  pool_c24                  1.27e-06 / 1.27e-06   2.14e-07 / 1.59e-07   0        / 0          2.68e-07 / 6.62e-08
  pool_c20                  1.23e-06 / 1.60e-06   5.94e-07 / 1.17e-07   0        / 0          4.20e-07 / 1.86e-07
  pool_c40                  1.20e-06 / 1.80e-06   2.87e-07 / 1.57e-07   0        / 0          3.61e-07 / 9.72e-08
  pool_c512                 1.89e-06 / 1.89e-06   2.24e-07 / 1.22e-07   4.79e-09 / 1.74e-06   1.81e-07 / 1.50e-07
  pool_c400                 1.44e-06 / 1.47e-06   1.82e-07 / 1.18e-07   3.39e-09 / 7.25e-07   1.42e-07 / 1.63e-07
  pool_c400_red_clamped     2.77e-06 / 2.52e-06   1.41e-06 / 1.64e-07   1.13e-07 / 8.91e-07   1.31e-06 / 1.74e-07
  pool_c512_red_clamped     3.35e-06 / 2.39e-06   1.16e-06 / 1.43e-07   1.20e-07 / 1.04e-06   1.55e-06 / 2.06e-07
  pool_c512_256_clamped     4.11e-07 / 4.46e-07   -                     -                     -
  cat_4_20_one_wg           1.60e-06 / 1.57e-06   -                     0 / 0                 -
  cat_24_48                 4.09e-07 / 4.09e-07   -                     0 / 3.69e-07          -
  cat_24_48_clamped         6.32e-07 / 5.00e-07   -                     0 / 8.43e-08          -
  adam_1 / _1000 / _second_trip   worst of p, m, v 6.50e-08 / 1.96e-07 / 3.76e-07, each equal to its o
  stats_offset50            -                     1.52e-07 / 3.60e-08 (variance; mean 3.73e-08 / 1.27e-07)
Every bound holds (the narrowest margin: bn_reduce_bwd's sums of flat_c512_both_clamped in bf16, 2.30e-06 of 2.78e-06; the sums
of the non-deterministic runs move in their last digits from run to run with the order of the atomics).

Two rows failed when this file was written, and csrc/unet_pointwise.hip was mended for both:
 1. bn_pool_elu_bwd was NOT bit-identical to bn_maxpool_bwd + bn_elu_bwd: fp32 rows differed in 0.2 - 0.6 % of the elements, last
    bits only.  In bn_pool_elu_bwd_kernel the compiler fused s0 * inv_n into the subtraction for the first voxel of a window and
    hoisted it as a separately rounded product for the other seven (read in the gfx950 assembly); elu_bwd_kernel fused it always.
    Both now call bn_bwd_map, which spells the two fused multiply-adds out with contraction off; elu_bwd_kernel's arithmetic is
    instruction for instruction what it was, bn_pool_elu_bwd_kernel's moved by last bits.
 2. stats_offset50: the variance of a tensor with mean 50 and standard deviation 1 came back 7.26e-04 of the largest variance from
    float64 (o 3.60e-08, bound 1.2e-06): the fp32 partials of x^2 ~ 2500 carry 1.5e-4 each.  bn_stats_kernel now sums x - k and
    (x - k)^2 with k the mean of the channel's first 32 values: 1.52e-07.  (A shift by the first value alone met neither this
    row, 1.32e-06, nor flat_c20, 1.52e-06: one sample can sit three deviations out.)"""
import collections
import functools
import math

import numpy as np
import pytest
import torch

from conftest import _unwindows, _windows

pytestmark = pytest.mark.gpu

GRAD_K, MAX_BOUND, STATS_BOUND = 6.0, 2e-5, 1e-6
BF16_ULP = 2.0 ** -8
RB, RED_GRID, GRID_256 = 384, 768, 4096     # unet_pointwise.hip RB, red_grid(); common.h syn_grid's default max_blocks = 256 * 16
EPS = float(np.float32(1e-3))               # ops.BN_EPS as the C float the entry points receive
MAX_BYTES = 160e6                           # largest fp32 tensor of a row

Case = collections.namedtuple('Case', 'id kind shape C B dtypes det red g256 body lds')
#   kind:  'flat'  the [nvox][C] kernels (bn_stats, bn_apply, bn_reduce_bwd, bn_bwd, scale_channels, the activation-backward family);
#                  B samples stacked along the first axis for the dropout kernels
#          'pool'  bn_maxpool, bn_maxpool_bwd (three forms), bn_pool_elu_bwd on `shape` (the un-pooled grid); n4 = the POOLED count
#          'cat'   upsample_concat / upsample_concat_bwd on `shape` (the high-resolution grid), C = (Cs, Cl)
#          'adam'  adam_step on shape[0] values
#          'stats' bn_stats alone (the offset-dominated row)
#   red / g256: the regime of the 384-thread reduction grids / the 256-thread grids ('cat': forward/backward); body: 'fixed' register
#   partials or 'atomics'; lds: trips of the LDS clear and flush loops over 2C floats (1, or 2 when 2C > 2 * 384 ... C > RB)
#   det:   every reduction also runs twice in deterministic mode (fixed rows only)


def _c(id, kind, shape, C, red, g256, body='-', lds=0, B=1, dtypes=('f32', 'bf16'), det=None):
    return Case(id, kind, tuple(shape), C, B, tuple(dtypes), (body == 'fixed') if det is None else det, red, g256, body, lds)


CASES = [
    # ---- [nvox][C] kernels
    _c('flat_c4_one_wg', 'flat', (2, 2, 2), 4, 'partial', 'partial', 'fixed', 1),                 # 8 lanes of one workgroup
    _c('flat_c24', 'flat', (6, 5, 7), 24, 'ragged', 'ragged', 'fixed', 1, B=3),                   # 1260 lanes: 4 / 5 workgroups
    _c('flat_c20', 'flat', (6, 5, 7), 20, 'ragged', 'ragged', 'atomics', 1, B=3),
    _c('flat_c40', 'flat', (6, 5, 7), 40, 'ragged', 'ragged', 'atomics', 1, B=3),
    _c('flat_c512', 'flat', (2, 5, 7), 512, 'ragged', 'even', 'fixed', 2),                        # 2C floats of LDS: two trips
    _c('flat_c400', 'flat', (2, 5, 7), 400, 'ragged', 'ragged', 'atomics', 2),
    _c('flat_c24_red_clamped', 'flat', (30, 41, 40), 24, 'clamped_ragged', 'ragged', 'fixed', 1, B=3),      # 295200 > 768 * 384
    _c('flat_c400_red_clamped', 'flat', (12, 13, 19), 400, 'clamped_ragged', 'ragged', 'atomics', 2, B=3),  # stride % C4 = 12
    _c('flat_c512_both_clamped', 'flat', (6, 37, 37), 512, 'clamped_ragged', 'clamped_ragged', 'fixed', 2, B=3),  # > 4096 * 256
    # ---- pooled kernels (three distinct even extents)
    _c('pool_c4_one_wg', 'pool', (2, 2, 2), 4, 'partial', 'partial', 'fixed', 1),
    _c('pool_c24', 'pool', (10, 6, 14), 24, 'ragged', 'ragged', 'fixed', 1),
    _c('pool_c20', 'pool', (10, 6, 14), 20, 'ragged', 'ragged', 'atomics', 1),
    _c('pool_c40', 'pool', (6, 4, 10), 40, 'partial', 'ragged', 'atomics', 1),
    _c('pool_c512', 'pool', (10, 4, 14), 512, 'ragged', 'even', 'fixed', 2),
    _c('pool_c400', 'pool', (6, 4, 10), 400, 'ragged', 'ragged', 'atomics', 2),
    _c('pool_c400_red_clamped', 'pool', (24, 26, 38), 400, 'clamped_ragged', 'ragged', 'atomics', 2),
    _c('pool_c512_red_clamped', 'pool', (10, 42, 44), 512, 'clamped_ragged', 'even', 'fixed', 2),
    # the 256-thread pooled kernels past 4096 workgroups: 137 MB; bn_maxpool and the plain bn_maxpool_bwd only, fp32 only
    _c('pool_c512_256_clamped', 'pool', (12, 68, 82), 512, '-', 'clamped_ragged', '-', 0, dtypes=('f32',), det=False),
    # ---- upsample + concat
    _c('cat_4_20_one_wg', 'cat', (2, 2, 2), (4, 20), '-', 'partial/partial'),
    _c('cat_24_48', 'cat', (6, 4, 10), (24, 48), '-', 'ragged/ragged'),
    _c('cat_24_48_clamped', 'cat', (50, 52, 54), (24, 48), '-', 'clamped_ragged/clamped_ragged'),
    # ---- Adam
    _c('adam_1', 'adam', (1,), 1, '-', 'partial', dtypes=('f32',)),
    _c('adam_1000', 'adam', (1000,), 1, '-', 'ragged', dtypes=('f32',)),
    _c('adam_second_trip', 'adam', (GRID_256 * 256 + 77,), 1, '-', 'clamped_ragged', dtypes=('f32',)),
    # ---- BatchNorm statistics of a tensor whose mean dwarfs its spread: E[x^2] - m^2 cancels
    _c('stats_offset50', 'stats', (6, 5, 7), 24, 'ragged', '-', 'fixed', 1, dtypes=('f32',), det=False),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
OFFSET = 50.0

# what the table must reach, per kind: (red regimes, 256-thread regimes, (body, lds) pairs, channel counts)
_THREE = {'partial', 'ragged', 'clamped_ragged'}
_BODIES = {('fixed', 1), ('atomics', 1), ('fixed', 2), ('atomics', 2)}
REGIMES = {
    'flat': (_THREE, _THREE, _BODIES, {4, 24, 20, 40, 512, 400}),
    'pool': (_THREE, _THREE, _BODIES, {4, 24, 20, 40, 512, 400}),
    'cat': (set(), {'partial/partial', 'ragged/ragged', 'clamped_ragged/clamped_ragged'}, set(), {(24, 48), (4, 20)}),
    'adam': (set(), _THREE, set(), {1}),
}


def _cases(kind):
    return [c for c in CASES if c.kind == kind]


def _params(kind):
    return [pytest.param(c.id, dt, id='%s-%s' % (c.id, dt)) for c in _cases(kind) for dt in c.dtypes]


# ---- the launch rules restated ----------------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _grid(n, block, cap):
    """csrc/common.h syn_grid"""
    return max(1, min(_cdiv(n, block), cap))


def _regime(n, block, cap):
    """'partial': one workgroup that is not full; 'ragged' / 'even': several workgroups, no clamp, the last one partly filled or
    full; 'clamped_ragged' / 'clamped_even': the grid is clamped, so the grid-stride loop takes at least two trips, the last one
    partly filled or full"""
    g = _cdiv(n, block)
    if g <= 1:
        return 'partial' if n < block else 'one_full'
    if g <= cap:
        return 'ragged' if n % block else 'even'
    return 'clamped_ragged' if n % (cap * block) else 'clamped_even'


def _lanes(c):
    """float4 lanes (Adam: values) the row's grids are sized by: (reduction kernels, 256-thread kernels [, the concat backward])"""
    nvox = int(np.prod(c.shape))
    if c.kind in ('flat', 'stats'):
        return nvox * (c.C // 4), nvox * (c.C // 4)
    if c.kind == 'pool':
        return nvox // 8 * (c.C // 4), nvox // 8 * (c.C // 4)
    if c.kind == 'cat':
        Cs, Cl = c.C
        return 0, nvox * ((Cs + Cl) // 4), nvox * (Cs // 4) + nvox // 8 * (Cl // 4)
    return 0, nvox


def _launch(c):
    """the declared fields of a row, computed: red, g256, body, lds, plus 'stride_off' (the clamped reduction grid's stride is no
    multiple of C / 4: a thread meets another channel group on its second trip) and 'bytes' (the largest fp32 tensor)"""
    lanes = _lanes(c)
    nvox = int(np.prod(c.shape))
    out = dict(red='-', body='-', lds=0, stride_off=False)
    if c.kind == 'cat':
        out['g256'] = '%s/%s' % (_regime(lanes[1], 256, GRID_256), _regime(lanes[2], 256, GRID_256))
        out['bytes'] = 4 * nvox * sum(c.C)
        return out
    out['g256'] = _regime(lanes[1], 256, GRID_256)
    out['bytes'] = 4 * nvox * c.C
    if c.kind == 'adam':
        return out
    C4 = c.C // 4
    out.update(red=_regime(lanes[0], RB, RED_GRID), body='fixed' if RB % C4 == 0 else 'atomics', lds=_cdiv(c.C, RB))
    out['stride_off'] = (_grid(lanes[0], RB, RED_GRID) * RB) % C4 != 0
    if c.id == 'pool_c512_256_clamped':      # runs no reduction kernel
        out.update(red='-', body='-', lds=0)
    if c.kind == 'stats':
        out['g256'] = '-'
    return out


def check_table():
    """computed == declared for every row; every regime of REGIMES is reached; the limits the table was built under"""
    for c in CASES:
        got = _launch(c)
        assert (got['red'], got['g256'], got['body'], got['lds']) == (c.red, c.g256, c.body, c.lds), (c.id, got)
        assert got['bytes'] <= MAX_BYTES, (c.id, got['bytes'])
        assert not c.det or c.body == 'fixed', c.id                 # the atomics body never runs in deterministic mode
        if c.kind in ('pool', 'cat'):
            assert all(v % 2 == 0 for v in c.shape), c.id
        if c.kind == 'flat':
            assert int(np.prod(c.shape)) % c.B == 0, c.id
    for kind, (red, g256, bodies, counts) in REGIMES.items():
        rows = _cases(kind)
        assert red <= {c.red for c in rows}, kind
        assert g256 <= {c.g256 for c in rows}, kind
        assert bodies <= {(c.body, c.lds) for c in rows}, kind
        assert counts <= {c.C for c in rows}, kind
    for kind in ('flat', 'pool'):
        clamped = [c for c in _cases(kind) if c.red == 'clamped_ragged']
        assert any(_launch(c)['stride_off'] and c.body == 'atomics' for c in clamped), kind
        assert any(c.body == 'fixed' and c.det for c in clamped), kind
    for kind in ('pool', 'cat'):     # an axis swap in the index decode needs three distinct extents to show
        assert any(len(set(c.shape)) == 3 for c in _cases(kind)), kind
    assert BY_ID['flat_c4_one_wg'].shape == (2, 2, 2) and BY_ID['pool_c4_one_wg'].shape == (2, 2, 2)
    for body in ('fixed', 'atomics'):    # the dropout kernels' sample index: three samples, both bodies
        assert any(c.B == 3 and c.body == body for c in _cases('flat')), body
    assert [c.shape[0] for c in _cases('adam')] == [1, 1000, GRID_256 * 256 + 77]
    assert _launch(BY_ID['stats_offset50'])['body'] == 'fixed'


# ---- measuring ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    torch.manual_seed(0)
    return torch


class _Checks:
    """collects the measured pairs of a row, prints each, and fails at the end with every figure that missed its bound"""

    def __init__(self, rid, dtype):
        self.id, self.bf16, self.bad = '%s-%s' % (rid, dtype), dtype == 'bf16', []

    def elem(self, y, r64, r32, what, exact_dtype=False):
        """an element-wise output: d <= 6 o + 2e-5 of the reference rms; bf16 outputs (unless exact_dtype: float32 results of a
        bf16 row) get one bf16 ulp of the reference on top"""
        yd = y.detach().double().cpu().reshape(r64.shape)
        scale = max(float(r64.pow(2).mean().sqrt()), 1e-300)
        o = float((r32.double() - r64).abs().max()) / scale
        err = (yd - r64).abs()
        rms = float(err.pow(2).mean().sqrt()) / scale
        if self.bf16 and not exact_dtype:
            err = err - BF16_ULP * r64.abs()
        d = float(err.max()) / scale
        print('%-34s %-34s d %.3g o %.3g rms %.3g of the reference rms%s' % (self.id, what, d, o, rms, ' (beyond one bf16 ulp)'
                                                                               if self.bf16 and not exact_dtype else ''))
        if not d <= GRAD_K * o + MAX_BOUND:
            self.bad.append((what, d, o))

    def sums(self, got, r64, r32, what, groups=1):
        """per-channel sums or moments, `groups` vectors of C laid end to end: per group d <= 6 o + 1e-6 of its largest value"""
        gd = got.detach().double().cpu().reshape(groups, -1)
        for i, (g, a, b) in enumerate(zip(gd, r64.reshape(groups, -1), r32.double().reshape(groups, -1))):
            top = max(float(a.abs().max()), 1e-300)
            d, o = float((g - a).abs().max()) / top, float((b - a).abs().max()) / top
            print('%-34s %-34s d %.3g o %.3g of the largest' % (self.id, '%s [%d]' % (what, i), d, o))
            if not d <= GRAD_K * o + STATS_BOUND:
                self.bad.append(('%s [%d]' % (what, i), d, o))

    def same(self, a, b, what):
        if not torch.equal(a, b):
            self.bad.append((what, 'differs in %d values' % int((a != b).sum())))

    def done(self):
        assert not self.bad, (self.id, self.bad)


class _Det:
    """`with _Det():` -- deterministic mode on, the previous mode restored afterwards"""

    def __enter__(self):
        from synthsr_amd import ops
        self.prev = ops.set_deterministic(True)

    def __exit__(self, *a):
        from synthsr_amd import ops
        assert ops.deterministic_status() == 1, 'an ordered wait timed out'
        ops.set_deterministic(self.prev)


def _rnd(dtype):
    return (lambda t: t.bfloat16().float()) if dtype == 'bf16' else (lambda t: t)


def _to_dev(dtype):
    dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
    return lambda t: t.cuda().to(dt).contiguous()


def _gen(c):
    return torch.Generator(device='cpu').manual_seed(1000 * sum(c.shape) + (c.C if isinstance(c.C, int) else sum(c.C)))


def _pattern(n):
    """what a `+=` target holds before the call: non-zero everywhere, no two neighbours alike"""
    return ((torch.arange(n) % 7).float() - 3.0) / 4.0 + 0.125


def _moments(x, dt):
    f = x.to(dt).reshape(-1, x.shape[-1])
    return torch.cat([f.mean(0), f.var(0, unbiased=False)])


def _affine(C, g):
    gamma, beta = torch.rand(C, generator=g) + .5, torch.randn(C, generator=g)
    gamma[3] = -0.7         # negative scale: the maximum must be taken AFTER the affine
    beta[1] = -10.0         # every BatchNorm output of channel 1 is negative
    return gamma, beta


def _act_dy(y, act):
    return torch.where(y > 0, torch.ones_like(y), y + 1) if act == 1 else (y > 0).to(y.dtype)


# ---- float64 / float32 formulas (dt = the dtype the formula is evaluated in; operands are what the kernel receives) -------------
def _bn_apply_ref(dt, x, stats, gamma, beta):
    C = x.shape[-1]
    sc = torch.rsqrt(stats[C:].to(dt) + EPS) * gamma.to(dt)
    return x.to(dt) * sc + (beta.to(dt) - stats[:C].to(dt) * sc)


def _xhat(dt, a, stats):
    C = a.shape[-1]
    return (a - stats[:C].to(dt)) * torch.rsqrt(stats[C:].to(dt) + EPS)


def _bn_back(dt, g, a, stats, gamma, sums):
    """gamma invstd (g - sum_dy / n - xhat sum_dyxhat / n), n = the voxels of a"""
    C = a.shape[-1]
    n = a.numel() // C
    inv = torch.rsqrt(stats[C:].to(dt) + EPS)
    return gamma.to(dt) * inv * (g - sums[:C].to(dt) / n - _xhat(dt, a, stats) * sums[C:].to(dt) / n)


def _bn_sums_ref(dt, dy, x, stats):
    g = dy.to(dt).reshape(-1, x.shape[-1])
    return torch.cat([g.sum(0), (g * _xhat(dt, x.to(dt).reshape(g.shape), stats)).sum(0)])


def _act_bwd_ref(dt, y, dy=None, dy2=None, bn=None, head=None, drop=None, act=1):
    """csrc/unet_pointwise.hip elu_bwd_kernel on [nvox][C] operands: -> (dz, sum over voxels of dz)"""
    yv = y.to(dt)
    g = dy.to(dt) if head is None else head[0].to(dt).reshape(-1, 1) * head[1].to(dt)
    sd = None if drop is None else drop.to(dt).repeat_interleave(yv.shape[0] // drop.shape[0], 0)
    if bn is not None:
        g = _bn_back(dt, g, yv if sd is None else yv * sd, *bn)
    if sd is not None:
        g = g * sd
    if dy2 is not None:
        g = g + dy2.to(dt)
    dz = g * _act_dy(yv, act)
    return dz, dz.sum(0)


# ---- [nvox][C] kernels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid,dtype', _params('flat'))
def test_flat_kernels_vs_float64(T, cid, dtype):
    """bn_stats (dirty scratch, sentinel-filled stats), bn_apply, scale_channels (in place = out of place), bn_reduce_bwd, bn_bwd,
    and the activation backward in every group: plain, BatchNorm, rank-1 head, per-sample dropout (plain, bn=, bn= + head=), act 1
    and 3, with and without dy2 / dbias; `sums` and `dbias` start from a pattern and come back as pattern + sum; fixed rows run
    every reduction twice more in deterministic mode, bit-identical"""
    from synthsr_amd import ops
    from oracle import unet_ref as U
    c, k, rnd, dev = BY_ID[cid], _Checks(cid, dtype), _rnd(dtype), _to_dev(dtype)
    g = _gen(c)
    C, B, nvox = c.C, c.B, int(np.prod(c.shape))
    rn = lambda *s: torch.randn(*s, generator=g)
    x = rnd(rn(nvox, C) * 2 + 0.5)
    y = rnd(torch.nn.functional.elu(rn(nvox, C)))
    dy, dy2 = rnd(rn(nvox, C) + 0.3), rnd(rn(nvox, C))
    gamma, beta = _affine(C, g)
    rate = 0.25
    drop = (torch.rand(B, C, generator=g) >= rate).float() / (1 - rate)
    drop[0, 0], drop[B - 1, 2] = 0.0, 1 / (1 - rate)
    assert set(drop.unique().tolist()) == {0.0, float(np.float32(1 / (1 - rate)))}
    dpred, whead = rn(nvox), rn(C)
    st_x, st_y = _moments(x, torch.float64).float(), _moments(y, torch.float64).float()
    sums_y = _bn_sums_ref(torch.float64, dy, y, st_y).float()      # an operand like any other
    pat, pat2 = _pattern(C), _pattern(2 * C)
    f64, f32 = torch.float64, torch.float32
    full = lambda t: dev(t).view(*c.shape, C)
    xd, yd, dyd, dy2d = full(x), full(y), full(dy), full(dy2)
    cu = lambda t: t.cuda().contiguous()
    gam, bet, dropd, dpredd, wheadd, st_xd, st_yd, sums_yd = (cu(t) for t in (gamma, beta, drop, dpred, whead, st_x, st_y, sums_y))

    def twice(call, what):      # a reduction in deterministic mode: two runs, bit-identical, each result returned for its bound
        if not c.det:
            return []
        with _Det():
            a, b = call(), call()
        for u, v in zip(a, b):
            k.same(u, v, what + ' (deterministic, second run)')
        return [a]

    # BatchNorm statistics: `stats` is overwritten, `ws` arrives dirty
    def stats_call():
        stats = torch.full((2 * C,), 7.25, device='cuda')
        ws = torch.full((2 * C,), 1e6, dtype=torch.float64, device='cuda')
        return (ops.bn_stats(xd, stats, ws),)
    m32 = torch.cat(U.batchnorm_train(x, gamma, beta)[1:])
    for (stats,) in [stats_call()] + twice(stats_call, 'bn_stats'):
        k.sums(stats, _moments(x, f64), m32, 'bn_stats mean | var', 2)
    k.elem(ops.bn_apply(xd, st_xd, gam, bet), _bn_apply_ref(f64, x, st_x, gamma, beta), _bn_apply_ref(f32, x, st_x, gamma, beta),
           'bn_apply')
    sc = lambda dt: x.to(dt) * drop.to(dt).repeat_interleave(nvox // B, 0)
    out = ops.scale_channels(xd, dropd)
    k.elem(out, sc(f64), sc(f32), 'scale_channels')
    inplace = xd.clone()
    ops.scale_channels(inplace, dropd, out=inplace)
    k.same(inplace, out, 'scale_channels in place')

    # BatchNorm backward: sums += [sum dy, sum dy xhat], then dx
    def reduce_call():
        return (ops.bn_reduce_bwd(dyd, xd, st_xd, pat2.cuda()),)
    s64, s32 = pat2.double() + _bn_sums_ref(f64, dy, x, st_x), pat2 + _bn_sums_ref(f32, dy, x, st_x)
    for (s,) in [reduce_call()] + twice(reduce_call, 'bn_reduce_bwd'):
        k.sums(s, s64, s32, 'bn_reduce_bwd pattern + sums', 2)
    if dtype == 'f32':       # synthsr_bn_bwd_apply has no bf16 twin
        s = pat2.cuda()
        dx = ops.bn_bwd(dyd, xd, st_xd, gam, s)
        k.sums(s, s64, s32, 'bn_bwd pattern + sums', 2)
        sh = s.cpu()         # the apply pass reads the sums the reduce pass left: its operand
        k.elem(dx, _bn_back(f64, dy.double(), x.double(), st_x, gamma, sh), _bn_back(f32, dy, x, st_x, gamma, sh), 'bn_bwd dx')

    # the activation backward, group by group
    bn, bnd = (st_y, gamma, sums_y), (st_yd, gam, sums_yd)
    variants = [
        ('elu_bwd dy2 dbias', lambda db: ops.elu_bwd(dyd, yd, dy2=dy2d, dbias=db), dict(dy=dy, dy2=dy2), True),
        ('elu_bwd act 3', lambda db: ops.elu_bwd(dyd, yd, act=3), dict(dy=dy, act=3), False),
        ('bn_elu_bwd dy2 dbias', lambda db: ops.bn_elu_bwd(dyd, yd, *bnd, dy2=dy2d, dbias=db), dict(dy=dy, dy2=dy2, bn=bn), True),
        ('bn_elu_bwd act 3 dbias', lambda db: ops.bn_elu_bwd(dyd, yd, *bnd, dbias=db, act=3), dict(dy=dy, bn=bn, act=3), True),
        ('bn_elu_bwd', lambda db: ops.bn_elu_bwd(dyd, yd, *bnd), dict(dy=dy, bn=bn), False),
        ('bn_elu_bwd_head dbias', lambda db: ops.bn_elu_bwd_head(dpredd, wheadd, yd, *bnd, dbias=db),
         dict(bn=bn, head=(dpred, whead)), True),
        ('elu_bwd_drop dy2 dbias', lambda db: ops.elu_bwd_drop(dyd, yd, dropd, dy2=dy2d, dbias=db), dict(dy=dy, dy2=dy2, drop=drop),
         True),
        ('elu_bwd_drop bn dy2 dbias', lambda db: ops.elu_bwd_drop(dyd, yd, dropd, dy2=dy2d, dbias=db, bn=bnd),
         dict(dy=dy, dy2=dy2, drop=drop, bn=bn), True),
        ('elu_bwd_drop bn head dbias', lambda db: ops.elu_bwd_drop(None, yd, dropd, dbias=db, bn=bnd, head=(dpredd, wheadd)),
         dict(drop=drop, bn=bn, head=(dpred, whead)), True),
    ]
    got = {}
    for what, call, kw, with_dbias in variants:
        (z64, b64), (z32, b32) = _act_bwd_ref(f64, y, **kw), _act_bwd_ref(f32, y, **kw)

        def run():
            db = pat.cuda() if with_dbias else None
            return (call(db),) + ((db,) if with_dbias else ())
        runs = [run()] + (twice(run, what) if with_dbias else [])
        got[what] = runs[0][0]
        k.elem(runs[0][0], z64, z32, what)
        for r in runs:
            k.same(r[0], runs[0][0], what + ' (dz in deterministic mode)')
            if with_dbias:
                k.sums(r[1], pat.double() + b64, pat + b32, what + ': pattern + dbias')
    if dtype == 'f32':      # the rank-1 gradient is one fp32 product per element: materialised the same way it gives the same bits
        prod = (dpredd.reshape(-1, 1) * wheadd).view(*c.shape, C)
        k.same(got['bn_elu_bwd_head dbias'], ops.bn_elu_bwd(prod, yd, *bnd), 'bn_elu_bwd_head vs bn_elu_bwd on dpred x whead')
    k.done()


# ---- pooled kernels ----------------------------------------------------------------------------------------------------------------
def _pool_input(c, g, rnd, gamma):
    """values (8 q + j) / 512 with j a permutation of 0 .. 7 inside every 2 x 2 x 2 window: no two of a window's values are closer than
    1 / 512 unless the row's rounding makes them EQUAL (bf16), so the top two BatchNorm outputs of a window are either bit-equal or
    thousands of ulp apart; in (-0.875, 3.1) like an ELU output.  Then exact ties are planted: in the first, a middle and the last
    window of channels 0, 2 and 3 the positions 2 and 5 (raster order) both get the value that wins the window after the affine."""
    C = c.C
    nw = int(np.prod(c.shape)) // 8 * C
    q = torch.randint(-56, 200, (nw, 8), generator=g)
    j = torch.rand(nw, 8, generator=g).argsort(1)
    W = rnd((8 * q + j).float() / 512.0)
    planted = []
    for w in sorted({0, nw // C // 2, nw // C - 1}):
        for ch in (0, 2, 3):
            W[w * C + ch, 2] = W[w * C + ch, 5] = 3.5 if gamma[ch] > 0 else -0.9375
            planted.append(w * C + ch)
    return _unwindows(W, c.shape + (C,)).contiguous(), torch.tensor(planted)


def _assert_unambiguous(x, stats, gamma, beta, planted):
    """on the host: outside exact ties (equal inputs, hence bit-equal outputs) no window's top two fp32 BatchNorm outputs lie within
    4 ulp, so the float64 arg-max is the only right answer; the planted windows are exact ties at positions 2 and 5"""
    t = _windows(_bn_apply_ref(torch.float32, x, stats, gamma, beta))
    top, idx = t.topk(2, dim=1)
    gap = top[:, 0] - top[:, 1]
    near = gap <= 4 * torch.finfo(torch.float32).eps * top[:, 0].abs()
    xs = _windows(x).gather(1, idx)
    assert bool(((gap == 0) & (xs[:, 0] == xs[:, 1]))[near].all()), 'a window with two distinct inputs within 4 ulp after the affine'
    assert bool((gap[planted] == 0).all()) and set(idx[planted].reshape(-1).tolist()) == {2, 5}
    return int(near.sum())


def _pool_refs(dt, x, stats, gamma, beta, dpool):
    """-> (pooled, routed gradient, [sum routed, sum routed xhat]) with the FIRST maximum of a window in raster order"""
    C = x.shape[-1]
    t = _windows(_bn_apply_ref(dt, x, stats, gamma, beta))
    idx = t.argmax(1)                      # the first of equal maxima
    rows = torch.arange(t.shape[0])
    g = dpool.to(dt).reshape(-1)
    routed = torch.zeros_like(t)
    routed[rows, idx] = g
    xa = _windows(x.to(dt))[rows, idx].reshape(-1, C)
    gx = g.reshape(-1, C) * _xhat(dt, xa, stats)
    pooled = t[rows, idx].reshape(x.shape[0] // 2, x.shape[1] // 2, x.shape[2] // 2, C)
    return pooled, _unwindows(routed, x.shape), torch.cat([g.reshape(-1, C).sum(0), gx.sum(0)])


@pytest.mark.parametrize('cid,dtype', _params('pool'))
def test_pooled_kernels_vs_float64(T, cid, dtype):
    """bn_maxpool, bn_maxpool_bwd (plain, with sums, sums only) and bn_pool_elu_bwd (act 1 and 3, with and without dy2 / dbias):
    negative gamma, an all-negative channel, planted exact ties routed to the first maximum; the three arg-max kernels agree on
    every window; bn_pool_elu_bwd is bit-identical to bn_maxpool_bwd + bn_elu_bwd on the same sums"""
    from synthsr_amd import ops
    c, k, rnd, dev = BY_ID[cid], _Checks(cid, dtype), _rnd(dtype), _to_dev(dtype)
    g = _gen(c)
    C = c.C
    pshape = tuple(v // 2 for v in c.shape) + (C,)
    f64, f32 = torch.float64, torch.float32
    gamma, beta = _affine(C, g)
    x, planted = _pool_input(c, g, rnd, gamma)
    stats = _moments(x, f64).float()
    ties = _assert_unambiguous(x, stats, gamma, beta, planted)
    print('%-34s %d of %d windows hold an exact tie (%d planted)' % (k.id, ties, x.numel() // 8, planted.numel()))
    dpool = rnd(torch.randn(*pshape, generator=g) + 0.3)
    cu = lambda t: t.cuda().contiguous()
    xd, dpoold, std, gam, bet = dev(x), dev(dpool), cu(stats), cu(gamma), cu(beta)
    p64, r64, s64 = _pool_refs(f64, x, stats, gamma, beta, dpool)
    if c.red == '-':         # the 137 MB row: the routed gradient is a selection, exact in any precision (o = 0); the maximum in fp32
        p32, r32 = _windows(_bn_apply_ref(f32, x, stats, gamma, beta)).amax(1).reshape(p64.shape), r64
    else:
        p32, r32, s32 = _pool_refs(f32, x, stats, gamma, beta, dpool)
    k.elem(ops.bn_maxpool(xd, std, gam, bet), p64, p32, 'bn_maxpool')
    dbn = ops.bn_maxpool_bwd(dpoold, xd, std, gam, bet)
    k.elem(dbn, r64, r32, 'bn_maxpool_bwd')
    assert torch.equal((dbn != 0).cpu(), r64 != 0), 'the gradient is not routed to the first maximum of every window'
    if c.red == '-':         # the 137 MB row: the 256-thread kernels only
        return k.done()
    pat, pat2 = _pattern(C), _pattern(2 * C)
    dy2 = rnd(torch.randn(*c.shape, C, generator=g))
    dy2d = dev(dy2)

    def twice(call, what):
        if not c.det:
            return []
        with _Det():
            a, b = call(), call()
        for u, v in zip(a, b):
            k.same(u, v, what + ' (deterministic, second run)')
        return [a]

    def with_sums():
        s = pat2.cuda()
        return ops.bn_maxpool_bwd(dpoold, xd, std, gam, bet, sums=s), s

    def sums_only():
        s = pat2.cuda()
        assert ops.bn_maxpool_bwd(dpoold, xd, std, gam, bet, out=False, sums=s) is None
        return (s,)
    for out, s in [with_sums()] + twice(with_sums, 'bn_maxpool_bwd sums='):
        k.same(out, dbn, 'bn_maxpool_bwd with sums: the same dbn as without')
        k.sums(s, pat2.double() + s64, pat2 + s32, 'bn_maxpool_bwd sums=: pattern + sums', 2)
    for (s,) in [sums_only()] + twice(sums_only, 'bn_maxpool_bwd out=False'):
        k.sums(s, pat2.double() + s64, pat2 + s32, 'bn_maxpool_bwd out=False: pattern + sums', 2)
    # the one-pass backward: against float64, and bit for bit against the two passes it replaces, on the same sums
    S = s64.float()
    Sd = cu(S)
    flat = lambda t: t.reshape(-1, C)
    for what, act, d2, with_dbias in (('act 1 dy2 dbias', 1, True, True), ('act 3 dy2 dbias', 3, True, True), ('act 1', 1, False, False)):
        def ref(dt, routed):
            gg = _bn_back(dt, flat(routed), flat(x.to(dt)), stats, gamma, S)
            dz = (gg + flat(dy2.to(dt)) if d2 else gg) * _act_dy(flat(x.to(dt)), act)
            return dz, dz.sum(0)
        (z64, b64), (z32, b32) = ref(f64, r64), ref(f32, r32)

        def one_pass():
            db = pat.cuda() if with_dbias else None
            return (ops.bn_pool_elu_bwd(dpoold, xd, std, gam, bet, Sd, dy2=dy2d if d2 else None, dbias=db, act=act),) + \
                ((db,) if with_dbias else ())
        runs = [one_pass()] + (twice(one_pass, 'bn_pool_elu_bwd ' + what) if with_dbias else [])
        k.elem(runs[0][0], z64, z32, 'bn_pool_elu_bwd ' + what)
        db2 = pat.cuda() if with_dbias else None
        two = ops.bn_elu_bwd(dbn, xd, std, gam, Sd, dy2=dy2d if d2 else None, dbias=db2, act=act)
        for r in runs:
            k.same(r[0], two, 'bn_pool_elu_bwd %s vs bn_maxpool_bwd + bn_elu_bwd' % what)
            if with_dbias:
                k.sums(r[1], pat.double() + b64, pat + b32, 'bn_pool_elu_bwd %s: pattern + dbias' % what)
    k.done()


# ---- upsample + concat --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid,dtype', _params('cat'))
def test_upsample_concat_vs_float64(T, cid, dtype):
    """out = [skip | upsample2(BN(lo))] and its backward (dskip a copy, dlo the sum over each 2 x 2 x 2 block)"""
    from synthsr_amd import ops
    from oracle import unet_ref as U
    c, k, rnd, dev = BY_ID[cid], _Checks(cid, dtype), _rnd(dtype), _to_dev(dtype)
    g = _gen(c)
    Cs, Cl = c.C
    lshape = tuple(v // 2 for v in c.shape)
    skip = rnd(torch.randn(*c.shape, Cs, generator=g))
    lo = rnd(torch.randn(*lshape, Cl, generator=g) * 2 + 0.5)
    dcat = rnd(torch.randn(*c.shape, Cs + Cl, generator=g))
    gamma, beta = _affine(Cl, g)
    stats = _moments(lo, torch.float64).float()
    cu = lambda t: t.cuda().contiguous()
    fwd = lambda dt: torch.cat([skip.to(dt), U.upsample2(_bn_apply_ref(dt, lo, stats, gamma, beta))], -1)
    k.elem(ops.upsample_concat(dev(skip), dev(lo), cu(stats), cu(gamma), cu(beta)), fwd(torch.float64), fwd(torch.float32),
           'upsample_concat')
    dskip, dlo = ops.upsample_concat_bwd(dev(dcat), Cs, Cl)
    k.same(dskip.cpu().float(), dcat[..., :Cs].contiguous(), 'upsample_concat_bwd dskip')
    back = lambda dt: dcat[..., Cs:].to(dt).reshape(lshape[0], 2, lshape[1], 2, lshape[2], 2, Cl).sum((1, 3, 5))
    k.elem(dlo, back(torch.float64), back(torch.float32), 'upsample_concat_bwd dlo')
    k.done()


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid,dtype', _params('adam'))
def test_adam_step_vs_float64(T, cid, dtype):
    """Keras 2.3.1 Adam as in adam_kernel, grad_scale != 1; where g = m = v = 0 the update is exactly 0, not NaN"""
    from synthsr_amd import ops
    c, k = BY_ID[cid], _Checks(cid, dtype)
    g = _gen(c)
    n = c.shape[0]
    p, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    v = torch.rand(n, generator=g) * 1e-2
    zero = torch.arange(0, n, 97)[1:] if n > 1 else torch.arange(0)      # n = 1 keeps its one live value
    zero = torch.cat([zero, torch.tensor([n - 1])]) if n > 1 else zero
    gr[zero], m[zero], v[zero] = 0.0, 0.0, 0.0
    lr, b1, b2, eps, gs = (float(np.float32(a)) for a in (1.3e-3, 0.9, 0.999, 1e-7, 0.37))

    def ref(dt):
        gi = gr.to(dt) * gs
        mi = b1 * m.to(dt) + (1 - b1) * gi
        vi = b2 * v.to(dt) + (1 - b2) * gi * gi
        return p.to(dt) - lr * mi / (vi.sqrt() + eps), mi, vi
    pd, gd, md, vd = (t.cuda() for t in (p, gr, m, v))
    ops.adam_step(pd, gd, md, vd, lr, b1, b2, eps, grad_scale=gs)
    for what, got, r64, r32 in zip(('p', 'm', 'v'), (pd, md, vd), ref(torch.float64), ref(torch.float32)):
        k.elem(got, r64, r32, 'adam ' + what)
    k.same(gd.cpu(), gr, 'adam leaves g alone')
    if n > 1:
        k.same(pd.cpu()[zero], p[zero], 'adam p where g = m = v = 0')
        k.same(md.cpu()[zero], torch.zeros(zero.numel()), 'adam m where g = m = v = 0')
        k.same(vd.cpu()[zero], torch.zeros(zero.numel()), 'adam v where g = m = v = 0')
    k.done()


# ---- statistics of an offset-dominated tensor ---------------------------------------------------------------------------------------
def test_bn_stats_of_an_offset_dominated_tensor(T):
    """mean 50, standard deviation 1: E[x^2] - m^2 cancels 2500 against 2501.  The kernel keeps fp32 per-thread partials of x and
    x^2, shifted by the mean of the channel's first values, and adds workgroups in float64; held to 6 o + 1e-6 of the largest moment
    like every other statistic.  Measured: variance d 1.52e-07, o 3.60e-08 (mean d 3.73e-08, o 1.27e-07); unshifted it was 7.26e-04"""
    from synthsr_amd import ops
    from oracle import unet_ref as U
    c = BY_ID['stats_offset50']
    k = _Checks(c.id, 'f32')
    g = _gen(c)
    x = torch.randn(*c.shape, c.C, generator=g) + OFFSET
    stats = torch.full((2 * c.C,), 7.25, device='cuda')
    ws = torch.full((2 * c.C,), 1e6, dtype=torch.float64, device='cuda')
    ops.bn_stats(x.cuda(), stats, ws)
    k.sums(stats, _moments(x, torch.float64), torch.cat(U.batchnorm_train(x, torch.ones(c.C), torch.zeros(c.C))[1:]),
           'bn_stats mean | var, offset %g' % OFFSET, 2)
    k.done()


# ---- refusals leave every output alone ------------------------------------------------------------------------------------------------
def test_refused_pointwise_calls_return_einval_and_write_nothing():
    """the C entry points directly: a channel count that is no multiple of 4 or beyond 4096, no voxels, an odd extent, an activation
    code other than 1 / 3, an incomplete or contradictory group of optional arguments -- each returns SYNTHSR_EINVAL (-1) before
    anything is queued: every buffer keeps every bit of its sentinel pattern"""
    from synthsr_amd import _lib
    lib, P, S, i3 = _lib.load(), _lib.ptr, _lib.stream, _lib.i3
    n = 8 * 4100
    make = lambda dt: (torch.arange(n, device='cuda') % 251 + 1).to(dt)
    buf = {nm: make(torch.float32) for nm in ('a', 'b', 'c', 'out', 'out2', 'dbias', 'stats', 'sums', 'gamma', 'beta', 'drop', 'dpred',
                                              'whead')}
    buf['ws'] = make(torch.float64)
    keep = {nm: t.clone() for nm, t in buf.items()}
    a, b, c3, out, out2, dbias, stats, sums, gamma, beta, drop, dpred, whead, ws = (
        P(buf[nm]) for nm in ('a', 'b', 'c', 'out', 'out2', 'dbias', 'stats', 'sums', 'gamma', 'beta', 'drop', 'dpred', 'whead', 'ws'))
    e, st = EPS, S()
    ok_shape = (2, 2, 2)

    def flat(nvox, C, act=1):        # every (nvox, C) entry point, otherwise well-formed
        return [
            ('act_bwd', lambda: lib.synthsr_act_bwd(a, b, c3, out, dbias, nvox, C, act, st)),
            ('bn_act_bwd', lambda: lib.synthsr_bn_act_bwd(a, b, c3, out, dbias, nvox, C, stats, gamma, e, sums, act, st)),
            ('bn_act_bwd_head', lambda: lib.synthsr_bn_act_bwd_head(dpred, whead, c3, out, dbias, nvox, C, stats, gamma, e, sums, act, st)),
            ('act_bwd_drop', lambda: lib.synthsr_act_bwd_drop(a, b, c3, out, dbias, nvox, C, stats, gamma, e, sums, None, None, drop,
                                                              max(nvox, 1), act, st)),
            ('bn_stats', lambda: lib.synthsr_bn_stats(a, nvox, C, stats, ws, st)),
            ('bn_apply', lambda: lib.synthsr_bn_apply(a, out, nvox, C, stats, gamma, beta, e, st)),
            ('bn_bwd_reduce', lambda: lib.synthsr_bn_bwd_reduce(a, b, nvox, C, stats, e, sums, st)),
            ('bn_bwd_apply', lambda: lib.synthsr_bn_bwd_apply(a, b, out, nvox, C, stats, gamma, e, sums, st)),
            ('scale_channels', lambda: lib.synthsr_scale_channels(a, out, nvox, C, drop, max(nvox, 1), st)),
        ]

    def shaped(shape, C, Cl=8, act=1):      # every entry point that takes a shape
        s = i3(shape)
        return [
            ('bn_maxpool', lambda: lib.synthsr_bn_maxpool(a, out, s, C, stats, gamma, beta, e, st)),
            ('bn_maxpool_bwd', lambda: lib.synthsr_bn_maxpool_bwd(a, b, out, s, C, stats, gamma, beta, e, st)),
            ('bn_maxpool_bwd_ex', lambda: lib.synthsr_bn_maxpool_bwd_ex(a, b, out, s, C, stats, gamma, beta, e, sums, st)),
            ('bn_pool_act_bwd', lambda: lib.synthsr_bn_pool_act_bwd(a, b, c3, out, dbias, s, C, stats, gamma, beta, sums, e, act, st)),
            ('upsample_concat', lambda: lib.synthsr_upsample_concat(a, b, out, s, C, Cl, stats, gamma, beta, e, st)),
            ('upsample_concat_bwd', lambda: lib.synthsr_upsample_concat_bwd(a, out, out2, s, C, Cl, st)),
        ]

    calls = []
    for C in (6, 4100):
        calls += [('C = %d: %s' % (C, nm), f) for nm, f in flat(8, C) + shaped(ok_shape, C)]
        calls += [('Cl = %d: %s' % (C, nm), f) for nm, f in shaped(ok_shape, 8, Cl=C)[-2:]]
    calls += [('nvox = 0: ' + nm, f) for nm, f in flat(0, 8) + shaped((0, 2, 2), 8)]
    for shape in ((3, 2, 2), (2, 3, 2), (2, 2, 3)):
        calls += [('shape %r: %s' % (shape, nm), f) for nm, f in shaped(shape, 8)]
    for act in (0, 2):
        calls += [('act %d: %s' % (act, nm), f) for nm, f in flat(8, 8, act)[:4] + shaped(ok_shape, 8, act=act)[3:4]]
    calls += [
        ('BatchNorm group without sums: bn_act_bwd', lambda: lib.synthsr_bn_act_bwd(a, b, c3, out, dbias, 8, 8, stats, gamma, e, None, 1, st)),
        ('BatchNorm group without sums: act_bwd_drop',
         lambda: lib.synthsr_act_bwd_drop(a, b, c3, out, dbias, 8, 8, stats, gamma, e, None, None, None, drop, 8, 1, st)),
        ('head group together with dy',
         lambda: lib.synthsr_act_bwd_drop(a, None, c3, out, dbias, 8, 8, stats, gamma, e, sums, dpred, whead, drop, 8, 1, st)),
        ('head group without BatchNorm',
         lambda: lib.synthsr_act_bwd_drop(None, None, c3, out, dbias, 8, 8, None, None, e, None, dpred, whead, drop, 8, 1, st)),
        ('head group without whead',
         lambda: lib.synthsr_act_bwd_drop(None, None, c3, out, dbias, 8, 8, stats, gamma, e, sums, dpred, None, drop, 8, 1, st)),
        ('drop with nvox % nvox_per_sample != 0: act_bwd_drop',
         lambda: lib.synthsr_act_bwd_drop(a, b, c3, out, dbias, 8, 8, None, None, e, None, None, None, drop, 3, 1, st)),
        ('drop with nvox % nvox_per_sample != 0: scale_channels', lambda: lib.synthsr_scale_channels(a, out, 8, 8, drop, 3, st)),
        ('bn_maxpool_bwd_ex with neither dbn nor sums',
         lambda: lib.synthsr_bn_maxpool_bwd_ex(a, b, None, i3(ok_shape), 8, stats, gamma, beta, e, None, st)),
    ]
    for what, f in calls:
        assert f() == -1, what
    torch.cuda.synchronize()
    for nm, t in buf.items():
        assert torch.equal(t, keep[nm]), 'a refused call wrote to `%s`' % nm
    # the same calls well-formed are served (the refusals above are about the one argument each names)
    for what, f in flat(8, 8) + shaped(ok_shape, 8):
        assert f() == 0, what
    torch.cuda.synchronize()
