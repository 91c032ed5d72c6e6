"""Every forward and data-gradient conv variant on its own against float64.

One table (CASES) reaches every kernel the forward dispatchers know (csrc/conv3d.hip plan_fwd / dispatch_fwd2 / launch_fwd /
parity_split, csrc/conv_split.hip split_fwd_route / launch_split_fwd, csrc/common.h syn_split_plan_mt,
csrc/conv_bf16.hip plan_bf16 and the split-K rule of synthsr_conv3d_bf16_fwd_ex) at the smallest shape its rule admits, ragged in
every axis the rule allows.  Every row states its route; _route restates the dispatcher's rules, the tests assert
_route(c) == c.route and that the restated plan agrees with the library's own answer (synthsr_conv3d_plan) -- the routing half
runs without a GPU in tests/test_conv_variants_cpu.py.

Comparand: a float64 evaluation of the same operation on the host (F.conv3d on .double() operands; folded rows on
repeat_interleave(2, ...) of the low-resolution tensor; bf16 rows on the bf16-rounded operands -- for the bf16 FOLDED rows the
operands are the eight parity kernels, sums of up to eight taps that the pack rounds to bf16 once more (_parity_weights): against
the un-folded rounded taps those two rows measure 0.014 worst / 0.0023 rms of the reference rms, the second rounding of the weights).
Bounds, f32 rows: rms error < 4e-6 and worst element < 2e-5 of the reference's rms (tests/test_split_gpu.py and MAX_BOUND of
tests/test_wgrad_scratch_gpu.py; every row has K <= 27 * 192), statistics to 1e-6 of the largest float64 moment.
bf16 rows: |y - ref| <= 2**-8 |ref| + 2e-5 rms(ref) per element (one bf16 rounding of one fp32 sum), statistics to 1e-6 of the
float64 moments of the stored bf16 values.

Branches the list of the routes names that the public entry points cannot reach (so no row and no refusal can be written):
 * `c2` under a folded mode: plan_fwd sets c2 only for kind 1 (plain); synthsr_conv3d_up_fwd / _up_dgrad plan with kind 2 / 0,
   so dispatch_fwd2's `pl.c2 && ext.mode != 0` refusal is dead code behind the public API;
 * a stacked split layout with MT != 2: plan_fwd stacks only Cout == 24, whose two 16-column tiles always give MT = 2, and
   syn_split_fwd is not exported;
 * split-K under a folded mode (splitk_begin, the prologue launch_fwd and launch_fwd_brick share, returns SYNTHSR_EINVAL before
   it touches the output): plan_fwd gives ksplit > 1 to plain convs only.

Measured on an MI355X (worst element / rms error of the reference rms; forward with bias and the data gradient; bf16 rows include
the one bf16 rounding of the result).  The file takes 12 s there.
  c2_cin1             c2_cin1             fwd 7.01e-07 / 8.72e-08 dgrad 8.12e-07 / 8.5e-08
  c2_cin2             c2_cin2             fwd 1.28e-06 / 1.23e-07 dgrad 1.26e-06 / 1.2e-07
  p4                  p4                  fwd 5.72e-06 / 4.47e-07 dgrad 7.72e-06 / 4.48e-07
  persist_nt1         persist_nt1         fwd 5.15e-06 / 4.49e-07 dgrad 6.1e-06 / 4.51e-07
  persist_nt2_cout20  persist_nt2         fwd 5.64e-06 / 4.43e-07 dgrad 5.5e-06 / 4.52e-07
  persist_nt3         persist_nt3         fwd 6.23e-06 / 4.49e-07 dgrad 6.18e-06 / 4.51e-07
  tile4_ck8           tile4_ck8           fwd 3.58e-06 / 2.61e-07 dgrad 2.96e-06 / 2.64e-07
  tile4_ck24_nt4      tile4_ck24_nt4plus  fwd 6.01e-06 / 4.46e-07 dgrad 5.66e-06 / 4.51e-07
  lean                lean                fwd 3.32e-06 / 4.05e-07 dgrad 4.14e-06 / 4.12e-07
  lean_ks             lean_ks             fwd 4.13e-06 / 5.74e-07 dgrad 4.77e-06 / 5.75e-07
  generic_ck8         generic_ck8         fwd 1.9e-06 / 2.35e-07  dgrad 2.87e-06 / 2.35e-07
  generic_ck8_ks      generic_ck8_ks      fwd 3.26e-06 / 3.79e-07 dgrad 3.08e-06 / 3.85e-07
  generic_ck32        generic_ck32        fwd 5.75e-06 / 4.59e-07 dgrad 4.12e-06 / 4.71e-07
  generic_ck32_ks     generic_ck32_ks     fwd 5.26e-06 / 6.57e-07 dgrad 4.8e-06 / 6.75e-07
  generic_cout18      generic_ck8_cout%4  fwd 2.24e-06 / 2.37e-07 dgrad 1.88e-06 / 2.33e-07
  brick_4x1           brick_4x1           fwd 4.84e-06 / 4.06e-07 dgrad 5.24e-06 / 4.06e-07
  brick_4x1_ks        brick_4x1_ks        fwd 3.59e-06 / 4.04e-07 dgrad 3.85e-06 / 4.08e-07
  brick_2x2           brick_2x2           fwd 4.43e-06 / 4.08e-07 dgrad 4.55e-06 / 4.11e-07
  brick_2x2_ks        brick_2x2_ks        fwd 3.17e-06 / 4.06e-07 dgrad 3.79e-06 / 4.1e-07
  brick_2x1           brick_2x1           fwd 4.53e-06 / 4.2e-07  dgrad 4.79e-06 / 4.25e-07
  brick_2x1_ks        brick_2x1_ks        fwd 3.84e-06 / 4.28e-07 dgrad 3.73e-06 / 4.31e-07
  up_p4               up_p4               fwd 3.78e-06 / 2.36e-07 dgrad -
  up_lean8            up_lean8            fwd 2.65e-06 / 2.23e-07 dgrad -
  up_generic8         up_generic8         fwd 1.09e-06 / 1.33e-07 dgrad -
  updgrad_ps1         updgrad_ps1         fwd -                   dgrad 3.94e-06 / 5.72e-07
  updgrad_ps2         updgrad_ps2         fwd -                   dgrad 3.95e-06 / 4.89e-07
  updgrad_ps4         updgrad_ps4         fwd -                   dgrad 2.51e-06 / 3.47e-07
  updgrad_ps8         updgrad_ps8         fwd -                   dgrad 1.35e-06 / 2.32e-07
  split_stacked       split_stacked       fwd 1.8e-06 / 1.46e-07  dgrad 1.74e-06 / 1.46e-07
  split_fwd2_mt1      split_fwd2_mt1      fwd 2.61e-06 / 2.21e-07 dgrad 2.46e-06 / 2.21e-07
  split_fwd2_mt2      split_fwd2_mt2      fwd 3.12e-06 / 2.2e-07  dgrad 2.84e-06 / 2.19e-07
  split_fwd2_mt3      split_fwd2_mt3      fwd 2.7e-06 / 2.21e-07  dgrad 2.78e-06 / 2.19e-07
  split_fwd2_halves   split_fwd2_halves   fwd 3.16e-06 / 3.12e-07 dgrad 3.15e-06 / 3.12e-07
  split_fwd3          split_fwd3          fwd 3.06e-06 / 2.22e-07 dgrad 3.44e-06 / 2.22e-07
  split_replanned     split_replanned     fwd 3.19e-06 / 2.23e-07 dgrad 2.99e-06 / 2.22e-07
  split_updgrad       split_updgrad       fwd -                   dgrad 3.95e-06 / 3.43e-07
  split_upfwd_mt1     split_upfwd_mt1     fwd 1.66e-06 / 1.07e-07 dgrad -
  split_upfwd_mt2     split_upfwd_mt2     fwd 1.6e-06 / 1.04e-07  dgrad -
  split_upfwd_mt3     split_upfwd_mt3     fwd 1.5e-06 / 1.03e-07  dgrad -
  split9_generic      split9_generic      fwd 2.79e-06 / 2.19e-07 dgrad 2.34e-06 / 2.2e-07
  split9_upfwd        split9_upfwd        fwd 1.66e-06 / 1.07e-07 dgrad -
  bf16_ck8_mt1        bf16_ck8_mt1        fwd 0.00897 / 0.00168   dgrad 0.00891 / 0.00167
  bf16_ck24_mt2       bf16_ck24_mt2       fwd 0.00891 / 0.00165   dgrad 0.011 / 0.00165
  bf16_ck32_mt3       bf16_ck32_mt3       fwd 0.00901 / 0.00164   dgrad 0.00917 / 0.00166
  bf16_ck8_mt4        bf16_ck8_mt4        fwd 0.0116 / 0.00165    dgrad 0.00914 / 0.00165
  bf16_ks             bf16_ck24_mt2_ks    fwd 0.00877 / 0.00161   dgrad 0.00889 / 0.00167
  bf16_up_fwd         bf16_up_fwd         fwd 0.014 / 0.00166     dgrad -
  bf16_up_dgrad       bf16_up_dgrad       fwd -                   dgrad 0.0125 / 0.0017"""
import collections
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RMS_BOUND, MAX_BOUND, STATS_BOUND = 4e-6, 2e-5, 1e-6
BF16_ULP = 2.0 ** -8

Case = collections.namedtuple('Case', 'id entry arith dtype shape cin cout det route')
#   entry: 'plain' ops.conv3d / conv3d_add / conv3d_stats (Cin -> Cout on `shape`)
#          'up_fwd' ops.conv3d_up, 'up_dgrad' ops.conv3d_up_dgrad: shape = the LOW-RES grid, cin = Cl (low-res channels), cout = the
#          layer's output channels (the data gradient's effective conv runs Cout -> Cl)
#   det:   deterministic mode on (no split-K, no parity split; the row runs twice and must be bit-identical)


def _c(id, entry, arith, dtype, shape, cin, cout, route, det=True):
    return Case(id, entry, arith, dtype, tuple(shape), cin, cout, det, route)


T768 = (61, 47, 53)      # 16 x 12 x 4 = 768 tiles of 4 x 4 x 16: the smallest count at which plan_fwd takes the 4-row kernels
T200 = (18, 19, 113)     # 5 x 5 x 8 = 200 tiles: PLAN_SPLIT_MIN_WGS with one co-chunk
CASES = [
    # ---- fp32 matrix instructions, plain 27-tap conv
    _c('c2_cin1', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 1, 24, 'c2_cin1'),
    _c('c2_cin2', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 2, 24, 'c2_cin2'),
    _c('c2_cin2_below_tile', 'plain', 'fp32_mfma', 'f32', (3, 5, 7), 2, 24, 'c2_cin2'),   # z and x extents below the 4 x 4 x 16 tile
    _c('p4', 'plain', 'fp32_mfma', 'f32', T768, 24, 24, 'p4'),
    _c('persist_nt1', 'plain', 'fp32_mfma', 'f32', T768, 24, 16, 'persist_nt1'),
    _c('persist_nt2_cout20', 'plain', 'fp32_mfma', 'f32', T768, 24, 20, 'persist_nt2'),
    _c('persist_nt3', 'plain', 'fp32_mfma', 'f32', T768, 24, 48, 'persist_nt3'),
    _c('tile4_ck8', 'plain', 'fp32_mfma', 'f32', T768, 8, 16, 'tile4_ck8'),
    _c('tile4_ck24_nt4', 'plain', 'fp32_mfma', 'f32', T768, 24, 64, 'tile4_ck24_nt4plus'),
    _c('lean', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 24, 48, 'lean'),
    _c('lean_ks', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 96, 48, 'lean_ks', det=False),
    _c('generic_ck8', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 8, 16, 'generic_ck8'),
    _c('generic_ck8_ks', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 40, 40, 'generic_ck8_ks', det=False),
    _c('generic_ck32', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 32, 48, 'generic_ck32'),
    _c('generic_ck32_ks', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 128, 16, 'generic_ck32_ks', det=False),
    _c('generic_cout18', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 8, 18, 'generic_ck8_cout%4'),
    _c('brick_4x1', 'plain', 'fp32_mfma', 'f32', (8, 4, 20), 24, 128, 'brick_4x1'),
    _c('brick_4x1_ks', 'plain', 'fp32_mfma', 'f32', (8, 4, 20), 48, 128, 'brick_4x1_ks', det=False),
    _c('brick_2x2', 'plain', 'fp32_mfma', 'f32', (4, 16, 12), 24, 64, 'brick_2x2'),
    _c('brick_2x2_ks', 'plain', 'fp32_mfma', 'f32', (4, 16, 12), 48, 64, 'brick_2x2_ks', det=False),
    _c('brick_2x1', 'plain', 'fp32_mfma', 'f32', (8, 12, 20), 24, 64, 'brick_2x1'),
    _c('brick_2x1_ks', 'plain', 'fp32_mfma', 'f32', (8, 12, 20), 48, 64, 'brick_2x1_ks', det=False),
    # ---- fp32 matrix instructions, folded decoder conv (8 parity convs on the low-resolution grid)
    _c('up_p4', 'up_fwd', 'fp32_mfma', 'f32', T768, 24, 24, 'up_p4'),
    _c('up_lean8', 'up_fwd', 'fp32_mfma', 'f32', (3, 5, 7), 24, 48, 'up_lean8'),
    _c('up_generic8', 'up_fwd', 'fp32_mfma', 'f32', (3, 5, 7), 8, 16, 'up_generic8'),
    _c('updgrad_ps1', 'up_dgrad', 'fp32_mfma', 'f32', (3, 5, 7), 24, 24, 'updgrad_ps1'),
    _c('updgrad_ps2', 'up_dgrad', 'fp32_mfma', 'f32', (14, 26, 50), 24, 24, 'updgrad_ps2', det=False),    # 208 workgroups
    _c('updgrad_ps4', 'up_dgrad', 'fp32_mfma', 'f32', (10, 18, 49), 24, 24, 'updgrad_ps4', det=False),    # 108
    _c('updgrad_ps8', 'up_dgrad', 'fp32_mfma', 'f32', (3, 5, 7), 24, 24, 'updgrad_ps8', det=False),       # 3
    # ---- split arithmetic (six products on the bf16 matrix cores)
    _c('split_stacked', 'plain', 'split', 'f32', T200, 8, 24, 'split_stacked'),
    _c('split_fwd2_mt1', 'plain', 'split', 'f32', T200, 8, 16, 'split_fwd2_mt1'),
    _c('split_fwd2_mt2', 'plain', 'split', 'f32', T200, 8, 32, 'split_fwd2_mt2'),
    _c('split_fwd2_mt3', 'plain', 'split', 'f32', T200, 8, 40, 'split_fwd2_mt3'),
    _c('split_fwd2_halves', 'plain', 'split', 'f32', T200, 32, 16, 'split_fwd2_halves'),
    _c('split_fwd3', 'plain', 'split', 'f32', (30, 31, 50), 8, 64, 'split_fwd3'),          # 256 tiles x 2 co-chunks
    _c('split_replanned', 'plain', 'split', 'f32', (30, 31, 66), 8, 96, 'split_replanned'),   # 320 tiles, co-chunks of 32
    _c('split_updgrad', 'up_dgrad', 'split', 'f32', T200, 16, 8, 'split_updgrad'),
    _c('split_upfwd_mt1', 'up_fwd', 'split', 'f32', T200, 8, 16, 'split_upfwd_mt1'),
    _c('split_upfwd_mt2', 'up_fwd', 'split', 'f32', T200, 8, 24, 'split_upfwd_mt2'),
    _c('split_upfwd_mt3', 'up_fwd', 'split', 'f32', T200, 8, 40, 'split_upfwd_mt3'),
    # ---- nine products: the generic split kernel
    _c('split9_generic', 'plain', 'split9', 'f32', T200, 8, 24, 'split9_generic'),
    _c('split9_upfwd', 'up_fwd', 'split9', 'f32', T200, 8, 16, 'split9_upfwd'),
    # ---- bf16 (one input-channel chunk: never split-K; two and more on a small volume: split-K)
    _c('bf16_ck8_mt1', 'plain', 'split', 'bf16', (6, 5, 17), 8, 16, 'bf16_ck8_mt1'),
    _c('bf16_ck24_mt2', 'plain', 'split', 'bf16', (6, 5, 17), 24, 24, 'bf16_ck24_mt2'),
    _c('bf16_ck32_mt3', 'plain', 'split', 'bf16', (6, 5, 17), 32, 40, 'bf16_ck32_mt3'),
    _c('bf16_ck8_mt4', 'plain', 'split', 'bf16', (6, 5, 17), 8, 64, 'bf16_ck8_mt4'),
    _c('bf16_ks', 'plain', 'split', 'bf16', (6, 5, 17), 48, 24, 'bf16_ck24_mt2_ks'),
    _c('bf16_up_fwd', 'up_fwd', 'split', 'bf16', (3, 5, 7), 24, 24, 'bf16_up_fwd'),
    _c('bf16_up_dgrad', 'up_dgrad', 'split', 'bf16', (3, 5, 7), 24, 24, 'bf16_up_dgrad'),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
F32_CASES = [c for c in CASES if c.dtype == 'f32']
BF16_CASES = [c for c in CASES if c.dtype == 'bf16']
_ids = lambda cs: [c.id for c in cs]

# the variants the issue of this file lists; test_the_conv_table_reaches_every_variant holds the table to it
ROUTES = {
    'c2_cin1', 'c2_cin2', 'p4', 'persist_nt1', 'persist_nt2', 'persist_nt3', 'tile4_ck8', 'tile4_ck24_nt4plus', 'lean', 'lean_ks',
    'generic_ck8', 'generic_ck8_ks', 'generic_ck32', 'generic_ck32_ks', 'generic_ck8_cout%4',
    'brick_4x1', 'brick_4x1_ks', 'brick_2x2', 'brick_2x2_ks', 'brick_2x1', 'brick_2x1_ks',
    'up_p4', 'up_lean8', 'up_generic8', 'updgrad_ps1', 'updgrad_ps2', 'updgrad_ps4', 'updgrad_ps8',
    'split_stacked', 'split_fwd2_mt1', 'split_fwd2_mt2', 'split_fwd2_mt3', 'split_fwd2_halves', 'split_fwd3', 'split_replanned',
    'split_updgrad', 'split_upfwd_mt1', 'split_upfwd_mt2', 'split_upfwd_mt3', 'split9_generic', 'split9_upfwd',
    'bf16_ck8_mt1', 'bf16_ck24_mt2', 'bf16_ck32_mt3', 'bf16_ck8_mt4', 'bf16_ck24_mt2_ks', 'bf16_up_fwd', 'bf16_up_dgrad'}
PLAN_FIELDS = ('ck', 'ncc', 'pack_nt', 'nchunks', 'mt', 'ksplit', 'nv')
KIND = {'plain': 1, 'up_fwd': 2, 'up_dgrad': 0}


# ---- the dispatchers' rules restated ------------------------------------------------------------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _replanned(vox_tiles, co_tiles, mt):
    """csrc/common.h syn_split_replanned"""
    if mt != 2 or co_tiles <= 3 or co_tiles % 3 or co_tiles % 2:
        return False
    return 512 < vox_tiles * (co_tiles // 3) < 768


def _split_plan_mt(vox_tiles, co_tiles, replan):
    """csrc/common.h syn_split_plan_mt"""
    mt = co_tiles if co_tiles <= 3 else (3 if co_tiles % 3 == 0 else (2 if co_tiles % 2 == 0 else 1))
    return 2 if replan and mt == 3 and _replanned(vox_tiles, co_tiles, 2) else mt


def _grid_x(ntiles, nchunks, slots=512):
    """csrc/conv_split.hip split_grid_x (and the bf16 forward's own copy of it)"""
    gx = max(8, (slots // nchunks) // 8 * 8)
    while gx > 8 and gx - 8 >= ntiles:
        gx -= 8
    return ntiles if ntiles < 8 else gx


def _expect(c, det=None):
    """csrc/conv3d.hip plan_fwd + dispatch_fwd2 + launch_fwd + parity_split and csrc/conv_split.hip launch_split_fwd, restated for
    an f32 row: the plan fields synthsr_conv3d_plan reports, and 'route' = the kernel the launch reaches.  (The 2 GB limits of
    the raw buffer addressing never bind at this table's sizes.)"""
    det = c.det if det is None else det
    s, kind = c.shape, KIND[c.entry]
    ci, co = (c.cout, c.cin) if c.entry == 'up_dgrad' else (c.cin, c.cout)     # the effective conv
    plain = kind == 1
    vt = _cdiv(s[0], 4) * _cdiv(s[1], 4) * _cdiv(s[2], 16)
    ct = _cdiv(co, 16)
    if c.arith != 'fp32_mfma' and ci % 8 == 0 and co % 8 == 0:
        mt = _split_plan_mt(vt, ct, kind != 2)
        nch = _cdiv(ct, mt)
        if vt * nch >= 200 and (kind != 2 or nch == 1):
            stacked = plain and co == 24 and c.arith == 'split'
            p = dict(ck=8, ncc=ci // 8, mt=mt, nchunks=nch, ksplit=1, nv=0,
                     pack_nt=-400 if stacked else (-300 - mt if kind == 2 else (-200 - mt if kind == 0 else -100 - mt)))
            fwd3 = nch >= 2 and 512 <= vt * nch < 1024
            if kind == 2:
                p['route'] = 'split9_upfwd' if c.arith == 'split9' else 'split_upfwd_mt%d' % mt
            elif kind == 0:
                p['route'] = 'split_updgrad'
            elif c.arith == 'split9':
                p['route'] = 'split9_generic'
            elif stacked:
                p['route'] = 'split_stacked'
            elif _replanned(vt, ct, mt):
                p['route'] = 'split_replanned'
            elif fwd3:
                p['route'] = 'split_fwd3'
            elif _grid_x(vt, nch) * nch <= 256 and p['ncc'] >= 4 and p['ncc'] % 2 == 0:
                p['route'], p['ksplit'] = 'split_fwd2_halves', 2      # the plan query reports the halves as ksplit 2
            else:
                p['route'] = 'split_fwd2_mt%d' % mt
            return p
    ck = 24 if ci % 24 == 0 else (32 if ci % 32 == 0 else 8)
    ncc = _cdiv(ci, ck)
    wgs = lambda mt, nt: _cdiv(s[0], 4) * _cdiv(s[1], mt) * _cdiv(s[2], 16) * _cdiv(ct, nt)
    mt, max_nt = 4, 6
    if wgs(4, min(6, ct)) < 768 or ck == 32:
        mt, max_nt = 2, 3
    nch = _cdiv(ct, max_nt)
    nt = _cdiv(ct, nch)
    ks = 1
    persist = mt == 4 and ck == 24 and nt <= 3 and co % 4 == 0
    p4 = persist and kind in (1, 2) and co == 24 and ci % 24 == 0
    c2 = ci if plain and co == 24 and ci <= 2 else 0
    brick, wn, wm = False, 1, 1
    if ck == 24 and mt == 2 and co % 16 == 0 and all(v % 4 == 0 for v in s) and s[2] % 16 != 0:
        bnt = 3 if ct % 3 == 0 else (2 if ct % 2 == 0 else 1)
        wn = 4 if (ct // bnt) % 4 == 0 else (2 if (ct // bnt) % 2 == 0 else 1)
        if wn > 1:
            brick, nt, nch = True, bnt, ct // bnt
            wm = 2 if wn <= 2 and s[1] % 8 == 0 else 1
    if brick:
        w = (s[0] // 4) * (s[1] // (4 * wm)) * (s[2] // 4) * (nch // wn)
        k = min(_cdiv(1024, w), ncc, 16)
        if w < 400 and ncc >= 2 and plain and k >= 2 and not det:
            ks = k
    else:
        w = wgs(mt, nt)
        k = min(_cdiv(1024, w), ncc // 2, 8)
        if w < 512 and ncc >= 4 and plain and k >= 2 and not det:
            ks = k
    p = dict(ck=ck, ncc=ncc, mt=mt, nchunks=nch, ksplit=ks, nv=0, pack_nt=-c2 if c2 else (0 if p4 else nt))

    def parity_split(workgroups):       # up_dgrad: no bias, no activation, no addend
        ps = 1
        while not det and ps < 8 and workgroups * ps < 400:
            ps *= 2
        return ps

    tiles = lambda m: _cdiv(s[0], 4) * _cdiv(s[1], m) * _cdiv(s[2], 16)
    if brick:
        r = 'brick_%dx%d' % (wn, wm)
        if kind == 2:
            r = 'up_' + r
        elif kind == 0:
            r = 'updgrad_%s_ps%d' % (r, parity_split((s[0] // 4) * (s[1] // (4 * wm)) * (s[2] // 4) * (nch // wn)))
    elif c2:
        r = 'c2_cin%d' % c2
    elif p4:
        r = 'up_p4' if kind == 2 else 'p4'
    elif mt == 4 and persist and plain:
        r = 'persist_nt%d' % nt
    elif ck == 24 and nt <= 3:      # conv3d_fwd_lean_kernel (27 taps, or the 8 taps of a parity set)
        r = {1: 'lean' if mt == 2 else 'lean4', 2: 'up_lean8', 0: 'updgrad_ps%d' % parity_split(tiles(mt) * nch)}[kind]
    elif mt == 4:
        r = {1: '', 2: 'up_', 0: 'updgrad_'}[kind] + ('tile4_ck24_nt4plus' if ck == 24 else 'tile4_ck%d' % ck)
    else:
        r = {1: 'generic_ck%d' % ck, 2: 'up_generic8', 0: 'updgrad_generic'}[kind]
    if ks > 1:
        r += '_ks'
    if plain and co % 4 and not c2:
        r += '_cout%4'
    p['route'] = r
    return p


def _expect_bf16(c):
    """csrc/conv_bf16.hip plan_bf16 and the `ks` rule of synthsr_conv3d_bf16_fwd_ex (ops hands it scratch for either path)"""
    if c.entry != 'plain':
        return dict(route='bf16_' + c.entry)
    s = c.shape
    ck = 32 if c.cin % 32 == 0 else (24 if c.cin % 24 == 0 else 8)
    ncc, mt_all = _cdiv(c.cin, ck), _cdiv(c.cout, 16)
    nch = _cdiv(mt_all, 4)
    mt = _cdiv(mt_all, nch)
    wgs = _grid_x(_cdiv(s[0], 4) * _cdiv(s[1], 4) * _cdiv(s[2], 16), 1) * nch
    ks = min(ncc, _cdiv(512, max(wgs, 1)))
    splitk = wgs < 256 and ks >= 2
    return dict(ck=ck, ncc=ncc, mt=mt, nchunks=nch, ksplit=ks if splitk else 1, route='bf16_ck%d_mt%d%s' % (ck, mt, '_ks' if splitk else ''))


def _route(c):
    return (_expect_bf16(c) if c.dtype == 'bf16' else _expect(c))['route']


def _plan(c):
    """synthsr_conv3d_plan for the effective conv of an f32 row under the arithmetic (and, on a device, the deterministic mode) in
    force: a host-only query"""
    from synthsr_amd import _lib, ops
    ci, co = (c.cout, c.cin) if c.entry == 'up_dgrad' else (c.cin, c.cout)
    out = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().synthsr_conv3d_plan(ops.conv_ctx_host(), _lib.i3(c.shape), ci, co, KIND[c.entry], out), 'conv3d_plan')
    return dict(zip(PLAN_FIELDS + ('count',), (int(v) for v in out)))


def check_plan(c, det):
    """the restated plan of an f32 row against the library's; det: the deterministic mode the query runs under"""
    want, got = _expect(c, det), _plan(c)
    for f in PLAN_FIELDS:
        assert got[f] == want[f], (c.id, f, got, want)


def test_the_conv_table_reaches_every_variant():
    """the declared routes are exactly the listed variants, every row's declared route is what the rules give, split-K rows run with
    atomics allowed, and the bf16 rows cover MT 1 to 4"""
    assert {c.route for c in CASES} == ROUTES
    for c in CASES:
        assert _route(c) == c.route, (c.id, _route(c))
        assert c.shape[0] * c.shape[1] * c.shape[2] * max(c.cin, c.cout) * (8 if c.entry != 'plain' else 1) < 2 ** 29
        assert max(c.cin, c.cout) <= 192
        if c.route.endswith('_ks') or c.route[-3:] in ('ps2', 'ps4', 'ps8'):
            assert not c.det or c.dtype == 'bf16'
    assert {_expect_bf16(c)['mt'] for c in BF16_CASES if c.entry == 'plain'} == {1, 2, 3, 4}
    assert {_expect_bf16(c)['ck'] for c in BF16_CASES if c.entry == 'plain'} == {8, 24, 32}
    assert any(c.cout % 16 for c in CASES if c.route.startswith('persist'))


# ---- data and float64 references ----------------------------------------------------------------------------------------------
def _conv64(x, w):
    """float64 'same' 3x3x3 conv on the host: x [d0,d1,d2,Ci], w [3,3,3,Ci,Co] -> [d0,d1,d2,Co]"""
    y = F.conv3d(x.double().permute(3, 0, 1, 2)[None], w.double().permute(4, 3, 0, 1, 2), None, padding=1)
    return y[0].permute(1, 2, 3, 0).contiguous()


def _dgrad_weights(wd):
    """wd [3,3,3,A,B] (a layer A -> B) -> the [3,3,3,B,A] kernel of its data gradient: taps flipped, channels transposed"""
    return wd.flip(0, 1, 2).permute(0, 1, 2, 4, 3)


def _up2(x):
    return x.repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)


FOLD = ([[1., 0, 0], [0, 1, 1], [0, 0, 0]], [[0., 0, 0], [1, 1, 0], [0, 0, 1]])   # [parity][low-res offset -1, 0, +1][tap]


def _parity_weights(w, p, rnd):
    """the 3x3x3 LOW-RES kernel of output parity p = (pz, py, px) of a folded conv: per axis, parity 0 reads v - 1 with tap 0 and v
    with taps 1 + 2, parity 1 reads v with taps 0 + 1 and v + 1 with tap 2.  bf16: these SUMS are what the pack rounds to bf16
    and the kernel multiplies, so they are the rounded operands of a bf16 folded row"""
    m = [torch.tensor(FOLD[q], dtype=torch.float64) for q in p]
    return rnd(torch.einsum('az,by,cx,zyxio->abcio', m[0], m[1], m[2], w.double()).float()).double()


PARITIES = [(a, b, e) for a in (0, 1) for b in (0, 1) for e in (0, 1)]


def _elu64(v):
    return torch.where(v > 0, v, torch.expm1(v))


def _elu_dy64(y):
    return torch.where(y > 0, torch.ones_like(y), y + 1)


def _regions(hi):
    """the sub-volumes a large folded row is compared on: the two outermost planes of every face (every edge and corner) and one
    interior block"""
    full = [slice(0, n) for n in hi]
    out = []
    for ax in range(3):
        for sl in (slice(0, 2), slice(hi[ax] - 2, hi[ax])):
            r = list(full)
            r[ax] = sl
            out.append(tuple(r))
    out.append(tuple(slice(n // 2 - min(n - 4, 44) // 2, n // 2 - min(n - 4, 44) // 2 + min(n - 4, 44)) for n in hi))
    return out


def _select(t, regions):
    """[N, C]: the voxels of the regions, in order (the whole tensor without regions)"""
    if regions is None:
        return t.reshape(-1, t.shape[-1])
    return torch.cat([t[r].reshape(-1, t.shape[-1]) for r in regions])


Data = collections.namedtuple('Data', 'x w b add below wd regions lin lin_d')
#   x: the input (up_dgrad: dz on the 2x grid); w [3,3,3,cin,cout]; add / below [out voxels, out channels]; wd [3,3,3,cout,cin]: the
#   layer whose DATA GRADIENT (pack mode 1) is the row's effective conv Cin -> Cout, i.e. runs the row's kernel
#   lin: float64 conv without bias on the selected voxels [N, C]; lin_d: the same for the data-gradient weights


@functools.lru_cache(maxsize=None)
def _data(cid):
    c = BY_ID[cid]
    g = torch.Generator(device='cpu').manual_seed(sum(c.shape) + 7 * c.cin + c.cout)
    rn = lambda *s: torch.randn(*s, generator=g)
    rnd = (lambda t: t.bfloat16().float()) if c.dtype == 'bf16' else (lambda t: t)
    hi = tuple(2 * v for v in c.shape)
    w = rnd(rn(3, 3, 3, c.cin, c.cout) / math.sqrt(27 * c.cin))
    b = 0.1 * rn(c.cout)
    regions = lin_d = wd = None
    if c.entry == 'plain':
        x = rnd(rn(*c.shape, c.cin))
        wd = rnd(rn(3, 3, 3, c.cout, c.cin) / math.sqrt(27 * c.cin))
        add, below = rnd(rn(*c.shape, c.cout)), rnd(_elu64(rn(*c.shape, c.cout)))
        lin, lin_d = _conv64(x, w), _conv64(x, _dgrad_weights(wd))
    elif c.entry == 'up_fwd':
        x = rnd(rn(*c.shape, c.cin))
        add, below = rnd(rn(*hi, c.cout)), None
        if c.shape == T768:     # the float64 conv of the whole 2x volume is too slow: sub-volumes with their halo
            regions = _regions(hi)
            up = F.pad(_up2(x.double()), (0, 0, 1, 1, 1, 1, 1, 1))
            halo = lambda r: tuple(slice(q.start, q.stop + 2) for q in r)
            lin = torch.cat([_conv64(up[halo(r)], w)[1:-1, 1:-1, 1:-1].reshape(-1, c.cout) for r in regions])
        elif c.dtype == 'bf16':      # parity by parity, with the folded weights as the pack rounds them
            lin = torch.empty(*hi, c.cout, dtype=torch.float64)
            for p in PARITIES:
                lin[p[0]::2, p[1]::2, p[2]::2] = _conv64(x, _parity_weights(w, p, rnd))
        else:
            lin = _conv64(_up2(x), w)
    elif c.dtype == 'bf16':
        x = rnd(rn(*hi, c.cout))
        add = below = None
        lin = sum(_conv64(x[p[0]::2, p[1]::2, p[2]::2], _dgrad_weights(_parity_weights(w, p, rnd))) for p in PARITIES)
    else:
        x = rnd(rn(*hi, c.cout))
        add = below = None
        gi = _conv64(x, _dgrad_weights(w))        # [2 s, Cl]: gradient on the 2x grid, then summed over each 2 x 2 x 2 block
        lin = gi.reshape(c.shape[0], 2, c.shape[1], 2, c.shape[2], 2, c.cin).sum((1, 3, 5))
    flat = lambda t: None if t is None else t.reshape(-1, t.shape[-1])
    return Data(x, w, b, add, below, wd, regions, flat(lin), flat(lin_d))


def _err(y, ref):
    d = y.double().cpu() - ref
    scale = float(ref.pow(2).mean().sqrt())
    return float(d.abs().max()) / scale, float(d.pow(2).mean().sqrt()) / scale


class _Checks:
    """collects the measured pairs of a row, prints each, and fails at the end with every figure that missed its bound"""

    def __init__(self, c):
        self.c, self.bad, self.rows = c, [], []

    def f32(self, y, ref, what, regions=None):
        mx, rms = _err(_select(y, regions), ref)
        print('%-20s %-20s %-26s worst %.3g rms %.3g of the reference rms' % (self.c.id, self.c.route, what, mx, rms))
        if not (rms < RMS_BOUND and mx < MAX_BOUND):
            self.bad.append((what, mx, rms))

    def bf16(self, y, ref, what):
        yd = y.double().cpu().reshape(ref.shape)
        scale = float(ref.pow(2).mean().sqrt())
        excess = ((yd - ref).abs() - BF16_ULP * ref.abs()) / scale
        mx, rms = _err(yd, ref)
        print('%-20s %-20s %-26s worst %.3g rms %.3g of the reference rms; worst beyond one bf16 ulp %.3g' %
              (self.c.id, self.c.route, what, mx, rms, float(excess.max())))
        if not float(excess.max()) <= MAX_BOUND:
            self.bad.append((what, float(excess.max())))

    def stats(self, stats, y64, what):
        """mean | biased variance per channel against float64 moments, to STATS_BOUND of the largest moment"""
        y64 = y64.reshape(-1, y64.shape[-1])
        n = y64.shape[1]
        for name, got, ref in (('mean', stats[:n], y64.mean(0)), ('var', stats[n:], y64.var(0, unbiased=False))):
            err = float((got.double().cpu() - ref).abs().max()) / float(ref.abs().max())
            print('%-20s %-20s %-26s %.3g of the largest' % (self.c.id, self.c.route, what + ' ' + name, err))
            if not err < STATS_BOUND:
                self.bad.append((what + ' ' + name, err))

    def same(self, a, b, what):
        if not torch.equal(a, b):
            self.bad.append((what, 'a second run differs in %d values' % int((a != b).sum())))

    def done(self):
        assert not self.bad, (self.c.id, self.c.route, self.bad)


class _Modes:
    """`with _Modes(c):` -- the conv arithmetic and the deterministic switch of a row, restored afterwards"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        from synthsr_amd import ops
        self.prev_arith = ops.set_conv_arithmetic(self.c.arith)
        self.prev_det = ops.set_deterministic(self.c.det)
        return self

    def __exit__(self, *a):
        from synthsr_amd import ops
        ops.set_deterministic(self.prev_det)
        ops.set_conv_arithmetic(self.prev_arith)


def _route_holds(c):
    assert _route(c) == c.route, (c.id, _route(c))
    if c.dtype == 'f32':
        check_plan(c, c.det)


def _unchanged(out, sentinel, what):
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel), what + ': a refused call wrote to `out`'


# ---- f32 rows -------------------------------------------------------------------------------------------------------------------
HAS_STATS_KERNEL = ('p4', 'split_', 'split9_generic')     # kernels with a statistics epilogue of their own


def _plain_f32(c, d, k):
    from synthsr_amd import ops
    cu = lambda t: t.cuda().contiguous()
    x, b, add, below = cu(d.x), cu(d.b), cu(d.add), cu(d.below)
    wp = ops.pack_conv_weights(cu(d.w), c.shape)
    wpd = ops.pack_conv_weights(cu(d.wd), c.shape, mode=1)
    ks, c2 = c.route.endswith('_ks') or c.route.endswith('_ks_cout%4'), c.route.startswith('c2')
    b64, add64, below64 = d.b.double(), d.add.double().reshape(-1, c.cout), d.below.double().reshape(-1, c.cout)
    runs = 2 if c.det else 1
    # forward with bias, linear and ELU
    for act, ref in ((0, d.lin + b64), (1, _elu64(d.lin + b64))):
        ys = [ops.conv3d(x, wp, b, c.cout, act) for _ in range(runs)]
        k.f32(ys[0], ref, 'forward act %d' % act)
        k.same(ys[0], ys[-1], 'forward act %d' % act)
    # the data gradient: weights packed with mode 1, against the conv by the flipped, transposed kernel
    ys = [ops.conv3d(x, wpd, None, c.cout, 0) for _ in range(runs)]
    k.f32(ys[0], d.lin_d, 'data gradient')
    k.same(ys[0], ys[-1], 'data gradient')
    sent = torch.full_like(add, 7.25)
    if c2:      # the first-layer kernel has no addend epilogue: refused, nothing written
        for act in (0, 2):
            out = sent.clone()
            with pytest.raises(ValueError):
                ops.conv3d_add(x, wp, b if act == 0 else None, add, c.cout, act, out=out)
            _unchanged(out, sent, 'c2 + addend, act %d' % act)
    else:
        if ks:      # split-K accumulates onto the addend where it sits in `out`: elsewhere it is refused
            out = sent.clone()
            with pytest.raises(ValueError):
                ops.conv3d_add(x, wp, b, add, c.cout, 0, out=out)
            _unchanged(out, sent, 'split-K + addend elsewhere')
            out = add.clone()
            ops.conv3d_add(x, wp, b, out, c.cout, 0, out=out)
            k.f32(out, d.lin + b64 + add64, 'addend in place act 0')
            out = add.clone()
            ops.conv3d_add(x, wp, b, out, c.cout, 1, out=out)
            k.f32(out, _elu64(d.lin + b64 + add64), 'addend in place act 1')
        else:
            ys = [ops.conv3d_add(x, wp, b, add, c.cout, 0) for _ in range(runs)]
            k.f32(ys[0], d.lin + b64 + add64, 'addend act 0')
            k.same(ys[0], ys[-1], 'addend act 0')
            out = add.clone()
            ops.conv3d_add(x, wp, b, out, c.cout, 0, out=out)
            k.f32(out, d.lin + b64 + add64, 'addend in place act 0')
        # the data gradient times elu' of the layer below
        ys = [ops.conv3d_add(x, wpd, None, below, c.cout, 2) for _ in range(runs)]
        k.f32(ys[0], d.lin_d * _elu_dy64(below64), 'data gradient act 2')
        k.same(ys[0], ys[-1], 'data gradient act 2')
        # ... with `out` aliasing `below`: the split-K launch zero-fills `out` before its epilogue reads the addend, and the other
        # kernels' workgroups would read neighbours' results -- the entry point refuses it, on every route, and writes nothing
        out = below.clone()
        with pytest.raises(ValueError):
            ops.conv3d_add(x, wpd, None, out, c.cout, 2, out=out)
        _unchanged(out, below, 'act 2 with out = addend')
    # conv + BatchNorm statistics: the output as above, mean | variance against float64 moments of the float64 output
    if c.route.startswith(HAS_STATS_KERNEL):
        for act, ref in ((0, d.lin + b64), (1, _elu64(d.lin + b64))):
            stats = torch.full((2 * c.cout,), 3.0, device='cuda')
            ws = torch.empty(2 * c.cout, dtype=torch.float64, device='cuda')
            y = ops.conv3d_stats(x, wp, b, c.cout, stats, ws, act=act)
            k.f32(y, ref, 'stats output act %d' % act)
            k.stats(stats, ref, 'stats act %d' % act)


def _up_fwd_f32(c, d, k):
    from synthsr_amd import ops
    cu = lambda t: t.cuda().contiguous()
    x, b, add = cu(d.x), cu(d.b), cu(d.add)
    wp8 = ops.pack_conv_weights_ex(cu(d.w), c.shape, 0, c.cin, 0, True)
    b64, add64 = d.b.double(), _select(d.add.double(), d.regions)
    if d.regions is not None:
        hi = tuple(2 * v for v in c.shape)
        seen = torch.zeros(hi, dtype=torch.bool)
        for r in d.regions:
            seen[r] = True
        share = float(seen.float().mean())
        print('%-20s compared on %.1f %% of the output voxels' % (c.id, 100 * share))
        assert share >= 0.10
    runs = 2 if c.det else 1
    for what, args, ref in (('folded forward act 0', (b, None, 0), d.lin + b64),
                            ('folded forward act 1', (b, None, 1), _elu64(d.lin + b64)),
                            ('folded addend act 0', (b, add, 0), d.lin + b64 + add64),
                            ('folded addend act 1', (None, add, 1), _elu64(d.lin + add64))):
        ys = [ops.conv3d_up(x, wp8, args[0], args[1], c.cout, args[2]) for _ in range(runs)]
        k.f32(ys[0], ref, what, d.regions)
        k.same(ys[0], ys[-1], what)
    out = add.clone()       # in place: the decoder accumulates the up-sampled range onto the skip range's conv
    ops.conv3d_up(x, wp8, b, out, c.cout, 0, out=out)
    k.f32(out, d.lin + b64 + add64, 'folded addend in place', d.regions)


def _up_dgrad_f32(c, d, k):
    from synthsr_amd import ops
    dz = d.x.cuda().contiguous()
    wpd8 = ops.pack_conv_weights_ex(d.w.cuda().contiguous(), c.shape, 0, c.cin, 1, True)
    ys = [ops.conv3d_up_dgrad(dz, wpd8, c.cin) for _ in range(2 if c.det else 1)]
    k.f32(ys[0], d.lin, 'folded data gradient')
    k.same(ys[0], ys[-1], 'folded data gradient')
    out = torch.full_like(ys[0], 3.5)       # the parity split accumulates with atomics: onto zeros, whatever `out` held
    ops.conv3d_up_dgrad(dz, wpd8, c.cin, out=out)
    k.f32(out, d.lin, 'folded data gradient (used out)')


@pytest.mark.parametrize('cid', _ids(F32_CASES))
def test_every_f32_conv_variant_vs_float64(cid):
    """forward (bias, act 0 / 1), data gradient (mode-1 weights), addend epilogues (in place on the split-K rows), the data gradient
    times elu' (act 2), and conv + statistics where the kernel has that epilogue: each within 4e-6 rms / 2e-5 worst element of
    the float64 result; deterministic rows bit-identical on a second run; what a kernel does not implement is refused with
    `out` untouched; act 2 with `out` aliasing the addend is refused on every route"""
    c = BY_ID[cid]
    d, k = _data(cid), _Checks(c)
    with _Modes(c):
        _route_holds(c)
        {'plain': _plain_f32, 'up_fwd': _up_fwd_f32, 'up_dgrad': _up_dgrad_f32}[c.entry](c, d, k)
    k.done()


# ---- bf16 rows ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', _ids(BF16_CASES))
def test_every_bf16_conv_variant_vs_float64(cid):
    """the bf16 kernels round one fp32 sum to bf16: every element within one bf16 ulp of the float64 result of the rounded operands
    plus the fp32 bound; statistics to 1e-6 of the float64 moments of the stored bf16 values (both statistics paths: the plain
    one and the split-K one)"""
    from synthsr_amd import ops
    c = BY_ID[cid]
    d, k = _data(cid), _Checks(c)
    cb = lambda t: t.cuda().bfloat16().contiguous()
    with _Modes(c):
        _route_holds(c)
        runs = 2 if c.det else 1
        if c.entry == 'up_fwd':      # raw sums: bias, addend and activation come with the skip range's conv
            wp8 = ops.pack_conv_weights_bf16(d.w.cuda(), 0, 0, c.cin, up=True)
            ys = [ops.conv3d_up(cb(d.x), wp8, None, None, c.cout, 0) for _ in range(runs)]
            k.bf16(ys[0], d.lin, 'bf16 folded forward')
            k.same(ys[0], ys[-1], 'bf16 folded forward')
        elif c.entry == 'up_dgrad':
            wpd8 = ops.pack_conv_weights_bf16(d.w.cuda(), 1, 0, c.cin, up=True)
            ys = [ops.conv3d_up_dgrad(cb(d.x), wpd8, c.cin) for _ in range(runs)]
            k.bf16(ys[0], d.lin, 'bf16 folded data gradient')
            k.same(ys[0], ys[-1], 'bf16 folded data gradient')
        else:
            x, b, below = cb(d.x), d.b.cuda(), cb(d.below)
            wp, wpd = ops.pack_conv_weights_bf16(d.w.cuda()), ops.pack_conv_weights_bf16(d.wd.cuda(), 1)
            b64, below64, add64 = d.b.double(), d.below.double().reshape(-1, c.cout), d.add.double().reshape(-1, c.cout)
            for act, ref in ((0, d.lin + b64), (1, _elu64(d.lin + b64))):
                ys = [ops.conv3d_bf16(x, wp, b, c.cout, act) for _ in range(runs)]
                k.bf16(ys[0], ref, 'bf16 forward act %d' % act)
                k.same(ys[0], ys[-1], 'bf16 forward act %d' % act)
                stats = torch.full((2 * c.cout,), 3.0, device='cuda')
                y = ops.conv3d_bf16(x, wp, b, c.cout, act, stats=stats)
                k.bf16(y, ref, 'bf16 stats output act %d' % act)
                k.stats(stats, y.double().cpu(), 'bf16 stats act %d' % act)
            k.bf16(ops.conv3d_bf16(x, wpd, None, c.cout, 0), d.lin_d, 'bf16 data gradient')
            k.bf16(ops.conv3d_bf16(x, wpd, None, c.cout, 2, below=below), d.lin_d * _elu_dy64(below64), 'bf16 data gradient act 2')
            k.bf16(ops.conv3d_bf16(x, wp, b, c.cout, 5, below=cb(d.add)), _elu64(d.lin + b64 + add64), 'bf16 addend act 5')
    k.done()


# ---- refusals leave the output alone ----------------------------------------------------------------------------------------------
def test_refused_conv_calls_return_einval_and_write_nothing():
    """the C entry points directly: every call a kernel cannot serve returns SYNTHSR_EINVAL (-1) before any kernel or memset is
    queued -- `out` keeps every bit of a sentinel pattern.  (c2 under a folded mode and a stacked layout with MT != 2 cannot be
    asked for through the exported entry points: see the module docstring.)"""
    from synthsr_amd import _lib, ops
    lib, p = _lib.load(), _lib.ptr

    def sentinel(*shape, dtype=torch.float32):
        n = int(torch.tensor(shape).prod())
        v = (torch.arange(n, device='cuda') % 251 + 1).to(dtype).view(shape)
        return v, v.clone()

    # fp32: the first-layer kernel with an addend; split-K (lean, generic, brick) with an addend that is not `out`, act 0 / 1;
    # act 2 with out = addend on every kind of route
    for cid, acts in (('c2_cin2', (0, 1, 2)), ('c2_cin1', (0,)), ('lean_ks', (0, 1)), ('generic_ck8_ks', (0, 1)),
                      ('generic_ck32_ks', (0,)), ('brick_4x1_ks', (0, 1)), ('brick_2x2_ks', (0,)), ('brick_2x1_ks', (0,))):
        c, d = BY_ID[cid], _data(cid)
        with _Modes(c):
            _route_holds(c)
            x, b, add = d.x.cuda(), d.b.cuda(), d.add.cuda()
            wp = ops.pack_conv_weights(d.w.cuda(), c.shape)
            for act in acts:
                out, out0 = sentinel(*c.shape, c.cout)
                rc = lib.synthsr_conv3d_fwd_add(ops.conv_ctx(), p(x), p(wp), p(b), p(add), p(out), _lib.i3(c.shape), c.cin, c.cout,
                                                act, _lib.stream())
                assert rc == -1, (cid, act, rc)
                _unchanged(out, out0, '%s act %d' % (cid, act))
    for cid in ('lean_ks', 'brick_4x1_ks', 'lean', 'persist_nt1', 'split_fwd2_mt1'):
        c, d = BY_ID[cid], _data(cid)
        with _Modes(c):
            x = d.x.cuda()
            wp = ops.pack_conv_weights(d.w.cuda(), c.shape)
            out, out0 = sentinel(*c.shape, c.cout)
            rc = lib.synthsr_conv3d_fwd_add(ops.conv_ctx(), p(x), p(wp), None, p(out), p(out), _lib.i3(c.shape), c.cin, c.cout, 2,
                                            _lib.stream())
            assert rc == -1, (cid, rc)
            _unchanged(out, out0, '%s act 2, out = addend' % cid)
    # bf16: act 5 / 6 with statistics; act 2 / 4 / 5 / 6 without `below`; statistics with too little scratch
    c, d = BY_ID['bf16_ck24_mt2'], _data('bf16_ck24_mt2')
    x, b, below = d.x.cuda().bfloat16(), d.b.cuda(), d.below.cuda().bfloat16()
    wp = ops.pack_conv_weights_bf16(d.w.cuda())
    scratch = torch.zeros(1 << 20, device='cuda')
    stats, stats0 = sentinel(2 * c.cout)

    def bf16_call(out, act, below, stats, nscratch):
        return lib.synthsr_conv3d_bf16_fwd_ex(p(x), p(wp), p(b), p(out), _lib.i3(c.shape), c.cin, c.cout, act, 0.0, p(below), p(stats),
                                              p(scratch), nscratch, _lib.stream())

    for what, act, bl, st, nscr in [('act %d with stats' % a, a, below, stats, scratch.numel()) for a in (5, 6)] + \
                                   [('act %d without below' % a, a, None, None, scratch.numel()) for a in (2, 4, 5, 6)] + \
                                   [('stats with too little scratch', 0, None, stats, 16)]:
        out, out0 = sentinel(*c.shape, c.cout, dtype=torch.bfloat16)
        assert bf16_call(out, act, bl, st, nscr) == -1, what
        _unchanged(out, out0, 'bf16 ' + what)
        _unchanged(stats, stats0, 'bf16 ' + what + ' (stats)')
    assert float(scratch.abs().max()) == 0.0
    out = torch.empty(*c.shape, c.cout, dtype=torch.bfloat16, device='cuda')
    assert bf16_call(out, 0, None, stats, scratch.numel()) == 0      # the same call with room: served
