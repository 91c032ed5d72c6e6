#!/usr/bin/env python
"""time per byte of the K-channel head kernels at the benchmark size (160^3 x 24, fp32): head_loss_fwd and head_bwd_multi for
K = 4 (the per-width kernels) next to K = 6, 8, 16 (the padded kernels), alternated in one process.

    python tools/head_width_bench.py [--size 160] [--rounds 5] [--iters 20]

Bytes: forward x + target + pred + dpred, backward x + dpred + dbn (what the kernels have to move; weights and sums are KB)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from synthsr_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument('--size', type=int, default=160)
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--iters', type=int, default=20)
ap.add_argument('--json', default=None)
a = ap.parse_args()
D, C = a.size, 24
nvox = D ** 3
g = torch.Generator().manual_seed(3)
x = torch.randn(D, D, D, C, generator=g).cuda()
stats = torch.zeros(2 * C, device='cuda')
ws = torch.zeros(2 * C, dtype=torch.float64, device='cuda')
ops.bn_stats(x, stats, ws)
gamma, beta = (torch.rand(C, generator=g) + .5).cuda(), torch.randn(C, generator=g).cuda()
dbn = torch.empty_like(x)
loss = torch.zeros(1, device='cuda')
CASES = [(4, 'l1'), (6, 'l1'), (8, 'l1'), (16, 'l1'), (6, 'laplace'), (8, 'laplace'), (16, 'laplace')]
bufs = {}
for K, kind in CASES:
    n = K // 2 if kind == 'laplace' else K
    bufs[(K, kind)] = dict(w=(torch.randn(C, K, generator=g) * .2).cuda(), b=(torch.randn(K, generator=g) * .1).cuda(),
                           target=torch.rand(nvox * n, generator=g).cuda(), pred=torch.empty(nvox * K, device='cuda'),
                           dpred=torch.empty(nvox * K, device='cuda'), dw=torch.zeros(C, K, device='cuda'),
                           db=torch.zeros(K, device='cuda'), n=n)


def fwd(K, kind):
    d = bufs[(K, kind)]
    ops.head_loss_fwd(x, stats, gamma, beta, d['w'], d['b'], d['target'], loss, kind, None, d['pred'], d['dpred'])


def bwd(K, kind):
    d = bufs[(K, kind)]
    ops.head_bwd_multi(d['dpred'], x, stats, gamma, beta, d['w'], dbn, d['dw'], d['db'])


def timed(fn, K, kind):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        fn(K, kind)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / a.iters   # microseconds per call


for case in CASES:   # warm-up: every kernel, every shape of the timed window
    for _ in range(3):
        fwd(*case)
        bwd(*case)
torch.cuda.synchronize()
samples = {(fn.__name__,) + case: [] for case in CASES for fn in (fwd, bwd)}
for _ in range(a.rounds):   # alternate the cases inside every round
    for case in CASES:
        for fn in (fwd, bwd):
            samples[(fn.__name__,) + case].append(timed(fn, *case))
rows = []
base = {}
for fn in ('fwd', 'bwd'):
    for K, kind in CASES:
        s = sorted(samples[(fn, K, kind)])
        us = s[len(s) // 2]
        n = bufs[(K, kind)]['n']
        nbytes = 4 * nvox * ((C + n + 2 * K) if fn == 'fwd' else (2 * C + K))
        ps_per_byte = us * 1e6 / nbytes
        if K == 4:
            base[fn] = ps_per_byte
        rows.append(dict(kernel=fn, K=K, kind=kind, us=round(us, 1), us_min=round(s[0], 1), us_max=round(s[-1], 1),
                         MB=round(nbytes / 1e6, 1), TBps=round(nbytes / us / 1e6, 3),
                         time_per_byte_vs_K4=round(ps_per_byte / base[fn], 3)))
print('%-4s %3s %-8s %9s %9s %9s %9s %7s %s' % ('', 'K', 'kind', 'us(med)', 'us(min)', 'us(max)', 'MB', 'TB/s', 'time/byte vs K=4'))
for r in rows:
    print('%-4s %3d %-8s %9.1f %9.1f %9.1f %9.1f %7.3f %.3f' % (r['kernel'], r['K'], r['kind'], r['us'], r['us_min'], r['us_max'],
                                                           r['MB'], r['TBps'], r['time_per_byte_vs_K4']))
if a.json:
    with open(a.json, 'w') as f:
        json.dump(rows, f, indent=1)
