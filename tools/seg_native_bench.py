#!/usr/bin/env python
"""time of the label map on the input's own voxel grid, in one process: a 160^3 source of 33-channel posteriors (softmax of
random logits), resampled to
  'fine'   a 256^3 grid of 0.625 mm voxels, and
  'thick'  a 160 x 160 x 32 grid with 5 mm slices,
both by
 (a) ops.seg_resample_argmax (csrc/seg_resample.hip), without and with the interpolated posteriors written, and
 (b) the composition one would write in torch on the same device: permute to channel-first (contiguous), torch.nn.functional.
     grid_sample(mode='bilinear', padding_mode='border', align_corners=True) with a sampling grid built beforehand (not timed),
     argmax over the channels, the label values gathered.
Each is warmed up, then timed by HIP events call by call, (a) and (b) alternating; median / min / max.  The achieved GB/s of (a)
is its minimum traffic, one read of the source box plus 4 bytes per output voxel, over its median time.  The label maps of the two
paths are compared (they round differently, so a few voxels with two nearly equal posteriors may differ).  Exits 1 when (a) is
slower than (b) in either case.

    python tools/seg_native_bench.py [--size 160] [--N 33] > profiles/seg_native_bench.txt"""
import argparse
import os
import platform
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd import ops  # noqa: E402


def timed(calls, reps, warmup=3):
    """median / min / max ms per call of every function of `calls`, taken in turns"""
    for _ in range(warmup):
        for f in calls:
            f()
    torch.cuda.synchronize()
    evs = [[] for _ in calls]
    for _ in range(reps):
        for f, e in zip(calls, evs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e.append((e0, e1))
    torch.cuda.synchronize()
    out = []
    for e in evs:
        t = sorted(a.elapsed_time(b) for a, b in e)
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--N', type=int, default=33)
    ap.add_argument('--reps', type=int, default=10)
    args = ap.parse_args()
    S, N = args.size, args.N
    dev = torch.device('cuda')
    print('%s on %s; torch %s' % (torch.cuda.get_device_name(0), platform.node(), torch.__version__))
    g = torch.Generator(device='cuda').manual_seed(0)
    probs = torch.softmax(3.0 * torch.randn(S, S, S, N, generator=g, device=dev), dim=-1).contiguous()
    labels = torch.arange(N, dtype=torch.int32, device=dev) * 2 + 1
    box = [0, 0, 0, S - 1, S - 1, S - 1]
    fine = int(round(S * 1.6))
    cases = (('fine', (fine, fine, fine), np.array([0.625, 0.625, 0.625])),
             ('thick', (S, S, S // 5), np.array([1.0, 1.0, 5.0])))
    print('source %d^3 x %d channels fp32 (%.0f MB), the whole source as the box' % (S, N, probs.numel() * 4 / 1e6))
    ok = True
    for name, shape, step in cases:
        M = np.concatenate([np.diag(step), ((step - 1.0) / 2.0).reshape(3, 1)], axis=1)       # voxel centres
        nvox = int(np.prod(shape))
        out = torch.empty(shape, dtype=torch.int32, device=dev)
        pout = torch.empty(shape + (N,), dtype=torch.float32, device=dev)
        # the sampling grid of (b): x, y, z = source axes 2, 1, 0, normalised with align_corners=True
        axes = [torch.arange(n, device=dev, dtype=torch.float64) * float(s) + float(o) for n, s, o in zip(shape, step, M[:, 3])]
        axes = [(2.0 * a.clamp(0, S - 1) / (S - 1) - 1.0).float() for a in axes]
        zz, yy, xx = torch.meshgrid(*axes, indexing='ij')
        grid = torch.stack([xx, yy, zz], dim=-1)[None].contiguous()
        del zz, yy, xx
        keep = {}

        def fused():
            ops.seg_resample_argmax(probs, box, M, shape, labels, 0, out=out)

        def fused_probs():
            ops.seg_resample_argmax(probs, box, M, shape, labels, 0, out=out, probs_out=pout)

        def composed():
            first = probs.permute(3, 0, 1, 2)[None].contiguous()
            sampled = torch.nn.functional.grid_sample(first, grid, mode='bilinear', padding_mode='border', align_corners=True)
            keep['labels'] = labels[torch.argmax(sampled[0], dim=0)]

        (a, a_lo, a_hi), (p, p_lo, p_hi), (b, b_lo, b_hi) = timed([fused, fused_probs, composed], args.reps)
        fused()
        torch.cuda.synchronize()
        differ = int((out != keep['labels']).sum())
        least = probs.numel() * 4 + nvox * 4
        print('%s: %s voxels of %s mm from 1 mm' % (name, 'x'.join(str(n) for n in shape), 'x'.join('%g' % s for s in step)))
        print('(a) seg_resample_argmax:                  %8.3f ms (%.3f .. %.3f), median / min / max of %d calls; minimum traffic '
              '%.0f MB -> %.0f GB/s' % (a, a_lo, a_hi, args.reps, least / 1e6, least / a / 1e6))
        print('    with the posteriors written (%4.0f MB): %8.3f ms (%.3f .. %.3f)' % (nvox * N * 4 / 1e6, p, p_lo, p_hi))
        print('(b) permute + grid_sample + argmax, torch: %8.3f ms (%.3f .. %.3f)' % (b, b_lo, b_hi))
        print('    (b) / (a): %.1f; the two label maps differ at %d of %d voxels' % (b / a, differ, nvox))
        ok = ok and a <= b and differ <= 1e-3 * nvox
        del grid, out, pout, keep
        torch.cuda.empty_cache()
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
