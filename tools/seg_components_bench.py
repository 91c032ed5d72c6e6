#!/usr/bin/env python
"""time of the connected components and the largest-component filter at the benchmark size, in one process, on two maps:
 'blocky': 8^3-voxel blocks of random labels; 'noisy': the same with 1 % of the voxels set to random labels (many components
 of a voxel or two), and, as the case one address takes every count of, 'solid': one label throughout.  Per map:
 (a) ops.seg_components + ops.seg_keep_largest, every listed label but the first a group of its own (N - 1 groups),
     connectivity 6: median / min / max of 20 calls by HIP events, and the time per kernel from the profiler's kernel records
     of 5 further calls;
 (b) the same on the host: scipy.ndimage.label per group, the smallest linear index per component, the largest component by
     size and then by root; once, wall clock;
 and the component map, the filtered map and the per-group stats of the two paths are asserted equal.

    python tools/seg_components_bench.py [--size 160] [--N 33] > profiles/seg_components_bench.txt"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd import ops  # noqa: E402
from synthsr_amd.predict_segmentation import component_groups  # noqa: E402


def host_path(m, lut, G, fill_value, connectivity=6):
    from scipy import ndimage
    structure = ndimage.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    grp = np.where((m >= 0) & (m < len(lut)), lut[np.clip(m, 0, len(lut) - 1)], -1)
    index = np.arange(m.size, dtype=np.int64).reshape(m.shape)
    comp = np.full(m.shape, -1, dtype=np.int32)
    out = m.copy()
    stats = np.zeros((G, 4), dtype=np.int64)
    t_label = 0.0
    for g in range(G):
        mask = grp == g
        t0 = time.perf_counter()
        lab, n = ndimage.label(mask, structure=structure)
        t_label += time.perf_counter() - t0
        if n == 0:
            stats[g] = (-1, 0, 0, 0)
            continue
        ids = np.arange(1, n + 1)
        roots = ndimage.minimum(index, lab, ids).astype(np.int64)
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)[1:]
        comp[mask] = roots[lab[mask] - 1]
        best = np.lexsort((roots, -sizes))[0]
        stats[g] = (roots[best], sizes[best], n, sizes.sum())
        out[mask & (lab != best + 1)] = fill_value
    return comp, out, stats, t_label


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--N', type=int, default=33)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    S, N = args.size, args.N
    g = torch.Generator().manual_seed(0)
    blocks = torch.randint(0, N, ((S + 7) // 8,) * 3, generator=g, dtype=torch.int32)
    blocky = blocks.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:S, :S, :S].contiguous()
    noisy = torch.where(torch.rand(S, S, S, generator=g) < .01, torch.randint(0, N, (S, S, S), generator=g, dtype=torch.int32),
                        blocky).contiguous()
    solid = torch.full((S, S, S), 1, dtype=torch.int32)
    lut, G, fill_value = component_groups(np.arange(N), 'per_label')
    dl = torch.from_numpy(lut).cuda()
    need = ops.seg_components_workspace_bytes((S, S, S))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    print('%d^3 voxels, %d labels, %d groups, connectivity 6; workspace %.1f MB; 3 + 4 launches per call'
          % (S, N, G, need / 1e6))
    ok = True
    for name, m in (('blocky', blocky), ('noisy', noisy), ('solid', solid)):
        dm = m.cuda()
        comp, out = torch.empty_like(dm), torch.empty_like(dm)
        stats = torch.empty(G, 4, dtype=torch.int64, device='cuda')

        def call():
            ops.seg_components(dm, dl, G, 6, comp, ws)
            ops.seg_keep_largest(dm, comp, dl, G, fill_value, out, stats, ws)
        for _ in range(3):
            call()
        evs = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            evs.append((e0, e1))
        torch.cuda.synchronize()
        t = sorted(x.elapsed_time(y) for x, y in evs)
        st = stats.cpu().numpy()
        print('%s: %d components, the largest of %d voxels, %d voxels removed' % (name, st[:, 2].sum(), st[:, 1].max(), int((out != dm).sum())))
        print('(a) seg_components + seg_keep_largest: %.3f ms (%.3f .. %.3f), median / min / max of %d calls'
              % (t[len(t) // 2], t[0], t[-1], args.reps))
        try:
            from torch.profiler import profile, ProfilerActivity
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                for _ in range(5):
                    call()
                torch.cuda.synchronize()
            rows = [(e.key, e.count, getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0))
                    for e in prof.key_averages() if 'seg_cc_' in e.key]
            for key, count, total in sorted(rows, key=lambda r: -r[2]):
                print('    %-26s %.3f ms per call' % (re.search(r'seg_cc_\w+', key).group(0), total / 5e3))
            if not rows:
                print('    (the profiler returned no kernel records)')
        except Exception as e:   # the timing above stands without the per-kernel split
            print('    (per-kernel times unavailable: %s)' % e)
        t0 = time.perf_counter()
        h_comp, h_out, h_stats, t_label = host_path(m.numpy(), lut, G, fill_value)
        t_host = time.perf_counter() - t0
        print('(b) scipy on the host, %d groups: %.1f ms, of which scipy.ndimage.label %.1f ms; on %d CPUs (scipy labels on one)'
              % (G, t_host * 1e3, t_label * 1e3, cpus))
        print('    host / device: %.0f' % (t_host * 1e3 / t[len(t) // 2]))
        equal = (np.array_equal(comp.cpu().numpy(), h_comp) and np.array_equal(out.cpu().numpy(), h_out) and np.array_equal(st, h_stats))
        print('    component map, filtered map and stats of the two paths equal: %s' % equal)
        ok = ok and equal
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
