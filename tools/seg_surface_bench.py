#!/usr/bin/env python
"""time of the surface distances of two label maps at the benchmark size, in one process:
 (a) ops.seg_surface_dist2 (both directions, every class): median / min / max of 20 calls by HIP events, and the time per
     kernel from the profiler's kernel records of 5 further calls;
 (b) predict_segmentation.surface_distances end to end (host label maps in, float64 score table out), once, wall clock;
 (c) the same scores on the host: per label and map scipy.ndimage.distance_transform_edt of the complement of the surface,
     read at the other map's surface voxels, once, wall clock, on the CPUs this process may use;
 and whether the two score tables are equal (squared distances are rounded to integers on the host side: rint(edt^2)).
The first map is made of 8^3-voxel blocks of random labels (N listed values and 3 without a class), the second is the first
shifted by one voxel along every axis with 1 % of its voxels relabelled at random (seed 0).

    python tools/seg_surface_bench.py [--size 160] [--N 33] > profiles/seg_surface_bench.txt"""
import argparse
import os
import re
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd import ops  # noqa: E402
from synthsr_amd.predict_segmentation import surface_distances, surface_scores_from_d2, SURFACE_KEYS  # noqa: E402
from synthsr_amd.segmentation_training import segmentation_lut  # noqa: E402


def host_scores(a, b, lut, N, percentile=95):
    from scipy.ndimage import distance_transform_edt
    ka, kb = [np.where((m >= 0) & (m < len(lut)), lut[np.clip(m, 0, len(lut) - 1)], -1) for m in (a, b)]

    def surface(k):
        p = np.pad(k, 1, constant_values=-2)
        inner = (slice(1, -1),) * 3
        differs = np.zeros(k.shape, dtype=bool)
        for axis in range(3):
            for step in (-1, 1):
                differs |= np.roll(p, step, axis=axis)[inner] != k
        return np.where((k >= 0) & differs, k, -1)
    sa, sb = surface(ka), surface(kb)
    far = np.iinfo(np.int32).max
    d2 = [np.full(a.shape, -1, dtype=np.int64) for _ in range(2)]
    n_edt = 0
    for k in range(N):
        for out, sq, ss in ((d2[0], sa, sb), (d2[1], sb, sa)):
            q = sq == k
            if not q.any():
                continue
            if not (ss == k).any():
                out[q] = far
                continue
            out[q] = np.rint(distance_transform_edt(ss != k)[q] ** 2).astype(np.int64)
            n_edt += 1
    return surface_scores_from_d2(sa, d2[0], sb, d2[1], N, percentile), n_edt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--N', type=int, default=33)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    S, N = args.size, args.N
    nvox = S ** 3
    g = torch.Generator().manual_seed(0)
    blocks = torch.randint(0, N + 3, ((S + 7) // 8,) * 3, generator=g, dtype=torch.int32)
    a = blocks.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:S, :S, :S].contiguous()
    b = a.roll((1, 1, 1), (0, 1, 2))
    b = torch.where(torch.rand(S, S, S, generator=g) < .01, torch.randint(0, N + 3, (S, S, S), generator=g, dtype=torch.int32), b)
    labels = np.arange(N)
    lut = segmentation_lut(labels)
    da, db, dl = a.cuda(), b.contiguous().cuda(), torch.from_numpy(lut).cuda()
    need = ops.seg_surface_workspace_bytes((S, S, S), N)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    o1, o2 = torch.empty_like(da), torch.empty_like(da)
    call = lambda: ops.seg_surface_dist2(da, db, dl, N, o1, o2, ws)
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
    n_surf = int((o1 >= 0).sum()), int((o2 >= 0).sum())
    print('(a) ops.seg_surface_dist2, %d^3 voxels, N = %d, both directions: %.3f ms (%.3f .. %.3f), median / min / max of %d calls'
          % (S, N, t[len(t) // 2], t[0], t[-1], args.reps))
    print('    surface voxels: %d and %d of %d; workspace %.1f MB; %d launches per call'
          % (n_surf + (nvox, need / 1e6, 2 + 3 * ((N + 7) // 8))))
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(5):
                call()
            torch.cuda.synchronize()
        rows = [(e.key, e.count, getattr(e, 'device_time_total', None) or getattr(e, 'cuda_time_total', 0.0))
                for e in prof.key_averages() if 'seg_surface' in e.key]
        for key, count, total in sorted(rows, key=lambda r: -r[2]):
            print('    %-34s %3d launches per call   %.3f ms per call' % (re.search(r'seg_surface_\w+', key).group(0), count // 5, total / 5e3))
        if not rows:
            print('    (the profiler returned no kernel records)')
    except Exception as e:   # the timing above stands without the per-kernel split
        print('    (per-kernel times unavailable: %s)' % e)

    an, bn = a.numpy(), b.numpy()
    surface_distances(an, bn, labels)   # warm: allocations, first launches
    t0 = time.perf_counter()
    dev = surface_distances(an, bn, labels)
    t_dev = time.perf_counter() - t0
    print('(b) surface_distances end to end (host maps in, score table out): %.1f ms' % (t_dev * 1e3))
    t0 = time.perf_counter()
    host, n_edt = host_scores(an, bn, lut, N)
    t_host = time.perf_counter() - t0
    cpus = len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else os.cpu_count()
    print('(c) scipy on the host: %d distance transforms of %d^3: %.1f ms on %d CPUs (scipy\'s transform runs on one)'
          % (n_edt, S, t_host * 1e3, cpus))
    print('    host / device, end to end: %.1f' % (t_host / t_dev))
    equal = all(np.array_equal(dev[k], host[k], equal_nan=True) for k in SURFACE_KEYS + ('n_seg', 'n_truth'))
    print('score tables of the two paths equal: %s' % equal)
    present = ~np.isnan(dev['hausdorff'])
    print('labels present in both maps: %d of %d; mean Hausdorff %.4f, mean HD95 %.4f, mean surface distance %.4f'
          % (present.sum(), N, dev['hausdorff'][present].mean(), dev['hd_percentile'][present].mean(), dev['mean'][present].mean()))
    if not equal:
        sys.exit(1)


if __name__ == '__main__':
    main()
