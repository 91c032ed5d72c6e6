#!/usr/bin/env python
"""time of segmentation inference at the benchmark size, in one process (HIP events, median / min / max):
 (a) the head alone on the same activations: seg_head_argmax (fused BatchNorm + head + argmax -> int32 label map) against the
     path composed from seg_head_fwd (posteriors) + torch.argmax + table gather, the two alternating; the label maps of the
     two paths are compared;
 (b) SegmentationPredictor.segment_volume with and without flip averaging (host <-> device copies included);
 and the Dice counts of two label maps (seg_label_counts).

    python tools/seg_predict_bench.py [--size 160] [--C 24] [--N 33] > profiles/seg_predict_bench.txt"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd import ops  # noqa: E402

HBM = 8e12   # bytes / s (MI355X peak)


def _event_pair(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def timed_alternating(fns, warm=3, reps=20):
    """[(median, min, max) ms] of each function, run in turn `reps` times after `warm` rounds"""
    for _ in range(warm):
        for fn in fns:
            fn()
    evs = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            evs[i].append(_event_pair(fn))
    torch.cuda.synchronize()
    out = []
    for e in evs:
        t = sorted(a.elapsed_time(b) for a, b in e)
        out.append((t[len(t) // 2], t[0], t[-1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--C', type=int, default=24)
    ap.add_argument('--N', type=int, default=33)
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--reps', type=int, default=20)
    a = ap.parse_args()
    S, C, N = a.size, a.C, a.N
    nvox = S ** 3
    g = torch.Generator().manual_seed(0)
    x = torch.randn(S, S, S, C, generator=g).cuda()
    stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
    w, b = (torch.randn(C, N, generator=g) * .3).cuda(), (torch.randn(N, generator=g) * .1).cuda()
    labels = torch.randperm(2 * N + 8, generator=g)[:N].to(torch.int32).cuda()
    out = torch.empty(nvox, dtype=torch.int32).cuda()
    probs = torch.empty(nvox, N).cuda()
    composed = [None]

    def fused():
        ops.seg_head_argmax(x, stats, gamma, beta, w, b, labels, out)

    def compose():
        ops.seg_head_fwd(x, stats, gamma, beta, w, b, probs)
        composed[0] = labels[torch.argmax(probs, dim=1)]

    def posteriors_only():
        ops.seg_head_fwd(x, stats, gamma, beta, w, b, probs)

    print('(a) head alone, %d^3 voxels, C = %d, N = %d, fp32 (median / min / max of %d launches each, alternating, HIP events)'
          % (S, C, N, a.reps))
    res = timed_alternating([fused, compose, posteriors_only], reps=a.reps)
    nbytes = nvox * 4 * (C + 1)
    floor = nbytes / HBM * 1e3
    print('seg_head_argmax (fused)                       %.3f ms (%.3f .. %.3f)   compulsory %.1f MB = %.3f ms at 8 TB/s -> '
          '%.0f %% of the HBM floor rate' % (res[0] + (nbytes / 1e6, floor, 100 * floor / res[0][0])))
    print('seg_head_fwd + torch.argmax + table gather    %.3f ms (%.3f .. %.3f)   posteriors written and read back: %.1f MB'
          % (res[1] + (2 * nvox * N * 4 / 1e6,)))
    print('  of which seg_head_fwd                       %.3f ms (%.3f .. %.3f)' % res[2])
    print('fused / composed = %.3f (median times)' % (res[0][0] / res[1][0]))
    differ = int((out != composed[0]).sum())
    print('label maps of the two paths differ at %d of %d voxels (rounding ties of the two evaluation orders)' % (differ, nvox))

    other = torch.where(torch.rand(nvox, generator=g).cuda() < .8, out, out.roll(1))
    lut = torch.full((2 * N + 8,), -1, dtype=torch.int32).cuda()
    lut[labels.long()] = torch.arange(N, dtype=torch.int32).cuda()
    counts = torch.empty(3, N, dtype=torch.int64).cuda()
    res = timed_alternating([lambda: ops.seg_label_counts(out, other, lut, N, counts)], reps=a.reps)
    print('seg_label_counts (two maps, N = %d)             %.3f ms (%.3f .. %.3f)   compulsory %.1f MB = %.3f ms at 8 TB/s'
          % ((N,) + res[0] + (nvox * 8 / 1e6, nvox * 8 / HBM * 1e3)))
    del x, probs, out, other
    torch.cuda.empty_cache()

    from synthsr_amd.predict_segmentation import SegmentationPredictor
    from synthsr_amd.unet import UNet3D
    label_list = np.arange(N)
    net = UNet3D(C, [S, S, S, 1], a.levels, 3, N, feat_mult=2, nb_conv_per_level=2, batch_norm=-1,
                 final_pred_activation='softmax', seed=1)
    state = {k: v.numpy() for k, v in net.state_dict().items()}
    del net
    torch.cuda.empty_cache()
    pred = SegmentationPredictor(None, label_list, n_levels=a.levels, unet_feat_count=C, state_dict=state)
    vol = np.random.default_rng(0).random((S, S, S))
    pairs = [(2 * i + 1, 2 * i + 2) for i in range((N - 1) // 2)]
    print('(b) SegmentationPredictor.segment_volume, %d^3, %d levels, %d features, %d labels (numpy in, numpy out; median / min / '
          'max of %d)' % (S, a.levels, C, N, max(a.reps // 2, 10)))
    for name, kw in (('flipping=False', dict(flipping=False)), ('flipping=True, %d left/right pairs' % len(pairs),
                                                                dict(flipping=True, lr_pairs=pairs))):
        med, lo, hi = timed_alternating([lambda: pred.segment_volume(vol, **kw)], warm=2, reps=max(a.reps // 2, 10))[0]
        print('%-40s %.2f ms (%.2f .. %.2f)   device memory in use %.0f MB' % (name, med, lo, hi, torch.cuda.memory_allocated() / 1e6))


if __name__ == '__main__':
    main()
