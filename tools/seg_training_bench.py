#!/usr/bin/env python
"""time of the two soft-Dice head kernels (synthsr_seg_head_dice_fwd / _bwd) at the benchmark size next to their compulsory
HBM traffic, and of one segmentation training step next to the regression step of the same network, in one process:

    python tools/seg_training_bench.py [--size 160] [--C 24] [--N 33] > profiles/seg_training_kernels.txt

With --dice_class_weights -1 and / or --dice_boundary_weights B the weighted forms are timed (and the boundary-mask kernel, on a
label map of 8^3-voxel blocks: per-voxel random labels put every class into every window, which no anatomy does).
With --loss wl2 | ce the two kernels of the losses on the logits (synthsr_seg_head_logit_loss_fwd / _bwd: no posteriors, so
4 nvox (C + 1) bytes forward and 4 nvox (2 C + 1) backward) and a training step with that loss are timed instead."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd import ops  # noqa: E402
from synthsr_amd.unet import UNet3D  # noqa: E402

HBM = 8e12   # bytes / s (MI355X peak)


def timed(fn, warm=3, reps=20):
    for _ in range(warm):
        fn()
    evs = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    t = sorted(a.elapsed_time(b) for a, b in evs)
    return t[len(t) // 2], t[0], t[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--C', type=int, default=24)
    ap.add_argument('--N', type=int, default=33)
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--dice_class_weights', type=str, default=None, help='-1 (dynamic) or a .npy of N values')
    ap.add_argument('--dice_boundary_weights', type=float, default=0.)
    ap.add_argument('--dice_boundary_dist', type=int, default=3)
    ap.add_argument('--dice_no_skip_background', dest='dice_skip_background', action='store_false')
    ap.add_argument('--loss', type=str, default='dice', choices=('dice', 'wl2', 'ce'))
    a = ap.parse_args()
    from synthsr_amd.segmentation_training import dice_settings
    dice = dice_settings(a.N, a.dice_class_weights, a.dice_boundary_weights, a.dice_boundary_dist, a.dice_skip_background)
    weighted = dice['class_weights'] is not None or dice['boundary_weights'] > 0
    S, C, N = a.size, a.C, a.N
    nvox = S ** 3
    g = torch.Generator().manual_seed(0)
    x = torch.randn(S, S, S, C, generator=g).cuda()
    stats = torch.cat([torch.zeros(C), torch.ones(C)]).cuda()
    gamma, beta = torch.ones(C).cuda(), torch.zeros(C).cuda()
    w, b = (torch.randn(C, N, generator=g) * .3).cuda(), torch.zeros(N).cuda()
    lut = torch.arange(N, dtype=torch.int32).cuda()
    seg = torch.randint(0, N + 3, (nvox,), generator=g, dtype=torch.int32).cuda()
    probs, sums = torch.empty(nvox, N).cuda(), torch.empty((3 if weighted else 2) * N).cuda()
    mask, kw_w = None, {}
    if weighted:
        blocks = torch.randint(0, N + 3, ((S + 7) // 8,) * 3, generator=g, dtype=torch.int32)
        seg = blocks.repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:S, :S, :S].contiguous().cuda()
        cw = torch.full((N,), 1.0 / N).cuda()   # (the kernels' time does not depend on the values)
        if dice['boundary_weights'] > 0:
            mask = torch.empty(nvox, dtype=torch.int64).cuda()
        kw_w = dict(mask=mask, boundary_weights=dice['boundary_weights'], class_weights=cw)
    dbn, dw, db = torch.empty_like(x), torch.zeros(C, N).cuda(), torch.zeros(N).cuda()
    if a.loss != 'dice':
        if weighted:
            ap.error('--loss %s has no weights' % a.loss)
        del probs
        name = {'wl2': 'weighted-L2', 'ce': 'cross-entropy'}[a.loss]
        print('%s head kernels (on the logits), %d^3 voxels, C = %d, N = %d, fp32 (median / min / max of 20 launches, HIP events)'
              % (name, S, C, N))
        sums3 = torch.empty(3).cuda()
        rows = [('seg_head_%s_fwd' % a.loss, lambda: ops.seg_head_logit_loss_fwd(x, stats, gamma, beta, w, b, seg, lut, sums3, a.loss),
                 nvox * 4 * (C + 1)),            # x + label map read
                ('seg_head_%s_bwd' % a.loss, lambda: ops.seg_head_logit_loss_bwd(seg, lut, x, stats, gamma, beta, w, b, sums3, dbn, dw,
                                                                                 db, a.loss), nvox * 4 * (2 * C + 1))]   # + dbn written
        report(rows)
        del x, dbn
        steps(a, g, seg, lut, name)
        return
    print('soft-Dice head kernels, %d^3 voxels, C = %d, N = %d, fp32 (median / min / max of 20 launches, HIP events)' % (S, C, N))
    fwd_bytes = nvox * 4 * (C + 1 + N)           # x + label map read, probs written
    bwd_bytes = nvox * 4 * (N + 1 + C + C)       # probs + label map + x read, dbn written
    rows = []
    if mask is not None:   # label map read, mask written; then the two head kernels read it
        rows.append(('seg_boundary_mask', lambda: ops.seg_boundary_mask(seg.view(S, S, S), lut, N, dice['boundary_dist'],
                                                                        dice['skip_background'], mask=mask), nvox * 12))
        fwd_bytes += nvox * 8
        bwd_bytes += nvox * 8
    seg = seg.reshape(-1)
    rows += [('seg_head_dice_fwd', lambda: ops.seg_head_dice_fwd(x, stats, gamma, beta, w, b, seg, lut, probs, sums, **kw_w),
              fwd_bytes),
             ('seg_head_dice_bwd', lambda: ops.seg_head_dice_bwd(probs, seg, lut, x, stats, gamma, beta, w, sums, dbn, dw, db,
                                                                 **kw_w), bwd_bytes)]
    if weighted:
        print('weighted soft Dice: class weights %s, boundary weights %g within %d voxels' % (
            'dynamic' if dice['class_weights'] == -1 else ('fixed' if dice['class_weights'] is not None else 'none'),
            dice['boundary_weights'], dice['boundary_dist']))
    report(rows)
    del x, probs, dbn
    steps(a, g, seg, lut, 'soft Dice', dice)


def report(rows):
    for name, fn, nbytes in rows:
        med, lo, hi = timed(fn)
        floor = nbytes / HBM * 1e3
        print('%-18s %.3f ms (%.3f .. %.3f)   compulsory %.1f MB = %.3f ms at 8 TB/s   -> %.0f %% of the HBM floor rate'
              % (name, med, lo, hi, nbytes / 1e6, floor, 100 * floor / med))


def steps(a, g, seg, lut, loss_name, dice=None):
    S, C, N = a.size, a.C, a.N
    nvox = S ** 3
    torch.cuda.empty_cache()
    kw = dict(feat_mult=2, nb_conv_per_level=2, batch_norm=-1)
    img = torch.rand(S, S, S, 1, generator=g).cuda()
    target = torch.rand(nvox, generator=g).cuda()
    segnet = UNet3D(C, [S, S, S, 1], a.levels, 3, N, final_pred_activation='softmax', **kw)
    regnet = UNet3D(C, [S, S, S, 1], a.levels, 3, 1, final_pred_activation='linear', **kw)

    def seg_step():
        if a.loss == 'wl2':
            segnet.loss_wl2(img, seg, lut)
        elif a.loss == 'ce':
            segnet.loss_cross_entropy(img, seg, lut)
        else:
            segnet.loss_dice(img, seg, lut, **dice)
        segnet.backward()
        segnet.adam_step(1e-4)
        segnet.update_moving_stats()

    def reg_step():
        regnet.loss(img, target, 'l1', fuse_head_bwd=True)
        regnet.backward()
        regnet.adam_step(1e-4)
        regnet.update_moving_stats()
    print('one training step of UNet3D(%d, %d^3 x 1, %d levels), forward + loss + backward + Adam (median / min / max of 10)' % (C, S, a.levels))
    for name, fn in (('regression step (1-channel l1 head)', reg_step), ('segmentation step (%d-class %s)' % (N, loss_name), seg_step)):
        med, lo, hi = timed(fn, warm=3, reps=10)
        print('%-40s %.2f ms (%.2f .. %.2f)' % (name, med, lo, hi))


if __name__ == '__main__':
    main()
