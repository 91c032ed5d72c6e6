#!/usr/bin/env python
"""time of a training()-shaped step with the segmentation regulariser at the benchmark size, the frozen segmentation network
in fp32 or in bf16, and of each phase of the regulariser (HIP events on the stream), in one process on one device:

    python tools/segreg_bench.py [--size 160] [--N 33] [--reps 10] > profiles/segnet_bf16_step.txt

Three arms, alternated step by step, medians reported:
    dtype bf16, segnet f32    (what training(dtype='bf16', segmentation_model_file=...) runs without segnet_dtype)
    dtype bf16, segnet bf16   (segnet_dtype='bf16')
    dtype f32,  segnet f32
A step = regression loss + prediction, SegmentationRegulariser, backward, Adam, moving statistics (Trainer.step without the
generator).  Phases: frozen forward (predict_probs without its head), seg_head_fwd, seg_dice_sums, seg_dice_bwd,
backward_input."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from synthsr_amd import ops  # noqa: E402
from synthsr_amd.seg_loss import SegmentationRegulariser  # noqa: E402
from synthsr_amd.unet import UNet3D  # noqa: E402

PHASES = ('frozen forward', 'seg_head_fwd', 'seg_dice_sums', 'seg_dice_bwd', 'backward_input')


class Spans:
    """HIP-event spans around calls, by name; the events of one step are collected with take()"""

    def __init__(self):
        self.open = {}

    def wrap(self, name, fn):
        def timed(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.open.setdefault(name, []).append((e0, e1))
            return out
        return timed

    def take(self):
        out, self.open = self.open, {}
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--C', type=int, default=24)
    ap.add_argument('--N', type=int, default=33)
    ap.add_argument('--levels', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--reps', type=int, default=10)
    a = ap.parse_args()
    S, C, N = a.size, a.C, a.N
    nvox = S ** 3
    g = torch.Generator().manual_seed(0)
    kw = dict(feat_mult=2, nb_conv_per_level=2, batch_norm=-1)
    image = torch.rand(S, S, S, 2, generator=g).cuda()
    target = torch.rand(nvox, generator=g).cuda()
    seg = torch.randint(0, N, (S, S, S), generator=g, dtype=torch.int32).cuda()
    spans = Spans()
    for name in ('seg_head_fwd', 'seg_dice_sums', 'seg_dice_bwd'):   # unet.py and seg_loss.py call them through the module
        setattr(ops, name, spans.wrap(name, getattr(ops, name)))
    reg_nets, regs = {}, {}
    for dt in ('bf16', 'f32'):
        reg_nets[dt] = UNet3D(C, [S, S, S, 2], a.levels, 3, 1, final_pred_activation='linear', dtype=dt, **kw)
        segnet = UNet3D(C, [S, S, S, 1], a.levels, 3, N, final_pred_activation='softmax', dtype=dt, seed=1, **kw)
        regs[dt] = SegmentationRegulariser(segnet, np.arange(N), np.arange(N), 0.25)
        segnet.predict_probs = spans.wrap('predict_probs', segnet.predict_probs)
        segnet.backward_input = spans.wrap('backward_input', segnet.backward_input)
    arms = [('dtype bf16, segnet f32', 'bf16', 'f32'), ('dtype bf16, segnet bf16', 'bf16', 'bf16'), ('dtype f32,  segnet f32', 'f32', 'f32')]

    def step(net, reg):
        loss, pred = net.loss(image, target, 'l1', None, want_pred=True, fuse_head_bwd=False)
        dice = reg(pred, seg, net.dpred)
        net.backward()
        net.adam_step(1e-4)
        net.update_moving_stats()
        return loss, dice

    rec = {name: [] for name, _, _ in arms}
    for it in range(a.warmup + a.reps):
        for name, dt, sdt in arms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            spans.take()
            e0.record()
            loss, dice = step(reg_nets[dt], regs[sdt])
            e1.record()
            if it >= a.warmup:
                rec[name].append((e0, e1, spans.take(), loss, dice))
    torch.cuda.synchronize()
    print('segmentation-regularised training step, %d^3, %d-feature %d-level U-Nets, %d segmentation labels = %d Dice classes, '
          'frozen_bn batch' % (S, C, a.levels, N, N))
    print('%s; median of %d steps per arm, arms alternated step by step, HIP events; ms' % (torch.cuda.get_device_name(0), a.reps))
    print('%-26s %9s | %s | %9s %9s' % ('arm', 'step', ' '.join('%14s' % p for p in PHASES), 'image loss', 'Dice'))
    med = {}
    for name, _, _ in arms:
        steps = [e0.elapsed_time(e1) for e0, e1, _, _, _ in rec[name]]
        ph = {p: [] for p in PHASES}
        for _, _, sp, _, _ in rec[name]:
            t = {k: sum(x.elapsed_time(y) for x, y in v) for k, v in sp.items()}
            ph['frozen forward'].append(t['predict_probs'] - t['seg_head_fwd'])
            for p in PHASES[1:]:
                ph[p].append(t[p])
        med[name] = float(np.median(steps))
        print('%-26s %9.2f | %s | %9.5f %9.5f' % (name, med[name], ' '.join('%14.3f' % np.median(ph[p]) for p in PHASES),
                                                  float(rec[name][-1][3]), float(rec[name][-1][4])))
    base, new = med[arms[0][0]], med[arms[1][0]]
    print('segnet bf16 against segnet f32 under dtype bf16: %.2f ms -> %.2f ms (%.2fx)' % (base, new, base / new))


if __name__ == '__main__':
    main()
