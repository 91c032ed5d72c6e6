#!/usr/bin/env python
"""Times one training step of the training()-default U-Net (5 levels, 24 features, feat_mult 2, two convs per level, L1 head)
with activation='elu' and with activation='relu', alternating in one process (E R E R ...), on a fixed random input:

    python tools/activation_ab.py [--size 160] [--steps 20] [--rounds 3]

Prints one JSON line: per activation the median step time over all rounds (ms) and the ratio relu / elu."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=160)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from synthsr_amd.unet import unet
    S = args.size
    g = torch.Generator().manual_seed(0)
    x = torch.rand(S, S, S, 2, generator=g).cuda()
    target = torch.rand(S * S * S, generator=g).cuda()
    nets = {a: unet(nb_features=24, input_shape=[S, S, S, 2], nb_levels=5, conv_size=3, nb_labels=1, feat_mult=2,
                    nb_conv_per_level=2, final_pred_activation='linear', batch_norm=-1, activation=a, seed=0)
            for a in ('elu', 'relu')}

    def step(net):
        net.loss_l1(x, target)
        net.backward()
        net.adam_step(lr=1e-4)

    for net in nets.values():
        for _ in range(args.warmup):
            step(net)
    torch.cuda.synchronize()
    times = {a: [] for a in nets}
    for _ in range(args.rounds):
        for a, net in nets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(net)
            torch.cuda.synchronize()
            times[a].append((time.perf_counter() - t0) * 1e3 / args.steps)
    med = {a: float(np.median(v)) for a, v in times.items()}
    print(json.dumps({'size': S, 'steps': args.steps, 'rounds': args.rounds, 'ms_per_step': med, 'all_ms': times,
                      'relu_over_elu': med['relu'] / med['elu']}))


if __name__ == '__main__':
    main()
