#!/usr/bin/env python
"""Times the three image-score kernels (csrc/sr_scores.hip) at 160^3, 192^3 and 256^3 against the same scores formed with
torch on the same device in the same process: sums and elementwise ops for the moments and errors, three separable conv3d
passes over the five stacked moment fields, then elementwise and sum, for the SSIM.

    python tools/sr_scores_bench.py [--sizes 160 192 256] [--iters 20] [--torch_iters 5] [--out profiles/sr_scores_bench.txt]

Times are device events around `iters` back-to-back calls after a warm-up.  The HBM floor of a kernel is its two fp32 volumes
read once at 8.0 TB/s (the SSIM map is not written here)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8.0e12


def timed(torch, fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / iters


def torch_scores(torch, taps):
    F = torch.nn.functional
    w = [taps.view(1, 1, 11, 1, 1), taps.view(1, 1, 1, 11, 1), taps.view(1, 1, 1, 1, 11)]

    def moments(p, t):
        dp, dt = p - p.flatten()[0], t - t.flatten()[0]
        return torch.stack([dp.sum(), dt.sum(), (dp * dp).sum(), (dt * dt).sum(), (dp * dt).sum(), p.min(), p.max(), t.min(), t.max()])

    def errors(p, t, a, b):
        d = a * p + b - t
        return torch.stack([d.abs().sum(), (d * d).sum(), d.abs().max()])

    def ssim(p, t, a, b, inv):
        x, y = (a * p + b) * inv, t * inv
        f = torch.stack([x, y, x * x, y * y, x * y])[:, None]
        for k in w:
            f = F.conv3d(f, k)
        mx, my, xx, yy, xy = f[:, 0]
        vx, vy, vxy = xx - mx * mx, yy - my * my, xy - mx * my
        S = ((2 * mx * my + 1e-4) * (2 * vxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (vx + vy + 9e-4))
        return S.sum()
    return moments, errors, ssim


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[160, 192, 256])
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--torch_iters', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from synthsr_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit('sr_scores_bench needs the GPU: there is no CPU path to time')
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
    import _sr_scores_oracle as O
    taps = torch.from_numpy(O.taps('float32')).cuda()
    t_moments, t_errors, t_ssim = torch_scores(torch, taps)
    lines = ['device: %s' % torch.cuda.get_device_name(0),
             'size    kernel      hip_us  torch_us  torch/hip  hbm_floor_us  hip_share_of_floor   agreement']
    for n in args.sizes:
        g = torch.Generator(device='cuda').manual_seed(n)
        t = torch.rand((n, n, n), device='cuda', generator=g)
        p = (t + 0.05 * torch.randn((n, n, n), device='cuda', generator=g)).contiguous()
        ws = torch.empty(ops.sr_scores_workspace_bytes(p.shape), dtype=torch.uint8, device='cuda')
        a, b, inv = 0.98, 0.01, 1.0
        out_m, out_e, out_s = (torch.empty(k, dtype=torch.float64, device='cuda') for k in (12, 4, 2))
        floor = 2 * 4 * n ** 3 / HBM_BYTES_PER_S
        hm = ops.sr_moments(p, t, out=out_m, workspace=ws).clone()
        he = ops.sr_errors(p, t, None, a, b, out=out_e, workspace=ws).clone()
        hs = ops.sr_ssim3d(p, t, None, a, b, inv, out=out_s, workspace=ws)[0].clone()
        tm, te, ts = t_moments(p, t).double(), t_errors(p, t, a, b).double(), t_ssim(p, t, a, b, inv).double()
        agree = {
            'moments': float(abs(hm[7] - tm[4] - 0 * hm[0]) / abs(hm[7])) if float(hm[1]) == float(p.flatten()[0]) else float('nan'),
            'errors': float(abs(he[2] - te[1]) / abs(he[2])),
            'ssim3d': float(abs(hs[0] - ts) / abs(hs[0])),
        }
        rows = [('moments', lambda: ops.sr_moments(p, t, out=out_m, workspace=ws), lambda: t_moments(p, t)),
                ('errors', lambda: ops.sr_errors(p, t, None, a, b, out=out_e, workspace=ws), lambda: t_errors(p, t, a, b)),
                ('ssim3d', lambda: ops.sr_ssim3d(p, t, None, a, b, inv, out=out_s, workspace=ws), lambda: t_ssim(p, t, a, b, inv))]
        for name, hip, ref in rows:
            th, tt = timed(torch, hip, args.iters), timed(torch, ref, args.torch_iters, warmup=2)
            lines.append('%-7s %-10s %8.1f %9.1f %10.2f %13.1f %19.3f   rel %.1e'
                         % ('%d^3' % n, name, th * 1e6, tt * 1e6, tt / th, floor * 1e6, floor / th, agree[name]))
            print(lines[-1], flush=True)
        del p, t, ws
        torch.cuda.empty_cache()
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
