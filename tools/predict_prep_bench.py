#!/usr/bin/env python
"""Times what predict() does around the U-Net, on the host and on the device, on one box in one run:

  host    predict.prepare_volume, the flip average (0.5 a + 0.5 flip(b) in float32 numpy, what Predictor.__call__ forms with
          torch on the device and downloads whole) and predict.postprocess: numpy, float64, one thread;
  device  predict.prepare_volume_device (upload included) and ops.sr_postprocess with the download of the crop.

The network itself is not run: both paths hand it the same padded volume.  Then every kernel of csrc/volume_prep.hip alone, with
the bytes its contract moves (below) over its time.

    python tools/predict_prep_bench.py [--cases 256 thick 320] [--iters 5] [--kernel_iters 20] [--out profiles/predict_prep_bench.txt]

Host times are medians of a host clock around the call; device-path times are medians of a host clock around work that ends in a
device synchronise or a download; kernel times are device events around `kernel_iters` back-to-back launches after a warm-up.

Bytes per voxel counted for a kernel (fp32; what the algorithm has to move, caches ignored):
  blur            4 read + 4 written per voxel of the volume;
  resample        4 read per SOURCE voxel (each is needed at least once) + 4 written per output voxel;
  normalise_pad   4 read + 4 written per voxel of the box, 4 written per padding voxel;
  sr_postprocess  8 read (two network outputs) + 4 written per voxel of the crop."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {'256': ((256, 256, 256), (1.0, 1.0, 1.0)),        # 1 mm isotropic: blur on every axis, no resampling to speak of
         'thick': ((256, 256, 30), (0.9, 0.9, 5.0)),       # clinical thick slices: two axes blurred and shrunk, one 5x up-sampled
         '320': ((320, 320, 320), (0.5, 0.5, 0.5))}        # 0.5 mm isotropic: blurred, 2x down-sampled


def median_time(fn, iters, warmup=1):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def event_time(torch, fn, iters, warmup=3):
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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', nargs='+', default=list(CASES), choices=list(CASES))
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--kernel_iters', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    import torch
    from synthsr_amd import ops, volumes as V
    from synthsr_amd.predict import prepare_volume, prepare_volume_device, postprocess
    assert torch.cuda.is_available(), 'this benchmark needs the GPU'
    lines = ['predict pre/post-processing, host (numpy float64) against device (csrc/volume_prep.hip); device %s; medians of %d '
             'runs, kernels: mean of %d launches' % (torch.cuda.get_device_name(0), args.iters, args.kernel_iters)]
    for name in args.cases:
        shape, vox = CASES[name]
        rng = np.random.default_rng(0)
        im = rng.random(shape) * 1000.0
        aff = np.diag(list(vox) + [1.0])
        # ---- host path
        S, idx, shp, _ = prepare_volume(im, aff)
        a, b = rng.standard_normal(S.shape, dtype=np.float32), rng.standard_normal(S.shape, dtype=np.float32)
        t_prep_h = median_time(lambda: prepare_volume(im, aff), args.iters)
        t_post_h = median_time(lambda: postprocess(0.5 * a + 0.5 * np.flip(b, 0), idx, shp), args.iters)
        # ---- device path
        da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        buf = torch.empty(S.shape, dtype=torch.float32, device='cuda')

        def prep_d():
            prepare_volume_device(im, aff, out=buf)
            torch.cuda.synchronize()
        t_prep_d = median_time(prep_d, args.iters)
        t_post_d = median_time(lambda: ops.sr_postprocess(da, idx, shp, netf=db, a=255.0, lo=0.0, hi=128.0).cpu().numpy(), args.iters)
        x32 = np.ascontiguousarray(im, dtype=np.float32)
        t_cast = median_time(lambda: np.ascontiguousarray(im, dtype=np.float32), args.iters)

        def upload():
            torch.from_numpy(x32).cuda()
            torch.cuda.synchronize()
        t_up = median_time(upload, args.iters)
        lines.append('')
        lines.append('%s: %s voxels of %s mm -> %s in %s' % (name, shape, vox, tuple(int(s) for s in shp), S.shape))
        lines.append('  prepare      host %9.1f ms   device %8.2f ms   (x %.0f; of the device time: float32 cast on the host %.2f ms, '
                     'upload %.2f ms)' % (t_prep_h * 1e3, t_prep_d * 1e3, t_prep_h / t_prep_d, t_cast * 1e3, t_up * 1e3))
        lines.append('  flip + post  host %9.1f ms   device %8.2f ms   (x %.0f; the device time includes the download of the crop)'
                     % (t_post_h * 1e3, t_post_d * 1e3, t_post_h / t_post_d))
        lines.append('  both         host %9.1f ms   device %8.2f ms   (x %.0f)'
                     % ((t_prep_h + t_post_h) * 1e3, (t_prep_d + t_post_d) * 1e3, (t_prep_h + t_post_h) / (t_prep_d + t_post_d)))
        # ---- the kernels alone
        sigmas, M, out_shape, _ = V.resample_plan(shape, aff)
        x = torch.from_numpy(x32).cuda()
        y = torch.empty_like(x)
        nsrc, nbox, npad = x.numel(), int(np.prod(out_shape)), buf.numel()
        rows = []
        for ax in range(3):
            if sigmas[ax] > 0:
                taps = V.gaussian_taps(sigmas[ax])
                t = event_time(torch, lambda: ops.volume_blur_axis(x, ax, taps, out=y), args.kernel_iters)
                rows.append(('blur axis %d (radius %d)' % (ax, len(taps) // 2), t, 8 * nsrc))
        mm = torch.empty(2, dtype=torch.float32, device='cuda')
        ws = torch.empty(ops.VOLUME_RESAMPLE_WORKSPACE_BYTES, dtype=torch.uint8, device='cuda')
        t = event_time(torch, lambda: ops.volume_resample(x, M, out_shape, 'clamp', out=buf, offset=idx, minmax=mm, workspace=ws),
                       args.kernel_iters)
        rows.append(('resample + min/max', t, 4 * nsrc + 4 * nbox))
        mm.copy_(torch.tensor([0.0, 1000.0]))   # a fixed range: the buffer is normalised in place over and over
        t = event_time(torch, lambda: ops.volume_normalise_pad(buf, idx, out_shape, mm), args.kernel_iters)
        rows.append(('normalise_pad', t, 8 * nbox + 4 * (npad - nbox)))
        out = torch.empty(tuple(int(s) for s in shp), dtype=torch.float32, device='cuda')
        t = event_time(torch, lambda: ops.sr_postprocess(da, idx, shp, netf=db, a=255.0, lo=0.0, hi=128.0, out=out), args.kernel_iters)
        rows.append(('sr_postprocess (flip average)', t, 12 * nbox))
        for what, t, nbytes in rows:
            lines.append('    %-32s %8.1f us   %7.1f MB   %6.0f GB/s' % (what, t * 1e6, nbytes * 1e-6, nbytes / t * 1e-9))
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
