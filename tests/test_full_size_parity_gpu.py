"""ONE training step at the BASELINE.json shapes, HIP path vs the oracle on the identical generator output:

  * configs[1]: 160^3, training() defaults, 1 synthetic channel + reliability map (Cin = 2), 24..384 features,
    fold_upsample='auto' -- exactly bench.py's network / kernel plan;
  * configs[3] (in fp32): 192^3 Hyperfine-like [False, True, True] at 1.5 x 1.5 x 5 mm with registration error,
    Cin = 2, residual on the first input channel.

The generator runs on the GPU (its own parity is covered in test_generator_gpu.py); its image / target are copied to
the host and pushed through oracle/unet_ref.py (PyTorch-CPU float32, autograd).  Compared: loss (1e-4 relative), every
BatchNorm layer's batch mean / variance (5e-4 of range), the prediction (1e-3 of range) and EVERY parameter gradient
(per-tensor max error relative to the tensor's max-abs, max-pool rounding ties aligned: 1e-3 against the fp32 oracle, plus
that oracle's own distance from float64;
at 160^3 also against a FLOAT64 run of the oracle: 4e-4 of range and at most 6x the fp32 oracle's own distance).  This closes "kernel variants
chosen at the bench shape are only covered by isolated conv cases at other shapes" (VERDICT r01).

Run time on the GPU box (128 host cores): see the measured figures printed by the test (-s); the oracle step
dominates (about 1 min at 160^3, 2 min at 192^3)."""
import time
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _run(S, hyperfine, f64=False):
    import torch
    from synthsr_amd.brain_generator import BrainGenerator
    from synthsr_amd.unet import unet
    from synthsr_amd.synthetic import (synthetic_label_pool, GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR,
                                       PRIOR_STDS_T1_HR)
    from oracle import unet_ref as U
    pool = synthetic_label_pool(1, (S, S, S), 1234)
    common = dict(generation_classes=GENERATION_CLASSES, n_neutral_labels=19, output_shape=S, output_div_by_n=32,
                  flipping=True, scaling_bounds=.15, rotation_bounds=15, shearing_bounds=.02, translation_bounds=5,
                  nonlin_std=4., nonlin_shape_factor=.03125, randomise_res=False, downsample=True, blur_range=1.15,
                  bias_field_std=.3, bias_shape_factor=.03125, label_maps=pool,
                  rng=np.random.Generator(np.random.Philox(key=5)))
    if hyperfine:
        res = np.array([[1.5, 1.5, 5.], [1.5, 1.5, 5.]])
        bg = BrainGenerator(None, np.concatenate([PRIOR_MEANS_T1_HR] * 3), np.concatenate([PRIOR_STDS_T1_HR] * 3), 'normal',
                            GENERATION_LABELS, input_channels=[False, True, True], output_channel=0, data_res=res,
                            thickness=res, build_reliability_maps=False, simulate_registration_error=True, **common)
        residual = 0
    else:
        bg = BrainGenerator(None, PRIOR_MEANS_T1_HR, PRIOR_STDS_T1_HR, 'normal', GENERATION_LABELS,
                            build_reliability_maps=True, **common)
        residual = None
    gen = bg.labels_to_image_model
    gen.seed(0, 0)
    assert list(bg.model_output_shape) == [S, S, S, 2]
    net = unet(24, bg.model_output_shape, 5, 3, 1, feat_mult=2, nb_conv_per_level=2, final_pred_activation='linear',
               batch_norm=-1, activation='elu', seed=0, fold_upsample='auto')
    g = torch.Generator().manual_seed(11)                    # non-trivial BatchNorm affine / biases
    for nm, v in net.named_parameters():
        if nm.endswith('/gamma'):
            v.copy_(torch.rand(v.shape, generator=g) + .5)
        elif nm.endswith('/beta') or nm.endswith('/bias'):
            v.copy_(torch.randn(v.shape, generator=g) * .05)
    net.repack()
    labels, means, stds = next(bg.model_inputs_generator)[:3]
    t0 = time.time()
    image, target, seg = gen.generate(np.asarray(labels)[0, ..., 0], np.asarray(means)[0], np.asarray(stds)[0])
    kw = {} if residual is None else dict(residual=image, res_stride=image.shape[-1], res_off=residual)
    loss, pred = net.loss(image, target.reshape(-1), 'l1', None, want_pred=True, **kw)
    pred = pred.clone()
    net.backward()
    torch.cuda.synchronize()
    t_gpu = time.time() - t0
    # ---- oracle on the identical image / target
    x, tgt = image.cpu().clone(), target.cpu().clone().reshape(S, S, S, 1)
    P = {nm: v.detach().cpu().clone().requires_grad_(True) for nm, v in net.named_parameters()}
    # the device's own max-pool choices: where the oracle pools differently the two candidates must be within float32 rounding
    # of each other (a tie: which one wins is a property of the summation order, not of the algorithm) and the oracle is re-run
    # breaking those ties the device's way -- the protocol of every whole-network test (tests/conftest.py), here at full size
    from conftest import _pool_choices, align_pool_ties
    dev_pool = [(m.cpu(), None) for m, _ in _pool_choices(net)]
    res = None if residual is None else x[..., residual:residual + 1]
    # the device's own d(loss)/d(prediction) and prediction (without the residual), [S, S, S, 1] on the host
    dev_dp = net.dpred.view(S, S, S, 1).float().cpu().clone()
    dev_pr = pred.view(S, S, S, 1).float().cpu() - (0 if res is None else res)

    tie_report = {}

    def bn_distance(stats_):   # worst BatchNorm batch statistic, device vs this oracle run, relative to the largest statistic of its layer
        worst = 0.0
        for bn in net.bn_layers:
            o, C = bn['soff'], bn['C']
            for got, ref in ((net.bn_batch[o:o + C], stats_[bn['name']][0]), (net.bn_batch[o + C:o + 2 * C], stats_[bn['name']][1])):
                worst = max(worst, float((got.cpu().double() - ref.double()).abs().max() / ref.double().abs().max()))
        return worst

    def oracle_step(Pd, xin, tg, rs):
        stats_, pin = {}, []
        pr_ = U.unet_forward(xin, Pd, net.prefix, 5, 2, training=True, collect=stats_, pool_inputs=pin)
        # A tie here: every candidate of a pooling window is a BatchNorm output (x - mean) / std, and the two implementations'
        # batch statistics over up to 4 M voxels differ by `bnd` of their scale (measured on THIS run, about 1e-5): two candidates
        # that close cannot be ordered by either implementation.  Bound: 4 x that distance in ulp (no less than 64).  Count and
        # shape: the aligned windows must stay below 2 % of all pooling windows (measured 0.41 % at 160^3, 1.05 % on the smooth
        # thick-slice inputs of the 192^3 Hyperfine case) and be rounding-sized -- at most 5 % of them further apart than 16 ulp
        # (measured 1.2 %: 33 709 within 1 ulp, 24 004 within 4, 8 714 within 16, 829 within 64, 1 beyond, worst 116 of the 379
        # allowed); a systematic error of the device would fill the upper bins.  (Round 4: a flat 512 ulp and any count.)
        bnd = bn_distance(stats_)
        max_ulp = max(64.0, 4.0 * bnd / float(torch.finfo(torch.float32).eps))
        rep_ = {}
        nudges, n_ties = align_pool_ties(dev_pool, pin, max_ties=1000000, max_ulp=max_ulp, report=rep_)
        assert n_ties <= 0.02 * rep_['windows'], '%d of %d pooling windows aligned' % (n_ties, rep_['windows'])
        ulps = torch.cat(rep_.get('ulps', [torch.zeros(0)]))
        assert int((ulps > 16).sum()) <= 0.05 * max(n_ties, 1), '%d of %d aligned windows further apart than 16 ulp' % (
            int((ulps > 16).sum()), n_ties)
        tie_report[str(xin.dtype)] = dict(bn_distance=bnd, max_ulp_allowed=max_ulp, windows=rep_['windows'], ties=n_ties,
                                          worst_ulp=float(ulps.max()) if ulps.numel() else 0.0,
                                          histogram=[int(((ulps > lo) & (ulps <= hi)).sum()) for lo, hi in
                                                     ((-1, 1), (1, 4), (4, 16), (16, 64), (64, 256), (256, 1e9))])
        if n_ties:
            print('%d max-pool rounding tie(s) between device and oracle (%s): oracle re-run with the device\'s choices'
                  % (n_ties, xin.dtype))
            stats_ = {}
            pr_ = U.unet_forward(xin, Pd, net.prefix, 5, 2, training=True, collect=stats_,
                                 pool_nudge=[None if n is None else n.to(xin.dtype) for n in nudges])
        # kinks of the L1 loss (tests/conftest.py: "kinks of the loss"): voxels where sign(pred + residual - target) of the oracle
        # and of the device differ.  Each must have the kink BETWEEN the two predictions (|oracle error| <= their distance + 4 ulp:
        # a rounding tie at the accuracy the two forward passes agree to) and there may be few of them (<= 1e-4 of the voxels);
        # the oracle's prediction is moved onto the device's side at exactly those voxels -- one flipped sign of 4 M moves a
        # weight gradient by up to 2 / sqrt(N) = 1e-3 of its size.
        with torch.no_grad():
            err = (pr_ + (0 if rs is None else rs) - tg).float()
            mism = ((torch.sign(err) != torch.sign(dev_dp)) & (dev_dp != 0)).nonzero(as_tuple=True)
            n_kinks = int(mism[0].numel())
            knudge, kworst = None, 0.0
            if n_kinks:
                o_pr = pr_.detach().float()
                gap = dev_pr[mism] - o_pr[mism]
                ulp = float(torch.finfo(torch.float32).eps) * o_pr[mism].abs().clamp_min(float(o_pr.pow(2).mean().sqrt()))
                assert bool((err[mism].abs() <= gap.abs() + 4.0 * ulp).all()), 'a loss-kink disagreement that is no rounding tie'
                assert n_kinks <= 1e-4 * err.numel(), '%d voxels on different sides of the L1 kink' % n_kinks
                kworst = float((gap.abs() / ulp).max())
                knudge = torch.zeros_like(o_pr)
                knudge[mism] = gap + 4.0 * ulp * torch.where(gap != 0, gap.sign(), dev_dp[mism].sign())
        tie_report[str(xin.dtype)].update(loss_kink_ties=n_kinks, loss_kink_worst_ulp=kworst)
        if knudge is not None:
            print('%d L1-kink rounding tie(s) between device and oracle (%s, predictions up to %.1f ulp apart): the oracle takes the '
                  "device's side" % (n_kinks, xin.dtype, kworst))
            pr_ = pr_ + knudge.to(pr_.dtype)
            with torch.no_grad():
                left = int(((torch.sign((pr_ + (0 if rs is None else rs) - tg).float()) != torch.sign(dev_dp)) & (dev_dp != 0)).sum())
            assert left == 0, '%d kink disagreements left after the nudge' % left
        l_ = U.regression_loss(pr_, tg, 'l1', residual=rs)
        l_.backward()
        return pr_, l_, stats_, n_ties

    t0 = time.time()
    pr, lr, stats, n_ties32 = oracle_step(P, x, tgt, res)
    t_cpu = time.time() - t0
    rep = {'tie_report': tie_report}
    expect = pr.detach() + (0 if res is None else res)
    scale = float(expect.abs().max())
    rep['pred'] = float((pred.view(S, S, S, 1).cpu() - expect).abs().max()) / scale
    rep['loss'] = abs(loss.item() - float(lr)) / abs(float(lr))
    worst_bn = 0.0
    for bn in net.bn_layers:
        o, C = bn['soff'], bn['C']
        for got, ref in ((net.bn_batch[o:o + C], stats[bn['name']][0]), (net.bn_batch[o + C:o + 2 * C], stats[bn['name']][1])):
            worst_bn = max(worst_bn, float((got.cpu() - ref).abs().max() / ref.abs().max()))
    rep['bn'] = worst_bn
    grads = {}
    for nm, _, kind in net.specs:
        got = net.view(nm, net.grads).cpu().double()
        ref = P[nm].grad.double()
        grads[nm] = (float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30)), kind)
    if f64:
        # attribution: the same step once more in FLOAT64 on the host; the device's and the fp32 oracle's
        # errors are then both measured against it, per tensor -- who is further from the truth, and by how much
        t0 = time.time()
        P64 = {nm: v.detach().double().clone().requires_grad_(True) for nm, v in P.items()}
        pr64, l64, _, n_ties64 = oracle_step(P64, x.double(), tgt.double(), None if res is None else res.double())
        rep['t_f64'] = time.time() - t0
        rep['pool_ties'] = (n_ties32, n_ties64)
        e64 = pr64.detach() + (0 if res is None else res.double())
        s64 = float(e64.abs().max())
        rep['pred_vs_f64'] = (float((pred.view(S, S, S, 1).cpu().double() - e64).abs().max()) / s64,
                              float((expect.double() - e64).abs().max()) / s64)
        rep['loss_vs_f64'] = (abs(loss.item() - float(l64)) / abs(float(l64)), abs(float(lr) - float(l64)) / abs(float(l64)))
        attr = {}
        for nm, _, kind in net.specs:
            ref = P64[nm].grad
            sc = max(float(ref.abs().max()), 1e-300)
            dev = net.view(nm, net.grads).cpu().double()
            rms = max(float(ref.pow(2).mean().sqrt()), 1e-300)
            attr[nm] = (float((dev - ref).abs().max()) / sc, float((P[nm].grad.double() - ref).abs().max()) / sc, kind,
                        float((dev - ref).pow(2).mean().sqrt()) / rms, float((P[nm].grad.double() - ref).pow(2).mean().sqrt()) / rms)
        rep['attr'] = attr
    if hyperfine:
        # configs[3] as BASELINE.json names it: the same step in bf16 (bf16 activations / packed weights, fp32 accumulation,
        # fp32 BatchNorm statistics, fp32 master weights) against the SAME fp32 oracle result -- stated bf16 tolerances
        sd = net.state_dict()
        net_prefix = net.prefix
        del net
        torch.cuda.empty_cache()
        nb = unet(24, bg.model_output_shape, 5, 3, 1, feat_mult=2, nb_conv_per_level=2, final_pred_activation='linear',
                  batch_norm=-1, activation='elu', seed=0, dtype='bf16')
        nb.load_state_dict(sd)
        lb, pb = nb.loss(image, target.reshape(-1), 'l1', None, want_pred=True, **kw)
        pb = pb.clone()
        nb.backward()
        rep['bf16_pred'] = float((pb.view(S, S, S, 1).cpu() - expect).abs().max()) / scale
        rep['bf16_loss'] = abs(lb.item() - float(lr)) / abs(float(lr))
        worst_bn = 0.0
        for bn in nb.bn_layers:
            o, C = bn['soff'], bn['C']
            for got, ref in ((nb.bn_batch[o:o + C], stats[bn['name']][0]), (nb.bn_batch[o + C:o + 2 * C], stats[bn['name']][1])):
                worst_bn = max(worst_bn, float((got.cpu() - ref).abs().max() / ref.abs().max()))
        rep['bf16_bn'] = worst_bn
        cos = {}
        for nm, _, kind in nb.specs:
            got = nb.view(nm, nb.grads).cpu().double().reshape(-1)
            ref = P[nm].grad.double().reshape(-1)
            cos[nm] = float(torch.dot(got, ref) / (got.norm() * ref.norm()).clamp_min(1e-30))
        rep['bf16_min_cos'] = min(cos.values())
        rep['bf16_min_cos_layer'] = min(cos, key=cos.get)
        # (b) the oracle with the bf16 STORAGE roundings restated (oracle.unet_ref.round_bf16 wherever the bf16 network stores a
        # tensor: tests/test_bf16_gpu.py::test_unet_bf16_step_vs_oracle) -- same pooling decisions up to rounding flips, so
        # every gradient gets a PER-TENSOR bound (the bf16 leg asserted one global cosine)
        Pq = {nm: v.detach().clone().requires_grad_(True) for nm, v in P.items()}
        t0 = time.time()
        sq = {}
        prq = U.unet_forward(x, Pq, net_prefix, 5, 2, training=True, collect=sq, quant=U.round_bf16)
        lq = U.regression_loss(prq, tgt, 'l1', residual=res)
        lq.backward()
        rep['t_bf16_oracle'] = time.time() - t0
        eq = prq.detach() + (0 if res is None else res)
        rep['bf16q_pred'] = float((pb.view(S, S, S, 1).cpu() - eq).abs().max()) / float(eq.abs().max())
        rep['bf16q_loss'] = abs(lb.item() - float(lq)) / abs(float(lq))
        worst_bn = 0.0
        for bn in nb.bn_layers:
            o, C = bn['soff'], bn['C']
            for got, ref in ((nb.bn_batch[o:o + C], sq[bn['name']][0]), (nb.bn_batch[o + C:o + 2 * C], sq[bn['name']][1])):
                worst_bn = max(worst_bn, float((got.cpu() - ref).abs().max() / ref.abs().max()))
        rep['bf16q_bn'] = worst_bn
        bq = {}
        for nm, _, kind in nb.specs:
            got = nb.view(nm, nb.grads).cpu().double().reshape(-1)
            ref = Pq[nm].grad.double().reshape(-1)
            bq[nm] = (float(torch.dot(got, ref) / (got.norm() * ref.norm()).clamp_min(1e-30)),
                      float((got - ref).abs().max() / ref.abs().max().clamp_min(1e-300)),
                      abs(float(got.norm() / ref.norm().clamp_min(1e-300)) - 1.0), kind)
        rep['bf16q'] = bq
    return rep, grads, t_gpu, t_cpu


@pytest.mark.parametrize('S,hyperfine', [(160, False), (192, True)])
def test_one_training_step_at_baseline_shape_vs_oracle(S, hyperfine):
    rep, grads, t_gpu, t_cpu = _run(S, hyperfine, f64=True)
    worst = sorted(((e, nm) for nm, (e, _) in grads.items()), reverse=True)[:6]
    print('\n%d^3 %s: HIP step %.2fs (first call, incl. allocation), oracle step %.1fs; pred %.2e loss %.2e bn %.2e; worst '
          'gradients %s' % (S, 'configs[3]' if hyperfine else 'configs[1]', t_gpu, t_cpu, rep['pred'], rep['loss'],
                            rep['bn'], ', '.join('%s %.2e' % (nm, e) for e, nm in worst)))
    import os
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(out_dir):   # scratch report (every per-tensor error) for profiles/
        with open(os.path.join(out_dir, 'full_size_parity_%d.txt' % S), 'w') as f:
            f.write('%d^3: gpu %.2fs oracle %.1fs %r\n' % (S, t_gpu, t_cpu, rep))
            for nm, (e, kind) in grads.items():
                f.write('%-40s %-8s %.3e\n' % (nm, kind, e))
    if 'attr' in rep:
        # device vs float64 next to fp32-oracle vs float64, per tensor (max-pool ties aligned in both oracle runs).  Measured
        # (profiles/r04_full_size_parity_160_vs_float64.txt): every device gradient within 2.5e-4 of its tensor's range of the
        # float64 result, typically 5e-5; that is 1-5x (typically 2-3x) the distance of the fp32 host evaluation (PyTorch CPU:
        # blocked vector sums, where the device has sequential fp32 accumulator chains and float atomics).  The 1.9e-3 that
        # rounds 1-3 reported for the encoder kernels were max-pool tie flips, not arithmetic.  Bounds: 4e-4 of range
        # absolute, and never further from float64 than 6x the fp32 host evaluation (+ 2e-5 of range)
        attr = rep.pop('attr')
        anchor = {nm: v[1] for nm, v in attr.items()}
        lines = ['%-40s %-8s max/range: device %.3e  fp32 oracle %.3e  ratio %5.2f   rms/rms: device %.3e  fp32 oracle %.3e  ratio %5.2f'
                 % (nm, kind, d, o, d / max(o, 1e-30), dr, orr, dr / max(orr, 1e-30)) for nm, (d, o, kind, dr, orr) in attr.items()]
        print('float64 step %.1fs; prediction: device %.2e / oracle %.2e of range from float64; loss %.2e / %.2e'
              % ((rep['t_f64'],) + rep['pred_vs_f64'] + rep['loss_vs_f64']))
        print('\n'.join(lines))
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, 'full_size_parity_%d_vs_float64.txt' % S), 'w') as f:
                f.write('# one training step at %d^3: per-tensor max gradient error / tensor range, against a float64 run of the '
                        'oracle: device | fp32 oracle (PyTorch CPU)\n# prediction %r loss %r\n' % (S, rep['pred_vs_f64'], rep['loss_vs_f64']))
                f.write('\n'.join(lines) + '\n')
        for nm, (d, o, kind, dr, orr) in attr.items():
            assert d <= 6.0 * o + 2e-5, 'gradient of %s: device %.3e of range from float64, fp32 oracle %.3e' % (nm, d, o)
            # absolute cap: every tensor at 160^3; at 192^3 (thick-slice Hyperfine inputs) the conv / head kernels -- the
            # per-channel sums in front of a BatchNorm (its backward removes the mean of the signal: cancelling terms over 7 M
            # voxels, tiny range) are held by the anchored rule alone there
            assert d <= 4e-4 or (hyperfine and kind != 'kernel'), 'gradient of %s: device %.3e of range from float64' % (nm, d)
        assert rep['pred_vs_f64'][0] <= 4.0 * rep['pred_vs_f64'][1] + 1e-6 and rep['pred_vs_f64'][0] < 5e-5, rep['pred_vs_f64']
        assert rep['loss_vs_f64'][0] < 2e-6, rep['loss_vs_f64']
    assert rep['loss'] < 1e-4, rep
    assert rep['bn'] < 5e-4, rep
    assert rep['pred'] < 1e-3, rep
    if hyperfine:   # bf16 vs the fp32 oracle (stated bf16 tolerances; gradients: see tests/test_bf16_gpu.py on pooling flips)
        assert rep['bf16_loss'] < 1e-2 and rep['bf16_pred'] < 5e-2 and rep['bf16_bn'] < 3e-2 and rep['bf16_min_cos'] > 0.98, rep   # measured 0.991
        # ... and against the oracle with the bf16 storage roundings restated, PER TENSOR (BF16Q_* below)
        bq = rep.pop('bf16q')
        lines = ['%-40s %-8s cos %.6f  max err / range %.3e  |norm ratio - 1| %.3e' % (nm, kind, c, e, r) for nm, (c, e, r, kind) in bq.items()]
        print('bf16 step vs the bf16-storage oracle (%.1fs): prediction %.2e loss %.2e bn %.2e\n%s'
              % (rep['t_bf16_oracle'], rep['bf16q_pred'], rep['bf16q_loss'], rep['bf16q_bn'], '\n'.join(lines)))
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, 'full_size_parity_%d_bf16_vs_storage_oracle.txt' % S), 'w') as f:
                f.write('# one bf16 training step at %d^3 vs oracle.unet_ref with round_bf16 storage roundings: prediction %.3e loss '
                        '%.3e batch statistics %.3e\n' % (S, rep['bf16q_pred'], rep['bf16q_loss'], rep['bf16q_bn']))
                f.write('\n'.join(lines) + '\n')
        assert rep['bf16q_loss'] < BF16Q_LOSS and rep['bf16q_pred'] < BF16Q_PRED and rep['bf16q_bn'] < BF16Q_BN, rep
        for nm, (c, e, r, kind) in bq.items():
            cmin, rmax = (BF16Q_COS_KERNEL, BF16Q_NORM_KERNEL) if kind == 'kernel' else (BF16Q_COS_SUM, BF16Q_NORM_SUM)
            assert c > cmin and r < rmax, 'bf16 gradient of %s vs the bf16-storage oracle: cosine %.5f, norm off by %.3e' % (nm, c, r)
    for nm, (err, kind) in grads.items():
        # device vs the fp32 oracle with the max-pool ties and L1 kinks aligned (rounds 1-3 allowed 3e-3 / 3e-2 here: tie flips);
        # measured worst 3e-4 at 160^3.  At 192^3 the per-channel sums in front of a BatchNorm have almost no range of their own
        # (cancelling terms over 7 M voxels): there the bound follows from the float64 anchor of the SAME tensor -- device and fp32
        # oracle each within (6 o + 2e-5 | o) of float64, so at most 7 o + 2e-5 apart (round 5: flat 3e-3 / 3e-2, no anchor).
        # At 160^3 the 1e-3 is a bound on the device's distance from the exact result, for which the fp32 oracle stands in; the
        # oracle's own distance o from float64 is added.  o depends on the host: PyTorch-CPU splits the sums over the voxels
        # into one chunk per thread: the kernel / bias gradients of the level-0 conv in front of a BatchNorm measured o = 3.7e-5 /
        # 2.2e-4 on a 128-core host and 1.1e-3 / 1.6e-3 with 16 threads, the device 4e-5 .. 1.4e-4 on both.  The device's own
        # distance from float64 is held to 4e-4 above
        bound = 1e-3 + anchor[nm] if not hyperfine else max(1e-3, 7.0 * anchor[nm] + 2e-5)
        assert err < bound, 'gradient of %s: %.3e of its range (bound %.1e; worst: %s)' % (nm, err, bound, worst)


# bf16 step at 192^3 against the bf16-storage oracle, per tensor.  Measured (profiles/r06_full_size_parity_192_bf16_vs_storage_oracle.txt):
# prediction 2.0e-2 of range (one flipped bf16 rounding = 2^-8), loss 2.0e-4, batch statistics 7.9e-4; conv / head kernels cosine
# >= 0.99924 with norms within 1.5e-2; per-channel sums (biases, BatchNorm beta / gamma) cosine >= 0.9976 and norms within 1e-2
# except the bias in front of the first BatchNorm (cancelling terms over 7 M voxels: 0.9817 / 0.124)
BF16Q_LOSS, BF16Q_PRED, BF16Q_BN = 1e-3, 3e-2, 3e-3
BF16Q_COS_KERNEL, BF16Q_NORM_KERNEL = 0.998, 3e-2
BF16Q_COS_SUM, BF16Q_NORM_SUM = 0.97, 0.2


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_critic_update_at_160_vs_oracle(dtype):
    """BASELINE.json configs[4] at size: ONE critic update and the critic's share of ONE generator update of the adversarial
    fine-tuning (SynthSR/fine_tuning_with_adversary.py:482-508 make_discriminator, :579-595 build_discriminator_loss with
    the gradient penalty's double backward, :541-560 the generator's -D(G) term) at 160^3 -- 134.6 M critic parameters, 131 M
    of them in Dense(512) -- against oracle/unet_ref.critic_loss in float32 under autograd (create_graph).  Compared:
    D(real), D(fake), ||grad_x D(x_hat)||, the loss, EVERY parameter gradient (fp32: 1e-2 of the tensor's range and cosine
    > 0.9999; bf16 =
    'mixed bf16' of configs[4], bf16 conv stack with fp32 accumulation / Dense / master weights: cosine > 0.98 and norm
    within 5 %), the norm of the Dense(512) weight gradient, and the input gradient the generator update receives.  Bias gradients (sums of
    the nearly cancelling signals of the -D(real) and +D(fake) passes over every voxel) are bounded by 5e-2 of their range
    and a cosine > 0.999 in fp32.
    Oracle time: about 25 s on 16 host cores (the whole loss incl. the double backward)."""
    import torch
    from synthsr_amd.critic import Critic3D
    from oracle import unet_ref as U
    S, n_levels = 160, 4
    net = Critic3D([S, S, S, 1], seed=1, dtype=dtype)
    assert net.n_params > 134e6 and net.dense[0]['n_in'] == 256000 and net.dense[0]['n_out'] == 512
    g = torch.Generator().manual_seed(7)
    for nm, _ in net.specs:       # non-zero biases, weights of the initialisation's scale (|grad D| << 1: the penalty is active)
        v = net.view(nm)
        scale = 0.1 if nm.endswith('bias') else v.abs().max().item()
        v.copy_(torch.randn(v.shape, generator=g) * scale)
    net.repack()
    real, fake = torch.rand(S, S, S, 1, generator=g), torch.rand(S, S, S, 1, generator=g)
    u = 0.3
    t0 = time.time()
    loss, d_real, d_fake, norm = net.critic_loss_and_grads(real.cuda(), fake.cuda(), u, gp_weight=10.0)
    torch.cuda.synchronize()
    t_gpu = time.time() - t0
    P = {k: v.clone().requires_grad_(True) for k, v in net.state_dict().items()}
    t0 = time.time()
    ref, nref = U.critic_loss(real, fake, u, P, net.name, n_levels, 10.0)
    ref.backward()
    t_cpu = time.time() - t0
    with torch.no_grad():
        Pd = {k: v.detach() for k, v in P.items()}
        dr_ref = float(U.critic_forward(real, Pd, net.name, n_levels))
        df_ref = float(U.critic_forward(fake, Pd, net.name, n_levels))
    nref, ref = float(nref.detach()), float(ref.detach())
    anchor = None
    if dtype == 'f32':
        # float64 anchor (these bounds were fixed numbers): the same loss + double backward once more in
        # float64; per tensor d = |device - float64|, o = |fp32 oracle - float64| relative to the tensor's range
        t0 = time.time()
        P64 = {k: v.detach().double().requires_grad_(True) for k, v in P.items()}
        ref64, _ = U.critic_loss(real.double(), fake.double(), u, P64, net.name, n_levels, 10.0)
        ref64.backward()
        t_f64 = time.time() - t0
        top = max(float(P64[nm].grad.abs().max()) for nm, _ in net.specs)
        anchor = {}
        for nm, _ in net.specs:
            r64 = P64[nm].grad.reshape(-1)
            rng = max(float(r64.abs().max()), 1e-3 * top, 1e-300)
            ed = net.view(nm, net.grads).cpu().double().reshape(-1) - r64
            eo = P[nm].grad.double().reshape(-1) - r64
            anchor[nm] = (float(ed.abs().max()) / rng, float(eo.abs().max()) / rng,
                          float(ed.pow(2).mean().sqrt()) / rng, float(eo.pow(2).mean().sqrt()) / rng)
        del P64
    tol = 2e-4 if dtype == 'f32' else 3e-2
    dscale = max(1.0, abs(dr_ref), abs(df_ref))
    rep = dict(d_real=(d_real, dr_ref), d_fake=(d_fake, df_ref), norm=(norm, nref), loss=(loss, ref))
    worst_cos, worst_rel, worst_max, worst_bias = (2.0, ''), (0.0, ''), (0.0, ''), (0.0, '')
    lines, cos_all, rel_all = [], [], []
    for nm, _ in net.specs:
        a, b = net.view(nm, net.grads).cpu().double().reshape(-1), P[nm].grad.double().reshape(-1)
        if float(b.abs().max()) == 0.0:     # dense_1/bias: d(-D(real) + D(fake)) / d(last bias) = -1 + 1, exactly zero
            assert float(a.abs().max()) < 1e-6, (nm, float(a.abs().max()))
            continue
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-300))
        rel = abs(float(a.norm() / b.norm().clamp_min(1e-300)) - 1.0)
        mx = float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))
        lines.append('%-32s cos %.6f  |norm ratio - 1| %.2e  max err / range %.2e' % (nm, cos, rel, mx))
        worst_cos, worst_rel = min(worst_cos, (cos, nm)), max(worst_rel, (rel, nm))
        cos_all.append((cos, nm))
        rel_all.append((rel, nm))
        if nm.endswith('/bias'):   # a bias gradient is the sum of the three passes' signals over every voxel: -D(real) and
            worst_bias = max(worst_bias, (mx, nm))   # +D(fake) nearly cancel, what is left is small against the terms summed
        else:
            worst_max = max(worst_max, (mx, nm))
    dn = net.view(net.dense[0]['w'], net.grads).double().norm().item()
    dn_ref = P[net.dense[0]['w']].grad.double().norm().item()
    print('\ncritic 160^3 %s: HIP loss + gradients %.2fs (first call), oracle %.1fs; %r; Dense(512) dW norm %.6g vs %.6g; '
          'gradients: min cosine %.5f (%s), worst norm error %.2e (%s), worst max error %.2e of range (%s)'
          % (dtype, t_gpu, t_cpu, rep, dn, dn_ref, worst_cos[0], worst_cos[1], worst_rel[0], worst_rel[1], worst_max[0],
             worst_max[1]))
    import os
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'gpurun_out')
    if os.path.isdir(out_dir):   # scratch report (every per-tensor figure) for profiles/
        with open(os.path.join(out_dir, 'critic_parity_160_%s.txt' % dtype), 'w') as f:
            f.write('critic 160^3 %s: gpu %.2fs oracle %.1fs %r dense dW norm %.6g vs %.6g; worst bias %r\n'
                    % (dtype, t_gpu, t_cpu, rep, dn, dn_ref, worst_bias))
            f.write('\n'.join(lines) + '\n')
    assert abs(nref - 1.0) > 0.05                                     # the penalty contributes
    assert abs(d_real - dr_ref) < tol * dscale and abs(d_fake - df_ref) < tol * dscale, rep
    assert abs(norm - nref) < tol * nref, rep
    assert abs(loss - ref) < tol * max(1.0, abs(ref)), rep
    assert abs(dn - dn_ref) < (2e-3 if dtype == 'f32' else 5e-2) * dn_ref, (dn, dn_ref)
    if dtype == 'f32':
        # every gradient anchored on float64 (the rule of tests/conftest.py): the device is never more than K times further from
        # the float64 result than the fp32 host evaluation of the same graph, plus a floor of 2e-5 of range (4x for the
        # per-channel sums).  Both distances are dominated by LeakyReLU kinks -- a pre-activation within rounding of zero takes
        # slope 1 in one evaluation and 0.2 in another, the same discontinuity as a max-pool tie, and the critic has eight such
        # layers over up to 4.1 M voxels --, i.e. by a handful of discrete events per tensor: the rms error (all entries) is
        # held to K = 6, the single worst entry to K = 12.  Measured (profiles/r06_critic_parity_160_f32_vs_float64.txt): worst
        # entry 0.64-5.9x the fp32 oracle's, 3.4e-4 ... 6.2e-3 of range for the conv tensors.  (Round 5 held kernels to a flat
        # 1e-2 of range and biases to 5e-2 against the fp32 oracle.)
        alines = ['%-32s max: device %.3e  fp32 oracle %.3e of range from float64  ratio %5.2f   rms: %.3e  %.3e  ratio %5.2f'
                  % (nm, d, o, d / max(o, 1e-30), dr, orr, dr / max(orr, 1e-30)) for nm, (d, o, dr, orr) in anchor.items()]
        print('float64 critic loss + double backward %.1fs\n%s' % (t_f64, '\n'.join(alines)))
        if os.path.isdir(out_dir):
            with open(os.path.join(out_dir, 'critic_parity_160_f32_vs_float64.txt'), 'w') as f:
                f.write('# critic update at 160^3: per-tensor gradient error / range against a float64 run of the oracle (max | rms)\n')
                f.write('\n'.join(alines) + '\n')
        for nm, (d, o, dr, orr) in anchor.items():
            fl = 2e-5 * (1.0 if nm.endswith('/kernel') else 4.0)
            assert dr <= 6.0 * orr + fl and d <= 12.0 * o + fl, \
                'critic gradient of %s: device %.3e (rms %.3e) of range from float64, fp32 oracle %.3e (rms %.3e)' % (nm, d, dr, o, orr)
        assert worst_cos[0] > 0.9999, worst_cos      # measured 0.999997
    else:   # bf16 conv stack: kernels cosine > 0.98, norm within 5 %; biases (cancelling sums) cosine > 0.97, norm within 15 %
        kc = min((c, n) for c, n in cos_all if not n.endswith('/bias'))
        kr = max((r, n) for r, n in rel_all if not n.endswith('/bias'))
        assert kc[0] > 0.98 and kr[0] < 5e-2, (kc, kr)
        assert worst_cos[0] > 0.97 and worst_rel[0] < 0.15, (worst_cos, worst_rel)   # measured 0.986 / 8.2e-2 on the biases
    # generator side (build_generator_loss: w * mean(-D(G(x)))): the gradient the U-Net's prediction receives
    x = fake.clone().requires_grad_(True)
    gx, = torch.autograd.grad(U.critic_forward(x, Pd, net.name, n_levels), x)
    got = net.input_gradient(fake.cuda(), dout=-0.01).cpu().double().reshape(-1)
    want = (-0.01 * gx).double().reshape(-1)
    gcos = float(torch.dot(got, want) / (got.norm() * want.norm()))
    gmax = float((got - want).abs().max() / want.abs().max())
    gnorm = abs(float(got.norm() / want.norm()) - 1.0)
    print('critic 160^3 %s: input gradient of the generator update: cosine %.6f, |norm ratio - 1| %.2e, max error %.2e of range'
          % (dtype, gcos, gnorm, gmax))
    if os.path.isdir(out_dir):
        with open(os.path.join(out_dir, 'critic_parity_160_%s.txt' % dtype), 'a') as f:
            f.write('input gradient (generator update): cos %.6f  |norm ratio - 1| %.2e  max err / range %.2e\n' % (gcos, gnorm, gmax))
    if dtype == 'f32':
        # a 4.1 M-voxel gradient image through 8 LeakyReLU layers: a pre-activation within rounding of zero takes slope 1
        # in one implementation and 0.2 in the other (the same discontinuity as the max-pool ties of the U-Net tests), so
        # isolated voxels differ by percents of the range (measured max 5.5e-2) while the image as a whole agrees: cosine
        # > 0.9999 (measured 0.999997), norm to 1e-3 (measured 1e-6), fewer than 1e-2 of the voxels off by > 1e-2 of range
        frac = float(((got - want).abs() > 1e-2 * want.abs().max()).double().mean())
        print('   fraction of voxels off by more than 1e-2 of the range: %.2e' % frac)
        assert gcos > 0.9999 and gnorm < 1e-3 and frac < 1e-2, (gcos, gnorm, gmax, frac)
    else:
        assert gcos > 0.98 and gnorm < 5e-2, (gcos, gnorm, gmax)
