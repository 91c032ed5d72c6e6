"""activation='relu' on the GPU: the ReLU conv epilogues (act 3 / 4, bf16 3 / 4 / 6), the activation-generic backward entry
points (act 3), the whole network against the oracle with its ELU swapped for ReLU, and training() end to end."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def T():
    import torch
    assert torch.cuda.is_available()
    return torch


def close(a, b, rel, name=''):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)
    assert err < rel, '%s: max rel err %.3e' % (name, err)


def same(a, b, name=''):
    """bit for bit as floats (+0 == -0)"""
    a, b = a.detach().float(), b.detach().float()
    bad = int((a != b).sum())
    assert bad == 0, '%s: %d of %d values differ' % (name, bad, a.numel())


def _addend(torch, shape, g):
    """values with exact zeros, negatives and positives"""
    a = torch.randn(*shape, generator=g)
    a[torch.rand(*shape, generator=g) < 0.3] = 0.0
    return a


def _plan(shape, cin, cout, kind=1):
    """synthsr_conv3d_plan under the current arithmetic / deterministic mode: {ck, ncc, pack_nt, nchunks, mt, ksplit, nv, count}"""
    import ctypes
    from synthsr_amd import _lib, ops
    out = (ctypes.c_int64 * 8)()
    _lib.check(_lib.load().synthsr_conv3d_plan(ops.conv_ctx_host(), _lib.i3(shape), int(cin), int(cout), int(kind), out),
               'conv3d_plan')
    return dict(zip(('ck', 'ncc', 'pack_nt', 'nchunks', 'mt', 'ksplit', 'nv', 'count'), (int(v) for v in out)))


def _family(shape, cin, cout, kind):
    """the forward kernel the dispatcher takes (csrc/conv3d.hip plan_fwd / dispatch_fwd2, conv_split.hip launch_split_fwd)"""
    from synthsr_amd import ops
    p = _plan(shape, cin, cout, kind)
    pn, arith = p['pack_nt'], ops.conv_arithmetic()
    if pn == -400:
        return 'split stacked'
    if -400 < pn <= -300:
        return 'split upfwd'
    if -200 < pn <= -100:
        if arith == 'split9':
            return 'split generic'
        vox_tiles = -(-shape[0] // 4) * -(-shape[1] // 4) * -(-shape[2] // 16)
        co_tiles, units = -(-cout // 16), vox_tiles * p['nchunks']
        replanned = p['mt'] == 2 and co_tiles > 3 and co_tiles % 6 == 0 and 512 < vox_tiles * (co_tiles // 3) < 768
        if p['nchunks'] >= 2 and 512 <= units < 1024 and not replanned:
            return 'split fwd3'
        return 'split fwd2 halves' if p['ksplit'] == 2 else 'split fwd2'
    if pn in (-1, -2):
        return 'c2'
    if pn == 0:
        return 'up p4' if kind == 2 else 'p4'
    if p['ksplit'] > 1:
        return 'split-K'
    if p['mt'] == 4 and p['ck'] == 24 and p['pack_nt'] <= 3 and p['nv'] == 0 and kind == 1 and cout % 4 == 0:
        return 'persist'
    return 'fp32 tiles'


# (arithmetic, deterministic, kind 1 plain | 2 folded forward, shape (kind 2: the low-resolution grid), Cin, Cout, family)
FAMILY_CASES = [
    ('split', True, 1, (16, 16, 32), 2, 24, 'c2'),                       # first layer
    ('split', True, 1, (64, 64, 64), 24, 24, 'split stacked'),           # Cout 24 on the stacked split layout
    ('split9', True, 1, (64, 64, 64), 24, 24, 'split generic'),          # nine products: conv3d_split_fwd_kernel
    ('fp32_mfma', True, 1, (64, 64, 64), 24, 24, 'p4'),
    ('fp32_mfma', True, 1, (64, 64, 64), 24, 48, 'persist'),
    ('split', True, 1, (32, 32, 64), 48, 96, 'split fwd3'),              # 256 tiles x 2 co-chunks = 512 units
    ('split', True, 1, (40, 40, 40), 48, 96, 'split fwd2'),              # re-planned onto 32-channel co-chunks
    ('split', True, 1, (20, 20, 20), 192, 192, 'split fwd2 halves'),     # 200 units: the split-K halves of fwd2
    ('fp32_mfma', True, 1, (20, 20, 20), 192, 192, 'fp32 tiles'),        # brick, deterministic: no split-K
    ('fp32_mfma', False, 1, (20, 20, 20), 192, 192, 'split-K'),          # brick + atomics + bias_act
    ('fp32_mfma', False, 1, (10, 10, 10), 384, 384, 'split-K'),          # lean + atomics + bias_act
    ('split', True, 2, (32, 32, 64), 48, 24, 'split upfwd'),
    ('fp32_mfma', True, 2, (64, 64, 64), 48, 24, 'up p4'),
    ('fp32_mfma', True, 2, (8, 8, 16), 48, 24, 'fp32 tiles'),            # the 8-tap lean kernel
]


@pytest.mark.parametrize('arith,det,kind,shape,cin,cout,family', FAMILY_CASES,
                         ids=['%s-%s-%s' % (c[0], 'det' if c[1] else 'atomics', c[6].replace(' ', '_')) for c in FAMILY_CASES])
def test_fp32_relu_epilogues(T, arith, det, kind, shape, cin, cout, family):
    """act 3 = fmax(act 0, 0) and act 4 = act 0 * (addend > 0) on every forward kernel family, the family asserted from the
    plan: bit for bit in deterministic mode; with the split-K atomics (two runs sum in different orders) to 1e-5 of range and
    exactly 0 where the addend is <= 0.  act 3 statistics against float64 moments of the conv's own output."""
    torch = T
    from synthsr_amd import ops
    prev_arith, prev_det = ops.conv_arithmetic(), ops.set_deterministic(det)
    ops.set_conv_arithmetic(arith)
    try:
        assert _family(shape, cin, cout, kind) == family, _plan(shape, cin, cout, kind)
        g = torch.Generator(device='cuda').manual_seed(5)
        rn = lambda *s: torch.randn(*s, generator=g, device='cuda')

        def addend(shp):
            a = rn(*shp)
            a[torch.rand(*shp, generator=g, device='cuda') < 0.3] = 0.0
            return a

        def check(a, ref, name, zero=None):
            if det:
                same(a, ref, name)
            else:
                close(a, ref, 1e-5, name)
                if zero is not None:
                    assert bool((a[zero] == 0).all()), name + ': not exactly 0 where the addend is <= 0'

        x = rn(*shape, cin)
        w = rn(3, 3, 3, cin, cout) / np.sqrt(27 * cin)
        b = 0.1 * rn(cout)
        if kind == 2:
            wp8 = ops.pack_conv_weights_ex(w, shape, 0, cin, up=True)
            add = addend(tuple(2 * s for s in shape) + (cout,))
            lin = ops.conv3d_up(x, wp8, b, add, cout, 0)
            check(ops.conv3d_up(x, wp8, b, add, cout, 3), lin.clamp_min(0), 'up act 3')
            return
        wp = ops.pack_conv_weights(w, shape)
        lin = ops.conv3d(x, wp, b, cout, 0)
        check(ops.conv3d(x, wp, b, cout, 3), lin.clamp_min(0), 'act 3')
        if cin != 2:    # addend epilogues (the first-layer kernel has none)
            add = addend(tuple(shape) + (cout,))
            lin_add = add.clone()   # in place: the split-K layers accumulate onto `out`
            ops.conv3d_add(x, wp, b, lin_add, cout, 0, out=lin_add)
            out = add.clone()
            check(ops.conv3d_add(x, wp, b, out, cout, 3, out=out), lin_add.clamp_min(0), 'act 3 + addend')
            # the data gradient fused with the ReLU backward of the layer below
            nob = ops.conv3d(x, wp, None, cout, 0)
            check(ops.conv3d_add(x, wp, None, add, cout, 4), nob * (add > 0).float(), 'act 4', zero=add <= 0)
        stats = torch.empty(2 * cout, device='cuda')
        ws = torch.empty(2 * cout, dtype=torch.float64, device='cuda')
        y = ops.conv3d_stats(x, wp, b, cout, stats, ws, act=3)
        check(y, lin.clamp_min(0), 'act 3 (stats)')
        y64 = y.double().reshape(-1, cout)
        close(stats[:cout], y64.mean(0), 1e-6, 'mean')
        close(stats[cout:], y64.var(0, unbiased=False), 1e-6, 'var')
    finally:
        ops.set_conv_arithmetic(prev_arith)
        ops.set_deterministic(prev_det)


def test_fp32_act_codes_rejected(T):
    """codes the fp32 kernels do not implement, or an act 4 without the layer below's output"""
    torch = T
    from synthsr_amd import ops
    x = torch.randn(8, 8, 16, 24, device='cuda')
    wp = ops.pack_conv_weights(torch.randn(3, 3, 3, 24, 24, device='cuda'), (8, 8, 16))
    with pytest.raises(ValueError):
        ops.conv3d(x, wp, None, 24, 4)
    with pytest.raises(ValueError):
        ops.conv3d(x, wp, None, 24, 5)


@pytest.mark.parametrize('shape,cin,cout', [((16, 16, 32), 24, 24), ((64, 64, 64), 24, 24), ((20, 20, 20), 48, 96),
                                             ((10, 10, 10), 192, 192)])
def test_bf16_relu_epilogues(T, shape, cin, cout):
    """bf16: act 3 (also with statistics) = fmax(act 0, 0) and act 4 = act 0 * (below > 0) bit for bit; act 6 =
    ReLU(conv + bias + below) against the act-0 output plus below"""
    torch = T
    from synthsr_amd import ops
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(*shape, cin, generator=g).cuda().bfloat16()
    w = (torch.randn(3, 3, 3, cin, cout, generator=g) / np.sqrt(27 * cin)).cuda()
    b = (0.1 * torch.randn(cout, generator=g)).cuda()
    wp = ops.pack_conv_weights_bf16(w)
    below = _addend(torch, tuple(shape) + (cout,), g).cuda().bfloat16()
    lin = ops.conv3d_bf16(x, wp, b, cout, 0)
    same(ops.conv3d_bf16(x, wp, b, cout, 3), lin.float().clamp_min(0), 'bf16 act 3')
    stats = torch.empty(2 * cout, device='cuda')
    y = ops.conv3d_bf16(x, wp, b, cout, 3, stats=stats)
    same(y, lin.float().clamp_min(0), 'bf16 act 3 (stats)')
    y64 = y.double().reshape(-1, cout)
    close(stats[:cout], y64.mean(0), 1e-6, 'bf16 mean')
    close(stats[cout:], y64.var(0, unbiased=False), 1e-6, 'bf16 var')
    nob = ops.conv3d_bf16(x, wp, None, cout, 0)
    same(ops.conv3d_bf16(x, wp, None, cout, 4, below=below), nob.float() * (below > 0).float(), 'bf16 act 4')
    y6 = ops.conv3d_bf16(x, wp, b, cout, 6, below=below)
    ref = (lin.float() + below.float()).clamp_min(0)
    close(y6.float(), ref, 1.5e-2, 'bf16 act 6')
    same(ops.conv3d_add(x, wp, b, below, cout, 3), y6, 'conv3d_add act 3 (bf16 -> 6)')
    with pytest.raises(ValueError):
        ops.conv3d_bf16(x, wp, b, cout, 6, below=below, stats=stats)


@pytest.mark.parametrize('dtype', ['f32', 'bf16'])
def test_pointwise_relu_backward(T, dtype):
    """act 3 of the five backward families (plain, BN-fused, head, dropout with batch 2, pool-fused): dz exactly 0 where
    y <= 0 and = where(y > 0, dz of act 1, 0) bit for bit; fp32: dz and dbias against float64 torch to 1e-5 of range"""
    torch = T
    from synthsr_amd import ops
    dt = torch.float32 if dtype == 'f32' else torch.bfloat16
    g = torch.Generator().manual_seed(2)
    shape, C = (8, 6, 10), 24
    n = int(np.prod(shape))
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    y = r(*shape, C).clamp_min(-0.9)
    y[torch.rand(*shape, C, generator=g).cuda() < 0.3] = 0.0
    y = y.to(dt)
    dy, dy2 = r(*shape, C).to(dt), r(*shape, C).to(dt)
    stats = torch.cat([r(C) * .1, r(C).abs() + .5])
    gamma, beta, sums = r(C).abs() + .5, r(C) * .1, r(2 * C)
    dpred, whead = r(n), r(C)
    drop = (torch.rand(2, C, generator=g).cuda() > .3).float() * 2.0

    # float64 torch references of act 3 (fp32 only: bf16 inputs put exact ties into the 2x2x2 pooling windows)
    yd, eps = y.double(), ops.BN_EPS
    mask = (yd > 0).double()
    mean, var = stats[:C].double(), stats[C:].double()
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (yd - mean) * rstd

    def bn_bwd(dbn):
        return gamma.double() * rstd * (dbn - sums[:C].double() / n - xhat * sums[C:].double() / n)

    def pooled(dp):     # MaxPooling3D backward of BN(y): dp routed to each window's arg-max
        t = (xhat * gamma.double() + beta.double()).permute(3, 0, 1, 2).unsqueeze(0)
        _, idx = torch.nn.functional.max_pool3d(t, 2, return_indices=True)
        src = dp.double().permute(3, 0, 1, 2).unsqueeze(0)
        return torch.nn.functional.max_unpool3d(src, idx, 2, output_size=t.shape[2:])[0].permute(1, 2, 3, 0)

    dd, dd2 = dy.double(), dy2.double()
    sc = drop.double().repeat_interleave(shape[0] // 2, 0)[:, None, None, :]

    def check(name, run, ref):
        de, dr = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
        ze, zr = run(1, de), run(3, dr)
        same(zr, torch.where(y.float() > 0, ze.float(), torch.zeros_like(ze.float())), name)
        assert bool((zr.float()[y.float() <= 0] == 0).all()), name
        if dtype == 'f32':
            z64 = ref() * mask
            close(zr, z64, 1e-5, name + ' vs float64')
            close(dr, z64.reshape(-1, C).sum(0), 1e-5, name + ' dbias vs float64')
        else:   # dbias sums the fp32 products, dz holds them rounded to bf16
            close(dr, zr.double().reshape(-1, C).sum(0), 1e-2, name + ' dbias')

    check('act_bwd', lambda a, db: ops.elu_bwd(dy, y, dy2=dy2, dbias=db, act=a), lambda: dd + dd2)
    check('bn_act_bwd', lambda a, db: ops.bn_elu_bwd(dy, y, stats, gamma, sums, dy2=dy2, dbias=db, act=a),
          lambda: bn_bwd(dd) + dd2)
    check('bn_act_bwd_head', lambda a, db: ops.bn_elu_bwd_head(dpred, whead, y, stats, gamma, sums, dbias=db, act=a),
          lambda: bn_bwd(dpred.double().view(*shape, 1) * whead.double()))
    check('act_bwd_drop', lambda a, db: ops.elu_bwd_drop(dy, y, drop, dy2=dy2, dbias=db, act=a), lambda: dd * sc + dd2)
    dpool = r(shape[0] // 2, shape[1] // 2, shape[2] // 2, C).to(dt)
    check('bn_pool_act_bwd', lambda a, db: ops.bn_pool_elu_bwd(dpool, y, stats, gamma, beta, sums, dy2=dy2, dbias=db, act=a),
          lambda: bn_bwd(pooled(dpool)) + dd2)
    with pytest.raises(ValueError):
        ops.elu_bwd(dy, y, act=2)


def _relu_net(torch, fold='auto', dtype='f32', dropout=0.0, batch=1, shape=(16, 16, 32), cin=2, feats=24, levels=3):
    from synthsr_amd.unet import unet
    net = unet(nb_features=feats, input_shape=list(shape) + [cin], nb_levels=levels, conv_size=3, nb_labels=1, feat_mult=2,
               nb_conv_per_level=2, final_pred_activation='linear', batch_norm=-1, activation='relu', seed=3,
               fold_upsample=fold, dtype=dtype, conv_dropout=dropout)
    g = torch.Generator().manual_seed(11)    # non-trivial BatchNorm affine parameters and biases
    for nm, v in net.named_parameters():
        if nm.endswith('/gamma'):
            v.copy_(torch.rand(v.shape, generator=g) + .5)
        elif nm.endswith('/beta') or nm.endswith('/bias'):
            v.copy_(torch.randn(v.shape, generator=g) * .1)
    net.repack()
    if batch > 1:
        net.set_batch(batch)
    return net


class _ReluOracle:
    """oracle.unet_ref with its ELU swapped for ReLU (the oracle file stays as it is).  Records, per conv of a forward, the
    pre-activation z and S = conv3d(|x|, |w|) + |b| (float64, the scale of z's rounding error); `force[i]` = (sites, mask)
    makes ReLU i take the given side at those sites (gradient 1 or 0), i.e. the device's side of a rounding tie."""

    def __init__(self, monkeypatch, torch):
        from oracle import unet_ref as U
        import torch.nn.functional as F
        self.U, self.torch, self.conv = U, torch, U.conv3d_same
        self.rec, self.force, self.i, self.S, self.zs, self.Ss = False, None, 0, None, [], []
        ns = types.SimpleNamespace(**{k: getattr(F, k) for k in dir(F) if not k.startswith('__')})
        ns.elu = self._relu
        monkeypatch.setattr(U, 'F', ns)
        monkeypatch.setattr(U, 'conv3d_same', self._conv)

    def _conv(self, x, w, b=None):
        if self.rec:
            with self.torch.no_grad():
                d = lambda t: t.detach().double().abs()
                self.S = self.conv(d(x), d(w), None if b is None else d(b))
        return self.conv(x, w, b)

    def _relu(self, z):
        i = self.i
        self.i += 1
        if self.rec:
            self.zs.append(z.detach().double())
            self.Ss.append(self.S)
        m = z > 0
        if self.force is not None and self.force[i] is not None:
            m = m.clone().reshape(-1)
            m[self.force[i][0]] = self.force[i][1]
            m = m.view_as(z)
        return z * m.to(z.dtype)

    def forward(self, x, P, prefix, levels, rec=False, **kw):
        self.i, self.rec, self.zs, self.Ss = 0, rec, [], []
        try:
            return self.U.unet_forward(x, P, prefix, levels, 2, training=True, **kw)
        finally:
            self.rec = False


@pytest.mark.parametrize('fold,batch,rate', [(False, 1, 0.0), (True, 1, 0.0), ('auto', 2, 0.3)])
def test_relu_network_vs_oracle(T, monkeypatch, fold, batch, rate):
    """one deterministic step of a ReLU network against the oracle with its ELU swapped for ReLU.  ReLU adds a tie class ELU
    does not have: a pre-activation within rounding of 0.  A site counts as a tie only where the device's mask y > 0 differs
    from the float64 oracle's AND |z64| <= 64 eps32 S (S = conv3d(|x|, |w|) + |b| in float64); at most 8 per network, and
    there the oracle takes the device's side.  Then prediction, loss and BatchNorm statistics against the float32 oracle and
    every gradient by the float64-anchored rule of the other parity tests (conftest.assert_grads_anchored).  Batch 2 with
    feature-wise dropout: one mask per sample, the oracle multiplies by the same [B, C] factors (ReLU backward through
    synthsr_act_bwd_drop, the fused act-4 data gradient followed by scale_channels)."""
    torch = T
    from synthsr_amd import ops
    from conftest import assert_grads_anchored, net_grads
    R = _ReluOracle(monkeypatch, torch)
    U = R.U
    shape, cin, levels = (16, 16, 32), 2, 3
    g = torch.Generator().manual_seed(11)
    x = torch.rand(batch, *shape, cin, generator=g)
    if batch > 1:
        x[1] *= 1.7
    target = torch.rand(batch, *shape, 1, generator=g)
    if batch == 1:
        x, target = x[0], target[0]
    prev = ops.set_deterministic(True)
    try:
        net = _relu_net(torch, fold=fold, dropout=rate, batch=batch)
        drop = None
        if rate:
            rng = np.random.default_rng(5)
            sc = {}
            for c in net.all_convs():
                keep = rng.random((batch, c['cout'])) >= rate
                keep[0, 0], keep[1, 0], keep[:, 1] = False, True, False     # dropped for one sample / for both
                sc[c['name']] = (keep / (1.0 - rate)).astype(np.float32)
            net.set_dropout_scales(sc)
            drop = {k: torch.from_numpy(v) for k, v in sc.items()}
        xs = x.reshape(batch * shape[0], *shape[1:], cin)
        loss, pred = net.loss_l1(xs.cuda(), target.reshape(-1).cuda(), want_pred=True)
        masks = [a.detach().cpu().reshape(-1) > 0 for lv in net.saved['enc'] + net.saved['dec'] for a in lv]
        net.backward()
        dev = net_grads(net)
        loss, pred = loss.item(), pred.detach().cpu().double()
    finally:
        ops.set_deterministic(prev)

    P0 = {nm: v.detach().cpu().clone() for nm, v in net.named_parameters()}
    with U.compute_dtype(torch.float64):
        with torch.no_grad():
            R.forward(x, P0, net.prefix, levels, rec=True, dropout=drop)
    assert len(R.zs) == len(masks)
    force, ties, worst = [], 0, 0.0
    eps32 = float(torch.finfo(torch.float32).eps)
    for m, z, S in zip(masks, R.zs, R.Ss):
        z, S = z.reshape(-1), S.reshape(-1)
        diff = m != (z > 0)
        if not bool(diff.any()):
            force.append(None)
            continue
        r = z.abs()[diff] / S[diff].clamp_min(1e-300)
        assert bool((r <= 64 * eps32).all()), 'ReLU masks differ at a site %.1f eps32 S from 0: not a rounding tie' % (
            float(r.max()) / eps32)
        ties += int(diff.sum())
        worst = max(worst, float(r.max()))
        force.append((diff, m[diff]))
    print('relu fold=%s: %d ReLU rounding tie(s), worst |z64| / S = %.2e (%.1f eps32)' % (fold, ties, worst, worst / eps32))
    assert ties <= 8, '%d ReLU ties in one network' % ties
    R.force = force

    def oracle(dtype):
        P = {nm: v.clone().requires_grad_(True) for nm, v in P0.items()}
        stats = {}
        if dtype == torch.float64:
            with U.compute_dtype(torch.float64):
                pr = R.forward(x, P, net.prefix, levels, collect=stats, dropout=drop)
                lr = U.l1_loss(pr, target)
        else:
            pr = R.forward(x, P, net.prefix, levels, collect=stats, dropout=drop)
            lr = U.l1_loss(pr, target)
        lr.backward()
        return {nm: v.grad.double() for nm, v in P.items()}, stats, pr.detach(), lr.item()

    g32, stats, pr32, lr32 = oracle(torch.float32)
    g64, _, _, _ = oracle(torch.float64)
    close(pred.view(pr32.shape), pr32, 5e-4, 'prediction')
    assert abs(loss - lr32) < 2e-5 * max(1.0, abs(lr32))
    for bn in net.bn_layers:
        o, C = bn['soff'], bn['C']
        close(net.bn_batch[o:o + C], stats[bn['name']][0], 1e-4, bn['name'] + ' mean')
        close(net.bn_batch[o + C:o + 2 * C], stats[bn['name']][1], 1e-4, bn['name'] + ' var')
    assert_grads_anchored(dev, g32, g64, tag='relu fold=%s' % fold)


@pytest.mark.parametrize('dtype,batch,dropout', [('f32', 1, 0.0), ('bf16', 1, 0.0), ('f32', 2, 0.25)])
def test_relu_network_deterministic(T, monkeypatch, dtype, batch, dropout):
    """two deterministic steps of a ReLU network give bit-identical gradients; bf16: the prediction follows the float64
    ReLU oracle to bf16 accuracy"""
    torch = T
    from synthsr_amd import ops
    R = _ReluOracle(monkeypatch, torch)
    shape, cin = (16, 16, 32), 2
    g = torch.Generator().manual_seed(12)
    x = torch.rand(batch, *shape, cin, generator=g)
    target = torch.rand(batch, *shape, 1, generator=g)
    prev = ops.set_deterministic(True)
    try:
        def run():
            net = _relu_net(torch, dtype=dtype, dropout=dropout, batch=batch)
            xin = x.reshape(batch * shape[0], *shape[1:], cin).cuda()
            loss, pred = net.loss_l1(xin, target.reshape(-1).cuda(), want_pred=True)
            net.backward()
            return net, loss.clone(), pred.detach().cpu().clone(), net.grads.detach().cpu().clone()

        net, loss, pred, grads = run()
        _, loss2, _, grads2 = run()
        assert torch.equal(loss, loss2) and torch.equal(grads, grads2), 'deterministic ReLU runs differ'
        assert torch.isfinite(grads).all() and bool(torch.isfinite(loss).all())
        if dtype == 'bf16':
            P = {nm: v.detach().cpu().double() for nm, v in net.named_parameters()}
            with torch.no_grad():
                pr = R.forward(x[0].double(), P, net.prefix, 3)
            close(pred.reshape(pr.shape), pr, 5e-2, 'bf16 prediction')
    finally:
        ops.set_deterministic(prev)


def test_relu_training_decreases_loss(T):
    """a ReLU network trained on one fixed sample: the loss is finite and goes down"""
    torch = T
    from synthsr_amd.unet import unet
    g = torch.Generator().manual_seed(4)
    shape = (16, 16, 32)
    x = torch.rand(*shape, 2, generator=g).cuda()
    target = torch.rand(*shape, 1, generator=g).reshape(-1).cuda()
    net = unet(nb_features=8, input_shape=list(shape) + [2], nb_levels=3, conv_size=3, nb_labels=1, feat_mult=2,
               nb_conv_per_level=2, final_pred_activation='linear', batch_norm=-1, activation='relu', seed=1)
    losses = []
    for _ in range(12):
        loss = net.loss_l1(x, target)
        losses.append(float(loss[0].item()))
        net.backward()
        net.adam_step(lr=1e-3)
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_training_entry_point_with_relu(tmp_path):
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import (synthetic_label_map, GENERATION_LABELS, GENERATION_CLASSES, PRIOR_MEANS_T1_HR,
                                       PRIOR_STDS_T1_HR)
    from synthsr_amd.training import training
    d = tmp_path / 'labels'
    d.mkdir()
    write_nifti(str(d / 'brain0_labels.nii.gz'), synthetic_label_map((40, 36, 48), 10).astype(np.float32))
    for nm, v in (('gl', GENERATION_LABELS), ('gc', GENERATION_CLASSES), ('pm', PRIOR_MEANS_T1_HR), ('ps', PRIOR_STDS_T1_HR)):
        np.save(tmp_path / (nm + '.npy'), v)
    net = training(str(d), str(tmp_path / 'models'), str(tmp_path / 'pm.npy'), str(tmp_path / 'ps.npy'),
                   str(tmp_path / 'gl.npy'), path_generation_classes=str(tmp_path / 'gc.npy'), output_shape=32, n_levels=3,
                   unet_feat_count=8, nonlin_shape_factor=.125, bias_shape_factor=.125, steps_per_epoch=2, epochs=1,
                   activation='relu', verbose=False)
    assert net.iterations == 2 and net.activation == 'relu'
    log = open(str(tmp_path / 'models' / 'logs' / 'loss.csv')).read().strip().split('\n')
    assert np.isfinite(float(log[0].split(',')[1]))


def test_fine_tuning_with_adversary_with_relu(tmp_path):
    """one critic and one generator update of fine_tuning_with_adversary.training(activation='relu'): the generator (and the
    frozen segmentation network, when one is given) are ReLU U-Nets; the losses are finite"""
    import os
    from synthsr_amd.fine_tuning_with_adversary import training
    from synthsr_amd.nifti import write_nifti
    from synthsr_amd.synthetic import GENERATION_LABELS, synthetic_label_map
    ldir, idir = tmp_path / 'labels', tmp_path / 'images'
    ldir.mkdir(), idir.mkdir()
    rng = np.random.RandomState(0)
    lut = rng.uniform(30, 220, 64)
    lab = synthetic_label_map((40, 36, 48), 10)
    write_nifti(str(ldir / 'brain0_labels.nii.gz'), lab.astype(np.float32))
    write_nifti(str(idir / 'brain0.nii.gz'), (lut[lab % 64] + rng.randn(*lab.shape)).astype(np.float32))
    np.save(tmp_path / 'gl.npy', GENERATION_LABELS)
    gen, critic = training(str(ldir), str(idir), str(tmp_path / 'models'), None, None, str(tmp_path / 'gl.npy'),
                           output_shape=32, n_levels=3, nonlin_shape_factor=.125, bias_shape_factor=.125, epochs=1,
                           steps_per_epoch=1, first_training_ratio=1, training_ratio=1, activation='relu', verbose=False)
    assert gen.activation == 'relu' and gen.iterations == 1 and critic.iterations == 1
    mdir = str(tmp_path / 'models')
    d, g = np.load(os.path.join(mdir, 'logs', 'discriminator_loss.npy')), np.load(os.path.join(mdir, 'logs', 'generator_loss.npy'))
    assert np.isfinite(d).all() and np.isfinite(g).all()
