"""The scratch contracts of the weight-gradient kernels, and every weight-gradient variant against float64 on its own.

Two promises carry the training step:
 1. deterministic planes: a weight gradient whose registered plane buffer is too small "returns SYNTHSR_EWORKSPACE and does nothing"
    (include/synthsr_hip_tuning.h) -- ops._check_wgrad registers a larger buffer and REPEATS the call on the strength of it;
 2. dwc is consumed: synthsr_conv3d_up_unpack leaves the [8,27,Cl,Cout] partials all zero, so UNet3D zeroes its persistent buffer
    once and vouches for it afterwards (ops.conv3d_up_wgrad(dwc_is_zero=True)).
One table (CASES) reaches every variant the dispatchers know (csrc/conv3d.hip dispatch_wgrad / launch_wgrad, csrc/conv_split.hip,
csrc/conv_bf16.hip) at its smallest shape; every row states its route and the test asserts it (_route mirrors the dispatcher, and
ops.conv_runs_split is the dispatcher's own answer).

Bounds: the error of a result against the float64 weight gradient of the same (bf16 rows: bf16-rounded) operands, in the _err sense
of tests/test_split_gpu.py: rms < 2e-6 and worst element < 2e-5 of the reference's rms -- that file's bounds for fp32 sums of up to
2 x 16 384 products (test_split_weight_gradient_small_and_ragged_layers_vs_float64); every row here sums at most 2 x 8 x 315 of them.
The one large row ('up_p4': the dispatcher takes that kernel from 768 tiles up, 172 032 low-resolution voxels) is outside that
product count and its float64 reference takes tens of seconds on the host: it is left out of the float64 test and runs in the
EWORKSPACE and dwc tests only, where the comparand is the default-mode (atomics) result of the same kernel."""
import collections
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

RMS_BOUND, MAX_BOUND = 2e-6, 2e-5
SMALL_PLANES = 4096     # bytes: less than one plane of any row (the smallest dW here has 27 * 8 * 16 floats)

Case = collections.namedtuple('Case', 'id entry arith dtype shape cin cout ci_off cin_total dbias route split planes f64')
#   entry: 'plain' ops.conv3d_wgrad_part | 'pad' ops.conv3d_wgrad_bf16 (x carries more channels than dW has rows) | 'up'
#          ops.conv3d_up_wgrad (shape = LOW-RES shape, cin = Cl, ci_off = the skip channels in front, cin_total = ci_off + Cl)
#   route: the kernel the dispatcher picks (_route); split: what ops.conv_runs_split answers; planes: takes deterministic planes
#          (c2 reduces through the conv context's workspace instead); f64: has a float64 reference (all but up_p4)


def _c(id, entry, arith, dtype, shape, cin, cout, route, ci_off=0, cin_total=None, dbias=True, split=False, planes=True, f64=True):
    if entry == 'up':
        ci_off, dbias = 8, False
    cin_total = ci_off + cin if cin_total is None else cin_total
    return Case(id, entry, arith, dtype, tuple(shape), cin, cout, ci_off, cin_total, dbias, route, split, planes, f64)


CASES = [
    # plain 27-tap weight gradient, fp32 matrix instructions (launch_wgrad<CK, NT, MS, 27> and the p4 / c2 kernels)
    _c('generic_ck8', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 8, 16, 'generic'),
    _c('generic_ck8_nt3_part', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 40, 40, 'generic', ci_off=8, cin_total=56),
    _c('generic_ck24_cout18', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 24, 18, 'generic'),
    _c('lean', 'plain', 'fp32_mfma', 'f32', (5, 6, 18), 24, 48, 'lean'),
    _c('box_x8', 'plain', 'fp32_mfma', 'f32', (4, 8, 8), 48, 96, 'box_x8'),
    _c('box_x4', 'plain', 'fp32_mfma', 'f32', (4, 4, 12), 48, 96, 'box_x4'),
    # ... the tile kernel's (NT, MS, tile) matrix and its mask edges: NT 1 / MS 1; NT 2 over two input-channel chunks of a partial
    # range (dbias from chunk 0 only); a masked last output-channel quad on either dy stager; every extent below the 2x4x16 tile
    _c('lean_nt1', 'plain', 'fp32_mfma', 'f32', (5, 6, 18), 24, 16, 'lean'),
    _c('lean_nt2_cc2_part', 'plain', 'fp32_mfma', 'f32', (5, 6, 18), 48, 32, 'lean', ci_off=8, cin_total=64),
    _c('lean_cout20', 'plain', 'fp32_mfma', 'f32', (5, 6, 18), 24, 20, 'lean'),
    _c('lean_below_tile', 'plain', 'fp32_mfma', 'f32', (1, 3, 7), 24, 48, 'lean'),
    _c('box_x8_nt2', 'plain', 'fp32_mfma', 'f32', (4, 8, 8), 24, 32, 'box_x8'),
    _c('box_x4_cout20', 'plain', 'fp32_mfma', 'f32', (4, 4, 12), 24, 20, 'box_x4'),
    _c('p4', 'plain', 'fp32_mfma', 'f32', (5, 6, 18), 48, 24, 'p4'),
    _c('p4_below_tile', 'plain', 'fp32_mfma', 'f32', (3, 5, 7), 24, 24, 'p4'),   # z and x extents below the 4 x 4 x 16 tile
    _c('c2_cin2', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 2, 24, 'c2', planes=False),
    _c('c2_cin2_below_tile', 'plain', 'fp32_mfma', 'f32', (3, 5, 7), 2, 24, 'c2', planes=False),
    _c('c2_cin1', 'plain', 'fp32_mfma', 'f32', (6, 5, 17), 1, 24, 'c2', planes=False),
    # ... split arithmetic (conv_split.hip: 8 / 24 / 16 input channels per workgroup), and a layer it hands back
    _c('split_8x24', 'plain', 'split', 'f32', (6, 6, 6), 8, 24, 'split', split=True),
    _c('split_24x24_part', 'plain', 'split', 'f32', (5, 7, 9), 24, 24, 'split', ci_off=16, cin_total=48, split=True),
    _c('split_48x48', 'plain', 'split', 'f32', (5, 7, 9), 48, 48, 'split', split=True),
    _c('split_fallback_40x40', 'plain', 'split', 'f32', (6, 5, 17), 40, 40, 'generic'),
    # the up-sampled channel range of a folded decoder conv
    _c('up_split', 'up', 'split', 'f32', (5, 7, 9), 32, 48, 'up_split', split=True),
    _c('up_lean', 'up', 'fp32_mfma', 'f32', (3, 2, 3), 24, 48, 'up_lean'),
    _c('up_lean_nt1_cc2', 'up', 'fp32_mfma', 'f32', (3, 2, 3), 48, 16, 'up_lean'),   # parity view, NT 1, two chunks
    _c('up_generic', 'up', 'fp32_mfma', 'f32', (3, 5, 7), 16, 24, 'up_generic'),
    _c('up_p4', 'up', 'fp32_mfma', 'f32', (64, 48, 56), 24, 24, 'up_p4', f64=False),
    # bf16 (conv_bf16.hip: chunks of 32 / 24 / 8 input channels)
    _c('bf16_part', 'plain', 'split', 'bf16', (5, 7, 9), 24, 24, 'bf16', ci_off=8, cin_total=40),
    _c('bf16_up', 'up', 'split', 'bf16', (5, 7, 9), 32, 48, 'bf16_up'),
    _c('bf16_cin_valid', 'pad', 'split', 'bf16', (6, 5, 17), 8, 24, 'bf16', cin_total=2),   # x: 8 channels, dW: the first 2
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
PLANE_CASES = [c for c in CASES if c.planes]
UP_CASES = [c for c in CASES if c.entry == 'up']
_ids = lambda cs: [c.id for c in cs]


def _route(c):
    """the dispatcher's rules restated (csrc/conv3d.hip dispatch_wgrad + launch_wgrad, wgrad_takes_split / up_wgrad_takes_split;
    csrc/conv_bf16.hip bf16_wgrad_common): which kernel a row reaches"""
    s, ci, co = c.shape, c.cin, c.cout
    if c.dtype == 'bf16':
        return 'bf16_up' if c.entry == 'up' else 'bf16'
    split = c.arith != 'fp32_mfma'
    tiles = -(-s[0] // 4) * -(-s[1] // 4) * -(-s[2] // 16)
    if c.entry == 'up':
        if split and c.arith == 'split' and ci % 16 == 0 and co % 24 == 0:
            return 'up_split'
        if co == 24 and ci % 24 == 0 and tiles >= 768:
            return 'up_p4'
        return 'up_lean' if ci % 24 == 0 and co % 4 == 0 else 'up_generic'
    if ci <= 2 and co == 24:
        return 'c2'
    if split and ci % 8 == 0 and co % 24 == 0:
        return 'split'
    if co == 24 and ci % 24 == 0:
        return 'p4'
    if ci % 24 == 0 and co % 4 == 0:
        if all(v % 4 == 0 for v in s) and s[2] % 16 != 0:
            return 'box_x8' if s[2] % 8 == 0 else 'box_x4'
        return 'lean'
    return 'generic'


def test_the_table_reaches_every_variant():
    """every kernel the dispatchers can pick has a row, and every row's declared route is what the rules give"""
    assert {c.route for c in CASES} == {'generic', 'lean', 'box_x8', 'box_x4', 'p4', 'c2', 'split', 'up_split', 'up_lean', 'up_generic',
                                        'up_p4', 'bf16', 'bf16_up'}
    for c in CASES:
        assert _route(c) == c.route, c.id
    for arith in ('fp32_mfma', 'split'):   # a partial channel range with dbias, in each arithmetic
        assert any(c.arith == arith and c.dtype == 'f32' and c.ci_off > 0 and c.cin_total > c.ci_off + c.cin and c.dbias
                   for c in CASES if c.entry == 'plain')


# ---- references -------------------------------------------------------------------------------------------------------------
def _wgrad64(x, dy):
    xi = x.double().cpu().permute(3, 0, 1, 2)[None]
    g = dy.double().cpu().permute(3, 0, 1, 2)[None]
    w = torch.zeros(dy.shape[3], x.shape[3], 3, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv3d(xi, w, None, padding=1).backward(g)
    return w.grad.permute(2, 3, 4, 1, 0)


def _up_wgrad64(lo, dz):
    """float64 weight gradient of conv3(UpSampling3D(2)(lo)) w.r.t. its [3,3,3,Cl,Cout] kernel"""
    up = lo.double().cpu().repeat_interleave(2, 0).repeat_interleave(2, 1).repeat_interleave(2, 2)
    return _wgrad64(up, dz)


def _err(y, ref):
    d = y.double().cpu() - ref.double().cpu()
    scale = float(ref.double().pow(2).mean().sqrt())
    return float(d.abs().max()) / scale, float(d.pow(2).mean().sqrt()) / scale


def _within_bounds(y, ref, what):
    mx, rms = _err(y, ref)
    print('%s: worst element %.3g, rms %.3g of the reference rms' % (what, mx, rms))
    assert rms < RMS_BOUND and mx < MAX_BOUND, (what, mx, rms)


def _layer_data(dtype, entry, shape, cin, cout, seed, nvol=2, on_device=False):
    """nvol (x, dy) pairs on the device; the second volume's gradient is 1.7x larger, as in tests/test_split_gpu.py"""
    dt = torch.bfloat16 if dtype == 'bf16' else torch.float32
    g = torch.Generator(device='cuda' if on_device else 'cpu').manual_seed(seed)
    dev = 'cuda' if on_device else 'cpu'
    hi = tuple(2 * v for v in shape) if entry == 'up' else tuple(shape)
    out = []
    for s in (1.0, 1.7)[:nvol]:
        x = torch.randn(*shape, cin, generator=g, device=dev)
        dy = torch.randn(*hi, cout, generator=g, device=dev) * s
        out.append((x.to(dt).cuda().contiguous(), dy.to(dt).cuda().contiguous()))
    return out


@functools.lru_cache(maxsize=None)
def _data(cid):
    c = BY_ID[cid]
    return _layer_data(c.dtype, c.entry, c.shape, c.cin, c.cout, seed=sum(c.shape) + 7 * c.cin + c.cout, on_device=not c.f64)


@functools.lru_cache(maxsize=None)
def _ref64(cid):
    """(dW rows [ci_off, ci_off + n) in float64, dbias in float64) of the two volumes of a row (bf16: of the rounded operands)"""
    c = BY_ID[cid]
    assert c.f64
    n = c.cin_total if c.entry == 'pad' else c.cin    # 'pad': only the first cin_total channels of x have rows in dW
    fn = _up_wgrad64 if c.entry == 'up' else _wgrad64
    return (sum(fn(x[..., :n], dy) for x, dy in _data(cid)), sum(dy.double().cpu().sum((0, 1, 2)) for _, dy in _data(cid)))


def _mode(c):
    """asserts what can be asserted about the route of a row under the arithmetic in force"""
    from synthsr_amd import ops
    assert ops.conv_arithmetic() == c.arith
    if c.dtype == 'f32':
        kind = 'conv3d_up_wgrad' if c.entry == 'up' else 'conv3d_wgrad'
        assert ops.conv_runs_split(kind, c.shape, c.cin, c.cout) == c.split, c.id
    assert _route(c) == c.route


def _new_grads(c):
    dw = torch.zeros(3, 3, 3, c.cin_total, c.cout, device='cuda')
    return dw, (torch.zeros(c.cout, device='cuda') if c.dbias else None)


def _new_dwc(c, fill=None):
    if c.entry != 'up':
        return None
    dwc = torch.empty(8, 27, c.cin, c.cout, device='cuda')
    return dwc if fill is None else dwc.fill_(fill)


def _run(c, data, dw, db, dwc=None, dwc_is_zero=False):
    from synthsr_amd import ops
    for x, dy in data:
        if c.entry == 'up':
            ops.conv3d_up_wgrad(x, dy, dwc, dw, c.ci_off, dwc_is_zero=dwc_is_zero)
        elif c.entry == 'pad':
            ops.conv3d_wgrad_bf16(x, dy, dw, db)
        else:
            ops.conv3d_wgrad_part(x, dy, dw, c.ci_off, db)
    return dw, db


def _c_call(c, x, dy, dw, db, dwc):
    """the C entry point ops calls for this row, directly: returns its code"""
    from synthsr_amd import _lib, ops
    lib, p, st, s3 = _lib.load(), _lib.ptr, _lib.stream(), _lib.i3(c.shape)
    if c.entry == 'up' and c.dtype == 'bf16':
        return lib.synthsr_conv3d_bf16_up_wgrad(p(x), p(dy), p(dwc), s3, c.cin, c.cout, st)
    if c.entry == 'up':
        return lib.synthsr_conv3d_up_wgrad(ops.conv_ctx(), p(x), p(dy), p(dwc), s3, c.cin, c.cout, st)
    if c.entry == 'pad':
        return lib.synthsr_conv3d_bf16_wgrad(p(x), p(dy), p(dw), p(db), s3, c.cin_total, 0, c.cin, c.cout, st)
    if c.dtype == 'bf16':
        return lib.synthsr_conv3d_bf16_wgrad_part(p(x), p(dy), p(dw), p(db), s3, c.cin_total, c.ci_off, c.cin, c.cout, st)
    return lib.synthsr_conv3d_wgrad_bias(ops.conv_ctx(), p(x), p(dy), p(dw), p(db), s3, c.cin_total, c.ci_off, c.cin, c.cout, st)


def _rows(c, dw):
    """(the rows of dW a row of the table writes, all other rows)"""
    n = c.cin_total if c.entry == 'pad' else c.cin
    return dw[:, :, :, c.ci_off:c.ci_off + n], torch.cat([dw[:, :, :, :c.ci_off], dw[:, :, :, c.ci_off + n:]], 3)


class _Modes:
    """`with _Modes(arith, det):` -- the conv arithmetic and the deterministic switch of a row, restored afterwards together with
    a normally sized plane registration"""

    def __init__(self, arith, det):
        self.arith, self.det = arith, det

    def __enter__(self):
        from synthsr_amd import ops
        self.prev_arith = ops.set_conv_arithmetic(self.arith)
        self.prev_det = ops.set_deterministic(self.det)
        return self

    def __exit__(self, *a):
        from synthsr_amd import ops
        try:
            if self.det:
                ops._register_det_planes(64 << 20)
        finally:
            ops.set_deterministic(self.prev_det)
            ops.set_conv_arithmetic(self.prev_arith)


@functools.lru_cache(maxsize=None)
def _result(cid, det):
    """(dW, dbias) of the two volumes of a row accumulated from zero, planes amply registered; computed once per row and mode"""
    from synthsr_amd import ops
    c = BY_ID[cid]
    with _Modes(c.arith, det):
        _mode(c)
        dw, db = _run(c, _data(cid), *_new_grads(c), dwc=_new_dwc(c))
        if det:
            assert ops.deterministic_status() == 1
    return dw, db


def _check_result(c, dw, db, what):
    """part B's assertions on one result: float64 bounds on dW (and dbias), rows outside the channel range exactly zero"""
    own, other = _rows(c, dw)
    assert other.numel() == 0 or float(other.abs().max()) == 0.0, (what, 'rows outside the channel range were written')
    if c.f64:
        ref_w, ref_b = _ref64(c.id)
        _within_bounds(own, ref_w, '%s %s dW' % (c.id, what))
        if c.dbias:
            _within_bounds(db, ref_b, '%s %s dbias' % (c.id, what))


# ---- B: every variant against float64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('det', [True, False], ids=['ordered', 'atomics'])
@pytest.mark.parametrize('cid', _ids([c for c in CASES if c.f64]))
def test_every_weight_gradient_variant_vs_float64(cid, det):
    """two volumes accumulated into one dW / dbias (the second onto a non-zero gradient) in either mode: within 2e-6 rms / 2e-5
    worst element of the float64 gradient, the fp32-MFMA and bf16 kernels measured directly and not as the split kernels'
    yardstick; rows of dW outside [ci_off, ci_off + Cin) exactly zero; ordered sums bit-identical on a second run.  (up_p4: see
    the module docstring; it is held by the EWORKSPACE and dwc tests.)"""
    from synthsr_amd import ops
    c = BY_ID[cid]
    dw, db = _result(cid, det)
    _check_result(c, dw, db, 'ordered' if det else 'atomics')
    if det:
        with _Modes(c.arith, True):
            dw2, db2 = _run(c, _data(cid), *_new_grads(c), dwc=_new_dwc(c))
            assert ops.deterministic_status() == 1
        assert torch.equal(dw2, dw) and (db is None or torch.equal(db2, db))


# ---- C: SYNTHSR_EWORKSPACE = nothing happened ---------------------------------------------------------------------------------
def _sentinel(t):
    if t is None:
        return None, None
    v = (torch.arange(t.numel(), device='cuda') % 251 + 1).to(t.dtype).view(t.shape)
    return v, v.clone()


def _plane_floats(c):
    """one plane of a row: include/../csrc/conv3d.hip det_prepare_impl (every call needs at least one)"""
    elems = 8 * 27 * c.cin * c.cout if c.entry == 'up' else 27 * c.cin_total * c.cout
    return (elems + c.cout + 3) // 4 * 4


@pytest.mark.parametrize('cid', _ids(PLANE_CASES))
def test_too_small_planes_return_eworkspace_and_do_nothing(cid):
    """the C entry point under a 4 KB plane registration: -3, and dW, dbias and dwc keep every bit of a sentinel pattern -- no
    kernel, no memset ran before the size check (include/synthsr_hip_tuning.h: "returns SYNTHSR_EWORKSPACE and does nothing";
    the generic fp32 kernel used to add its column sums to dbias first); the demand the library reports covers the call"""
    from synthsr_amd import _lib, ops
    c = BY_ID[cid]
    x, dy = _data(cid)[0]
    with _Modes(c.arith, True):
        _mode(c)
        ops._resize_det_planes(SMALL_PLANES)
        dw, db = _new_grads(c)
        (dw, dw0), (db, db0), (dwc, dwc0) = _sentinel(dw), _sentinel(db), _sentinel(_new_dwc(c))
        rc = _c_call(c, x, dy, dw, db, dwc)
        torch.cuda.synchronize()
        assert rc == -3
        assert torch.equal(dw, dw0)
        assert db is None or torch.equal(db, db0), 'dbias changed by a call that reported SYNTHSR_EWORKSPACE'
        assert dwc is None or torch.equal(dwc, dwc0)
        assert int(_lib.load().synthsr_deterministic_workspace_demand()) >= max(4 * _plane_floats(c), SMALL_PLANES + 1)


@pytest.mark.parametrize('cid', _ids(PLANE_CASES))
def test_too_small_planes_are_regrown_and_the_call_repeated_once(cid):
    """the same through ops: no exception, the registration grows to the demand, and dW / dbias are bit-identical to a run that
    found a large buffer (dbias NOT doubled by the repeat) -- and within the float64 bounds, which two equally wrong runs would miss
    (up_p4: within the same bounds of the default-mode result)"""
    from synthsr_amd import _lib, ops
    c = BY_ID[cid]
    want_w, want_b = _result(cid, True)
    with _Modes(c.arith, True):
        _mode(c)
        ops._resize_det_planes(SMALL_PLANES)
        dev = torch.cuda.current_device()
        assert ops._det_planes[dev].numel() == SMALL_PLANES
        dw, db = _run(c, _data(cid), *_new_grads(c), dwc=_new_dwc(c))
        assert ops.deterministic_status() == 1
        demand = int(_lib.load().synthsr_deterministic_workspace_demand())
        assert ops._det_planes[dev].numel() >= demand >= 4 * _plane_floats(c)
    if db is not None:
        print('%s dbias[:4] after the repeat %s, single shot %s' % (cid, db[:4].tolist(), want_b[:4].tolist()))
        assert torch.equal(db, want_b), 'dbias differs after the repeated call (counted twice?)'
    assert torch.equal(dw, want_w)
    _check_result(c, dw, db, 'regrown planes')
    if not c.f64:
        _within_bounds(_rows(c, dw)[0], _rows(c, _result(cid, False)[0])[0], '%s ordered vs atomics' % cid)


# ---- D: dwc is all zeros after the unpack ----------------------------------------------------------------------------------------
FOLLOWERS = {'up_generic': (((4, 6, 5), 8, 24), ((6, 5, 9), 8, 8))}   # smaller layers, in the order a decoder visits them
FOLLOWERS_DEFAULT = (((4, 6, 5), 16, 24), ((6, 5, 9), 8, 8))


@functools.lru_cache(maxsize=None)
def _follower(dtype, lo_shape, cl, co):
    (lo, dz), = _layer_data(dtype, 'up', lo_shape, cl, co, seed=11 * cl + co, nvol=1)
    return lo, dz, _up_wgrad64(lo, dz)


@pytest.mark.parametrize('det', [True, False], ids=['ordered', 'atomics'])
@pytest.mark.parametrize('cid', _ids(UP_CASES))
def test_dwc_is_all_zeros_after_unpack_and_reusable(cid, det):
    """every folded variant (split, fp32 lean / generic / up-p4, bf16) leaves a zeroed dwc ALL zero -- the whole buffer, not only the
    view -- so that a prefix of it, viewed as [8,27,Cl',Cout'] of a smaller layer, serves the next two decoder levels with
    dwc_is_zero=True: their dW within the float64 bounds and, with ordered sums, bit-identical to a run on a freshly zeroed buffer"""
    from synthsr_amd import ops
    c = BY_ID[cid]
    n = 8 * 27 * c.cin * c.cout
    buf = torch.zeros(n + 4099, device='cuda')
    with _Modes(c.arith, det):
        _mode(c)
        dw, _ = _run(c, _data(cid), _new_grads(c)[0], None, dwc=buf[:n].view(8, 27, c.cin, c.cout), dwc_is_zero=True)
        assert int(torch.count_nonzero(buf)) == 0, 'partials left behind by %s' % c.route
        if det:
            assert torch.equal(dw, _result(cid, True)[0])
        else:
            _within_bounds(_rows(c, dw)[0], _rows(c, _result(cid, True)[0])[0], '%s atomics vs ordered' % cid)
        for lo_shape, cl, co in FOLLOWERS.get(cid, FOLLOWERS_DEFAULT):
            assert 8 * 27 * cl * co < n
            lo, dz, ref = _follower(c.dtype, lo_shape, cl, co)
            res = []
            for dwc, vouched in ((buf[:8 * 27 * cl * co].view(8, 27, cl, co), True), (torch.zeros(8, 27, cl, co, device='cuda'), False)):
                d = torch.zeros(3, 3, 3, 8 + cl, co, device='cuda')
                ops.conv3d_up_wgrad(lo, dz, dwc, d, 8, dwc_is_zero=vouched)
                res.append(d)
            assert int(torch.count_nonzero(buf)) == 0
            assert float(res[0][:, :, :, :8].abs().max()) == 0.0
            _within_bounds(res[0][:, :, :, 8:], ref, '%s -> reused prefix as %d x %d' % (cid, cl, co))
            if det:
                assert torch.equal(res[0], res[1])
        assert not det or ops.deterministic_status() == 1


# ---- E: the U-Net's zero record ---------------------------------------------------------------------------------------------------
def test_unet_zero_record_survives_an_interrupted_step(monkeypatch):
    """an exception between a folded weight gradient and its unpack leaves partials in the network's persistent dwc: the record
    that lets later layers and steps skip the memset (UNet3D._dwc_zeroed) must not vouch for that buffer -- the next full step
    of the interrupted network is bit-identical (ordered sums) to the same step of a fresh network"""
    from synthsr_amd import ops
    from synthsr_amd.unet import unet
    shape = (16, 16, 32)
    g = torch.Generator(device='cpu').manual_seed(21)
    x = torch.randn(*shape, 2, generator=g).cuda()
    target = torch.randn(*shape, 1, generator=g).cuda()

    def make():
        return unet(nb_features=24, input_shape=list(shape) + [2], nb_levels=3, conv_size=3, nb_labels=1, feat_mult=2,
                    nb_conv_per_level=2, batch_norm=-1, activation='elu', final_pred_activation='linear', seed=5, fold_upsample=True)

    def step(net):
        loss = net.loss_l1(x, target.reshape(-1))[0].clone()
        net.backward()
        return loss, net.grads.clone()

    with _Modes('split', True):
        net, control = make(), make()
        assert sum(1 for d in net.dec if d['fold']) == 2
        real, calls = ops.conv3d_up_wgrad, []

        def interrupted(lo, dout, dwc, dw, ci_off, dwc_is_zero=False):
            calls.append(dwc_is_zero)
            if len(calls) == 2:
                dwc.fill_(0.5)
                raise RuntimeError('interrupted between the weight gradient and its unpack')
            return real(lo, dout, dwc, dw, ci_off, dwc_is_zero=dwc_is_zero)

        with monkeypatch.context() as m:
            m.setattr(ops, 'conv3d_up_wgrad', interrupted)
            with pytest.raises(RuntimeError, match='interrupted between'):
                step(net)
        assert len(calls) == 2
        loss, grads = step(net)
        loss_c, grads_c = step(control)
        assert ops.deterministic_status() == 1
    worst = float((grads - grads_c).abs().max())
    print('interrupted vs fresh network: largest gradient difference %.3g (largest gradient %.3g)' % (worst, float(grads_c.abs().max())))
    assert torch.equal(loss, loss_c)
    assert torch.equal(grads, grads_c), 'stale dwc partials entered dW: largest difference %g' % worst


# ---- F: a failed plane allocation ---------------------------------------------------------------------------------------------------
def test_failed_plane_allocation_leaves_no_stale_registration(monkeypatch):
    """growing the plane buffer releases the old one: when the larger allocation raises, the library must not be left holding the
    released pointer (torch may hand it to another tensor) -- the registration is withdrawn, the next weight gradient finds none
    (-3, nothing written), and ops registers afresh: result bit-identical to the usual one and within the float64 bounds"""
    from synthsr_amd import ops
    c = BY_ID['generic_ck8_nt3_part']
    x, dy = _data(c.id)[0]
    want_w, want_b = _result(c.id, True)
    with _Modes(c.arith, True):
        _mode(c)
        dev = torch.cuda.current_device()
        held = ops._det_planes[dev]
        real = torch.empty

        def failing(*a, **k):
            if k.get('dtype') is torch.uint8:
                raise torch.cuda.OutOfMemoryError('no room for the planes')
            return real(*a, **k)

        with monkeypatch.context() as m:
            m.setattr(torch, 'empty', failing)
            with pytest.raises(torch.cuda.OutOfMemoryError):
                ops._register_det_planes(held.numel() + (1 << 20))
        # either the library still holds a live buffer that ops references, or it holds none
        assert ops._det_planes.get(dev) is held or dev not in ops._det_planes
        if dev not in ops._det_planes:
            dw, db = _new_grads(c)
            (dw, dw0), (db, db0) = _sentinel(dw), _sentinel(db)
            assert _c_call(c, x, dy, dw, db, None) == -3      # withdrawn: nothing registered, nothing written
            torch.cuda.synchronize()
            assert torch.equal(dw, dw0) and torch.equal(db, db0)
        del held
        dw, db = _run(c, _data(c.id), *_new_grads(c))
        assert ops.deterministic_status() == 1
        assert ops._det_planes[dev].numel() > 0
    assert torch.equal(dw, want_w) and torch.equal(db, want_b)
    _check_result(c, dw, db, 'after a failed allocation')
